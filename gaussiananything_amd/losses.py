"""Photometric loss on the device -- the host side of include/ga_loss.h (HIP kernels, csrc/photo_loss.hip).

    ssim, ssim_loss      the reference's ``_ssim`` / ``ssim_loss`` (nsr/losses/builder.py): 11-tap Gaussian window, sigma 1.5, zero
                         padding, C1 = 0.01^2 and C2 = 0.03^2 whatever the range of the images
    photometric_loss     the reference's ``calc_2d_rec_loss`` in its ``test_mode or not fg_mse`` branch with ``color_criterion='mse'``:
                         ``l2_lambda * MSE + l1_lambda * L1 + ssim_lambda * (1 - SSIM)`` and the dict of metrics it logs

One forward pass reads each pixel of both images once and yields the per-image means of SSIM, |x - y| and (x - y)^2; one backward
launch turns the gradient of those means into the gradient of the prediction.  The mean over the batch and the weighting are torch's
(the arrangement of ``pointcloud.chamfer_distance(differentiable=True)``), so ``grad_out`` reaches the kernel in device memory: no host
synchronisation, nothing frozen into a captured graph.  The gradient is with respect to the prediction only.  There is no CPU
fallback: without the HIP library, or on a CPU tensor, the calls raise.

Not built: LPIPS, the identity loss, the ``fg_mse`` masked branch.  ``PSNR`` restates
``kornia.metrics.psnr(x / 2 + 0.5, y / 2 + 0.5, 1.0)`` = ``10 log10(4 / MSE)``; kornia is absent, so that value is UNPINNED.

The geometry half (csrc/geo_loss.hip), for the maps ``GaussianRenderer2DGS.render`` returns:

    depth_to_normal      the reference's ``depth_to_normal_2`` (utils/point_utils.py) for V views at once, differentiable in depth
    surface_normal       the ``surf_normal`` the reference's renderer comments out: those normals times ``alpha.detach()``
    geo_means            per view the means of ``1 - <rend_normal, surf_normal>``, ``dist`` and ``|alpha - mask|``
    geometric_loss       ``lambda_normal * normal + lambda_dist * dist + lambda_alpha * alpha`` and its dict (nsr/train_nv_util.py,
                         ``calc_alpha_loss`` of nsr/losses/builder.py)

One forward and one backward launch; gradients reach ``rend_normal``, ``depth``, ``dist`` and ``alpha``.  Two conventions meet here:
``depth_to_normal`` takes the column-vector world-to-camera matrix, as the reference's function does; everything that takes ``cam_view``
takes what ``render`` takes, its transpose.  Either way THE MATRIX MUST BE RIGID: the reference inverts it, this transposes its rotation
block.  Where the cross product of a pixel vanishes (both row or both column neighbours are holes) the gradient through that pixel's
normal is zero, where torch's ``F.normalize`` hands back ``G / 1e-12``."""
from __future__ import annotations

import ctypes

import torch

from . import _lib

WINDOW_SIZE = 11


def plan(num_images: int, channels: int, height: int, width: int) -> dict:
    """What the launches do for this shape (``ga_photo_loss_plan``): tile, grid, LDS bytes, partial count."""
    pl = _lib.GaPhotoLossPlan()
    _lib.check(_lib.lib().ga_photo_loss_plan(int(num_images), int(channels), int(height), int(width), ctypes.byref(pl)), "ga_photo_loss_plan")
    return {name: int(getattr(pl, name)) for name, _ in _lib.GaPhotoLossPlan._fields_}


def _validate(img1, img2, window_size=WINDOW_SIZE):
    """host-side checks, before anything is enqueued -> the library handle"""
    for name, t in (("img1", img1), ("img2", img2)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor, not {type(t).__name__}")
        if not t.is_floating_point():
            raise TypeError(f"{name} must be a floating-point tensor, not {t.dtype}")
    if int(window_size) != WINDOW_SIZE:
        raise ValueError(f"window_size must be {WINDOW_SIZE}: the kernel is built for the reference's window")
    if img1.dim() != 4 or img1.shape != img2.shape or img1.numel() == 0:
        raise ValueError(f"img1 and img2 are [N, C, H, W] tensors of one shape, not {tuple(img1.shape)} and {tuple(img2.shape)}")
    if img2.requires_grad and torch.is_grad_enabled():
        raise ValueError("img2 (the target) requires grad: the gradient is with respect to img1 only")
    if img1.device.type != "cuda" or img2.device != img1.device:
        raise ValueError("img1 and img2 must be on one GPU (no CPU fallback)")
    return _lib.lib()   # raises when the library is missing


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _forward(L, x, y, save):
    """x, y fp32 contiguous on one GPU -> (out [N,3], workspace)"""
    N, C, H, W = x.shape
    flags = _lib.GA_PHOTO_LOSS_SAVE if save else 0
    nbytes = int(L.ga_photo_loss_workspace_bytes(N, C, H, W, flags))
    if nbytes == 0:
        raise ValueError(f"ga_photo_loss: shape {tuple(x.shape)} is out of range")
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    out = torch.empty(N, 3, dtype=torch.float32, device=x.device)
    args = _lib.GaPhotoLossArgs(N, C, H, W, flags, 0, x.data_ptr(), y.data_ptr(), out.data_ptr(), None, None, None,
                                workspace.data_ptr(), nbytes)
    with torch.cuda.device(x.device):
        _lib.check(L.ga_photo_loss_forward(ctypes.byref(args), _stream(x.device)), "ga_photo_loss_forward")
    return out, workspace


class _PhotoMeans(torch.autograd.Function):
    """per-image means [N,3] (SSIM, L1, L2): forward ``ga_photo_loss_forward`` with the derivative maps saved, backward
    ``ga_photo_loss_backward`` on them"""

    @staticmethod
    def forward(ctx, img1, x, y):
        out, workspace = _forward(_lib.lib(), x, y, True)
        ctx.save_for_backward(x, y, workspace)
        ctx.dtype = img1.dtype
        return out

    @staticmethod
    def backward(ctx, grad):
        x, y, workspace = ctx.saved_tensors
        N, C, H, W = x.shape
        g = grad.to(torch.float32).contiguous()
        grad_img1 = torch.empty_like(x)
        args = _lib.GaPhotoLossArgs(N, C, H, W, _lib.GA_PHOTO_LOSS_SAVE, 0, x.data_ptr(), y.data_ptr(), None, None, g.data_ptr(),
                                    grad_img1.data_ptr(), workspace.data_ptr(), workspace.numel())
        with torch.cuda.device(x.device):
            _lib.check(_lib.lib().ga_photo_loss_backward(ctypes.byref(args), _stream(x.device)), "ga_photo_loss_backward")
        return grad_img1.to(ctx.dtype), None, None


def photo_means(img1: torch.Tensor, img2: torch.Tensor, window_size: int = WINDOW_SIZE) -> torch.Tensor:
    """-> [N, 3] fp32: per image the mean SSIM, the mean |img1 - img2| and the mean (img1 - img2)^2, from one pass.  Carries the
    gradient with respect to ``img1`` when it requires grad; a forward-only call does not store the derivative maps."""
    L = _validate(img1, img2, window_size)
    x = img1.detach().float().contiguous()
    y = img2.detach().float().contiguous()
    if torch.is_grad_enabled() and img1.requires_grad:
        return _PhotoMeans.apply(img1, x, y)
    return _forward(L, x, y, False)[0]


def ssim(img1: torch.Tensor, img2: torch.Tensor, window_size: int = WINDOW_SIZE, size_average: bool = True) -> torch.Tensor:
    """The reference's ``_ssim``: a scalar, or one value per image ``[N]`` with ``size_average=False``."""
    per_image = photo_means(img1, img2, window_size)[:, 0]
    return per_image.mean() if size_average else per_image


def ssim_loss(img1: torch.Tensor, img2: torch.Tensor, window_size: int = WINDOW_SIZE, size_average: bool = True) -> torch.Tensor:
    """``1 - ssim(...)``, the reference's method of the same name."""
    return 1 - ssim(img1, img2, window_size, size_average)


def photometric_loss(input: torch.Tensor, gt: torch.Tensor, l2_lambda: float = 1.0, l1_lambda: float = 0.0, ssim_lambda: float = 0.0):
    """-> (loss, loss_dict) with ``loss = l2_lambda * MSE + l1_lambda * L1 + ssim_lambda * (1 - SSIM)`` and the reference's keys
    ``loss``, ``loss_l2`` (= l2_lambda * MSE), ``loss_ssim`` (= 1 - SSIM), ``mae``, ``PSNR``, ``SSIM``.

    Departure from the reference: all three sums come from the one pass, so ``mae``, ``loss_ssim`` and ``SSIM`` always hold the true
    values; the reference leaves them at 0 / 0 / 1 when their lambda is 0.  A term whose lambda is 0 still adds nothing to ``loss``.
    ``PSNR = 10 log10(4 / MSE)`` (images in [-1, 1] mapped to [0, 1]) is restated from kornia's definition and unpinned."""
    means = photo_means(input, gt).mean(0)   # equal-sized images: the mean of the per-image means is the mean over everything
    ssim_value, l1, mse = means[0], means[1], means[2]
    loss_ssim = 1 - ssim_value
    rec_loss = mse * l2_lambda
    loss = rec_loss + loss_ssim * ssim_lambda + l1_lambda * l1
    with torch.no_grad():
        psnr = 10.0 * torch.log10(4.0 / mse.detach())
    return loss, {"loss": loss, "loss_l2": rec_loss, "loss_ssim": loss_ssim, "mae": l1, "PSNR": psnr, "SSIM": ssim_value}


# ---- geometry losses (include/ga_loss.h: ga_geo_loss_*) ----------------------------------------------------------------------------
def geo_plan(num_views: int, height: int, width: int) -> dict:
    """What the launches do for this shape (``ga_geo_loss_plan``): tile, grid, LDS bytes of both kernels, partial count."""
    pl = _lib.GaGeoLossPlan()
    _lib.check(_lib.lib().ga_geo_loss_plan(int(num_views), int(height), int(width), ctypes.byref(pl)), "ga_geo_loss_plan")
    return {name: int(getattr(pl, name)) for name, _ in _lib.GaGeoLossPlan._fields_}


def _validate_geo(maps, view, tanfov, constants=()):
    """host-side checks, before anything is enqueued.  ``maps``: (name, tensor, channels), every one [V, channels, H, W] on one GPU;
    ``view`` [V, 4, 4]; ``constants``: names of maps that must not require grad -> (V, H, W, the library handle)"""
    for name, t, _ in tuple(maps) + (("view", view, None),):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor, not {type(t).__name__}")
        if not t.is_floating_point():
            raise TypeError(f"{name} must be a floating-point tensor, not {t.dtype}")
    if isinstance(tanfov, torch.Tensor):
        raise TypeError("tanfov must be a number: a tensor would have to be read back from the device")
    if not (float(tanfov) > 0.0 and float(tanfov) < float("inf")):
        raise ValueError(f"tanfov must be positive and finite, not {tanfov}")
    first = maps[0][1]
    if first.dim() != 4 or first.numel() == 0:
        raise ValueError(f"{maps[0][0]} is a [V, {maps[0][2]}, H, W] tensor, not {tuple(first.shape)}")
    V, _, H, W = first.shape
    for name, t, ch in maps:
        if tuple(t.shape) != (V, ch, H, W):
            raise ValueError(f"{name} must be [{V}, {ch}, {H}, {W}] (as {maps[0][0]}), not {tuple(t.shape)}")
        if name in constants and t.requires_grad and torch.is_grad_enabled():
            raise ValueError(f"{name} requires grad: it is a constant of the loss")
    if tuple(view.shape) != (V, 4, 4):
        raise ValueError(f"the view matrices must be [{V}, 4, 4], not {tuple(view.shape)}")
    if view.requires_grad and torch.is_grad_enabled():
        raise ValueError("the view matrices require grad: there is no gradient with respect to the camera")
    for name, t, _ in tuple(maps) + (("view", view, None),):
        if t.device.type != "cuda" or t.device != first.device:
            raise ValueError(f"{name} must be on the GPU of {maps[0][0]} (no CPU fallback)")
    return V, H, W, _lib.lib()   # raises when the library is missing


def _f32(t):
    return None if t is None else t.detach().float().contiguous()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _geo_args(flags, tanfov, view, rn, depth, alpha, dist, target, mask, shape):
    V, H, W = shape
    a = _lib.GaGeoLossArgs()
    a.num_views, a.height, a.width, a.flags, a.tanfov = V, H, W, flags, float(tanfov)
    a.view, a.rend_normal, a.depth, a.alpha, a.dist = _ptr(view), _ptr(rn), _ptr(depth), _ptr(alpha), _ptr(dist)
    a.target_normal, a.mask = _ptr(target), _ptr(mask)
    return a


class _GeoMeans(torch.autograd.Function):
    """per-view means [V,3] (normal, dist, alpha): ``ga_geo_loss_forward`` / ``ga_geo_loss_backward``; the backward recomputes the
    normals from depth, so only the inputs are kept"""

    @staticmethod
    def forward(ctx, rend_normal, depth, dist, alpha, tanfov, view, rn, d, a, ds, target, mask):
        V, _, H, W = rn.shape
        L = _lib.lib()
        flags = _lib.GA_GEO_LOSS_TARGET if target is not None else 0
        nbytes = int(L.ga_geo_loss_workspace_bytes(V, H, W))
        if nbytes == 0:
            raise ValueError(f"ga_geo_loss: shape {(V, H, W)} is out of range")
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=rn.device)
        out = torch.empty(V, 3, dtype=torch.float32, device=rn.device)
        args = _geo_args(flags, tanfov, view, rn, d, a, ds, target, mask, (V, H, W))
        args.out, args.workspace, args.workspace_bytes = out.data_ptr(), workspace.data_ptr(), nbytes
        with torch.cuda.device(rn.device):
            _lib.check(L.ga_geo_loss_forward(ctypes.byref(args), _stream(rn.device)), "ga_geo_loss_forward")
        ctx.save_for_backward(view, rn, d, a, ds, target, mask)
        ctx.flags, ctx.tanfov = flags, float(tanfov)
        ctx.dtypes = (rend_normal.dtype, depth.dtype, dist.dtype, alpha.dtype)
        return out

    @staticmethod
    def backward(ctx, grad):
        view, rn, d, a, ds, target, mask = ctx.saved_tensors
        V, _, H, W = rn.shape
        g = grad.to(torch.float32).contiguous()
        want = ctx.needs_input_grad[:4]
        outs = [torch.empty_like(t) if w else None for t, w in zip((rn, d, ds, a), want)]
        args = _geo_args(ctx.flags, ctx.tanfov, view, rn, d, a, ds, target, mask, (V, H, W))
        args.grad_out = g.data_ptr()
        args.grad_rend_normal, args.grad_depth, args.grad_dist, args.grad_alpha = (_ptr(t) for t in outs)
        with torch.cuda.device(rn.device):
            _lib.check(_lib.lib().ga_geo_loss_backward(ctypes.byref(args), _stream(rn.device)), "ga_geo_loss_backward")
        return tuple(None if t is None else t.to(dt) for t, dt in zip(outs, ctx.dtypes)) + (None,) * 8


class _SurfNormal(torch.autograd.Function):
    """[V,3,H,W] normals of the depth map (times alpha when given): the kernels with GA_GEO_LOSS_NORMALS; gradient to depth only"""

    @staticmethod
    def forward(ctx, depth, tanfov, view, d, a):
        V, _, H, W = d.shape
        out = torch.empty(V, 3, H, W, dtype=torch.float32, device=d.device)
        args = _geo_args(_lib.GA_GEO_LOSS_NORMALS, tanfov, view, None, d, a, None, None, None, (V, H, W))
        args.surf_normal_out = out.data_ptr()
        with torch.cuda.device(d.device):
            _lib.check(_lib.lib().ga_geo_loss_forward(ctypes.byref(args), _stream(d.device)), "ga_geo_loss_forward")
        ctx.save_for_backward(view, d, a)
        ctx.tanfov, ctx.dtype = float(tanfov), depth.dtype
        return out

    @staticmethod
    def backward(ctx, grad):
        view, d, a = ctx.saved_tensors
        V, _, H, W = d.shape
        g = grad.to(torch.float32).contiguous()
        grad_depth = torch.empty_like(d)
        args = _geo_args(_lib.GA_GEO_LOSS_NORMALS, ctx.tanfov, view, None, d, a, None, None, None, (V, H, W))
        args.grad_out, args.grad_depth = g.data_ptr(), grad_depth.data_ptr()
        with torch.cuda.device(d.device):
            _lib.check(_lib.lib().ga_geo_loss_backward(ctypes.byref(args), _stream(d.device)), "ga_geo_loss_backward")
        return grad_depth.to(ctx.dtype), None, None, None, None


def _surf_normal(depth, alpha, view, tanfov):
    """depth [V,1,H,W], alpha [V,1,H,W] or None, view [V,4,4] in cam_view's convention (validated by the caller)"""
    return _SurfNormal.apply(depth, float(tanfov), _f32(view), _f32(depth), _f32(alpha))


def depth_to_normal(world_view_transform: torch.Tensor, tanfov: float, depth: torch.Tensor) -> torch.Tensor:
    """The reference's ``depth_to_normal_2`` for V views: ``world_view_transform`` [V, 4, 4] is the COLUMN-vector world-to-camera
    matrix, as that function takes it (the transpose of ``render``'s ``cam_view``) and must be rigid; ``depth`` [V, 1, H, W] ->
    [V, 3, H, W] fp32 world-space normals, 0 on the one-pixel border.  Differentiable in ``depth``."""
    _validate_geo((("depth", depth, 1),), world_view_transform, tanfov)
    return _surf_normal(depth, None, world_view_transform.transpose(1, 2), tanfov)


def surface_normal(depth: torch.Tensor, alpha: torch.Tensor, cam_view: torch.Tensor, tanfov: float) -> torch.Tensor:
    """``depth``, ``alpha`` [B, V, 1, H, W] and ``cam_view`` [B, V, 4, 4] as ``render`` takes and returns them -> [B, V, 3, H, W]: the
    normals of the depth map times ``alpha.detach()``, the ``surf_normal`` of 2DGS.  Differentiable in ``depth``."""
    if not all(isinstance(t, torch.Tensor) for t in (depth, alpha, cam_view)):
        raise TypeError("depth, alpha and cam_view must be torch.Tensors")
    if depth.dim() != 5 or cam_view.dim() != 4:
        raise ValueError(f"depth is [B, V, 1, H, W] and cam_view [B, V, 4, 4], not {tuple(depth.shape)} and {tuple(cam_view.shape)}")
    d, a, view = depth.flatten(0, 1), alpha.detach().flatten(0, 1), cam_view.flatten(0, 1)
    _validate_geo((("depth", d, 1), ("alpha", a, 1)), view, tanfov)
    return _surf_normal(d, a, view, tanfov).unflatten(0, tuple(depth.shape[:2]))


def geo_means(rend_normal: torch.Tensor, depth: torch.Tensor, alpha: torch.Tensor, dist: torch.Tensor, cam_view: torch.Tensor,
              tanfov: float, normal: torch.Tensor = None, mask: torch.Tensor = None) -> torch.Tensor:
    """-> [V, 3] fp32: per view the mean of ``1 - sum_c rend_normal_c * s_c``, the mean of ``dist`` and the mean of ``|alpha - mask|``
    (0 without a mask), from one pass.  ``s`` is the normal of the depth map times alpha (alpha a constant there), or, with ``normal``
    given, ``normal * mask`` (``mask`` optional; depth then gets no gradient).  Maps are [V, C, H, W], ``cam_view`` [V, 4, 4] as
    ``render`` takes it.  Carries the gradient with respect to ``rend_normal``, ``depth``, ``dist`` and ``alpha``."""
    maps = [("rend_normal", rend_normal, 3), ("depth", depth, 1), ("alpha", alpha, 1), ("dist", dist, 1)]
    if normal is not None:
        maps.append(("normal", normal, 3))
    if mask is not None:
        maps.append(("mask", mask, 1))
    _validate_geo(tuple(maps), cam_view, tanfov, constants=("normal", "mask"))
    return _GeoMeans.apply(rend_normal, depth, dist, alpha, float(tanfov), _f32(cam_view), _f32(rend_normal), _f32(depth), _f32(alpha),
                           _f32(dist), _f32(normal), _f32(mask))


def geometric_loss(pred: dict, cam_view: torch.Tensor, tanfov: float, lambda_normal: float = 0.0, lambda_dist: float = 0.0,
                   lambda_alpha: float = 0.0, normal: torch.Tensor = None, mask: torch.Tensor = None):
    """-> (loss, loss_dict) for the dict ``pred`` that ``GaussianRenderer2DGS.render`` returns ([B, V, C, H, W] maps ``rend_normal``,
    ``depth``, ``alpha``, ``dist``) and the ``cam_view`` [B, V, 4, 4] and ``tanfov`` it was rendered with:
    ``loss = lambda_normal * mean(1 - <rend_normal, s>) + lambda_dist * mean(dist) + lambda_alpha * mean|alpha - mask|`` with the keys
    ``loss``, ``loss_normal``, ``loss_dist`` (the reference's names and weighting) and ``loss_alpha``.  ``s`` is 2DGS's regulariser,
    ``surface_normal(...)``, or with ``normal`` [B, V, 3, H, W] given the trainer's ``normal * mask``; ``mask`` [B, V, 1, H, W] also
    switches the alpha term on.

    Departure from the reference, as in ``photometric_loss``: the three means come from the one pass and the keys are always present,
    where the reference adds a key only once its lambda is positive and its step threshold has passed."""
    if not isinstance(pred, dict) or any(k not in pred for k in ("rend_normal", "depth", "alpha", "dist")):
        raise TypeError("pred must be the dict render returns, with the keys rend_normal, depth, alpha and dist")
    rn = pred["rend_normal"]
    if not isinstance(rn, torch.Tensor) or rn.dim() != 5 or not isinstance(cam_view, torch.Tensor) or cam_view.dim() != 4:
        raise ValueError("pred['rend_normal'] is [B, V, 3, H, W] and cam_view [B, V, 4, 4]")

    def flat(t):
        if t is not None and (not isinstance(t, torch.Tensor) or t.dim() != 5):
            raise ValueError("every map is a [B, V, C, H, W] tensor")
        return None if t is None else t.flatten(0, 1)

    means = geo_means(flat(rn), flat(pred["depth"]), flat(pred["alpha"]), flat(pred["dist"]), cam_view.flatten(0, 1), tanfov,
                      flat(normal), flat(mask)).mean(0)   # equal-sized views: the mean of the per-view means is the mean over everything
    loss_normal, loss_dist, loss_alpha = lambda_normal * means[0], lambda_dist * means[1], lambda_alpha * means[2]
    loss = loss_normal + loss_dist + loss_alpha
    return loss, {"loss": loss, "loss_normal": loss_normal, "loss_dist": loss_dist, "loss_alpha": loss_alpha}
