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

Not built: LPIPS, the identity loss, the ``fg_mse`` masked branch, the depth-to-normal regulariser.  ``PSNR`` restates
``kornia.metrics.psnr(x / 2 + 0.5, y / 2 + 0.5, 1.0)`` = ``10 log10(4 / MSE)``; kornia is absent, so that value is UNPINNED."""
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
