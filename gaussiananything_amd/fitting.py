"""Fitting 2D surfels to posed views on the device -- the host side of include/ga_fit.h (HIP kernels, csrc/surfel_fit.hip).

    to_raw           the inverse of the activation: a Gaussian tensor [N,13] -> the raw parameters the optimiser moves
    step_table       the per-step Adam step sizes and bias corrections, computed in double, stored fp32
    SurfelFitter     one iteration = ga_fit_activate -> ga_surfel_forward -> post-processing -> the two loss forwards -> the two loss
                     backwards -> ga_fit_pack_grads -> ga_surfel_backward -> ga_fit_adam -> ga_fit_advance: one chain on one stream,
                     captured once and replayed as one HIP graph per iteration

Nothing in an iteration reads the device: the Adam step index is a device word (``ga_fit_advance`` moves it), the loss weights are device
tensors the loss backwards read as ``grad_out``, the loss terms go to a device history that ``loss_history()`` reads back in one copy, and
the workspace overflow report of the rasterizer is folded into words that outlive the iteration and are read every ``check_every``
iterations.  The parametrisation is the project's own, after 2DGS: xyz identity, opacity and rgb a sigmoid, scale
an exponential, rotation a normalised quaternion.  There is no CPU fallback: without the HIP library or on CPU tensors the fitter raises.

Two fits of the same input are NOT bit-identical: ``ga_surfel_backward`` sums with floating-point atomics.

Not built: densification, pruning, opacity reset, LPIPS, view mini-batching on the device (``set_views`` between ``step`` calls is the
way).  ``GaussianRenderer2DGS.render`` and the autograd path are untouched.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib
from .diff_surfel_rasterization import SurfelForwardPlan, SurfelWorkspace, default_capacity

GROUPS = ("xyz", "opacity", "scale", "rotation", "rgb")
COLUMNS = {"xyz": (0, 3), "opacity": (3, 4), "scale": (4, 6), "rotation": (6, 10), "rgb": (10, 13)}
DEFAULT_LR = dict(xyz=(1.6e-4, 1.6e-6), opacity=0.05, scale=0.005, rotation=0.001, rgb=0.0025)   # 2DGS's published settings
DEFAULT_MAX_STEPS = 30000
HISTORY = ("loss", "ssim", "l1", "l2", "normal", "dist", "alpha")


def to_raw(gaussians: torch.Tensor) -> torch.Tensor:
    """[N,13] or [1,N,13] activated Gaussians (xyz, opacity, scale(2), rotation wxyz, rgb) -> raw [N,13] fp32 on the same device:
    logit of opacity and rgb after a clamp to [1e-6, 1 - 1e-6], log of scale after a clamp at 1e-8, xyz and rotation as they are.  A
    zero quaternion has no direction and is refused."""
    if not isinstance(gaussians, torch.Tensor) or not gaussians.is_floating_point():
        raise TypeError("gaussians must be a floating-point torch.Tensor")
    g = gaussians.detach()
    if g.dim() == 3 and g.shape[0] == 1:
        g = g[0]
    if g.dim() != 2 or g.shape[1] != 13 or g.shape[0] < 1:
        raise ValueError(f"gaussians must be [N,13] or [1,N,13], not {tuple(gaussians.shape)}")
    g = g.float()
    if bool((g[:, 6:10] == 0).all(dim=1).any()):
        raise ValueError("gaussians hold a zero quaternion: it cannot be normalised")
    p = torch.cat([g[:, 3:4], g[:, 10:13]], dim=1).clamp(1e-6, 1 - 1e-6)
    logit = torch.log(p) - torch.log1p(-p)
    return torch.cat([g[:, 0:3], logit[:, 0:1], torch.log(g[:, 4:6].clamp_min(1e-8)), g[:, 6:10], logit[:, 1:4]], dim=1).contiguous()


def _lr_at(spec, t, max_steps):
    if isinstance(spec, (tuple, list)):
        a, b = float(spec[0]), float(spec[1])
        return a if max_steps == 1 else math.exp(math.log(a) + (math.log(b) - math.log(a)) * (t / (max_steps - 1)))
    return float(spec)


def step_table(lr: dict, betas=(0.9, 0.999), max_steps: int = DEFAULT_MAX_STEPS) -> torch.Tensor:
    """-> [max_steps, 8] fp32 (host): row t holds ``lr_g(t) / (1 - beta1^(t+1))`` for the five groups, ``sqrt(1 - beta2^(t+1))`` and two
    unused words, each computed in double and rounded once.  A learning rate given as a pair decays log-linearly from its first value at
    step 0 to its second at step ``max_steps - 1``.  The last row is where the device counter stays once it gets there."""
    lr = _check_lr(lr)
    b1, b2 = float(betas[0]), float(betas[1])
    t = np.arange(max_steps, dtype=np.float64)
    out = np.zeros((max_steps, _lib.GA_FIT_TABLE_COLS), np.float64)
    bc1 = 1.0 - np.power(b1, t + 1.0)
    for k, name in enumerate(GROUPS):
        out[:, k] = np.array([_lr_at(lr[name], int(s), max_steps) for s in range(max_steps)], np.float64) / bc1
    out[:, len(GROUPS)] = np.sqrt(1.0 - np.power(b2, t + 1.0))
    return torch.from_numpy(out.astype(np.float32))


def _check_lr(lr):
    if not isinstance(lr, dict) or set(lr) != set(GROUPS):
        raise ValueError(f"lr must be a dict with the keys {GROUPS}")
    for name, spec in lr.items():
        vals = tuple(spec) if isinstance(spec, (tuple, list)) else (spec,)
        if len(vals) not in (1, 2) or not all(isinstance(x, (int, float)) and math.isfinite(x) and x >= 0 for x in vals):
            raise ValueError(f"lr[{name!r}] must be a non-negative number or a (first, last) pair")
        if len(vals) == 2 and min(vals) <= 0:
            raise ValueError(f"lr[{name!r}]: both ends of a decaying pair must be positive")
    return lr


def _ptr(t):
    return None if t is None else t.data_ptr()


class SurfelFitter:
    """Adam on the raw parameters of N surfels against V posed target views; see the module docstring.

    ``step(n)`` runs n iterations, ``gaussians()`` returns the activated ``[1,N,13]`` tensor ``render`` takes, ``raw`` the raw
    parameters, ``raw_grad`` the raw-space gradient of the last iteration, ``loss_history()`` the weighted loss terms of every iteration
    so far (one read-back), ``set_views`` replaces cameras and targets without a new capture.

    The loss is ``l2 * MSE + l1 * L1 + ssim * (1 - SSIM) + lambda_normal * normal + lambda_dist * dist + lambda_alpha * |alpha - mask|``
    as ``losses.photometric_loss`` and ``losses.geometric_loss`` define the terms (``normal`` / ``mask`` as in ``geometric_loss``).
    """

    def __init__(self, gaussians, cam_view, cam_view_proj, tanfov, targets, *, mask=None, normal=None, bg=None,
                 l2=0.0, l1=0.8, ssim=0.2, lambda_normal=0.05, lambda_dist=0.0, lambda_alpha=0.0, lr=None,
                 betas=(0.9, 0.999), eps=1e-15, max_steps=DEFAULT_MAX_STEPS, visible_only=False, check_every=50, capacity=None):
        # ---- everything the host can see is checked before anything is enqueued --------------------------------------------------
        lr = _check_lr(dict(DEFAULT_LR) if lr is None else lr)
        tensors = [("gaussians", gaussians), ("cam_view", cam_view), ("cam_view_proj", cam_view_proj), ("targets", targets)]
        tensors += [(k, t) for k, t in (("mask", mask), ("normal", normal), ("bg", bg)) if t is not None]
        for name, t in tensors:
            if not isinstance(t, torch.Tensor) or not t.is_floating_point():
                raise TypeError(f"{name} must be a floating-point torch.Tensor")
            if t.device.type != "cuda":
                raise ValueError(f"{name} is on {t.device}: the fitter only runs on an MI355X (HIP) device; there is no CPU path")
            if t.device != gaussians.device:
                raise ValueError(f"{name} is on {t.device}, expected {gaussians.device}")
        if isinstance(tanfov, torch.Tensor) or not (0.0 < float(tanfov) < float("inf")):
            raise ValueError("tanfov must be a positive finite number")
        g = gaussians[0] if gaussians.dim() == 3 and gaussians.shape[0] == 1 else gaussians
        if g.dim() != 2 or g.shape[1] != 13 or g.shape[0] < 1:
            raise ValueError(f"gaussians must be [N,13] or [1,N,13], not {tuple(gaussians.shape)}")
        if targets.dim() != 4 or targets.shape[1] != 3 or targets.numel() == 0:
            raise ValueError(f"targets must be [V,3,H,W], not {tuple(targets.shape)}")
        self.N, (self.V, _, self.H, self.W) = int(g.shape[0]), (int(x) for x in targets.shape)
        self._check_views(cam_view, cam_view_proj, targets, mask, normal)
        if bg is not None and bg.numel() != 3:
            raise ValueError("bg must hold three values")
        max_steps, check_every = int(max_steps), int(check_every)
        if max_steps < 1 or check_every < 1:
            raise ValueError("max_steps and check_every must be at least 1")
        if not (0.0 <= float(betas[0]) < 1.0 and 0.0 <= float(betas[1]) < 1.0 and float(eps) >= 0.0):
            raise ValueError("betas must lie in [0, 1) and eps must not be negative")
        if capacity is not None and int(capacity) < 1:
            raise ValueError("capacity must be positive")
        self._L = _lib.lib()
        raw = to_raw(g)                                   # (raises on a zero quaternion; still nothing enqueued by this class)

        dev = self.device = gaussians.device
        N, V, H, W = self.N, self.V, self.H, self.W
        self.tanfov, self.max_steps, self.check_every = float(tanfov), max_steps, check_every
        self.betas, self.eps, self.visible_only = (float(betas[0]), float(betas[1])), float(eps), bool(visible_only)
        self.weights = dict(l2=float(l2), l1=float(l1), ssim=float(ssim), lambda_normal=float(lambda_normal),
                            lambda_dist=float(lambda_dist), lambda_alpha=float(lambda_alpha))
        self.plan = _lib.GaFitPlan()
        _lib.check(self._L.ga_fit_plan(N, V, H, W, ctypes.byref(self.plan)), "ga_fit_plan")

        def f32(*shape):
            return torch.zeros(shape, dtype=torch.float32, device=dev)

        with torch.cuda.device(dev):
            # state
            self._raw, self._m, self._v, self._raw_grad = raw, f32(N, 13), f32(N, 13), f32(N, 13)
            self._counter = torch.zeros(1, dtype=torch.int32, device=dev)
            self._seen = torch.zeros(4, dtype=torch.int64, device=dev)
            self._history = f32(max_steps, _lib.GA_FIT_HISTORY_COLS)
            self._table = step_table(lr, self.betas, max_steps).to(dev)
            self._snap = [torch.empty_like(self._raw), torch.empty_like(self._m), torch.empty_like(self._v), torch.empty_like(self._counter)]
            # static inputs
            self._view, self._proj = f32(V, 16), f32(V, 16)
            self._targets = f32(V, 3, H, W)
            self._mask = f32(V, 1, H, W) if mask is not None else None
            self._normal = f32(V, 3, H, W) if normal is not None else None
            self._bg = torch.ones(3, dtype=torch.float32, device=dev) if bg is None else bg.detach().float().reshape(3).clone()
            self._copy_views(cam_view, cam_view_proj, targets, mask, normal)
            # the activated arrays, one buffer laid out by the plan
            pl = self.plan
            self._act_buffer = torch.zeros(pl.workspace_bytes + 256, dtype=torch.uint8, device=dev)
            base = (-self._act_buffer.data_ptr()) % 256

            def section(off, *shape):
                n = int(np.prod(shape)) * 4
                return self._act_buffer[base + off:base + off + n].view(torch.float32).view(*shape)

            self._means, self._opac, self._colors = section(pl.means, N, 3), section(pl.opacities, N), section(pl.colors, N, 3)
            self._scales, self._rots, self._inv_norm = section(pl.scales, N, 2), section(pl.rotations, N, 4), section(pl.inv_norm, N)
            # rasterizer outputs, the maps of render's differentiable branch and their gradients
            self._color, self._allmap = f32(V, 3, H, W), f32(V, 7, H, W)
            self._radii = torch.zeros(V, N, dtype=torch.int32, device=dev)
            self._image, self._rend_normal, self._depth = f32(V, 3, H, W), f32(V, 3, H, W), f32(V, 1, H, W)
            self._alpha, self._dist = f32(V, 1, H, W), f32(V, 1, H, W)
            self._g_image, self._g_rend_normal = f32(V, 3, H, W), f32(V, 3, H, W)
            self._g_depth, self._g_dist, self._g_alpha = f32(V, 1, H, W), f32(V, 1, H, W), f32(V, 1, H, W)
            self._g_color, self._g_allmap = f32(V, 3, H, W), f32(V, 7, H, W)
            self._g_means, self._g_opac, self._g_colors = f32(N, 3), f32(N), f32(N, 3)
            self._g_scales, self._g_rots = f32(N, 2), f32(N, 4)
            # loss means and their weights: divided by V (the mean over the views), SSIM with a minus sign (the term is 1 - SSIM)
            w = self.weights
            self._photo_out, self._geo_out = f32(V, 3), f32(V, 3)
            self._w_photo = torch.tensor([[-w["ssim"] / V, w["l1"] / V, w["l2"] / V]] * V, dtype=torch.float64).float().to(dev)
            self._w_geo = torch.tensor([[w["lambda_normal"] / V, w["lambda_dist"] / V, w["lambda_alpha"] / V]] * V,
                                       dtype=torch.float64).float().to(dev)
            nbytes = int(self._L.ga_photo_loss_workspace_bytes(V, 3, H, W, _lib.GA_PHOTO_LOSS_SAVE))
            gbytes = int(self._L.ga_geo_loss_workspace_bytes(V, H, W))
            if nbytes == 0 or gbytes == 0:
                raise ValueError(f"views of {H} x {W} are out of the loss kernels' range")
            self._photo_ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
            self._geo_ws = torch.zeros(gbytes, dtype=torch.uint8, device=dev)
            ws = SurfelWorkspace(dev, N, V, H, W, int(capacity) if capacity is not None else default_capacity(N, V))
            self._fwd = SurfelForwardPlan._bound((self._means, self._opac, self._colors, self._scales, self._rots, self._view, self._proj,
                                                  self._bg), H, W, 1.0, ws, for_backward=True,
                                                 outputs=(self._color, self._allmap, self._radii))
            self._steps = self._snap_steps = 0
            self._graph = None
            self._side = torch.cuda.Stream(dev)
            self._bind()
            self._warm_up_and_capture()

    # ---- validation and static inputs ------------------------------------------------------------------------------------------
    def _check_views(self, cam_view, cam_view_proj, targets, mask, normal):
        V, H, W = self.V, self.H, self.W
        for name, t, shape in (("cam_view", cam_view, (V, 4, 4)), ("cam_view_proj", cam_view_proj, (V, 4, 4)),
                               ("targets", targets, (V, 3, H, W)), ("mask", mask, (V, 1, H, W)), ("normal", normal, (V, 3, H, W))):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or not t.is_floating_point():
                raise TypeError(f"{name} must be a floating-point torch.Tensor")
            if t.device.type != "cuda":
                raise ValueError(f"{name} is on {t.device}: the fitter only runs on an MI355X (HIP) device; there is no CPU path")
            if tuple(t.shape) != shape:
                raise ValueError(f"{name} must be {list(shape)}, not {list(t.shape)}")
            if name not in ("cam_view", "cam_view_proj") and t.requires_grad:
                raise ValueError(f"{name} requires grad: it is a constant of the fit")

    def _copy_views(self, cam_view, cam_view_proj, targets, mask, normal):
        self._view.copy_(cam_view.detach().reshape(self.V, 16))
        self._proj.copy_(cam_view_proj.detach().reshape(self.V, 16))
        self._targets.copy_(targets.detach())
        if mask is not None:
            self._mask.copy_(mask.detach())
        if normal is not None:
            self._normal.copy_(normal.detach())

    def set_views(self, cam_view, cam_view_proj, targets, mask=None, normal=None):
        """Replace cameras and targets (same V, H, W): copies into the buffers the captured graph reads, no new capture.  ``mask`` /
        ``normal`` can be replaced only where the fitter was constructed with one."""
        self._check_views(cam_view, cam_view_proj, targets, mask, normal)
        if (mask is not None and self._mask is None) or (normal is not None and self._normal is None):
            raise ValueError("the fitter was constructed without a mask / normal target: the captured graph does not read one")
        self._copy_views(cam_view, cam_view_proj, targets, mask, normal)

    # ---- the launches ------------------------------------------------------------------------------------------------------------
    def _bind(self):
        """(re)build every argument block but the forward's (``self._fwd`` holds it): after construction and after the workspace has
        grown"""
        N, V, H, W, ws = self.N, self.V, self.H, self.W, self._fwd.ws
        self._a_act = _lib.GaFitActivateArgs(N, 0, self._raw.data_ptr(), self._means.data_ptr(), self._opac.data_ptr(),
                                             self._colors.data_ptr(), self._scales.data_ptr(), self._rots.data_ptr(),
                                             self._inv_norm.data_ptr())
        self._a_post = _lib.GaSurfelPostArgs(V, H, W, self._color.data_ptr(), self._allmap.data_ptr(), self._view.data_ptr(),
                                             self._image.data_ptr(), self._rend_normal.data_ptr(), self._depth.data_ptr())
        self._a_photo = _lib.GaPhotoLossArgs(V, 3, H, W, _lib.GA_PHOTO_LOSS_SAVE, 0, self._image.data_ptr(), self._targets.data_ptr(),
                                             self._photo_out.data_ptr(), None, self._w_photo.data_ptr(), self._g_image.data_ptr(),
                                             self._photo_ws.data_ptr(), self._photo_ws.numel())
        a = self._a_geo = _lib.GaGeoLossArgs()
        a.num_views, a.height, a.width, a.tanfov = V, H, W, self.tanfov
        a.flags = _lib.GA_GEO_LOSS_TARGET if self._normal is not None else 0
        a.view, a.rend_normal, a.depth = self._view.data_ptr(), self._rend_normal.data_ptr(), self._depth.data_ptr()
        a.alpha, a.dist = self._alpha.data_ptr(), self._dist.data_ptr()
        a.target_normal, a.mask = _ptr(self._normal), _ptr(self._mask)
        a.out, a.grad_out = self._geo_out.data_ptr(), self._w_geo.data_ptr()
        a.grad_rend_normal, a.grad_depth = self._g_rend_normal.data_ptr(), self._g_depth.data_ptr()
        a.grad_dist, a.grad_alpha = self._g_dist.data_ptr(), self._g_alpha.data_ptr()
        a.workspace, a.workspace_bytes = self._geo_ws.data_ptr(), self._geo_ws.numel()
        self._a_pack = _lib.GaFitPackArgs(V, H, W, 0, self._color.data_ptr(), self._allmap.data_ptr(), self._view.data_ptr(),
                                          self._g_image.data_ptr(), self._g_rend_normal.data_ptr(), self._g_depth.data_ptr(),
                                          self._g_dist.data_ptr(), self._g_alpha.data_ptr(), self._g_color.data_ptr(),
                                          self._g_allmap.data_ptr())
        fwd = self._fwd.backward_args()
        nbytes = int(self._L.ga_surfel_backward_scratch_bytes(ctypes.byref(fwd)))
        if nbytes == 0:
            raise RuntimeError("ga_surfel_backward_scratch_bytes: bad shape")
        if getattr(self, "_scratch", None) is None or self._scratch.numel() < nbytes:
            self._scratch = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        self._a_bwd = _lib.GaSurfelBackwardArgs(fwd, self._g_color.data_ptr(), self._g_allmap.data_ptr(), self._scratch.data_ptr(),
                                                self._scratch.numel(), self._g_means.data_ptr(), self._g_opac.data_ptr(),
                                                self._g_colors.data_ptr(), self._g_scales.data_ptr(), self._g_rots.data_ptr())
        b1, b2 = self.betas
        self._a_adam = _lib.GaFitAdamArgs(
            N, V, _lib.GA_FIT_VISIBLE_ONLY if self.visible_only else 0, self.max_steps, self._g_means.data_ptr(),
            self._g_opac.data_ptr(), self._g_colors.data_ptr(), self._g_scales.data_ptr(), self._g_rots.data_ptr(),
            self._opac.data_ptr(), self._colors.data_ptr(), self._scales.data_ptr(), self._rots.data_ptr(), self._inv_norm.data_ptr(),
            self._raw.data_ptr(), self._m.data_ptr(), self._v.data_ptr(), self._radii.data_ptr(), self._table.data_ptr(),
            self._counter.data_ptr(), b1, 1.0 - b1, b2, 1.0 - b2, self.eps, 0, self._raw_grad.data_ptr())
        self._a_adv = _lib.GaFitAdvanceArgs(V, self.max_steps, self._counter.data_ptr(), self._photo_out.data_ptr(),
                                            self._geo_out.data_ptr(), self._w_photo.data_ptr(), self._w_geo.data_ptr(),
                                            self._history.data_ptr(), self.weights["ssim"], 0, ws.status().data_ptr(),
                                            self._seen.data_ptr())

    def _enqueue(self):
        """one iteration on the current stream: a single chain, nothing synchronises"""
        L, ref = self._L, ctypes.byref
        s = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(L.ga_fit_activate(ref(self._a_act), s), "ga_fit_activate")
        self._fwd.run()
        _lib.check(L.ga_surfel_postprocess(ref(self._a_post), s), "ga_surfel_postprocess")
        self._alpha.copy_(self._allmap[:, 1:2])      # the loss kernels read contiguous [V,1,H,W] maps: two strided copies
        self._dist.copy_(self._allmap[:, 6:7])
        _lib.check(L.ga_photo_loss_forward(ref(self._a_photo), s), "ga_photo_loss_forward")
        _lib.check(L.ga_geo_loss_forward(ref(self._a_geo), s), "ga_geo_loss_forward")
        _lib.check(L.ga_photo_loss_backward(ref(self._a_photo), s), "ga_photo_loss_backward")
        _lib.check(L.ga_geo_loss_backward(ref(self._a_geo), s), "ga_geo_loss_backward")
        _lib.check(L.ga_fit_pack_grads(ref(self._a_pack), s), "ga_fit_pack_grads")
        _lib.check(L.ga_surfel_backward(ref(self._a_bwd), s), "ga_surfel_backward")
        _lib.check(L.ga_fit_adam(ref(self._a_adam), s), "ga_fit_adam")
        _lib.check(L.ga_fit_advance(ref(self._a_adv), s), "ga_fit_advance")

    def _save(self):
        for dst, src in zip(self._snap, (self._raw, self._m, self._v, self._counter)):
            dst.copy_(src)
        self._snap_steps = self._steps

    def _restore(self):
        for src, dst in zip(self._snap, (self._raw, self._m, self._v, self._counter)):
            dst.copy_(src)
        self._seen.zero_()
        self._steps = self._snap_steps

    def _warm_up_and_capture(self):
        """One eager iteration on the side stream (it sizes the workspace: grown until the forward fits), the state put back as it
        was, then the capture of one iteration.  Also the path after an overflow: the state is then the snapshot's."""
        dev = self.device
        with torch.cuda.device(dev):
            main = torch.cuda.current_stream(dev)
            self._side.wait_stream(main)
            with torch.cuda.stream(self._side):
                self._save()
                row = self._history[self._steps].clone()
                while True:
                    self._enqueue()
                    seen = self._seen.cpu()
                    self._restore()
                    if int(seen[0]) == 0:
                        break
                    self._grow(seen)
                self._history[self._steps].copy_(row)
                self._side.synchronize()
                self._graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self._graph, stream=self._side):
                    self._enqueue()
            main.wait_stream(self._side)

    def _grow(self, seen):
        self._graph = None
        self._fwd.rebind(self._fwd.ws.grown(need=int(seen[1]), seg_need=int(seen[2])))
        self._bind()

    # ---- the public surface ------------------------------------------------------------------------------------------------------
    def step(self, n: int = 1):
        """Run n iterations: n replays of the captured graph.  Every ``check_every`` iterations and at the end the overflow words are
        read (the one synchronisation) and a device snapshot of raw, m, v and the step counter is taken; if a forward in between did
        not fit its workspace, the snapshot is restored, the workspace grown, the iteration captured again and the iterations since
        the snapshot are run again."""
        n = int(n)
        if n < 0:
            raise ValueError("n must not be negative")
        if self._steps + n > self.max_steps:
            raise ValueError(f"{self._steps} + {n} steps exceed max_steps = {self.max_steps}: the step table has no more rows")
        target = self._steps + n
        with torch.cuda.device(self.device):
            while self._steps < target:
                k = min(self.check_every - (self._steps - self._snap_steps), target - self._steps)
                for _ in range(k):
                    self._graph.replay()
                self._steps += k
                seen = self._seen.cpu()
                if int(seen[0]) == 0:
                    self._save()
                else:
                    self._restore()
                    self._grow(seen)
                    self._warm_up_and_capture()
        return self

    @property
    def steps(self) -> int:
        return self._steps

    @property
    def raw(self) -> torch.Tensor:
        """the raw parameters [N,13] (the fitter's own buffer: clone it to keep a value)"""
        return self._raw

    @property
    def raw_grad(self) -> torch.Tensor:
        """the raw-space gradient [N,13] of the last iteration (the fitter's own buffer)"""
        return self._raw_grad

    @property
    def capacity(self) -> int:
        """binned (tile, surfel) entries the rasterizer workspace holds at present"""
        return self._fwd.ws.capacity

    def entries(self) -> int:
        """binned (tile, surfel) entries of the last forward (one read-back)"""
        return int(self._fwd.ws.status()[_lib.GA_STATUS_NUM_RENDERED].cpu())

    def state_dict(self) -> dict:
        """copies of raw, m, v and the loss history, and the number of steps taken: what ``load_state_dict`` of a fitter of the same N
        and ``max_steps`` continues from (views, weights and learning rates are the constructor's)"""
        return {"raw": self._raw.clone(), "m": self._m.clone(), "v": self._v.clone(), "steps": self._steps,
                "history": self._history[:self._steps].clone()}

    def load_state_dict(self, state: dict):
        steps = int(state["steps"])
        if not 0 <= steps <= self.max_steps:
            raise ValueError(f"the state has taken {steps} steps, this fitter's table has {self.max_steps} rows")
        for k in ("raw", "m", "v"):
            if tuple(state[k].shape) != (self.N, 13):
                raise ValueError(f"state[{k!r}] must be [{self.N}, 13], not {list(state[k].shape)}")
        if tuple(state["history"].shape) != (steps, _lib.GA_FIT_HISTORY_COLS):
            raise ValueError("state['history'] must hold one row per step taken")
        with torch.cuda.device(self.device):
            for dst, k in ((self._raw, "raw"), (self._m, "m"), (self._v, "v")):
                dst.copy_(state[k])
            self._history[:steps].copy_(state["history"])
            self._counter.fill_(min(steps, self.max_steps - 1))
            self._steps = steps
            self._save()
        return self

    def gaussians(self) -> torch.Tensor:
        """the activated Gaussians [1,N,13] of the present raw parameters, as ``render`` takes them"""
        with torch.cuda.device(self.device):
            s = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            _lib.check(self._L.ga_fit_activate(ctypes.byref(self._a_act), s), "ga_fit_activate")
            return torch.cat([self._means, self._opac[:, None], self._scales, self._rots, self._colors], dim=1).unsqueeze(0)

    def loss_history(self) -> dict:
        """-> dict of float32 arrays of length ``steps``: ``loss`` and its weighted terms ``ssim`` (= ssim * (1 - SSIM)), ``l1``, ``l2``,
        ``normal``, ``dist``, ``alpha``, each evaluated BEFORE that iteration's update.  One copy from the device."""
        h = self._history[:self._steps].cpu().numpy()
        return {name: h[:, k].copy() for k, name in enumerate(HISTORY)}
