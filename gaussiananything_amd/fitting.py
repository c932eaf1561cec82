"""Fitting 2D surfels to posed views on the device -- the host side of include/ga_fit.h and include/ga_densify.h (HIP kernels,
csrc/surfel_fit.hip and csrc/surfel_densify.hip).

    to_raw           the inverse of the activation: a Gaussian tensor [N,13] -> the raw parameters the optimiser moves
    surfels_from_points   a point cloud -> the Gaussian tensor [N,13] a fit can start from (``SurfelFitter.from_points`` wraps it)
    step_table       the per-step Adam step sizes and bias corrections, computed in double, stored fp32
    view_schedule    the table of view mini-batches: which views of a pool every iteration renders (epochs of random permutations)
    SurfelFitter     one iteration = ga_fit_activate -> ga_surfel_forward -> post-processing -> the two loss forwards -> the two loss
                     backwards -> ga_fit_pack_grads -> ga_surfel_backward -> ga_fit_adam -> ga_fit_advance: one chain on one stream,
                     captured once and replayed as one HIP graph per iteration; with ``densify=`` the number of surfels changes
                     between stretches of iterations (clone / split / prune rounds and opacity resets); with
                     ``batch_views=B`` the views given are a pool of P kept on the device and ``ga_fit_select_views`` heads the
                     chain: it copies the B views row ``*counter`` of the schedule names into the buffers the chain reads
                     
    densify_and_prune  one clone / split / prune round on raw, m, v and the three densification statistics
    reset_opacity      the opacity reset: raw opacity capped at logit(cap), its Adam moments zeroed

Nothing in an iteration reads the device: the Adam step index is a device word (``ga_fit_advance`` moves it), the loss weights are device
tensors the loss backwards read as ``grad_out``, the loss terms go to a device history that ``loss_history()`` reads back in one copy, and
the workspace overflow report of the rasterizer is folded into words that outlive the iteration and are read every ``check_every``
iterations.  The parametrisation is the project's own, after 2DGS: xyz identity, opacity and rgb a sigmoid, scale
an exponential, rotation a normalised quaternion.  There is no CPU fallback: without the HIP library or on CPU tensors the fitter raises.

Two fits of the same input are NOT bit-identical: ``ga_surfel_backward`` sums with floating-point atomics.

Not built: LPIPS, a view pool in host memory, per-view image sizes.  ``GaussianRenderer2DGS.render`` and the autograd path are
untouched.  The view schedule, like the parametrisation, is the project's own definition: no reference trainer runs here to pin it.
"""
from __future__ import annotations

import ctypes
import dataclasses
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


def surfels_from_points(points, colors=None, normals=None, K=16, opacity=0.1, scale_factor=1.0) -> torch.Tensor:
    """A point cloud [N,3] or [1,N,3] (SfM points, a scan, a stage-1 cloud) -> activated surfels [N,13] fp32 on its device, what
    ``SurfelFitter`` and ``to_raw`` take: the disc of every point lies in the plane PCA fits to its ``K`` nearest points (or is
    perpendicular to ``normals`` [N,3] when given), its two scales are ``scale_factor`` times the root mean squared distance to the
    three nearest other points (2DGS's ``create_from_pcd`` rule; 2DGS draws the rotations at random), its opacity ``opacity``, its
    colour ``colors`` [N,3] in [0, 1] or 0.5.  ``pointcloud.surfels_from_cloud`` on a batch of one: the kNN launch and two
    per-point launches, no host read.  A point whose neighbours all coincide with it gets opacity 0 (``pointcloud.estimate_normals``).
    Posed RGB-D views become such a cloud through ``pointcloud.unproject_depth_views`` (``SurfelFitter.from_rgbd``).
    Not built: anisotropic initial scales, SH colours, orientation propagation."""
    from . import pointcloud

    def batched(t, name):
        if t is None:
            return None
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise TypeError(f"{name} must be a floating-point torch.Tensor")
        if t.dim() == 2:
            t = t[None]
        if t.dim() != 3 or t.shape[0] != 1 or t.shape[2] != 3 or t.shape[1] < 1:
            raise ValueError(f"{name} must be [N,3] or [1,N,3], not {tuple(t.shape)}")
        return t

    p, c, n = batched(points, "points"), batched(colors, "colors"), batched(normals, "normals")
    return pointcloud.surfels_from_cloud(p, None, c, n, K, opacity, scale_factor)[0]


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


def view_schedule(max_steps: int, pool_views: int, batch_views: int, seed: int = 0) -> torch.Tensor:
    """-> int32 [max_steps, B] (host): row t names the B views of a pool of P that iteration t renders.  The definition, in numpy::

        rng = np.random.default_rng(seed)
        n = -(-P // B)                                     # rows per epoch: ceil(P / B)
        rows = []
        while len(rows) < max_steps:
            perm = rng.permutation(P)                      # one epoch
            rows.extend(np.concatenate([perm, perm[:n * B - P]]).reshape(n, B))
        table = np.stack(rows[:max_steps]).astype(np.int32)

    An epoch is one permutation of the pool cut into consecutive rows; a short last row is completed from the start of the same
    permutation, so no row holds a view twice and every epoch covers every view.  ``B > P`` is refused."""
    for name, x in (("max_steps", max_steps), ("pool_views", pool_views), ("batch_views", batch_views)):
        if not _is_int(x) or x < 1:
            raise ValueError(f"{name} must be a positive integer")
    if batch_views > pool_views:
        raise ValueError(f"batch_views = {batch_views} exceeds the pool of {pool_views} views")
    if not _is_int(seed) or seed < 0:
        raise ValueError("seed must be a non-negative integer")
    P, B = int(pool_views), int(batch_views)
    rng = np.random.default_rng(int(seed))
    n = -(-P // B)
    rows = []
    while len(rows) < max_steps:
        perm = rng.permutation(P)
        rows.extend(np.concatenate([perm, perm[:n * B - P]]).reshape(n, B))
    return torch.from_numpy(np.stack(rows[:max_steps]).astype(np.int32))


def _check_schedule(schedule, max_steps, pool_views, batch_views):
    """a schedule of the caller's -> a contiguous int32 host tensor [max_steps, B] with every value in [0, P): the kernel clamps what
    it reads, which keeps it inside the pool but would hide a wrong table"""
    if not isinstance(schedule, torch.Tensor) or schedule.is_floating_point() or schedule.is_complex() or schedule.dtype == torch.bool:
        raise TypeError("view_schedule must be an integer torch.Tensor")
    if tuple(schedule.shape) != (max_steps, batch_views):
        raise ValueError(f"view_schedule must be [max_steps, batch_views] = [{max_steps}, {batch_views}], not {list(schedule.shape)}")
    host = schedule.detach().cpu()
    if int(host.min()) < 0 or int(host.max()) >= pool_views:
        raise ValueError(f"view_schedule holds a value outside [0, {pool_views}): the pool has {pool_views} views")
    return host.to(torch.int32).contiguous()


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


# ---- adaptive density control (include/ga_densify.h) ---------------------------------------------------------------------------------
def _is_int(x):
    return isinstance(x, (int, np.integer)) and not isinstance(x, bool)


def _is_num(x):
    return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool)


def _check_densify_scalars(grad_threshold, min_opacity, percent_dense, extent, max_screen_size, seed, max_points):
    if not _is_num(grad_threshold) or math.isnan(grad_threshold) or grad_threshold < 0:
        raise ValueError("grad_threshold must be a non-negative number (inf: nothing is cloned or split)")
    if not _is_num(min_opacity) or not 0.0 <= min_opacity <= 1.0:
        raise ValueError("min_opacity must lie in [0, 1]")
    if not _is_num(percent_dense) or not (0.0 <= percent_dense < math.inf):
        raise ValueError("percent_dense must be a non-negative finite number")
    if not _is_num(extent) or not (0.0 < extent < math.inf):
        raise ValueError("extent (the scene radius) must be a positive finite number")
    if not _is_num(max_screen_size) or not (0.0 <= max_screen_size < math.inf):
        raise ValueError("max_screen_size must be a non-negative finite number (0: no pruning by size)")
    if not _is_int(seed) or not 0 <= seed < 1 << 64:
        raise ValueError("seed must be an integer in [0, 2^64)")
    if max_points is not None and (not _is_int(max_points) or max_points < 1):
        raise ValueError("max_points must be None or a positive integer")


@dataclasses.dataclass(frozen=True)
class DensifyConfig:
    """When and how ``SurfelFitter`` changes the number of surfels; the defaults are 2DGS's published settings.  ``t`` is the number
    of iterations taken.  A clone / split / prune round runs after iteration t when ``start <= t <= stop`` and ``t % every == 0``; its
    pruning by size (``max_screen_size``, in pixels of radius, and 0.1 * extent in world units) applies when ``t > screen_size_from``;
    the opacities are reset after iteration t when ``t <= stop`` and ``t % opacity_reset_every == 0`` (0: never), after the round of
    the same iteration.  ``extent`` is the scene radius.  A round that would leave more than ``max_points`` surfels only prunes."""
    extent: float
    start: int = 500
    stop: int = 15000
    every: int = 100
    grad_threshold: float = 2e-4
    min_opacity: float = 0.05
    percent_dense: float = 0.01
    max_screen_size: float = 20
    screen_size_from: int = 3000
    opacity_reset_every: int = 3000
    max_points: int | None = None
    seed: int = 0

    def __post_init__(self):
        _check_densify_scalars(self.grad_threshold, self.min_opacity, self.percent_dense, self.extent, self.max_screen_size, self.seed,
                               self.max_points)
        for name in ("start", "stop", "every", "screen_size_from", "opacity_reset_every"):
            if not _is_int(getattr(self, name)) or getattr(self, name) < 0:
                raise ValueError(f"{name} must be a non-negative integer")
        if self.every < 1:
            raise ValueError("every must be at least 1")
        if self.stop < self.start:
            raise ValueError("stop must not be smaller than start")


def _as_config(densify):
    if densify is None or isinstance(densify, DensifyConfig):
        return densify
    if isinstance(densify, dict):
        known = {f.name for f in dataclasses.fields(DensifyConfig)}
        if set(densify) - known:
            raise ValueError(f"densify: unknown fields {sorted(set(densify) - known)}")
        if "extent" not in densify:
            raise ValueError("densify: extent (the scene radius) is required")
        return DensifyConfig(**densify)
    raise TypeError("densify must be None, a DensifyConfig or a dict of its fields")


def _check_points(raw, m, v):
    for name, t in (("raw", raw), ("m", m), ("v", v)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"{name} must be a float32 torch.Tensor")
    for name, t in (("raw", raw), ("m", m), ("v", v)):
        if t.device.type != "cuda":
            raise ValueError(f"{name} is on {t.device}: density control only runs on an MI355X (HIP) device; there is no CPU path")
        if t.device != raw.device or t.dim() != 2 or t.shape[1] != 13 or t.shape[0] < 1 or t.shape != raw.shape:
            raise ValueError(f"{name} must be [N,13] on {raw.device}, not {list(t.shape)} on {t.device}")
    if raw.shape[0] > 1 << 30:
        raise ValueError("more than 2^30 surfels")
    return int(raw.shape[0])


def _activated(L, raw, stream):
    """ga_fit_activate into buffers of its own -> (opacities, scales, rotations)"""
    N, dev = raw.shape[0], raw.device
    means, opac, colors = (torch.empty(shape, dtype=torch.float32, device=dev) for shape in ((N, 3), (N,), (N, 3)))
    scales, rots, inv_norm = (torch.empty(shape, dtype=torch.float32, device=dev) for shape in ((N, 2), (N, 4), (N,)))
    args = _lib.GaFitActivateArgs(N, 0, raw.data_ptr(), means.data_ptr(), opac.data_ptr(), colors.data_ptr(), scales.data_ptr(),
                                  rots.data_ptr(), inv_norm.data_ptr())
    _lib.check(L.ga_fit_activate(ctypes.byref(args), stream), "ga_fit_activate")
    return opac, scales, rots


def densify_and_prune(raw, m, v, grad_accum, denom, max_radius, *, grad_threshold, min_opacity, percent_dense, extent,
                      max_screen_size=0, seed=0, round=0, max_points=None, return_noise=False):
    """One clone / split / prune round (include/ga_densify.h: ga_densify) on the raw parameters [N,13], their Adam moments and the
    three statistics ``ga_fit_accumulate`` keeps (float32 [N], int32 [N], int32 [N]) -> ``raw, m, v, parent, counts``: views of the
    first N' rows of buffers of 2 N rows, ``parent`` [N'] int32 the source row of every output row, ``counts`` a dict of ``N_before``,
    ``N_after``, ``kept``, ``cloned``, ``split``, ``pruned``, ``prune_only`` (and ``noise`` [N,4] with ``return_noise``).  A round that
    would leave more than ``max_points`` rows is run again as a prune-only round.  One synchronisation: the read of the counts.  N' may
    be 0: the tensors are then empty.  The inputs are left as they are."""
    _check_densify_scalars(grad_threshold, min_opacity, percent_dense, extent, max_screen_size, seed, max_points)
    if not _is_int(round) or not 0 <= round < 1 << 32:
        raise ValueError("round must be an integer in [0, 2^32)")
    N = _check_points(raw, m, v)
    for name, t, dtype in (("grad_accum", grad_accum, torch.float32), ("denom", denom, torch.int32), ("max_radius", max_radius, torch.int32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype:
            raise TypeError(f"{name} must be a torch.Tensor of {dtype}")
        if t.device != raw.device or tuple(t.shape) != (N,):
            raise ValueError(f"{name} must be [{N}] on {raw.device}, not {list(t.shape)} on {t.device}")
    L, dev = _lib.lib(), raw.device
    raw, m, v, grad_accum, denom, max_radius = (t.detach().contiguous() for t in (raw, m, v, grad_accum, denom, max_radius))
    with torch.cuda.device(dev):
        s = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        opac, scales, rots = _activated(L, raw, s)
        out_raw, out_m, out_v = (torch.empty(2 * N, 13, dtype=torch.float32, device=dev) for _ in range(3))
        parent = torch.empty(2 * N, dtype=torch.int32, device=dev)
        noise = torch.empty(N, 4, dtype=torch.float32, device=dev) if return_noise else None
        out_counts = torch.zeros(_lib.GA_DENSIFY_COUNTS, dtype=torch.int64, device=dev)
        ws = torch.empty(int(L.ga_densify_workspace_bytes(N)), dtype=torch.uint8, device=dev)
        a = _lib.GaDensifyArgs()
        a.num_points, a.flags, a.round, a.seed = N, 0, int(round), int(seed)
        a.grad_threshold, a.min_opacity, a.percent_dense = float(grad_threshold), float(min_opacity), float(percent_dense)
        a.extent, a.max_screen_size = float(extent), float(max_screen_size)
        a.raw, a.m, a.v = raw.data_ptr(), m.data_ptr(), v.data_ptr()
        a.opacities, a.scales, a.rotations = opac.data_ptr(), scales.data_ptr(), rots.data_ptr()
        a.grad_accum, a.denom, a.max_radius = grad_accum.data_ptr(), denom.data_ptr(), max_radius.data_ptr()
        a.out_raw, a.out_m, a.out_v, a.parent = out_raw.data_ptr(), out_m.data_ptr(), out_v.data_ptr(), parent.data_ptr()
        a.noise_out, a.out_counts = _ptr(noise), out_counts.data_ptr()
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        _lib.check(L.ga_densify(ctypes.byref(a), s), "ga_densify")
        c = out_counts.cpu().tolist()
        if max_points is not None and c[0] > max_points:
            a.flags = _lib.GA_DENSIFY_PRUNE_ONLY
            _lib.check(L.ga_densify(ctypes.byref(a), s), "ga_densify")
            c = out_counts.cpu().tolist()
    n = int(c[0])
    counts = {"N_before": N, "N_after": n, "kept": int(c[1]), "cloned": int(c[2]), "split": int(c[3]), "pruned": int(c[4]),
              "prune_only": bool(a.flags & _lib.GA_DENSIFY_PRUNE_ONLY)}
    if return_noise:
        counts["noise"] = noise
    return out_raw[:n], out_m[:n], out_v[:n], parent[:n], counts


def reset_opacity(raw, m, v, cap=0.01):
    """The opacity reset, in place (include/ga_densify.h: ga_fit_reset_opacity): the raw opacity of every surfel is capped at
    logit(cap), computed in double and rounded once, and the opacity column of the Adam moments is zeroed -> raw"""
    if not _is_num(cap) or not 0.0 < cap < 1.0:
        raise ValueError("cap must lie in (0, 1)")
    N = _check_points(raw, m, v)
    if not (raw.is_contiguous() and m.is_contiguous() and v.is_contiguous()):
        raise ValueError("raw, m and v are changed in place: they must be contiguous")
    with torch.cuda.device(raw.device):
        a = _lib.GaFitResetOpacityArgs(N, math.log(cap / (1.0 - cap)), raw.data_ptr(), m.data_ptr(), v.data_ptr())
        s = ctypes.c_void_p(torch.cuda.current_stream(raw.device).cuda_stream)
        _lib.check(_lib.lib().ga_fit_reset_opacity(ctypes.byref(a), s), "ga_fit_reset_opacity")
    return raw


class SurfelFitter:
    """Adam on the raw parameters of N surfels against V posed target views; see the module docstring.

    ``step(n)`` runs n iterations, ``gaussians()`` returns the activated ``[1,N,13]`` tensor ``render`` takes, ``raw`` the raw
    parameters, ``raw_grad`` the raw-space gradient of the last iteration, ``loss_history()`` the weighted loss terms of every iteration
    so far (one read-back), ``set_views`` replaces cameras and targets without a new capture.

    The loss is ``l2 * MSE + l1 * L1 + ssim * (1 - SSIM) + lambda_normal * normal + lambda_dist * dist + lambda_alpha * |alpha - mask|``
    as ``losses.photometric_loss`` and ``losses.geometric_loss`` define the terms (``normal`` / ``mask`` as in ``geometric_loss``).

    ``densify`` (a ``DensifyConfig`` or a dict of its fields; None: the number of surfels never changes and nothing below exists):
    ``ga_fit_accumulate`` joins the captured chain, ``step`` ends a stretch of iterations wherever a clone / split / prune round or
    an opacity reset is due, runs it, and captures the iteration again for the new number of surfels.  ``densify_now()`` runs a round
    at once, ``num_points`` is the present N, ``densify_log`` lists ``(step, N_before, N_after, cloned, split, pruned)`` per round.

    ``visible_only=True``: a surfel whose radius is 0 in every view of an iteration keeps raw, m and v in that iteration.  With view
    mini-batches "every view" is every view of the batch: a surfel outside every view of the batch keeps raw, m and v.

    ``batch_views=B`` (None: every iteration renders every view, and nothing below exists): view mini-batches.  ``cam_view``,
    ``cam_view_proj``, ``targets``, ``mask`` and ``normal`` are then a POOL of P >= B views kept on the device (``targets`` may be
    ``torch.uint8`` in this mode only: the batch receives ``u / 255``), and iteration t renders the B views row t of the view schedule
    names: ``view_schedule`` (an integer tensor ``[max_steps, B]`` with values in ``[0, P)``, checked here) or, if None,
    ``fitting.view_schedule(max_steps, P, B, view_seed)``.  The row is selected on the device by the step counter
    (``ga_fit_select_views``, the first launch of the captured chain), so nothing in an iteration touches the host.  Every internal
    buffer, loss weight (lambda / B) and densification statistic is that of the batch.  ``set_views`` replaces the pool (same P, H,
    W), ``set_view_schedule`` the table, neither with a new capture; ``last_views()`` returns the views of the last iteration.  The
    snapshot / redo path of ``step`` is unchanged: the counter is part of the snapshot, so a redone stretch draws the same rows.  The
    schedule is configuration, not state: ``state_dict`` does not hold it.
    """

    def __init__(self, gaussians, cam_view, cam_view_proj, tanfov, targets, *, mask=None, normal=None, bg=None,
                 l2=0.0, l1=0.8, ssim=0.2, lambda_normal=0.05, lambda_dist=0.0, lambda_alpha=0.0, lr=None,
                 betas=(0.9, 0.999), eps=1e-15, max_steps=DEFAULT_MAX_STEPS, visible_only=False, check_every=50, capacity=None,
                 densify=None, batch_views=None, view_schedule=None, view_seed=0):
        # ---- everything the host can see is checked before anything is enqueued --------------------------------------------------
        lr = _check_lr(dict(DEFAULT_LR) if lr is None else lr)
        self._densify = _as_config(densify)
        tensors = [("gaussians", gaussians), ("cam_view", cam_view), ("cam_view_proj", cam_view_proj), ("targets", targets)]
        tensors += [(k, t) for k, t in (("mask", mask), ("normal", normal), ("bg", bg)) if t is not None]
        u8 = isinstance(targets, torch.Tensor) and targets.dtype == torch.uint8
        if u8 and batch_views is None:
            raise TypeError("uint8 targets are taken only with batch_views=: the select launch is what converts them")
        schedule = self._check_minibatch(batch_views, view_schedule, view_seed, targets, max_steps)
        for name, t in tensors:
            if not isinstance(t, torch.Tensor) or not (t.is_floating_point() or (u8 and name == "targets")):
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
        self.N, (self._P, _, self.H, self.W) = int(g.shape[0]), (int(x) for x in targets.shape)
        # V: the views of an iteration, what every internal buffer is sized by; P: the views the caller hands over (V without mini-batches)
        self._batched = schedule is not None
        self.V = int(batch_views) if self._batched else self._P
        self._u8 = u8
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
        self._round, self.densify_log = 0, []

        def f32(*shape):
            return torch.zeros(shape, dtype=torch.float32, device=dev)

        with torch.cuda.device(dev):
            # state that does not depend on N
            self._counter = torch.zeros(1, dtype=torch.int32, device=dev)
            self._seen = torch.zeros(4, dtype=torch.int64, device=dev)
            self._history = f32(max_steps, _lib.GA_FIT_HISTORY_COLS)
            self._table = step_table(lr, self.betas, max_steps).to(dev)
            # static inputs
            self._view, self._proj = f32(V, 16), f32(V, 16)
            self._targets = f32(V, 3, H, W)
            self._mask = f32(V, 1, H, W) if mask is not None else None
            self._normal = f32(V, 3, H, W) if normal is not None else None
            self._bg = torch.ones(3, dtype=torch.float32, device=dev) if bg is None else bg.detach().float().reshape(3).clone()
            # what the caller's views are copied into: the buffers the chain reads or, with mini-batches, the pool the select launch reads
            self._in = {"view": self._view, "proj": self._proj, "targets": self._targets, "mask": self._mask, "normal": self._normal}
            if self._batched:
                P = self._P
                self._in = {"view": f32(P, 16), "proj": f32(P, 16),
                            "targets": torch.zeros(P, 3, H, W, dtype=torch.uint8 if u8 else torch.float32, device=dev),
                            "mask": f32(P, 1, H, W) if mask is not None else None,
                            "normal": f32(P, 3, H, W) if normal is not None else None}
                self._schedule = schedule.to(dev)
                self._selected = torch.zeros(V, dtype=torch.int32, device=dev)
            self._copy_views(cam_view, cam_view_proj, targets, mask, normal)
            # rasterizer outputs, the maps of render's differentiable branch and their gradients
            self._color, self._allmap = f32(V, 3, H, W), f32(V, 7, H, W)
            self._image, self._rend_normal, self._depth = f32(V, 3, H, W), f32(V, 3, H, W), f32(V, 1, H, W)
            self._alpha, self._dist = f32(V, 1, H, W), f32(V, 1, H, W)
            self._g_image, self._g_rend_normal = f32(V, 3, H, W), f32(V, 3, H, W)
            self._g_depth, self._g_dist, self._g_alpha = f32(V, 1, H, W), f32(V, 1, H, W), f32(V, 1, H, W)
            self._g_color, self._g_allmap = f32(V, 3, H, W), f32(V, 7, H, W)
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
            self._steps = self._snap_steps = 0
            self._graph = None
            self._side = torch.cuda.Stream(dev)
            self._allocate_points(raw, None, None, int(capacity) if capacity is not None else default_capacity(N, V))
            self._bind()
            self._warm_up_and_capture()

    @classmethod
    def from_points(cls, points, cam_view, cam_view_proj, tanfov, targets, *, colors=None, normals=None, K=16, opacity=0.1,
                    scale_factor=1.0, **fitter_kwargs):
        """A fitter that starts from a point cloud [N,3] or [1,N,3] instead of finished Gaussians: ``surfels_from_points(points, colors,
        normals, K, opacity, scale_factor)`` and then the constructor with ``fitter_kwargs``."""
        g = surfels_from_points(points, colors=colors, normals=normals, K=K, opacity=opacity, scale_factor=scale_factor)
        return cls(g, cam_view, cam_view_proj, tanfov, targets, **fitter_kwargs)

    @classmethod
    def from_rgbd(cls, depth, cam_view, cam_view_proj, tanfov, targets, *, mask=None, normal=None, pixel_stride=1,
                  max_points=200_000, depth_range=(0.0, float("inf")), mask_threshold=0.5, erode=0, consistency=None,
                  voxel_size=None, **from_points_kw):
        """A fitter that starts from its own posed RGB-D views: ``depth`` [V,1,H,W] or [V,H,W] (camera z, what ``render`` returns; 0,
        NaN and inf are holes) is unprojected through ``cam_view`` / ``tanfov`` (``pointcloud.unproject_depth_views``: every
        ``pixel_stride``-th row and column, foreground of ``mask`` eroded ``erode`` times when a mask is given), the colours are
        ``targets`` at the pixels, the normals ``normal`` [V,3,H,W] (world space) or, without it, ``losses.depth_to_normal`` of the
        depth.  The number of points is read back once, here; the trimmed cloud goes to ``from_points`` with ``from_points_kw``
        (``K``, ``opacity``, ``scale_factor`` and the constructor's keywords).  ``mask`` and ``normal`` are the constructor's as well:
        they supervise alpha and the normals as they would in ``SurfelFitter(...)``.  More than ``max_points`` valid pixels raise, with
        the stride that would fit: nothing is subsampled silently.

        ``consistency`` (None: off; True, or a dict of ``pointcloud.filter_view_consistency``'s keywords) drops the points that the
        depth maps of the other views contradict -- the same depth, mask, cameras, ``depth_range`` and ``mask_threshold``;
        ``voxel_size`` (None: off) then keeps one point per cell of that size (``pointcloud.voxel_thin``, the point nearest each
        cell's centre), which thins where views overlap and keeps what only one view sees.  Both run on the device before the one
        count read, and ``max_points`` applies to what they leave."""
        from . import cameras, losses, pointcloud
        if consistency is not None and consistency is not True and not isinstance(consistency, dict):
            raise TypeError("consistency is None, True or a dict of filter_view_consistency's keywords")
        if voxel_size is not None and not (0.0 < float(voxel_size) < float("inf")):
            raise ValueError("voxel_size must be positive and finite (None: no thinning)")
        if not isinstance(depth, torch.Tensor) or not isinstance(targets, torch.Tensor) or not isinstance(cam_view, torch.Tensor):
            raise TypeError("depth, cam_view and targets must be torch.Tensors")
        if int(max_points) < 4:
            raise ValueError("max_points must be at least 4: the initial scale needs the three nearest other points")
        if int(pixel_stride) < 1:
            raise ValueError("pixel_stride must be at least 1")
        if targets.dim() != 4 or targets.shape[1] != 3 or depth.dim() not in (3, 4) or \
                (int(depth.shape[0]), int(depth.shape[-2]), int(depth.shape[-1])) != (int(targets.shape[0]),) + tuple(targets.shape[2:]):
            raise ValueError("targets is [V,3,H,W] and depth [V,1,H,W] or [V,H,W] of the same views")
        cam = cameras.cameras_from_view(cam_view, tanfov)
        if depth.device.type != "cuda":
            raise RuntimeError("depth must be on the GPU (no CPU fallback)")
        with torch.no_grad():
            d4 = depth.detach().float().reshape(depth.shape[0], 1, depth.shape[-2], depth.shape[-1])
            nrm = normal if normal is not None else losses.depth_to_normal(cam_view.detach().float().transpose(1, 2), float(tanfov), d4)
            cloud = pointcloud.unproject_depth_views(d4, cam, mask=mask, color=targets, normal=nrm, depth_kind="z",
                                                     depth_range=depth_range, mask_threshold=mask_threshold, erode=erode,
                                                     pixel_stride=int(pixel_stride))
            if consistency is not None:
                rule = dict(depth_range=depth_range, mask_threshold=mask_threshold)
                rule.update(consistency if isinstance(consistency, dict) else {})
                cloud = pointcloud.filter_view_consistency(cloud, d4, cam, mask=mask, depth_kind="z", **rule)
            if voxel_size is not None:
                cloud = pointcloud.voxel_thin(cloud, float(voxel_size))
            n = int(cloud.count.item())                      # the one host read
        if n > int(max_points):
            fit = int(pixel_stride)
            while n * (int(pixel_stride) / fit) ** 2 > int(max_points):
                fit += 1
            raise ValueError(f"{n} valid pixels at pixel_stride={int(pixel_stride)} exceed max_points={int(max_points)}: "
                             f"pixel_stride={fit} would give about {int(n * (int(pixel_stride) / fit) ** 2)}"
                             + (f"; a voxel_size larger than {float(voxel_size)} thins further" if voxel_size is not None else
                                "; voxel_size= keeps one point per cell of space instead of thinning every view blindly"))
        if n < 4:
            raise ValueError(f"only {n} valid pixels: a fit needs at least 4 points")
        cloud = cloud.trimmed(n)
        extra = {k: v for k, v in (("mask", mask), ("normal", normal)) if v is not None}
        return cls.from_points(cloud.points, cam_view, cam_view_proj, tanfov, targets, colors=cloud.colors, normals=cloud.normals,
                               **extra, **from_points_kw)

    def _allocate_points(self, raw, m, v, capacity, seg_capacity=0):
        """everything whose size depends on the number of surfels: the state and its snapshot, the activated arrays, the radii, the
        per-surfel gradients, the densification statistics, the launch plan, the rasterizer workspace and the bound forward"""
        dev, V, H, W = self.device, self.V, self.H, self.W
        N = self.N = int(raw.shape[0])

        def f32(*shape):
            return torch.zeros(shape, dtype=torch.float32, device=dev)

        self.plan = _lib.GaFitPlan()
        _lib.check(self._L.ga_fit_plan(N, V, H, W, ctypes.byref(self.plan)), "ga_fit_plan")
        with torch.cuda.device(dev):
            self._raw, self._raw_grad = raw.contiguous(), f32(N, 13)
            self._m = f32(N, 13) if m is None else m.contiguous()
            self._v = f32(N, 13) if v is None else v.contiguous()
            if self._densify is not None:
                self._grad_accum = f32(N)
                self._denom, self._max_radius = (torch.zeros(N, dtype=torch.int32, device=dev) for _ in range(2))
            self._snap = [torch.empty_like(t) for t in self._state()]
            # the activated arrays, one buffer laid out by the plan
            pl = self.plan
            self._act_buffer = torch.zeros(pl.workspace_bytes + 256, dtype=torch.uint8, device=dev)
            base = (-self._act_buffer.data_ptr()) % 256

            def section(off, *shape):
                n = int(np.prod(shape)) * 4
                return self._act_buffer[base + off:base + off + n].view(torch.float32).view(*shape)

            self._means, self._opac, self._colors = section(pl.means, N, 3), section(pl.opacities, N), section(pl.colors, N, 3)
            self._scales, self._rots, self._inv_norm = section(pl.scales, N, 2), section(pl.rotations, N, 4), section(pl.inv_norm, N)
            self._radii = torch.zeros(V, N, dtype=torch.int32, device=dev)
            self._g_means, self._g_opac, self._g_colors = f32(N, 3), f32(N), f32(N, 3)
            self._g_scales, self._g_rots = f32(N, 2), f32(N, 4)
            ws = SurfelWorkspace(dev, N, V, H, W, capacity, seg_capacity)
            self._fwd = SurfelForwardPlan._bound((self._means, self._opac, self._colors, self._scales, self._rots, self._view, self._proj,
                                                  self._bg), H, W, 1.0, ws, for_backward=True,
                                                 outputs=(self._color, self._allmap, self._radii))

    def _state(self):
        """what a snapshot holds: raw, m, v and the step counter; with density control also its three statistics"""
        state = (self._raw, self._m, self._v, self._counter)
        return state if self._densify is None else state + (self._grad_accum, self._denom, self._max_radius)

    # ---- validation and static inputs ------------------------------------------------------------------------------------------
    @staticmethod
    def _check_minibatch(batch_views, view_schedule_, view_seed, targets, max_steps):
        """-> None without mini-batches, else the view schedule as a host int32 tensor [max_steps, B]: the caller's, checked, or
        ``view_schedule(max_steps, P, B, view_seed)``"""
        if batch_views is None:
            if view_schedule_ is not None:
                raise ValueError("view_schedule is given without batch_views")
            return None
        if not _is_int(batch_views) or batch_views < 1:
            raise ValueError("batch_views must be None or a positive integer")
        if not isinstance(targets, torch.Tensor) or targets.dim() != 4:
            raise ValueError("targets must be [P,3,H,W]")
        if int(max_steps) < 1:
            raise ValueError("max_steps and check_every must be at least 1")
        P = int(targets.shape[0])
        if batch_views > P:
            raise ValueError(f"batch_views = {batch_views} exceeds the pool of {P} views")
        if view_schedule_ is not None:
            return _check_schedule(view_schedule_, int(max_steps), P, int(batch_views))
        return view_schedule(int(max_steps), P, int(batch_views), view_seed)

    def _check_views(self, cam_view, cam_view_proj, targets, mask, normal):
        V, H, W = self._P, self.H, self.W
        for name, t, shape in (("cam_view", cam_view, (V, 4, 4)), ("cam_view_proj", cam_view_proj, (V, 4, 4)),
                               ("targets", targets, (V, 3, H, W)), ("mask", mask, (V, 1, H, W)), ("normal", normal, (V, 3, H, W))):
            if t is None:
                continue
            if name == "targets" and self._u8:
                if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
                    raise TypeError("targets must be a torch.uint8 tensor: the pool was constructed as one")
            elif not isinstance(t, torch.Tensor) or not t.is_floating_point():
                raise TypeError(f"{name} must be a floating-point torch.Tensor")
            if t.device.type != "cuda":
                raise ValueError(f"{name} is on {t.device}: the fitter only runs on an MI355X (HIP) device; there is no CPU path")
            if tuple(t.shape) != shape:
                raise ValueError(f"{name} must be {list(shape)}, not {list(t.shape)}")
            if name not in ("cam_view", "cam_view_proj") and t.requires_grad:
                raise ValueError(f"{name} requires grad: it is a constant of the fit")

    def _copy_views(self, cam_view, cam_view_proj, targets, mask, normal):
        self._in["view"].copy_(cam_view.detach().reshape(self._P, 16))
        self._in["proj"].copy_(cam_view_proj.detach().reshape(self._P, 16))
        self._in["targets"].copy_(targets.detach())
        if mask is not None:
            self._in["mask"].copy_(mask.detach())
        if normal is not None:
            self._in["normal"].copy_(normal.detach())

    def set_views(self, cam_view, cam_view_proj, targets, mask=None, normal=None):
        """Replace cameras and targets (same V, H, W): copies into the buffers the captured graph reads, no new capture.  ``mask`` /
        ``normal`` can be replaced only where the fitter was constructed with one.  With view mini-batches this replaces the pool: the
        same P, H, W and targets dtype, and the schedule stays."""
        self._check_views(cam_view, cam_view_proj, targets, mask, normal)
        if (mask is not None and self._mask is None) or (normal is not None and self._normal is None):
            raise ValueError("the fitter was constructed without a mask / normal target: the captured graph does not read one")
        self._copy_views(cam_view, cam_view_proj, targets, mask, normal)

    def set_view_schedule(self, view_schedule):
        """Replace the table of view mini-batches (an integer tensor ``[max_steps, B]`` with values in ``[0, P)``): a copy into the
        table the captured graph reads, no new capture.  The rows of iterations already taken are not looked at again."""
        if not self._batched:
            raise RuntimeError("this fitter was constructed without batch_views=")
        self._schedule.copy_(_check_schedule(view_schedule, self.max_steps, self._P, self.V))

    def last_views(self) -> torch.Tensor:
        """[B] int32: the pool views of the last iteration, as ``ga_fit_select_views`` wrote them (a copy)"""
        if not self._batched:
            raise RuntimeError("this fitter was constructed without batch_views=")
        return self._selected.clone()

    # ---- the launches ------------------------------------------------------------------------------------------------------------
    def _bind(self):
        """(re)build every argument block but the forward's (``self._fwd`` holds it): after construction and after the workspace has
        grown"""
        N, V, H, W, ws = self.N, self.V, self.H, self.W, self._fwd.ws
        if self._batched:
            pool = self._in
            self._a_sel = _lib.GaFitSelectArgs(
                self._P, V, H, W, self.max_steps, _lib.GA_FIT_SELECT_U8_TARGETS if self._u8 else 0, self._schedule.data_ptr(),
                self._counter.data_ptr(), pool["view"].data_ptr(), pool["proj"].data_ptr(), pool["targets"].data_ptr(),
                _ptr(pool["mask"]), _ptr(pool["normal"]), self._view.data_ptr(), self._proj.data_ptr(), self._targets.data_ptr(),
                _ptr(self._mask), _ptr(self._normal), self._selected.data_ptr())
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
        if self._densify is not None:
            self._a_acc = _lib.GaFitAccumulateArgs(N, V, self.tanfov, 0, self._g_means.data_ptr(), self._means.data_ptr(),
                                                   self._radii.data_ptr(), self._view.data_ptr(), self._grad_accum.data_ptr(),
                                                   self._denom.data_ptr(), self._max_radius.data_ptr())
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
        if self._batched:
            _lib.check(L.ga_fit_select_views(ref(self._a_sel), s), "ga_fit_select_views")
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
        if self._densify is not None:
            _lib.check(L.ga_fit_accumulate(ref(self._a_acc), s), "ga_fit_accumulate")
        _lib.check(L.ga_fit_adam(ref(self._a_adam), s), "ga_fit_adam")
        _lib.check(L.ga_fit_advance(ref(self._a_adv), s), "ga_fit_advance")

    def _save(self):
        for dst, src in zip(self._snap, self._state()):
            dst.copy_(src)
        self._snap_steps = self._steps

    def _restore(self):
        for src, dst in zip(self._snap, self._state()):
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
                at = min(self._steps, self.max_steps - 1)      # (the row the device counter, which stops at the last one, selects)
                row = self._history[at].clone()
                while True:
                    self._enqueue()
                    seen = self._seen.cpu()
                    self._restore()
                    if int(seen[0]) == 0:
                        break
                    self._grow(seen)
                self._history[at].copy_(row)
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
        the snapshot are run again.  With density control a stretch also ends at every iteration after which a round or an opacity
        reset is due: the overflow words are read first (an overflowed stretch is run again before anything else), then the round
        runs on the statistics of the iterations since the last one."""
        n = int(n)
        if n < 0:
            raise ValueError("n must not be negative")
        if self._steps + n > self.max_steps:
            raise ValueError(f"{self._steps} + {n} steps exceed max_steps = {self.max_steps}: the step table has no more rows")
        target = self._steps + n
        with torch.cuda.device(self.device):
            while self._steps < target:
                due = self._next_event(self._steps) if self._densify is not None else None
                stop = target if due is None else min(target, due)
                k = min(self.check_every - (self._steps - self._snap_steps), stop - self._steps)
                for _ in range(k):
                    self._graph.replay()
                self._steps += k
                seen = self._seen.cpu()
                if int(seen[0]) != 0:
                    self._restore()
                    self._grow(seen)
                    self._warm_up_and_capture()
                elif self._steps == due:
                    self._run_event()
                else:
                    self._save()
        return self

    # ---- density control -------------------------------------------------------------------------------------------------------
    def _round_due(self, t):
        c = self._densify
        return c.start <= t <= c.stop and t % c.every == 0

    def _reset_due(self, t):
        c = self._densify
        return c.opacity_reset_every > 0 and 0 < t <= c.stop and t % c.opacity_reset_every == 0

    def _next_event(self, t):
        """the first iteration count above t after which a round or a reset is due, or None"""
        c = self._densify
        first = -(-max(c.start, t + 1) // c.every) * c.every
        due = [first] if first <= c.stop else []
        if c.opacity_reset_every > 0 and (t // c.opacity_reset_every + 1) * c.opacity_reset_every <= c.stop:
            due.append((t // c.opacity_reset_every + 1) * c.opacity_reset_every)
        return min(due) if due else None

    def _run_event(self, force_round=False):
        """what is due after iteration ``self._steps``: the round, then the reset; then a snapshot -- after a round the new capture
        takes it"""
        t = self._steps
        entry = self._densify_round() if force_round or self._round_due(t) else None
        if self._reset_due(t) and not force_round:
            reset_opacity(self._raw, self._m, self._v)
        if self._graph is None:
            self._warm_up_and_capture()
        else:
            self._save()
        return entry

    def _densify_round(self):
        c, before = self._densify, self.N
        size = c.max_screen_size if self._steps > c.screen_size_from else 0
        raw, m, v, _, n = densify_and_prune(self._raw, self._m, self._v, self._grad_accum, self._denom, self._max_radius,
                                            grad_threshold=c.grad_threshold, min_opacity=c.min_opacity, percent_dense=c.percent_dense,
                                            extent=c.extent, max_screen_size=size, seed=c.seed, round=self._round,
                                            max_points=c.max_points)
        if n["N_after"] == 0:
            raise RuntimeError(f"the densify round after iteration {self._steps} pruned every one of the {before} surfels")
        self._round += 1
        entry = (self._steps, before, n["N_after"], n["cloned"], n["split"], n["pruned"])
        self.densify_log.append(entry)
        self._resize(raw.clone(), m.clone(), v.clone())
        return entry

    def _resize(self, raw, m, v):
        """another number of surfels: everything sized by N anew (the statistics zeroed), the workspace scaled with N, every argument
        block rebuilt; the captured graph is dropped -- ``_warm_up_and_capture`` is the caller's next call"""
        ws, before = self._fwd.ws, self.N
        self._graph = None
        capacity = max(ws.capacity, -(-ws.capacity * int(raw.shape[0]) // before))
        self._allocate_points(raw, m, v, capacity, ws.seg_capacity)
        self._bind()

    def densify_now(self):
        """Run one clone / split / prune round at once, on the statistics gathered since the last one -> its ``densify_log`` entry
        ``(step, N_before, N_after, cloned, split, pruned)``"""
        if self._densify is None:
            raise RuntimeError("this fitter was constructed without densify=")
        with torch.cuda.device(self.device):
            return self._run_event(force_round=True)

    def densify_stats(self) -> dict:
        """copies of the three statistics the next round decides on: ``grad_accum`` [N] float32, ``denom`` and ``max_radius`` [N] int32"""
        if self._densify is None:
            raise RuntimeError("this fitter was constructed without densify=")
        return {"grad_accum": self._grad_accum.clone(), "denom": self._denom.clone(), "max_radius": self._max_radius.clone()}

    @property
    def num_points(self) -> int:
        """the present number of surfels"""
        return self.N

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
        """copies of raw, m, v and the loss history, the number of steps taken, N and, with density control, its three statistics and
        the number of rounds run: what ``load_state_dict`` of a fitter of the same ``max_steps`` continues from (views, weights,
        learning rates and the densify settings are the constructor's)"""
        state = {"raw": self._raw.clone(), "m": self._m.clone(), "v": self._v.clone(), "steps": self._steps,
                 "history": self._history[:self._steps].clone(), "N": self.N, "round": self._round}
        if self._densify is not None:
            state.update(self.densify_stats())
        return state

    def load_state_dict(self, state: dict):
        steps = int(state["steps"])
        if not 0 <= steps <= self.max_steps:
            raise ValueError(f"the state has taken {steps} steps, this fitter's table has {self.max_steps} rows")
        n = int(state["raw"].shape[0]) if state["raw"].dim() == 2 else 0
        for k in ("raw", "m", "v"):
            if n < 1 or tuple(state[k].shape) != (n, 13):
                raise ValueError(f"state[{k!r}] must be [N, 13], not {list(state[k].shape)}")
        if int(state.get("N", n)) != n:
            raise ValueError(f"state['N'] is {state['N']}, state['raw'] holds {n} rows")
        if tuple(state["history"].shape) != (steps, _lib.GA_FIT_HISTORY_COLS):
            raise ValueError("state['history'] must hold one row per step taken")
        stats = ("grad_accum", "denom", "max_radius") if self._densify is not None and "grad_accum" in state else ()
        for k in stats:
            if tuple(state[k].shape) != (n,):
                raise ValueError(f"state[{k!r}] must be [{n}], not {list(state[k].shape)}")
        with torch.cuda.device(self.device):
            dev = self.device
            if n != self.N:       # a state of another N: everything sized by N anew, a new capture below
                self._resize(*(state[k].detach().to(dev, torch.float32).clone() for k in ("raw", "m", "v")))
            else:
                for dst, k in ((self._raw, "raw"), (self._m, "m"), (self._v, "v")):
                    dst.copy_(state[k])
                if self._densify is not None:
                    for t in (self._grad_accum, self._denom, self._max_radius):
                        t.zero_()
            for dst, k in zip((getattr(self, "_grad_accum", None), getattr(self, "_denom", None), getattr(self, "_max_radius", None)),
                              stats):
                dst.copy_(state[k])
            self._round = int(state.get("round", 0))
            self._history[:steps].copy_(state["history"])
            self._counter.fill_(min(steps, self.max_steps - 1))
            self._steps = steps
            if self._graph is None:
                self._warm_up_and_capture()
            else:
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
