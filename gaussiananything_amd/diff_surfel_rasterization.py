"""MI355X-native stand-in for the third-party ``diff_surfel_rasterization`` package.

Exports the two names the reference imports (``/root/reference/nsr/gs_surfel.py:15``) with the same call convention
(``:85-114``): ``GaussianRasterizationSettings`` (NamedTuple, 12 fields) and ``GaussianRasterizer(raster_settings)``
whose call returns ``(color[3,H,W], radii[N], allmap[7,H,W])``.  The arithmetic runs in hand-written HIP kernels behind
the C-ABI of ``include/ga_surfel.h``; there is no CPU path -- CPU tensors or a missing library raise.

``rasterize_views`` is the batched form the MI355X design is built around (all views of one Gaussian set in one
launch sequence); the per-view ``GaussianRasterizer`` call is a V=1 special case of it.
"""
from __future__ import annotations

import ctypes
import os
from collections import OrderedDict
import warnings
from typing import NamedTuple, Optional

import torch
import torch.nn as nn

from . import _lib


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def _default_seg_items(capacity):
    """(tile, segment) work items the library sizes the exchange scratch for when ``seg_capacity`` is 0 (csrc/surfel_api.hip)"""
    return capacity // 2048 + 128


class SurfelWorkspace:
    """Caller-owned device scratch for ``ga_surfel_forward`` (the C-ABI allocates nothing).

    ``capacity`` is the number of binned (tile, splat) entries the buffers can hold, ``seg_capacity`` the number of
    (tile, segment) work items of the segmented blend (lists of 2048 entries or more) its exchange scratch holds (0 = the
    library's default, ``_default_seg_items(capacity)``; the worst case is capacity / 256).  The device reports the real counts and an
    overflow flag in ``status``; on overflow nothing was rendered and the caller grows the workspace and re-runs
    (``SurfelForwardPlan.ensure_capacity`` does that; ``grown`` sizes the replacement).
    """

    def __init__(self, device, num_points, num_views, height, width, capacity, seg_capacity=0):
        self.key = (num_points, num_views, height, width)
        self.device = device
        self.capacity = int(capacity)
        self.seg_capacity = int(seg_capacity)
        self.seg_items = self.seg_capacity if self.seg_capacity > 0 else _default_seg_items(self.capacity)
        self.clean = False       # set by the first forward enqueued on it: its tile scan leaves the workspace head ready for the next
        self.seg_T = None        # ``transmittance_table()``, once a differentiable forward has asked for it
        self.layout = _lib.GaSurfelWorkspaceLayout()
        _lib.check(_lib.lib().ga_surfel_workspace_layout2(num_points, num_views, height, width, self.capacity,
                                                          self.seg_capacity, ctypes.byref(self.layout)),
                   "ga_surfel_workspace_layout2")
        self.buffer = torch.empty(self.layout.total_bytes + 256, dtype=torch.uint8, device=device)
        self.offset = (-self.buffer.data_ptr()) % 256
        self.ptr = self.buffer.data_ptr() + self.offset
        # launch epoch of the segmented blend's exchange words: any start value will do, but recycled device memory may still
        # hold words of an earlier workspace -- start somewhere random so that they only match by a 2^-32 coincidence
        self.section("seg_table", torch.int32, 128)[_lib.GA_SEG_EPOCH_WORD] = int.from_bytes(os.urandom(4), "little") - (1 << 31)

    def section(self, name, dtype, count):
        """Typed view of one workspace section (tests read the integer artefacts through this)."""
        off = self.offset + getattr(self.layout, name)
        nbytes = count * torch.empty((), dtype=dtype).element_size()
        return self.buffer[off:off + nbytes].view(dtype)

    def status(self):
        return self.section("status", torch.int64, _lib.GA_STATUS_WORDS)

    def clean_flag(self):
        """GA_SURFEL_FLAG_WORKSPACE_CLEAN once a forward has been enqueued on this workspace (include/ga_surfel.h)."""
        return _lib.GA_SURFEL_FLAG_WORKSPACE_CLEAN if self.clean else 0

    def transmittance_table(self):
        """The transmittance table a differentiable forward leaves for ``ga_surfel_backward`` (GaSurfelForwardArgs.seg_T): one row of
        256 floats per 128-entry list segment; kept with the workspace it was sized for.  ``GA_SURFEL_SEG_T=0``: do without (the
        backward then walks the lists once more for these products; A/B aid)."""
        if os.environ.get("GA_SURFEL_SEG_T", "1") == "0":
            return None
        if self.seg_T is None:
            n, v, h, w = self.key
            rows = self.capacity // 128 + v * ((h + 15) // 16) * ((w + 15) // 16) + 1     # what ga_surfel_forward holds seg_T_floats to
            self.seg_T = torch.empty(rows * 256, dtype=torch.float32, device=self.device)
        return self.seg_T

    def grown(self, st=None, *, need=None, seg_need=None):
        """A replacement workspace for the counts of an overflowed launch: its status words ``st`` (host tensor), or the binned
        entries ``need`` and the segment work items ``seg_need`` themselves."""
        if st is not None:
            need, seg_need = int(st[_lib.GA_STATUS_NUM_RENDERED]), int(st[_lib.GA_STATUS_SEG_WORK])
        if need > 0xFFFFFFFF:
            raise RuntimeError(f"{need} binned entries exceed the 2^32 limit of the tile ranges")
        cap = max(self.capacity, need + need // 4) if need > self.capacity else self.capacity
        seg = self.seg_capacity
        if seg_need > (seg if seg > 0 else _default_seg_items(cap)):
            seg = seg_need + seg_need // 4 + 16
        n, v, h, w = self.key
        return SurfelWorkspace(self.device, n, v, h, w, cap, seg)


_seg_T = SurfelWorkspace.transmittance_table


def default_capacity(n, v):
    """Binned entries a fresh workspace is sized for: two tiles per (view, splat) on average -- BASELINE configs[1] needs 1.8;
    scenes that need more are reported by the device and the workspace is re-sized once."""
    return max(2 * n * v, 1 << 16)


EXTRA_FLAGS = int(os.environ.get("GA_SURFEL_FLAGS", "0"))   # GA_SURFEL_FLAG_* ORed into every forward (4: the split walk of the blend; A/B aid)
_WS_CACHE_SLOTS = 8          # most recently used (device, N, V, H, W) workspaces kept alive; older ones are released
_ws_cache = OrderedDict()
_AUTOGRAD_POOL_KEYS = 4       # shapes whose idle workspaces are kept (least recently used shape dropped first), two per shape
_autograd_pool = OrderedDict()  # (device, N, V, H, W) -> idle workspaces of the differentiable path


class _WorkspaceLease:
    """Ownership of one workspace by one differentiable forward.  The backward reads the tile lists and transmittances of exactly
    that forward, possibly several times (``retain_graph=True``: the reference's adaptive loss weight runs ``autograd.grad`` twice
    before the final backward, dnnlib/util.py ``calculate_adaptive_weight``), so the workspace goes back to the pool when the
    autograd node is FREED, not when a backward has run; stream order protects the reuse by a later forward.  ``fwd`` is the
    forward's ``SurfelForwardPlan.backward_args()``: what that forward passed, whatever the environment says by the backward."""

    def __init__(self, ws, key, fwd):
        self.ws, self.key, self.fwd = ws, key, fwd

    def __del__(self):
        try:
            pool = _autograd_pool.setdefault(self.key, [])
            _autograd_pool.move_to_end(self.key)
            if len(pool) < 2 and not any(w is self.ws for w in pool):
                pool.append(self.ws)
            while len(_autograd_pool) > _AUTOGRAD_POOL_KEYS:
                _autograd_pool.popitem(last=False)
        except Exception:   # interpreter shutdown
            pass


def clear_workspaces():
    """drop every cached / pooled rasterizer workspace (their device memory returns to the caching allocator)"""
    _ws_cache.clear()
    _autograd_pool.clear()


def cached_workspace(device, n, v, h, w, replacement=None):
    """The workspace ``rasterize_views`` uses for this shape when it is given none: created at the default capacity (on the current
    stream) at the first call, kept while the shape is among the most recently used.  ``replacement``: a larger one that takes
    the place of one that overflowed."""
    key = (str(device), n, v, h, w)
    ws = replacement or _ws_cache.pop(key, None) or SurfelWorkspace(device, n, v, h, w, default_capacity(n, v))
    _ws_cache.pop(key, None)
    _ws_cache[key] = ws          # most recently used last
    while len(_ws_cache) > _WS_CACHE_SLOTS:
        _ws_cache.popitem(last=False)
    return ws


def _f32(t: torch.Tensor, name: str, device, detach: bool = True) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.device.type != "cuda":
        raise RuntimeError(f"{name} is on {t.device}: the surfel rasterizer only runs on an MI355X (HIP) device; "
                           "there is no CPU path")
    if t.device != device:
        raise RuntimeError(f"{name} is on {t.device}, expected {device}")
    return (t.detach() if detach else t).contiguous().float()


def _inputs(means3D, opacities, colors_precomp, scales, rotations, viewmatrix, projmatrix, bg, detach=True):
    """The eight tensors of a forward as the C-ABI reads them -- fp32, contiguous, on the device of ``means3D``, shapes checked.
    ``detach=False`` keeps the autograd graph of the five Gaussian tensors (the differentiable path)."""
    device = means3D.device
    m = _f32(means3D, "means3D", device, detach)
    n = m.shape[0]
    o = _f32(opacities, "opacities", device, detach).reshape(-1)
    c = _f32(colors_precomp, "colors_precomp", device, detach)
    s = _f32(scales, "scales", device, detach)
    r = _f32(rotations, "rotations", device, detach)
    if m.shape != (n, 3) or o.shape != (n,) or c.shape != (n, 3) or s.shape != (n, 2) or r.shape != (n, 4):
        raise ValueError("expected means3D[N,3], opacities[N,1], colors_precomp[N,3], scales[N,2], rotations[N,4]")
    vm = _f32(viewmatrix, "viewmatrix", device).reshape(-1, 16)
    pm = _f32(projmatrix, "projmatrix", device).reshape(-1, 16)
    if pm.shape[0] != vm.shape[0]:
        raise ValueError("viewmatrix and projmatrix must hold the same number of views")
    return m, o, c, s, r, vm, pm, _f32(bg, "bg", device).reshape(3)


def postprocess_views(color, allmap, viewmatrix, image=None, rend_normal=None, depth=None):
    """The per-pixel post-processing of ``GaussianRenderer2DGS.render`` (nsr/gs_surfel.py:121-163) over the stacked outputs
    of ``rasterize_views`` in ONE pass (``ga_surfel_postprocess``): ``image = clamp(color, 0, 1)``, ``rend_normal`` =
    ``allmap[:, 2:5]`` rotated from view to world space, ``depth = nan_to_num(allmap[:, 5:6], 0, 0)``.  The optional
    outputs are written in place (contiguous ``[V,3,H,W]``, ``[V,3,H,W]``, ``[V,1,H,W]``)."""
    if color.device.type != "cuda":
        raise RuntimeError("gaussiananything_amd surfel post-processing only runs on an MI355X (HIP) device")
    V, _, H, W = color.shape
    assert allmap.shape == (V, 7, H, W) and color.is_contiguous() and allmap.is_contiguous()
    vm = viewmatrix.detach().to(device=color.device, dtype=torch.float32).reshape(V, 16).contiguous()
    image = torch.empty_like(color) if image is None else image
    rend_normal = torch.empty_like(color) if rend_normal is None else rend_normal
    depth = torch.empty((V, 1, H, W), dtype=torch.float32, device=color.device) if depth is None else depth
    for t, shp in ((image, (V, 3, H, W)), (rend_normal, (V, 3, H, W)), (depth, (V, 1, H, W))):
        assert t.shape == shp and t.is_contiguous() and t.dtype == torch.float32 and t.device == color.device
    args = _lib.GaSurfelPostArgs(V, H, W, color.data_ptr(), allmap.data_ptr(), vm.data_ptr(), image.data_ptr(),
                                 rend_normal.data_ptr(), depth.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(color.device).cuda_stream)
    _lib.check(_lib.lib().ga_surfel_postprocess(ctypes.byref(args), stream), "ga_surfel_postprocess")
    return image, rend_normal, depth


class _RasterizeViews(torch.autograd.Function):
    """Differentiable ``rasterize_views``: forward = ``ga_surfel_forward`` on a workspace of its own (the backward reads the
    tile ranges and point lists of exactly this call again), backward = ``ga_surfel_backward`` (gradients with respect to
    means3D, opacities, colours, scales and rotations, summed over the views; include/ga_surfel.h)."""

    @staticmethod
    def forward(ctx, means3D, opacities, colors, scales, rotations, vm, pm, bg, h, w, scale_modifier):
        n, v = means3D.shape[0], vm.shape[0]
        # a workspace of its own until the backward has read it; taken from / returned to a small pool instead of a fresh
        # allocation per call
        key = (str(means3D.device), n, v, h, w)
        pool = _autograd_pool.get(key) or []
        ws = pool.pop() if pool else SurfelWorkspace(means3D.device, n, v, h, w, default_capacity(n, v))
        plan = SurfelForwardPlan._bound((means3D, opacities, colors, scales, rotations, vm, pm, bg), h, w, scale_modifier, ws,
                                        for_backward=True)
        with torch.cuda.device(means3D.device):
            plan.run()
            plan.ensure_capacity()      # (a replacement stays this call's own and goes to the pool with the lease)
        color, radii, allmap = plan.color, plan.radii, plan.allmap
        # the tensors whose addresses the lease's argument block holds stay alive with the node; the lease itself must not hold the
        # outputs (they own the node)
        ctx.save_for_backward(means3D, opacities, colors, scales, rotations, vm, pm, bg, color, allmap, radii)
        ctx.lease = _WorkspaceLease(plan.ws, key, plan.backward_args())
        ctx.mark_non_differentiable(radii)
        return color, radii, allmap

    @staticmethod
    def backward(ctx, g_color, g_radii, g_allmap):
        means3D, opacities, colors, scales, rotations, vm, pm, bg, color, allmap, radii = ctx.saved_tensors
        fwd, dev = ctx.lease.fwd, means3D.device   # (the workspace is owned by this node until it is freed: any number of backwards)
        g_color = torch.zeros_like(color) if g_color is None else g_color.detach().float().contiguous()
        g_allmap = torch.zeros_like(allmap) if g_allmap is None else g_allmap.detach().float().contiguous()
        L = _lib.lib()
        d_means, d_op = torch.empty_like(means3D), torch.empty_like(opacities)
        d_col, d_sc, d_rot = torch.empty_like(colors), torch.empty_like(scales), torch.empty_like(rotations)
        nbytes = int(L.ga_surfel_backward_scratch_bytes(ctypes.byref(fwd)))
        if nbytes == 0:
            raise RuntimeError("ga_surfel_backward_scratch_bytes: bad shape")
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        args = _lib.GaSurfelBackwardArgs(fwd, g_color.data_ptr(), g_allmap.data_ptr(), scratch.data_ptr(), scratch.numel(),
                                         d_means.data_ptr(), d_op.data_ptr(), d_col.data_ptr(), d_sc.data_ptr(), d_rot.data_ptr())
        with torch.cuda.device(dev):
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(L.ga_surfel_backward(ctypes.byref(args), stream), "ga_surfel_backward")
        return d_means, d_op, d_col, d_sc, d_rot, None, None, None, None, None, None


def rasterize_views(means3D, opacities, colors_precomp, scales, rotations, viewmatrix, projmatrix, bg,
                    image_height, image_width, scale_modifier=1.0, workspace: Optional[SurfelWorkspace] = None,
                    stage_events=None):
    """``_rasterize_views_nograd`` (below), differentiable when autograd is recording and a Gaussian tensor requires grad:
    ``color`` and ``allmap`` then carry a grad_fn whose backward is ``ga_surfel_backward`` (``radii`` is not differentiable; the median-depth
    channel passes its gradient to the depth of the median contributor; the workspace of such a call is its own)."""
    if torch.is_grad_enabled() and any(getattr(t, "requires_grad", False) for t in
                                       (means3D, opacities, colors_precomp, scales, rotations)):
        inputs = _inputs(means3D, opacities, colors_precomp, scales, rotations, viewmatrix, projmatrix, bg, detach=False)
        color, radii, allmap = _RasterizeViews.apply(*inputs, int(image_height), int(image_width), float(scale_modifier))
        return color, radii, allmap, None
    return _rasterize_views_nograd(means3D, opacities, colors_precomp, scales, rotations, viewmatrix, projmatrix, bg,
                                   image_height, image_width, scale_modifier, workspace, stage_events)


def _grow_in_cache(ws, st):
    return cached_workspace(ws.device, *ws.key, replacement=ws.grown(st))


def _refuse_to_grow(ws, st):
    raise RuntimeError(f"workspace capacity {ws.capacity} / {ws.seg_items} segment work items < "
                       f"{int(st[_lib.GA_STATUS_NUM_RENDERED])} binned entries / {int(st[_lib.GA_STATUS_SEG_WORK])} work items")


def _rasterize_views_nograd(means3D, opacities, colors_precomp, scales, rotations, viewmatrix, projmatrix, bg,
                            image_height, image_width, scale_modifier=1.0, workspace: Optional[SurfelWorkspace] = None,
                            stage_events=None, for_backward: bool = False):
    """Rasterize V views of one Gaussian set.  ``viewmatrix`` / ``projmatrix``: ``[V,4,4]`` row-vector matrices
    (``cam_view`` / ``cam_view_proj``).  Returns ``color [V,3,H,W]``, ``radii [V,N] int32``, ``allmap [V,7,H,W]`` and
    the workspace used (its ``status()`` holds D / overflow / longest tile list).

    The device status word is read after the launch (one host sync, as upstream's read-back of ``num_rendered``) and an
    overflowed forward is run again on a larger workspace, which replaces the cached one; a ``workspace`` of the caller's is
    not replaced: its overflow raises.  A caller that must not synchronise per call binds a ``SurfelForwardPlan`` itself.
    ``stage_events``: optional ctypes array of 5 ``hipEvent_t`` (see ``include/ga_surfel.h``), measurement only.
    """
    inputs = _inputs(means3D, opacities, colors_precomp, scales, rotations, viewmatrix, projmatrix, bg)
    plan = SurfelForwardPlan._bound(inputs, int(image_height), int(image_width), scale_modifier, workspace,
                                    for_backward=for_backward, stage_events=stage_events)
    with torch.cuda.device(plan.device):
        plan.run()
        plan.ensure_capacity(_grow_in_cache if workspace is None else _refuse_to_grow)
    return plan.color, plan.radii, plan.allmap, plan.ws


class GaussianRasterizer(nn.Module):
    """Same surface as ``diff_surfel_rasterization.GaussianRasterizer``; differentiable with respect to means3D, opacities,
    colors_precomp, scales and rotations (``means2D`` is accepted and ignored: the reference passes zeros without
    requires_grad, /root/reference/nsr/gs_surfel.py:104-106, and never reads its gradient)."""

    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None):
        rs = self.raster_settings
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        if shs is not None:
            raise NotImplementedError("spherical-harmonics colours are not on the GaussianAnything path "
                                      "(nsr/gs_surfel.py always passes colors_precomp, sh_degree=0)")
        if cov3D_precomp is not None:
            raise NotImplementedError("precomputed transforms are not on the GaussianAnything path "
                                      "(nsr/gs_surfel.py always passes scales/rotations)")
        color, radii, allmap, _ = rasterize_views(
            means3D, opacities, colors_precomp, scales, rotations, rs.viewmatrix.reshape(1, 4, 4),
            rs.projmatrix.reshape(1, 4, 4), rs.bg, rs.image_height, rs.image_width, rs.scale_modifier)
        return color[0], radii[0], allmap[0]


class SurfelForwardPlan:
    """Pre-bound ``ga_surfel_forward`` call for repeated rendering of a fixed problem shape: inputs are converted
    once, outputs and workspace are allocated once, ``run()`` is a single C-ABI call that enqueues the five kernels on
    the current stream without any host synchronisation (so it can also be captured into a HIP graph).

    The sampling scripts render 50 cameras x 4 LoDs per sample (/root/reference/nsr/lsgm/flow_matching_trainer.py:
    1545-1616); a plan per LoD removes the per-call tensor juggling of the reference's Python loop.

    It is also the package's one binding of ``ga_surfel_forward``: ``rasterize_views``, the autograd path, ``render_levels`` and
    the fitter each bind a plan, so the argument block, the clean-workspace rule and the grow-and-retry loop exist here only.
    """

    def __init__(self, means3D, opacities, colors_precomp, scales, rotations, viewmatrix, projmatrix, bg,
                 image_height, image_width, scale_modifier=1.0, capacity=None, flags=0, workspace=None):
        """``workspace``: one to run on (``cached_workspace``, or the caller's own) instead of a new one of ``capacity`` entries"""
        inputs = _inputs(means3D, opacities, colors_precomp, scales, rotations, viewmatrix, projmatrix, bg)
        n, v, h, w = inputs[0].shape[0], inputs[5].shape[0], int(image_height), int(image_width)
        if workspace is None:
            workspace = SurfelWorkspace(inputs[0].device, n, v, h, w, capacity or default_capacity(n, v))
        self._setup(inputs, h, w, scale_modifier, workspace, flags)

    @classmethod
    def _bound(cls, inputs, h, w, scale_modifier, ws, **kw):
        """The internal constructor: ``inputs`` are the eight tensors as ``_inputs`` returns them (or buffers of the caller's that
        meet the same conditions), ``ws`` the workspace to run on (None: the cached one of the shape)."""
        self = cls.__new__(cls)
        self._setup(inputs, h, w, scale_modifier, ws, **kw)
        return self

    def _setup(self, inputs, h, w, scale_modifier, ws, flags=0, for_backward=False, stage_events=None, outputs=None):
        """``for_backward``: the forward of a differentiable call, it leaves the transmittance table for ``ga_surfel_backward``;
        ``outputs``: (color, allmap, radii) buffers of the caller's instead of new ones"""
        self.means3D, self.opacities, self.colors, self.scales, self.rotations, self.vm, self.pm, self.bg = inputs
        self.device = device = self.means3D.device
        self.n, self.v, self.h, self.w = n, v, h, w = self.means3D.shape[0], self.vm.shape[0], h, w
        self.scale_modifier = float(scale_modifier)
        self.flags = int(flags) | EXTRA_FLAGS      # (the module's value at this moment: a test's patch of it reaches every caller)
        self.color, self.allmap, self.radii = outputs or (torch.empty((v, 3, h, w), dtype=torch.float32, device=device),
                                                          torch.empty((v, 7, h, w), dtype=torch.float32, device=device),
                                                          torch.empty((v, n), dtype=torch.int32, device=device))
        self._for_backward, self._stage_events = for_backward, stage_events
        self._L = _lib.lib()
        self.rebind(ws if ws is not None else cached_workspace(device, n, v, h, w))

    def rebind(self, ws):
        """(re)build the argument block for ``ws``: at construction and when a larger workspace replaces an overflowed one"""
        if ws.key != (self.n, self.v, self.h, self.w):
            raise ValueError("workspace was laid out for a different problem size")
        self.ws = ws
        seg_T = ws.transmittance_table() if self._for_backward else None
        self._args = _lib.GaSurfelForwardArgs(
            num_points=self.n, num_views=self.v, image_height=self.h, image_width=self.w, scale_modifier=self.scale_modifier,
            flags=self.flags | ws.clean_flag(), means3D=self.means3D.data_ptr(), opacities=self.opacities.data_ptr(),
            colors=self.colors.data_ptr(), scales=self.scales.data_ptr(), rotations=self.rotations.data_ptr(),
            viewmatrix=self.vm.data_ptr(), projmatrix=self.pm.data_ptr(), bg=self.bg.data_ptr(), out_color=self.color.data_ptr(),
            out_others=self.allmap.data_ptr(), radii=self.radii.data_ptr(), workspace=ws.ptr, workspace_bytes=ws.layout.total_bytes,
            capacity=ws.capacity, stage_events=self._stage_events, seg_capacity=ws.seg_capacity,
            seg_T=seg_T.data_ptr() if seg_T is not None else None, seg_T_floats=seg_T.numel() if seg_T is not None else 0)
        self._argp = ctypes.byref(self._args)

    def set_stage_events(self, stage_events):
        self._stage_events = stage_events
        self.rebind(self.ws)

    def run(self):
        stream = torch.cuda.current_stream(self.device).cuda_stream
        _lib.check(self._L.ga_surfel_forward(self._argp, ctypes.c_void_p(stream)), "ga_surfel_forward")
        if not self.ws.clean:     # its tile scan leaves the workspace head ready: from the second forward on no clearing memset
            self.ws.clean = True
            self._args.flags |= self.ws.clean_flag()

    def backward_args(self):
        """``GaSurfelBackwardArgs.fwd`` for the forward this plan enqueues: the same block -- workspace, outputs and the ``seg_T``
        that forward was given -- without flags and stage events.  It holds addresses only: the caller keeps the tensors alive."""
        fwd = _lib.GaSurfelForwardArgs.from_buffer_copy(self._args)
        fwd.flags, fwd.stage_events = 0, None
        return fwd

    def ensure_capacity(self, grow=SurfelWorkspace.grown):
        """One synchronising check (call once after the first run): while the device reports an overflow (nothing was rendered),
        rebind to the larger workspace ``grow(ws, status words)`` returns and run again.  The default keeps the replacement with the
        plan; ``rasterize_views`` passes its own policies (put it in the cache; raise for a caller's workspace).  Returns the entry
        count."""
        while True:
            st = self.ws.status().cpu()
            if int(st[_lib.GA_STATUS_OVERFLOW]) == 0:
                return int(st[_lib.GA_STATUS_NUM_RENDERED])
            self.rebind(grow(self.ws, st))
            self.run()
