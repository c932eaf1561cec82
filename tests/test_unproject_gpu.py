"""GPU tests of ``ga_pc_unproject`` (include/ga_pointcloud.h, csrc/pc_unproject.hip) and of what is built on it.

The raw C-ABI call is compared with the numpy float32 restatement (tests/_unproject_ref.py) for EQUALITY, bit for bit: points, colours,
normals, source pixels, ``count`` and ``view_counts``, padding included.  Every raw call poisons its outputs first, checks guard words
behind each of them and behind the workspace, and that its inputs are unchanged.  The front ends follow: ``cloud_from_render`` on a
rendered scene, the depth -> ``fps-K.ply`` hand-off, ``SurfelFitter.from_rgbd``."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _unproject_ref as ref

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 64            # int32 words behind every buffer
GUARD_WORD = 0x5A5A5A5A
POISON = -77          # as a float: a NaN pattern no arithmetic here produces


def _guarded(n_words, device):
    t = torch.full((n_words + GUARD,), GUARD_WORD, dtype=torch.int32, device=device)
    t[:n_words] = POISON
    return t


def _take(buf, n, shape, dtype=torch.float32):
    """the first n words of a guarded buffer as numpy; the guards intact, every word written"""
    assert bool((buf[n:] == GUARD_WORD).all()), "guard words overwritten"
    assert not bool((buf[:n] == POISON).any()), "an output element was not written"
    return buf[:n].view(dtype).reshape(shape).cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same(got, want, what):
    a, b = _bits(got), _bits(want)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = a != b
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ in bits, first at {np.argwhere(bad)[0].tolist()}: " \
                          f"got {np.asarray(got, F)[bad][0]!r}, want {np.asarray(want, F)[bad][0]!r}"


class Raw:
    """one bound ``ga_pc_unproject`` call: device copies of the inputs, guarded outputs and workspace; ``enqueue`` launches on a
    stream, ``outputs`` reads back after the checks"""

    def __init__(self, device, depth, cam, mask=None, color=None, normal=None, depth_kind=ref.DEPTH_Z, depth_min=0.0, depth_max=np.inf,
                 mask_threshold=0.5, erode=0, clip=0.0, drop_zero=False, pixel_stride=1, capacity=None):
        from gaussiananything_amd import _lib
        self._lib, self.L, self.device = _lib, _lib.lib(), device
        V, H, W = depth.shape
        self.V = V
        s = int(pixel_stride)
        self.cap = cap = V * (-(-H // s)) * (-(-W // s)) if capacity is None else int(capacity)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device) if a is not None else None
        self.host = dict(depth=depth, cam=cam, mask=mask, color=color, normal=normal)
        self.inp = {k: dev(v) for k, v in self.host.items()}
        self.points = _guarded(cap * 3, device)
        self.colors = _guarded(cap * 3, device) if color is not None else None
        self.normals = _guarded(cap * 3, device) if normal is not None else None
        self.source, self.count, self.view_counts = _guarded(cap, device), _guarded(1, device), _guarded(V, device)
        self.ws_bytes = int(self.L.ga_pc_unproject_workspace_bytes(V, H, W))
        assert self.ws_bytes > 0 and self.ws_bytes % 16 == 0
        self.ws = _guarded(self.ws_bytes // 4, device)
        p = lambda t: t.data_ptr() if t is not None else None
        i = self.inp
        self.args = _lib.GaUnprojectArgs(V, H, W, depth_kind, _lib.GA_PC_COLOR_U8 if color is not None and color.dtype == np.uint8 else
                                         _lib.GA_PC_COLOR_F32, erode, int(drop_zero), s, cap, depth_min, depth_max, mask_threshold, clip, 0,
                                         p(i["depth"]), p(i["mask"]), p(i["color"]), p(i["normal"]), p(i["cam"]), p(self.points),
                                         p(self.colors), p(self.normals), p(self.source), p(self.count), p(self.view_counts), p(self.ws),
                                         self.ws_bytes)

    def enqueue(self, stream):
        self._lib.check(self.L.ga_pc_unproject(ctypes.byref(self.args), ctypes.c_void_p(stream.cuda_stream)), "ga_pc_unproject")

    def outputs(self):
        cap = self.cap
        assert bool((self.ws[self.ws_bytes // 4:] == GUARD_WORD).all()), "guard words behind the workspace overwritten"
        out = dict(points=_take(self.points, cap * 3, (cap, 3)),
                   colors=_take(self.colors, cap * 3, (cap, 3)) if self.colors is not None else None,
                   normals=_take(self.normals, cap * 3, (cap, 3)) if self.normals is not None else None,
                   source=_take(self.source, cap, (cap,), torch.int32), count=int(_take(self.count, 1, (1,), torch.int32)[0]),
                   view_counts=_take(self.view_counts, self.V, (self.V,), torch.int32))
        for k, v in self.host.items():                       # the inputs are left alone
            if v is not None:
                assert np.array_equal(self.inp[k].cpu().numpy().view(np.uint8), np.ascontiguousarray(v).view(np.uint8)), k
        return out


def raw_unproject(device, depth, cam, **kw):
    with torch.cuda.device(device):
        r = Raw(device, depth, cam, **kw)
        r.enqueue(torch.cuda.current_stream())
        torch.cuda.synchronize()
        return r.outputs()


def _check(device, depth, cam, **kw):
    """the raw call against the restatement, every output bit for bit -> the restatement's dict"""
    got = raw_unproject(device, depth, cam, **kw)
    want = ref.unproject_f32(depth, cam, **kw)
    assert got["count"] == want["count"], (got["count"], want["count"])
    assert np.array_equal(got["view_counts"], want["view_counts"]), (got["view_counts"], want["view_counts"])
    assert np.array_equal(got["source"], want["source"]), "source pixels"
    for k in ("points", "colors", "normals"):
        assert (got[k] is None) == (want[k] is None), k
        if want[k] is not None:
            _same(got[k], want[k], k)
    return want


def _cameras(V):
    """the first V pinned poses as [V,21] rows; view 1 gets skew, unequal focal lengths and an off-centre principal point"""
    from gaussiananything_amd import synthetic
    cam = ref.cameras_from_pose25(synthetic.eval_cameras(8)["poses"][:V])
    if V > 1:
        cam[1, 13] *= F(1.1)
        cam[1, 14:17] = (0.47, 0.54, 0.03)
    return cam


def _views(V, H, W, seed):
    """-> depth with holes (0, negative, NaN, +-inf), a mask with values on the threshold 0.5 and zeros at the image border and along
    the borders of the flag pass's row bands, fp32 and uint8 colour, normals with zero-length entries"""
    rng = np.random.default_rng(seed)
    depth = rng.uniform(1.2, 2.4, size=(V, H, W)).astype(F)
    hole = rng.uniform(size=depth.shape)
    for lo, value in ((0.00, 0.0), (0.03, np.nan), (0.05, np.inf), (0.07, -np.inf), (0.09, -1.5)):
        depth[(hole >= lo) & (hole < lo + 0.02 + 0.01 * (lo == 0))] = value
    mask = rng.choice(np.array([0.0, 0.25, 0.5, 0.75, 1.0], F), size=(V, H, W), p=[0.02, 0.02, 0.16, 0.2, 0.6]).astype(F)
    rows = ref.plan(V, H, W)[0]
    for y in sorted({0, H - 1} | {b + d for b in range(rows, H, rows) for d in (-1, 0)}):
        mask[:, y, rng.integers(0, W, size=3)] = 0                      # features on the band borders and the top and bottom edge
    mask[:, rng.integers(0, H, size=3), 0] = 0
    mask[:, rng.integers(0, H, size=3), W - 1] = 0
    mask[0, 0, 0] = mask[V - 1, H - 1, W - 1] = 0.25
    color = rng.uniform(size=(V, 3, H, W)).astype(F)
    color8 = rng.integers(0, 256, size=(V, 3, H, W), dtype=np.uint8)
    normal = rng.standard_normal((V, 3, H, W)).astype(F)
    normal[:, :, rng.integers(0, H, size=20), rng.integers(0, W, size=20)] = 0
    return depth, mask, color, color8, normal


@pytest.fixture(scope="module")
def ragged():
    """V = 3, 40 x 56: 56 divides neither 1024 nor 256, the bands are 18 rows (18, 18 and 4), a band is 3.9 trips of 256 lanes"""
    V, H, W = 3, 40, 56
    assert ref.plan(V, H, W) == (18, 3, 9) and (18 * W) % ref.THREADS != 0
    return (_cameras(V),) + _views(V, H, W, 1)


@pytest.mark.parametrize("erode,stride,kind,colour,normals,masked", [
    (0, 1, ref.DEPTH_Z, "f32", True, True), (1, 1, ref.DEPTH_RAY, "u8", False, True), (3, 1, ref.DEPTH_Z, "u8", True, True),
    (0, 3, ref.DEPTH_RAY, "f32", False, True), (1, 3, ref.DEPTH_Z, None, True, True), (3, 3, ref.DEPTH_RAY, "u8", True, True),
    (0, 1, ref.DEPTH_RAY, "u8", True, False)])
def test_unproject_matches_the_restatement_bit_for_bit(gpu_device, ragged, erode, stride, kind, colour, normals, masked):
    cam, depth, mask, color, color8, normal = ragged
    want = _check(gpu_device, depth, cam, mask=mask if masked else None, color={"f32": color, "u8": color8, None: None}[colour],
                  normal=normal if normals else None, depth_kind=kind, erode=erode, pixel_stride=stride, depth_min=0.0)
    n = want["count"]
    assert 0 < n < len(want["source"]) and (want["view_counts"] > 0).all()         # something kept, something dropped, in every view
    if masked and erode == 0 and stride == 1:
        on_threshold = (mask.reshape(-1)[want["source"][:n]] == 0.5).sum()
        assert on_threshold > 0                                                      # mask == threshold is foreground
    if normals:
        assert (want["normals"][:n] == (0, 0, 1)).all(1).any() or stride > 1         # a zero-length normal became (0, 0, 1)


def test_unproject_clip_boundary_and_exact_zero(gpu_device, ragged):
    """view 2 is replaced by an axis-aligned camera at (0, 0, -2) with camera-z depth: depth 2.5 puts z exactly on +clip = 0.5, 1.5 on
    -clip, 2 on exactly 0; beyond the boundary the clamp puts points on it.  All of them are dropped, and only them."""
    cam, depth, mask, color, color8, normal = ragged
    cam, depth = cam.copy(), np.abs(np.nan_to_num(depth, nan=1.7, posinf=1.7, neginf=1.7)) + F(0.25)
    cam[2] = 0
    cam[2, [0, 4, 8]] = 1
    cam[2, 11] = -2
    cam[2, 12:16] = (1.4, 1.4, 0.5, 0.5)
    depth[2] = np.random.default_rng(3).choice(np.array([1.5, 1.75, 2.0, 2.25, 2.5, 2.75], F), size=depth[2].shape)
    free = ref.lift_f32(depth, cam, ref.DEPTH_Z)
    assert (free[2, ..., 2] == 0.5).any() and (free[2, ..., 2] == -0.5).any() and (free[2, ..., 2] == 0).any() and (free[2, ..., 2] > 0.5).any()
    both = _check(gpu_device, depth, cam, color=color, depth_kind=ref.DEPTH_Z, clip=0.5, drop_zero=True)
    n = both["count"]
    kept = both["points"][:n]
    assert n > 0 and (np.abs(kept) < 0.5).all() and (kept != 0).all()
    v2 = both["source"][:n] >= 2 * 40 * 56
    assert v2.any() and np.isin(kept[v2, 2], (F(-0.25), F(0.25))).all()
    only_clip = _check(gpu_device, depth, cam, depth_kind=ref.DEPTH_Z, clip=0.5)
    assert (only_clip["points"][:only_clip["count"], 2] == 0).any() and only_clip["count"] > n
    only_zero = _check(gpu_device, depth, cam, depth_kind=ref.DEPTH_Z, drop_zero=True)
    assert (only_zero["points"][:only_zero["count"], 2] == 0.5).any()


def test_unproject_more_bands_than_one_trip_of_the_scan(gpu_device):
    """2 x 130 x 520: a row is wider than half a tile, so every band is one row and the flag pass has 260 workgroups -- more than the
    256 band counts (GA_PC_UNPROJECT_THREADS) one trip of the single scan workgroup covers; a row is also more than two trips wide"""
    V, H, W = 2, 130, 520
    assert ref.plan(V, H, W) == (1, 130, 260) and 260 > ref.THREADS and W > 2 * ref.THREADS
    depth, mask, color, color8, normal = _views(V, H, W, 2)
    _check(gpu_device, depth, _cameras(V), mask=mask, color=color8, normal=normal, depth_kind=ref.DEPTH_RAY, erode=2)


def test_unproject_capacity_and_empty(gpu_device, ragged):
    cam, depth, mask, color, color8, normal = ragged
    kw = dict(mask=mask, color=color, normal=normal, depth_kind=ref.DEPTH_RAY)
    full = _check(gpu_device, depth, cam, **kw)
    n = full["count"]
    exact = _check(gpu_device, depth, cam, capacity=n, **kw)                        # capacity == count: no padding row at all
    assert exact["count"] == n and (exact["source"] >= 0).all()
    for cap in (n - 1, n // 2, 1):                                                  # capacity < count: the prefix, and the true count
        short = _check(gpu_device, depth, cam, capacity=cap, **kw)
        assert short["count"] == n and np.array_equal(short["source"], full["source"][:cap])
        _same(short["points"], full["points"][:cap], "prefix")
    more = _check(gpu_device, depth, cam, capacity=n + 1500, **kw)                   # padding over more than one padding workgroup
    assert (more["source"][n:] == -1).all() and not more["points"][n:].any() and not more["normals"][n:].any()
    none = _check(gpu_device, depth, cam, mask=np.zeros_like(mask), color=color, normal=normal)
    assert none["count"] == 0 and not none["view_counts"].any() and (none["source"] == -1).all() and not none["points"].any()
    also_none = _check(gpu_device, depth, cam, depth_min=5.0)
    assert also_none["count"] == 0


def test_unproject_in_a_captured_graph(gpu_device, ragged):
    """captured once, replayed after the inputs changed in place: the replay has the bits of the restatement on the new inputs"""
    cam, depth, mask, color, color8, normal = ragged
    kw = dict(depth_kind=ref.DEPTH_RAY, erode=1, clip=0.6)
    with torch.cuda.device(gpu_device):
        raw = Raw(gpu_device, depth, cam, mask=mask, color=color8, normal=normal, **kw)
        side = torch.cuda.Stream(device=gpu_device)
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            raw.enqueue(side)          # warm-up on the capture stream
            side.synchronize()
            with torch.cuda.graph(graph, stream=side):
                raw.enqueue(side)
        torch.cuda.synchronize()
        first = raw.outputs()
        depth2, mask2, _, color82, normal2 = _views(3, 40, 56, 7)
        cam2 = cam.copy()
        cam2[:, 9:12] *= F(0.9)
        new = dict(depth=depth2, cam=cam2, mask=mask2, color=color82, normal=normal2)
        for k, v in new.items():
            raw.inp[k].copy_(torch.from_numpy(v))
        raw.host = new
        for t in (raw.points, raw.colors, raw.normals, raw.source, raw.count, raw.view_counts):
            t[:-GUARD] = POISON
        graph.replay()
        torch.cuda.synchronize()
        second = raw.outputs()
    for got, inputs in ((first, (depth, cam, mask, color8, normal)), (second, (depth2, cam2, mask2, color82, normal2))):
        d, c, m, c8, nm = inputs
        want = ref.unproject_f32(d, c, mask=m, color=c8, normal=nm, **kw)
        assert got["count"] == want["count"] and np.array_equal(got["view_counts"], want["view_counts"])
        assert np.array_equal(got["source"], want["source"])
        for k in ("points", "colors", "normals"):
            _same(got[k], want[k], k)
    assert first["count"] != second["count"]


# ---- the front ends --------------------------------------------------------------------------------------------------------------------------
def test_python_front_end_is_the_raw_call(gpu_device, ragged):
    from gaussiananything_amd import pointcloud
    cam, depth, mask, color, color8, normal = ragged
    t = lambda a: torch.from_numpy(a).to(gpu_device)
    out = pointcloud.unproject_depth_views(t(depth)[:, None], t(cam), mask=t(mask), color=t(color8), normal=t(normal), depth_kind="ray",
                                           depth_range=(1.3, 2.3), erode=1, clip=0.7, drop_zero=True, pixel_stride=2)
    want = ref.unproject_f32(depth, cam, mask=mask, color=color8, normal=normal, depth_kind=ref.DEPTH_RAY, depth_min=1.3, depth_max=2.3,
                             erode=1, clip=0.7, drop_zero=True, pixel_stride=2)
    assert out.capacity == pointcloud.unproject_candidates(3, 40, 56, 2) == len(want["source"])
    assert int(out.count.item()) == want["count"] and np.array_equal(out.view_counts.cpu().numpy(), want["view_counts"])
    assert np.array_equal(out.source.cpu().numpy(), want["source"])
    for k in ("points", "colors", "normals"):
        _same(getattr(out, k).cpu().numpy(), want[k], k)
    cut = out.trimmed()
    assert cut.points.shape[0] == want["count"] == cut.source.shape[0] and cut.points.data_ptr() == out.points.data_ptr()
    small = pointcloud.unproject_depth_views(t(depth), t(cam), capacity=10)
    with pytest.raises(RuntimeError, match="capacity"):
        small.trimmed()


def test_cloud_from_render_lies_on_the_rendered_surfels(gpu_device):
    """256 opaque surfels far smaller than a pixel on a jittered lattice facing between two cameras, 2 views x 64 x 64.  Such a surfel
    is drawn by the rasterizer's screen-space low-pass filter with the depth of its CENTRE, so a pixel it dominates unprojects to the
    pixel's ray at the centre's depth: within the pixel's footprint 2 * tanfov * z / S of the centre when the pixel centre is within
    one pixel of the projected centre -- which alpha >= 0.75 of an opacity-0.99 surfel (exp(-r^2) >= 0.75: r <= 0.54 px) ensures."""
    from gaussiananything_amd import pointcloud, synthetic
    from gaussiananything_amd.gs_surfel import GaussianRenderer2DGS
    S, V = 64, 2
    cams = synthetic.eval_cameras(8)
    cv, cvp, cp = (cams[k][:V].to(gpu_device) for k in ("cam_view", "cam_view_proj", "cam_pos"))
    tanfov = cams["tanfov"]
    rng = np.random.default_rng(4)
    nrm = cams["cam_pos"][:V].numpy().astype(np.float64).sum(0)
    nrm /= np.linalg.norm(nrm)
    e1 = np.cross(nrm, [0.3, 0.5, 0.8]); e1 /= np.linalg.norm(e1)
    e2 = np.cross(nrm, e1)
    a, b = np.meshgrid(np.arange(16) - 7.5, np.arange(16) - 7.5, indexing="ij")
    a, b = a.reshape(-1) * 0.055 + rng.uniform(-0.004, 0.004, 256), b.reshape(-1) * 0.055 + rng.uniform(-0.004, 0.004, 256)
    centres = a[:, None] * e1 + b[:, None] * e2 + (0.04 * np.sin(5 * a) * np.cos(4 * b))[:, None] * nrm
    g = torch.zeros(1, 256, 13)
    g[0, :, 0:3] = torch.from_numpy(centres).float()
    g[0, :, 3] = 0.99
    g[0, :, 4:6] = 1e-4
    g[0, :, 6] = 1.0
    g[0, :, 10:13] = torch.from_numpy(rng.uniform(0.1, 0.9, size=(256, 3))).float()
    with torch.no_grad():
        out = GaussianRenderer2DGS(S, 3, {}).render(g.to(gpu_device), cv[None], cvp[None], cp[None], tanfov)
    cloud = pointcloud.cloud_from_render(out, cv[None], tanfov, mask_threshold=0.75).trimmed()
    n = cloud.points.shape[0]
    assert n >= 256 and cloud.colors.shape == (n, 3) and cloud.normals.shape == (n, 3)      # most surfels seen, in both views
    pts = cloud.points.double().cpu().numpy()
    z = out["depth"][0].reshape(-1)[cloud.source.long()].double().cpu().numpy()
    dist = np.sqrt(((pts[:, None, :] - g[0, :, 0:3].double().numpy()[None]) ** 2).sum(-1)).min(1)
    footprint = 2.0 * tanfov * z / S
    print(f"cloud_from_render: {n} points, worst distance to a surfel centre {float((dist / footprint).max()):.3f} pixel footprints")
    assert (dist <= footprint).all()
    assert np.abs(np.linalg.norm(cloud.normals.cpu().numpy(), axis=1) - 1).max() < 1e-5
    colours = out["image"][0].permute(0, 2, 3, 1).reshape(-1, 3)[cloud.source.long()]
    assert torch.equal(cloud.colors, colours)


def test_export_fps_points_from_depth(gpu_device, tmp_path):
    """the golden inputs of the CPU tests through the hand-off: the vertices written are ``sample_farthest_points`` of the
    restatement's cloud"""
    import os
    from gaussiananything_amd import io_formats, pointcloud
    z = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unproject_ref.pt"))
    c, depth, alpha, K = z["c"].numpy(), z["depth"].numpy(), z["alpha_mask"].numpy(), int(z["K"])
    lo = float(np.nextafter(F(1.05), F(-np.inf)))
    want = ref.unproject_f32(depth, ref.cameras_from_pose25(c), mask=(alpha == 1).astype(F), depth_kind=ref.DEPTH_RAY, depth_min=lo,
                             clip=0.45, drop_zero=True)
    cloud = torch.from_numpy(want["points"][:want["count"]]).to(gpu_device)
    fps = pointcloud.sample_farthest_points(cloud[None], K=K)[0][0].cpu().numpy()
    path = tmp_path / f"fps-{K}.ply"
    got = io_formats.export_fps_points_from_depth(z["depth"], z["c"], str(path), K=K, alpha_mask=z["alpha_mask"])
    _same(got, fps, "returned points")
    _same(io_formats.load_points_ply(str(path)), fps, "written vertices")


@pytest.fixture(scope="module")
def rgbd_scene(gpu_device):
    """the synthetic scene of tests/test_fit_gpu.py (2 views x 64 x 64) with its rendered depth"""
    from gaussiananything_amd import synthetic
    from gaussiananything_amd.gs_surfel import GaussianRenderer2DGS
    from tests.test_fit_gpu import _scene
    sc = _scene(gpu_device)
    g = synthetic.random_surfels(1000, seed=3)
    g[..., 4:6] *= 6.0
    with torch.no_grad():
        out = GaussianRenderer2DGS(64, 3, {}).render(g.to(gpu_device), sc["cv"][None], sc["cvp"][None], sc["cp"][None], sc["tanfov"])
    sc["depth"] = out["depth"][0].contiguous()
    return sc


def test_fitter_from_rgbd(gpu_device, rgbd_scene):
    from gaussiananything_amd import fitting
    from tests.test_fit_gpu import LAMBDAS, LR
    sc = rgbd_scene
    depth = sc["depth"].cpu().numpy()[:, 0]
    cam = ref.cameras_from_view(sc["cv"].cpu().numpy(), sc["tanfov"])
    want = ref.unproject_f32(depth, cam, mask=sc["mask"].cpu().numpy()[:, 0], pixel_stride=2)
    assert want["count"] > 100
    f = fitting.SurfelFitter.from_rgbd(sc["depth"], sc["cv"], sc["cvp"], sc["tanfov"], sc["targets"], mask=sc["mask"], pixel_stride=2,
                                       K=8, opacity=0.3, max_steps=64, lr=LR, **LAMBDAS)
    assert isinstance(f, fitting.SurfelFitter) and f.num_points == want["count"] and f.steps == 0
    f.step(5)
    h = f.loss_history()["loss"]
    assert len(h) == 5 and np.isfinite(h).all() and f.steps == 5 and bool(torch.isfinite(f.gaussians()).all())


def test_from_rgbd_refuses_more_points_than_max_points(gpu_device, rgbd_scene):
    from gaussiananything_amd import fitting
    sc = rgbd_scene
    with pytest.raises(ValueError, match="pixel_stride=") as e:
        fitting.SurfelFitter.from_rgbd(sc["depth"], sc["cv"], sc["cvp"], sc["tanfov"], sc["targets"], mask=sc["mask"], max_points=500)
    assert "max_points=500" in str(e.value)
