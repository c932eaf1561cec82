"""GPU tests of ``ga_pc_filter_views`` and ``ga_pc_voxel_thin`` (include/ga_pointcloud.h, csrc/pc_filter.hip) and of what is built on them.

Every raw C-ABI call is compared with the numpy float32 restatement (tests/_pc_filter_ref.py) for EQUALITY, bit for bit: rows,
``kept_rows``, counts, votes, multiplicities and padding.  Every raw call poisons its outputs first, checks guard words behind each of
them and behind the workspace, and that its inputs are unchanged.  The front ends follow."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _pc_filter_ref as ref
from tests import _unproject_ref as uref

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 64            # int32 words behind every buffer
GUARD_WORD = 0x5A5A5A5A
POISON = -77          # as a float: a NaN pattern no arithmetic here produces


def _guarded(n_words, device):
    t = torch.full((n_words + GUARD,), GUARD_WORD, dtype=torch.int32, device=device)
    t[:n_words] = POISON
    return t


def _take(buf, n, shape, dtype=torch.float32, written=True):
    assert bool((buf[n:] == GUARD_WORD).all()), "guard words overwritten"
    if written:
        assert not bool((buf[:n] == POISON).any()), "an output element was not written"
    return buf[:n].view(dtype).reshape(shape).cpu().numpy()


def _same(got, want, what):
    a, b = np.ascontiguousarray(got, F).view(np.uint32), np.ascontiguousarray(want, F).view(np.uint32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = a != b
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ in bits, first at {np.argwhere(bad)[0].tolist()}"


class Raw:
    """one bound ``ga_pc_filter_views`` (``depth`` given) or ``ga_pc_voxel_thin`` call: device copies of the inputs, guarded outputs and
    workspace; ``enqueue`` launches on a stream, ``outputs`` reads back after the checks"""

    def __init__(self, device, points, colors=None, normals=None, source=None, in_count=None, capacity=None, depth=None, cam=None,
                 mask=None, num_views=None, view_pixels=None, table_slots=0, votes=True, **scalars):
        from gaussiananything_amd import _lib
        self._lib, self.L, self.device = _lib, _lib.lib(), device
        self.rows = rows = points.shape[0]
        self.cap = cap = rows if capacity is None else int(capacity)
        self.filter = depth is not None
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device) if a is not None else None
        self.host = dict(points=points, colors=colors, normals=normals, source=source, depth=depth, cam=cam, mask=mask,
                         in_count=None if in_count is None else np.array([in_count], np.int32))
        self.inp = {k: dev(v) for k, v in self.host.items()}
        g = lambda n, on=True: _guarded(n, device) if on else None
        self.V = depth.shape[0] if self.filter else num_views
        want_views = source is not None and self.V is not None
        self.out = dict(points=g(cap * 3), colors=g(cap * 3, colors is not None), normals=g(cap * 3, normals is not None),
                        source=g(cap, source is not None), kept_rows=g(cap), count=g(1), view_counts=g(self.V or 1, want_views))
        p = lambda t: t.data_ptr() if t is not None else None
        i, o = self.inp, self.out
        if self.filter:
            self.votes = votes
            self.support, self.conflicts = g(-(-rows // 4), votes), g(-(-rows // 4), votes)
            self.ws_bytes = int(self.L.ga_pc_filter_views_workspace_bytes(rows))
        else:
            self.mult, self.dropped = g(cap), g(1)
            self.ws_bytes = int(self.L.ga_pc_voxel_thin_workspace_bytes(rows, table_slots))
        assert self.ws_bytes > 0 and self.ws_bytes % 16 == 0
        self.ws = _guarded(self.ws_bytes // 4, device)
        cloud = (p(i["in_count"]), p(i["points"]), p(i["colors"]), p(i["normals"]), p(i["source"]))
        outs = tuple(p(o[k]) for k in ("points", "colors", "normals", "source", "kept_rows", "count", "view_counts"))
        if self.filter:
            V, H, W = depth.shape
            s = dict(depth_kind=ref.DEPTH_Z, window=1, min_support=1, max_conflicts=0, carve=0, depth_min=0.0, depth_max=np.inf,
                     mask_threshold=0.5, tol_abs=0.0, tol_rel=0.01)
            s.update(scalars)
            self.args = _lib.GaFilterViewsArgs(rows, cap, V, H, W, s["depth_kind"], s["window"], s["min_support"], s["max_conflicts"],
                                               int(s["carve"]), s["depth_min"], s["depth_max"], s["mask_threshold"], s["tol_abs"],
                                               s["tol_rel"], 0, *cloud, p(i["depth"]), p(i["mask"]), p(i["cam"]), *outs,
                                               p(self.support), p(self.conflicts), p(self.ws), self.ws_bytes)
            self.call, self.name = self.L.ga_pc_filter_views, "ga_pc_filter_views"
        else:
            s = dict(keep=ref.VOXEL_CENTER, origin=(0.0, 0.0, 0.0), voxel_size=0.1, flags=0)
            s.update(scalars)
            self.args = _lib.GaVoxelThinArgs(rows, cap, s["keep"], num_views or 0, view_pixels or 0, s["flags"], (ctypes.c_float * 3)(*s["origin"]),
                                             s["voxel_size"], table_slots, *cloud, *outs, p(self.mult), p(self.dropped), p(self.ws),
                                             self.ws_bytes)
            self.call, self.name = self.L.ga_pc_voxel_thin, "ga_pc_voxel_thin"

    def enqueue(self, stream):
        self._lib.check(self.call(ctypes.byref(self.args), ctypes.c_void_p(stream.cuda_stream)), self.name)

    def poison(self):
        for t in list(self.out.values()) + ([self.support, self.conflicts] if self.filter else [self.mult, self.dropped]):
            if t is not None:
                t[:-GUARD] = POISON

    def outputs(self):
        cap, o = self.cap, self.out
        assert bool((self.ws[self.ws_bytes // 4:] == GUARD_WORD).all()), "guard words behind the workspace overwritten"
        f3 = lambda t: _take(t, cap * 3, (cap, 3)) if t is not None else None
        i1 = lambda t, n: _take(t, n, (n,), torch.int32) if t is not None else None
        out = dict(points=f3(o["points"]), colors=f3(o["colors"]), normals=f3(o["normals"]), source=i1(o["source"], cap),
                   kept_rows=i1(o["kept_rows"], cap), count=int(i1(o["count"], 1)[0]), view_counts=i1(o["view_counts"], self.V or 1))
        if self.filter:
            for k, t in (("support", self.support), ("conflicts", self.conflicts)):
                n = -(-self.rows // 4)
                out[k] = _take(t, n, (n * 4,), torch.uint8, written=False)[:self.rows] if t is not None else None
        else:
            out["multiplicity"], out["dropped"] = i1(self.mult, cap), int(i1(self.dropped, 1)[0])
        for k, v in self.host.items():                       # the inputs are left alone
            if v is not None:
                assert np.array_equal(self.inp[k].cpu().numpy().view(np.uint8), np.ascontiguousarray(v).view(np.uint8)), k
        return out


def _equal(got, want):
    """every output of a raw call against the restatement's dict"""
    assert got["count"] == want["count"], (got["count"], want["count"])
    assert np.array_equal(got["kept_rows"], want["kept_rows"]), "kept_rows"
    for k in ("points", "colors", "normals"):
        assert (got[k] is None) == (want[k] is None), k
        if want[k] is not None:
            _same(got[k], want[k], k)
    for k in ("source", "view_counts", "support", "conflicts", "multiplicity"):
        if got.get(k) is not None:
            assert np.array_equal(got[k], want[k]), (k, got[k][:8], want[k][:8])
    if "dropped" in got:
        assert got["dropped"] == want["dropped"], (got["dropped"], want["dropped"])


def _run(device, points, **kw):
    with torch.cuda.device(device):
        r = Raw(device, points, **kw)
        r.enqueue(torch.cuda.current_stream())
        torch.cuda.synchronize()
        return r.outputs()


_RULE = ("depth_kind", "depth_min", "depth_max", "mask_threshold", "tol_abs", "tol_rel", "window", "carve")


def _check_filter(device, sc, rows=None, colors=True, normals=True, source=True, mask=True, votes=True, **kw):
    """the raw filter call on the first ``rows`` rows of a scene against the restatement -> the restatement's dict"""
    n = sc["points"].shape[0] if rows is None else rows
    cloud = dict(colors=sc["colors"][:n] if colors else None, normals=sc["normals"][:n] if normals else None,
                 source=sc["source"][:n] if source else None)
    got = _run(device, sc["points"][:n], depth=sc["depth"], cam=sc["cam"], mask=sc["mask"] if mask else None, votes=votes, **cloud, **kw)
    want = ref.filter_views_f32(sc["points"][:n], sc["depth"], sc["cam"], mask=sc["mask"] if mask else None,
                                want_view_counts=source, **cloud, **kw)
    _equal(got, want)
    return want


def _check_voxel(device, points, **kw):
    """the raw thinning call, with the plain and with the wave-merged insert, against the restatement -> the restatement's dict"""
    got = _run(device, points, **kw)
    merged = _run(device, points, flags=1, **kw)
    want = ref.voxel_thin_f32(points, kw.pop("voxel_size", 0.1), kw.pop("origin", (0.0, 0.0, 0.0)), kw.pop("keep", ref.VOXEL_CENTER),
                              **{k: v for k, v in kw.items() if k != "table_slots"})
    _equal(got, want)
    _equal(merged, want)
    return want


# ---- the filter --------------------------------------------------------------------------------------------------------------------------
def _filter_scene(depth_kind=ref.DEPTH_Z, seed=5):
    """3 views of 40 x 56 of the two spheres: two from the ring (view 1 with skew, unequal focal lengths and an off-centre principal
    point), view 2 axis-aligned at (0, 0, -1.5) so that points can be put exactly on its image border and on its q_z = 0 plane.
    Floaters in 3 % of the surface pixels; the cloud is unprojected from these maps, THEN the maps get holes (0, NaN, +-inf, negative)
    and the mask values on the threshold.  Rows appended without a source: on the border, on q_z = 0, behind, far outside, NaN, and points lifted off the surface."""
    V, H, W = 3, 40, 56
    cam = ref.ring_cameras(8)[:3].copy()
    cam[1, 13] *= F(1.1)
    cam[1, 14:17] = (0.47, 0.54, 0.03)
    cam[2] = 0
    cam[2, [0, 4, 8]] = 1
    cam[2, 11] = -1.5
    cam[2, 12:16] = (2.0, 2.0, 0.5, 0.5)
    z = ref.raycast_z(cam, H, W)
    if depth_kind == ref.DEPTH_RAY:                                                  # distance along the normalised ray
        unit = uref.lift_f64(np.ones_like(z), cam, ref.DEPTH_Z) - cam[:, None, None, 9:12].astype(np.float64)
        z = (z.astype(np.float64) * np.linalg.norm(unit, axis=-1)).astype(F)
    depth, floater = ref.add_floaters(z, 0.03, seed=seed)
    rng = np.random.default_rng(seed)
    color = rng.uniform(size=(V, 3, H, W)).astype(F)
    normal = rng.standard_normal((V, 3, H, W)).astype(F)
    cloud = uref.unproject_f32(depth, cam, color=color, normal=normal, depth_kind=depth_kind)
    n = cloud["count"]
    extra = np.array([[-0.5, 0.0, 0.5], [0.5, 0.0, 0.5], [0.0, -0.5, 0.5], [0.0, 0.5, 0.5],      # a = 0, a = W, b = 0, b = H in view 2
                      [0.1, 0.1, -1.5], [0.0, 0.0, -2.0], [3.0, 3.0, 3.0], [np.nan, 0.0, 0.0]], F)
    lifted = (cloud["points"][:n:12] * F(1.12)).astype(F)                             # just off the large sphere: in front of what a view sees
    extra = np.concatenate([extra, lifted])
    pts = np.concatenate([cloud["points"][:n], extra])
    m = len(pts)
    hole = rng.uniform(size=depth.shape)
    for lo, value in ((0.00, 0.0), (0.01, np.nan), (0.02, np.inf), (0.03, -np.inf), (0.04, -1.5)):
        depth[(hole >= lo) & (hole < lo + 0.01)] = value
    mask = rng.choice(np.array([0.0, 0.25, 0.5, 0.75, 1.0], F), size=(V, H, W), p=[0.02, 0.02, 0.16, 0.2, 0.6]).astype(F)
    return dict(cam=cam, depth=depth, mask=mask, points=pts, colors=rng.uniform(size=(m, 3)).astype(F),
                normals=rng.standard_normal((m, 3)).astype(F), source=np.concatenate([cloud["source"][:n], np.full(len(extra), -1, np.int32)]),
                floater=np.concatenate([floater.reshape(-1)[cloud["source"][:n]], np.zeros(len(extra), bool)]), n=n)


@pytest.fixture(scope="module")
def scene_z():
    return _filter_scene(ref.DEPTH_Z)


@pytest.fixture(scope="module")
def scene_ray():
    return _filter_scene(ref.DEPTH_RAY)


def test_filter_scene_has_every_class(scene_z, scene_ray):
    """the premise of the bit comparisons below: every kind of answer a view can give occurs, and the border points land where intended"""
    for sc, kind in ((scene_z, ref.DEPTH_Z), (scene_ray, ref.DEPTH_RAY)):
        assert sc["points"].shape[0] > 2 * ref.BAND_ROWS                             # more than one band, the last one partial
        for mask in (sc["mask"], None):
            for window in (0, 1):
                s, c, cls = ref.votes_f32(sc["points"], sc["depth"], sc["cam"], source=sc["source"], mask=mask, depth_kind=kind, window=window)
                want = {ref.SKIPPED_OWN, ref.BEHIND, ref.OUTSIDE, ref.SUPPORT, ref.CONFLICT, ref.OCCLUDED}
                assert want | ({ref.UNDECIDED} if window else set()) <= set(np.unique(cls).tolist()), (kind, window)
                assert s.max() == 2 and c.max() >= 1
        cls = ref.votes_f32(sc["points"], sc["depth"], sc["cam"], source=sc["source"], depth_kind=kind, carve=True)[2]
        assert (cls == ref.CARVED).any()
        n = sc["n"]
        assert cls[n, 2] not in (ref.OUTSIDE, ref.BEHIND) and cls[n + 2, 2] not in (ref.OUTSIDE, ref.BEHIND)      # a = 0, b = 0: inside
        assert cls[n + 1, 2] == ref.OUTSIDE and cls[n + 3, 2] == ref.OUTSIDE                                       # a = W, b = H: outside
        assert cls[n + 4, 2] == ref.BEHIND and cls[n + 5, 2] == ref.BEHIND and (cls[n + 7] == ref.BEHIND).all()  # q_z = 0, < 0, NaN


@pytest.mark.parametrize("kind,mask,window,carve,min_support,max_conflicts", [
    ("z", True, 1, 0, 1, 0), ("ray", True, 1, 0, 1, 0), ("z", False, 1, 0, 1, 0), ("ray", False, 0, 1, 2, 1), ("z", True, 0, 0, 0, 0),
    ("z", True, 1, 1, 1, 1), ("ray", True, 0, 1, 0, 1), ("z", False, 0, 0, 2, 0), ("ray", True, 1, 0, 2, 1)])
def test_filter_matches_the_restatement_bit_for_bit(gpu_device, scene_z, scene_ray, kind, mask, window, carve, min_support, max_conflicts):
    sc = scene_z if kind == "z" else scene_ray
    want = _check_filter(gpu_device, sc, mask=mask, depth_kind=ref.DEPTH_Z if kind == "z" else ref.DEPTH_RAY, window=window, carve=carve,
                         min_support=min_support, max_conflicts=max_conflicts)
    assert 0 < want["count"] < sc["points"].shape[0] and want["view_counts"].sum() <= want["count"]
    if mask and window == 1 and not carve:
        on_threshold = sc["mask"] == 0.5                                              # mask == threshold is surface
        assert on_threshold.any()


def test_filter_foreign_cloud_and_optional_outputs(gpu_device, scene_z):
    """no source: every view votes, no view_counts; colours, normals and votes on and off"""
    own = _check_filter(gpu_device, scene_z, min_support=2)
    foreign = _check_filter(gpu_device, scene_z, source=False, colors=False, min_support=2)
    assert foreign["source"] is None and foreign["view_counts"] is None and foreign["count"] > own["count"]
    _check_filter(gpu_device, scene_z, normals=False, votes=False)
    _check_filter(gpu_device, scene_z, source=False, colors=False, normals=False, mask=False)


def test_filter_in_count_capacity_and_empty(gpu_device, scene_z):
    rows = scene_z["points"].shape[0]
    full = _check_filter(gpu_device, scene_z)
    n = full["count"]
    for in_count in (rows - 700, rows, rows + 5, 1, 0, -3):                           # below, at and above the rows; nothing live
        got = _check_filter(gpu_device, scene_z, in_count=in_count)
        assert got["count"] <= n and (in_count > 0 or (got["count"] == 0 and (got["kept_rows"] == -1).all() and not got["points"].any()))
    for cap in (n, n - 1, n // 2, 1, n + 1500):                                       # at, below and above the kept count
        got = _check_filter(gpu_device, scene_z, capacity=cap)
        assert got["count"] == n and np.array_equal(got["kept_rows"][:min(cap, n)], full["kept_rows"][:min(cap, n)])
        assert np.array_equal(got["view_counts"], full["view_counts"])                # the true counts, even past the capacity
    none = _check_filter(gpu_device, scene_z, depth_min=50.0, min_support=1)          # no surface anywhere: nothing is supported
    assert none["count"] == 0
    _check_filter(gpu_device, scene_z, rows=1)
    _check_filter(gpu_device, scene_z, rows=ref.BAND_ROWS)
    _check_filter(gpu_device, scene_z, rows=ref.BAND_ROWS + 1)


# ---- the thinning ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cloud5000():
    """5000 points in about 300 cells of 0.1: duplicates, points exactly on cell faces, negative coordinates, NaN, inf and
    out-of-range rows"""
    rng = np.random.default_rng(11)
    p = rng.uniform(-0.35, 0.35, size=(5000, 3)).astype(F)
    p[100:140] = p[60:100]
    p[200:230] = (np.round(p[200:230] / F(0.1)) * F(0.1)).astype(F)
    p[300], p[301], p[302], p[303] = (np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (0, 2e5, 0)
    return dict(points=p, colors=rng.uniform(size=(5000, 3)).astype(F), normals=rng.standard_normal((5000, 3)).astype(F),
                source=np.sort(rng.choice(4 * 2500, size=5000, replace=False)).astype(np.int32))


@pytest.mark.parametrize("keep", [ref.VOXEL_FIRST, ref.VOXEL_CENTER])
def test_voxel_matches_the_restatement_bit_for_bit(gpu_device, cloud5000, keep):
    c = cloud5000
    want = _check_voxel(gpu_device, c["points"], colors=c["colors"], normals=c["normals"], source=c["source"], num_views=4, view_pixels=2500,
                        keep=keep, voxel_size=0.1, origin=(0.013, -0.02, 0.0))
    n = want["count"]
    assert 200 < n < 600 and want["dropped"] == 4 and want["multiplicity"][:n].sum() == 4996 and want["view_counts"].sum() == n
    assert not np.isin(np.arange(100, 140), want["kept_rows"]).any()                 # of duplicated points the lowest row wins
    bare = _check_voxel(gpu_device, c["points"], keep=keep, voxel_size=0.1, origin=(0.013, -0.02, 0.0))
    assert bare["colors"] is None and bare["source"] is None and np.array_equal(bare["kept_rows"], want["kept_rows"])
    _check_voxel(gpu_device, c["points"], colors=c["colors"], keep=keep, voxel_size=0.05)


def test_voxel_contention_and_table_edges(gpu_device, cloud5000):
    rng = np.random.default_rng(2)
    one_cell = rng.uniform(0.01, 0.09, size=(5000, 3)).astype(F)                     # every point in ONE cell: maximum contention
    for keep in (ref.VOXEL_FIRST, ref.VOXEL_CENTER):
        want = _check_voxel(gpu_device, one_cell, keep=keep, voxel_size=0.1)
        assert want["count"] == 1 and want["multiplicity"][0] == 5000
    g = np.stack(np.meshgrid(np.arange(17), np.arange(17), np.arange(18), indexing="ij"), -1).reshape(-1, 3)
    own_cell = ((g[:5000] + 0.5) * 0.1 - 0.8).astype(F)                              # every point in its own cell, default table size
    want = _check_voxel(gpu_device, own_cell, voxel_size=0.1)
    assert want["count"] == 5000 and (want["multiplicity"] == 1).all()
    want = _check_voxel(gpu_device, own_cell[:1023], voxel_size=0.1, table_slots=1024)   # 1023 cells in 1024 slots: probes wrap round
    assert want["count"] == 1023
    want = _check_voxel(gpu_device, np.concatenate([own_cell[:1000], own_cell[:23]]), voxel_size=0.1, table_slots=1024)
    assert want["count"] == 1000
    faces = np.array([[0.0, 0.0, 0.0], [-0.0, 0.25, 0.5], [-1e-9, 0.0, 0.0], [0.5, 0.5, 0.5], [-0.5, -0.5, -0.5], [-0.5000001, 0, 0],
                      [ref.MAX_INDEX / 2 + 0.25, 0, 0], [ref.MAX_INDEX / 2 + 0.5, 0, 0], [-ref.MAX_INDEX / 2, 0, 0], [-ref.MAX_INDEX / 2 - 0.25, 0, 0]], F)
    want = _check_voxel(gpu_device, faces, voxel_size=0.5)
    assert want["count"] == 8 and want["dropped"] == 2
    one = _check_voxel(gpu_device, cloud5000["points"][:1], colors=cloud5000["colors"][:1], voxel_size=0.1)
    assert one["count"] == 1
    assert _check_voxel(gpu_device, cloud5000["points"][300:301], voxel_size=0.1)["count"] == 0      # the one row is NaN: dropped
    for in_count in (0, -1, 2500, 5000, 6000):
        want = _check_voxel(gpu_device, cloud5000["points"], in_count=in_count, voxel_size=0.1)
        assert in_count > 0 or (want["count"] == 0 and want["dropped"] == 0)
    n = _check_voxel(gpu_device, cloud5000["points"], voxel_size=0.1)["count"]
    for cap in (n, n - 1, 1, n + 1500):
        assert _check_voxel(gpu_device, cloud5000["points"], normals=cloud5000["normals"], voxel_size=0.1, capacity=cap)["count"] == n


def test_voxel_more_bands_than_one_trip_of_the_scan(gpu_device):
    """266 241 rows: 260 full bands and one row, more than the 256 band counts one trip of the scan covers; one cell per 7 rows"""
    rows = 260 * ref.BAND_ROWS + 1
    assert ref.plan(rows) == (261, 2)
    cell = np.arange(rows) // 7
    rng = np.random.default_rng(3)
    order = rng.permutation(rows)                                                    # the rows of a cell lie anywhere in the cloud
    i = np.stack([cell % 40, (cell // 40) % 40, cell // 1600], 1)[order]
    p = ((i + rng.uniform(0.05, 0.95, size=(rows, 3))) * 0.02 - 0.4).astype(F)
    want = _check_voxel(gpu_device, p, voxel_size=0.02, origin=(-0.4, -0.4, -0.4), colors=p)
    assert want["count"] == (rows + 6) // 7 and want["dropped"] == 0
    inv = np.argsort(order)                                                          # cell by cell: runs of 7 equal keys that cross waves
    want = _check_voxel(gpu_device, p[inv], voxel_size=0.02, origin=(-0.4, -0.4, -0.4), keep=ref.VOXEL_FIRST)
    assert want["count"] == (rows + 6) // 7 and np.array_equal(want["kept_rows"][:want["count"]], np.arange(0, rows, 7))


# ---- both: captured graphs ---------------------------------------------------------------------------------------------------------------
def test_both_in_a_captured_graph(gpu_device, scene_z, cloud5000):
    """captured once, replayed after the inputs and in_count changed in place: the replay has the bits of the restatement on the new
    inputs"""
    sc, c = scene_z, cloud5000
    rows = sc["points"].shape[0]
    with torch.cuda.device(gpu_device):
        flt = Raw(gpu_device, sc["points"], colors=sc["colors"], source=sc["source"], depth=sc["depth"], cam=sc["cam"], mask=sc["mask"],
                  in_count=rows, carve=1, max_conflicts=1)
        vox = Raw(gpu_device, c["points"], normals=c["normals"], in_count=5000, voxel_size=0.1)
        side = torch.cuda.Stream(device=gpu_device)
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            flt.enqueue(side)
            vox.enqueue(side)
            side.synchronize()
            with torch.cuda.graph(graph, stream=side):
                flt.enqueue(side)
                vox.enqueue(side)
        torch.cuda.synchronize()
        first = flt.outputs(), vox.outputs()
        sc2 = _filter_scene(ref.DEPTH_Z, seed=9)
        m = min(rows, sc2["points"].shape[0])
        new_f = dict(points=np.ascontiguousarray(np.resize(sc2["points"], (rows, 3))), colors=sc["colors"][::-1].copy(),
                     source=np.ascontiguousarray(np.resize(sc2["source"], rows)), depth=sc2["depth"], cam=sc2["cam"], mask=sc2["mask"],
                     in_count=np.array([m - 300], np.int32), normals=None)
        new_v = dict(points=np.ascontiguousarray(c["points"][::-1] * F(1.3)), normals=c["normals"], in_count=np.array([3000], np.int32),
                     colors=None, source=None, depth=None, cam=None, mask=None)
        for raw, new in ((flt, new_f), (vox, new_v)):
            for k, v in new.items():
                if v is not None:
                    raw.inp[k].copy_(torch.from_numpy(v))
            raw.host = new
            raw.poison()
        graph.replay()
        torch.cuda.synchronize()
        second = flt.outputs(), vox.outputs()
    old_f = dict(points=sc["points"], colors=sc["colors"], source=sc["source"], depth=sc["depth"], cam=sc["cam"], mask=sc["mask"], in_count=[rows])
    old_v = dict(points=c["points"], normals=c["normals"], in_count=[5000])
    for (gf, gv), f, v in ((first, old_f, old_v), (second, new_f, new_v)):
        _equal(gf, ref.filter_views_f32(f["points"], f["depth"], f["cam"], colors=f["colors"], source=f["source"], mask=f["mask"],
                                        in_count=int(f["in_count"][0]), carve=1, max_conflicts=1))
        _equal(gv, ref.voxel_thin_f32(v["points"], 0.1, normals=v["normals"], in_count=int(v["in_count"][0])))
    assert first[0]["count"] != second[0]["count"] and first[1]["count"] != second[1]["count"]


def _t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device) if a is not None else None


def test_unproject_filter_thin_in_one_captured_graph(gpu_device, scene_z):
    """``unproject_depth_views`` -> ``filter_view_consistency`` -> ``voxel_thin`` on the UNTRIMMED clouds inside one captured graph (no
    host read anywhere), against the chained restatements"""
    from gaussiananything_amd import pointcloud as pc
    sc = scene_z
    rng = np.random.default_rng(1)
    depth = sc["depth"].copy()
    color = rng.uniform(size=(3, 3, 40, 56)).astype(F)
    d, cam, mask, col = (_t(a, gpu_device) for a in (depth, sc["cam"], sc["mask"], color))

    def chain():
        a = pc.unproject_depth_views(d, cam, mask=mask, color=col)
        b = pc.filter_view_consistency(a, d, cam, mask=mask, return_votes=True, min_support=1)
        return a, b, pc.voxel_thin(b, 0.03, view_pixels=40 * 56)

    def restated(depth):
        a = uref.unproject_f32(depth, sc["cam"], mask=sc["mask"], color=color)
        b = ref.filter_views_f32(a["points"], depth, sc["cam"], colors=a["colors"], source=a["source"], mask=sc["mask"], in_count=a["count"])
        c = ref.voxel_thin_f32(b["points"], 0.03, colors=b["colors"], source=b["source"], in_count=b["count"], num_views=3, view_pixels=40 * 56)
        return a, b, c

    def compare(got, want):
        for g, w in zip(got[1:], want[1:]):
            assert int(g.count.item()) == w["count"] > 0
            assert np.array_equal(g.kept_rows.cpu().numpy(), w["kept_rows"]) and np.array_equal(g.source.cpu().numpy(), w["source"])
            assert np.array_equal(g.view_counts.cpu().numpy(), w["view_counts"])
            _same(g.points.cpu().numpy(), w["points"], "points")
            _same(g.colors.cpu().numpy(), w["colors"], "colors")
        assert np.array_equal(got[1].support.cpu().numpy(), want[1]["support"]) and np.array_equal(got[1].conflicts.cpu().numpy(), want[1]["conflicts"])
        assert np.array_equal(got[2].multiplicity.cpu().numpy(), want[2]["multiplicity"]) and int(got[2].dropped.item()) == want[2]["dropped"]

    with torch.cuda.device(gpu_device):
        side = torch.cuda.Stream(device=gpu_device)
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            chain()
            side.synchronize()
            with torch.cuda.graph(graph, stream=side):
                got = chain()
        graph.replay()
        torch.cuda.synchronize()
        compare(got, restated(depth))
        depth2 = np.where(depth > 0, depth * F(1.02), depth).astype(F)
        depth2[0, :10] = 0
        d.copy_(torch.from_numpy(depth2))
        graph.replay()
        torch.cuda.synchronize()
        compare(got, restated(depth2))
    cut = got[2].trimmed()
    assert cut.points.shape[0] == int(got[2].count.item()) == cut.kept_rows.shape[0] == cut.multiplicity.shape[0]


# ---- the front ends ----------------------------------------------------------------------------------------------------------------------
def test_front_ends_on_tensors(gpu_device, scene_ray, cloud5000):
    from gaussiananything_amd import pointcloud as pc
    sc = scene_ray
    out = pc.filter_view_consistency(_t(sc["points"], gpu_device), _t(sc["depth"], gpu_device)[:, None], _t(sc["cam"], gpu_device),
                                     mask=_t(sc["mask"], gpu_device), depth_kind="ray", depth_range=(0.5, 3.0), tolerance=(0.001, 0.02),
                                     window=0, min_support=2, max_conflicts=1, carve=True, return_votes=True, capacity=2000)
    want = ref.filter_views_f32(sc["points"], sc["depth"], sc["cam"], mask=sc["mask"], depth_kind=ref.DEPTH_RAY, depth_min=0.5, depth_max=3.0,
                                tol_abs=0.001, tol_rel=0.02, window=0, min_support=2, max_conflicts=1, carve=True, capacity=2000)
    assert isinstance(out, pc.FilteredCloud) and out.capacity == 2000 and out.source is None and out.view_counts is None
    assert int(out.count.item()) == want["count"] and np.array_equal(out.kept_rows.cpu().numpy(), want["kept_rows"])
    _same(out.points.cpu().numpy(), want["points"], "points")
    assert np.array_equal(out.support.cpu().numpy(), want["support"]) and np.array_equal(out.conflicts.cpu().numpy(), want["conflicts"])
    c = cloud5000
    thin = pc.voxel_thin(_t(c["points"], gpu_device), 0.1, origin=(0.013, -0.02, 0.0), keep="first", colors=_t(c["colors"], gpu_device),
                         normals=_t(c["normals"], gpu_device))
    want = ref.voxel_thin_f32(c["points"], 0.1, (0.013, -0.02, 0.0), ref.VOXEL_FIRST, colors=c["colors"], normals=c["normals"])
    assert int(thin.count.item()) == want["count"] and int(thin.dropped.item()) == want["dropped"] == 4
    assert np.array_equal(thin.kept_rows.cpu().numpy(), want["kept_rows"]) and np.array_equal(thin.multiplicity.cpu().numpy(), want["multiplicity"])
    for k in ("points", "colors", "normals"):
        _same(getattr(thin, k).cpu().numpy(), want[k], k)
    cut = thin.trimmed()
    assert cut.points.shape[0] == want["count"] and cut.points.data_ptr() == thin.points.data_ptr()
    again = pc.voxel_thin(cut, 0.1, origin=(0.013, -0.02, 0.0), keep="first")        # thinning again on the same grid changes nothing
    assert int(again.count.item()) == want["count"] and torch.equal(again.points[:want["count"]], cut.points)
    with pytest.raises(RuntimeError, match="capacity"):
        pc.voxel_thin(_t(c["points"], gpu_device), 0.1, capacity=10).trimmed()


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


VOXEL = 0.04
RULE = dict(tolerance=(0.0, 0.05), min_support=0)          # rendered, alpha-blended depth: keep what no view contradicts


def _chain_counts(sc):
    """the number of points ``from_rgbd`` sees without and with the two steps, through the front ends"""
    from gaussiananything_amd import cameras, pointcloud as pc
    cam = cameras.cameras_from_view(sc["cv"], sc["tanfov"])
    a = pc.unproject_depth_views(sc["depth"], cam, mask=sc["mask"])
    b = pc.filter_view_consistency(a, sc["depth"], cam, mask=sc["mask"], **RULE)
    return int(a.count.item()), int(b.count.item()), int(pc.voxel_thin(b, VOXEL).count.item())


def test_from_rgbd_filters_and_thins_before_max_points(gpu_device, rgbd_scene):
    from gaussiananything_amd import fitting
    from tests.test_fit_gpu import LAMBDAS, LR
    sc = rgbd_scene
    full, filtered, thinned = _chain_counts(sc)
    assert 4 <= thinned < filtered <= full
    kw = dict(mask=sc["mask"], K=8, opacity=0.3, max_steps=64, lr=LR, **LAMBDAS)
    budget = (full + thinned) // 2                                                   # the unthinned cloud exceeds it, the thinned one fits
    with pytest.raises(ValueError, match="voxel_size"):
        fitting.SurfelFitter.from_rgbd(sc["depth"], sc["cv"], sc["cvp"], sc["tanfov"], sc["targets"], max_points=budget, **kw)
    f = fitting.SurfelFitter.from_rgbd(sc["depth"], sc["cv"], sc["cvp"], sc["tanfov"], sc["targets"], max_points=budget, consistency=RULE,
                                       voxel_size=VOXEL, **kw)
    assert f.num_points == thinned and f.steps == 0
    f.step(1)
    assert f.steps == 1 and np.isfinite(f.loss_history()["loss"]).all() and bool(torch.isfinite(f.gaussians()).all())
    plain = fitting.SurfelFitter.from_rgbd(sc["depth"], sc["cv"], sc["cvp"], sc["tanfov"], sc["targets"], max_points=budget,
                                           consistency=True, voxel_size=VOXEL, **kw)
    assert 4 <= plain.num_points <= thinned                                          # the default rule asks for a supporting view as well
    plain.step(1)
    assert plain.steps == 1 and bool(torch.isfinite(plain.gaussians()).all())
    with pytest.raises(ValueError, match="voxel_size") as e:                         # even the thinned cloud is too large
        fitting.SurfelFitter.from_rgbd(sc["depth"], sc["cv"], sc["cvp"], sc["tanfov"], sc["targets"], max_points=thinned - 1,
                                       consistency=RULE, voxel_size=VOXEL, **kw)
    assert f"max_points={thinned - 1}" in str(e.value) and "pixel_stride=" in str(e.value)


def test_from_rgbd_without_the_keywords_is_unchanged(gpu_device, rgbd_scene):
    """the fitter ``from_rgbd`` builds without ``consistency`` and ``voxel_size`` has the bits of the unproject -> trim -> from_points
    chain it was before them"""
    from gaussiananything_amd import cameras, fitting, losses, pointcloud as pc
    from tests.test_fit_gpu import LAMBDAS, LR
    sc = rgbd_scene
    kw = dict(K=8, opacity=0.3, max_steps=64, lr=LR, **LAMBDAS)
    f = fitting.SurfelFitter.from_rgbd(sc["depth"], sc["cv"], sc["cvp"], sc["tanfov"], sc["targets"], mask=sc["mask"], pixel_stride=2, **kw)
    with torch.no_grad():
        nrm = losses.depth_to_normal(sc["cv"].float().transpose(1, 2), float(sc["tanfov"]), sc["depth"])
    cloud = pc.unproject_depth_views(sc["depth"], cameras.cameras_from_view(sc["cv"], sc["tanfov"]), mask=sc["mask"], color=sc["targets"],
                                     normal=nrm, pixel_stride=2).trimmed()
    g = fitting.SurfelFitter.from_points(cloud.points, sc["cv"], sc["cvp"], sc["tanfov"], sc["targets"], colors=cloud.colors,
                                         normals=cloud.normals, mask=sc["mask"], **kw)
    assert f.num_points == g.num_points and torch.equal(f.gaussians(), g.gaussians())
