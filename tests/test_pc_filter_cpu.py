"""CPU tests of the cross-view consistency filter and the voxel thinning (include/ga_pointcloud.h, csrc/pc_filter.hip): the C ABI's
refusals with fake addresses, the Python front ends' refusals, properties of the voxel restatement, and the filter's restatement
(tests/_pc_filter_ref.py) on an analytic scene against the two bars it must meet.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _pc_filter_ref as ref
from tests import _unproject_ref as uref

F = np.float32
FAKE = 0x1000           # a non-NULL, 16-byte aligned address nothing dereferences: every refusal comes before the device is touched


def _filter_args(**kw):
    from gaussiananything_amd import _lib
    rows = kw.get("rows", 100)
    ws = int(_lib.lib().ga_pc_filter_views_workspace_bytes(max(1, min(rows, 1 << 30))))
    base = dict(rows=rows, capacity=100, num_views=2, height=8, width=8, depth_kind=0, window=1, min_support=1, max_conflicts=0, carve=0,
                depth_min=0.0, depth_max=float("inf"), mask_threshold=0.5, tol_abs=0.0, tol_rel=0.01, reserved=0, in_count=None,
                points=FAKE, colors=None, normals=None, source=FAKE, depth=FAKE, mask=None, cameras=FAKE, out_points=FAKE,
                out_colors=None, out_normals=None, out_source=FAKE, kept_rows=FAKE, count=FAKE, view_counts=FAKE, support=None,
                conflicts=None, workspace=FAKE, workspace_bytes=ws)
    base.update(kw)
    return _lib.GaFilterViewsArgs(**base)


def _voxel_args(**kw):
    from gaussiananything_amd import _lib
    rows = kw.get("rows", 100)
    ws = int(_lib.lib().ga_pc_voxel_thin_workspace_bytes(max(1, min(rows, 1 << 30)), 0))
    base = dict(rows=rows, capacity=100, keep=1, num_views=0, view_pixels=0, flags=0, origin=(ctypes.c_float * 3)(0, 0, 0),
                voxel_size=0.1, table_slots=0, in_count=None, points=FAKE, colors=None, normals=None, source=None, out_points=FAKE,
                out_colors=None, out_normals=None, out_source=None, kept_rows=FAKE, count=FAKE, view_counts=None, multiplicity=None,
                dropped=None, workspace=FAKE, workspace_bytes=ws)
    base.update(kw)
    return _lib.GaVoxelThinArgs(**base)


NULL_ARG, BAD_SHAPE, WORKSPACE, BAD_FLAGS = -1, -2, -3, -5
NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("want,kw", [
    (NULL_ARG, dict(points=None)), (NULL_ARG, dict(depth=None)), (NULL_ARG, dict(cameras=None)), (NULL_ARG, dict(out_points=None)),
    (NULL_ARG, dict(kept_rows=None)), (NULL_ARG, dict(count=None)), (NULL_ARG, dict(workspace=None)),
    (NULL_ARG, dict(colors=FAKE)), (NULL_ARG, dict(out_colors=FAKE)), (NULL_ARG, dict(normals=FAKE)), (NULL_ARG, dict(out_normals=FAKE)),
    (NULL_ARG, dict(source=None)), (NULL_ARG, dict(out_source=None)), (NULL_ARG, dict(source=None, out_source=None)),   # view_counts needs source
    (BAD_SHAPE, dict(rows=0)), (BAD_SHAPE, dict(rows=-3)), (BAD_SHAPE, dict(rows=(1 << 30) + 1)), (BAD_SHAPE, dict(capacity=0)),
    (BAD_SHAPE, dict(num_views=0)), (BAD_SHAPE, dict(height=0)), (BAD_SHAPE, dict(width=-1)),
    (BAD_SHAPE, dict(num_views=8, height=1 << 14, width=1 << 14)),
    (BAD_FLAGS, dict(depth_kind=2)), (BAD_FLAGS, dict(window=2)), (BAD_FLAGS, dict(window=-1)), (BAD_FLAGS, dict(carve=2)),
    (BAD_FLAGS, dict(min_support=-1)), (BAD_FLAGS, dict(max_conflicts=-1)), (BAD_FLAGS, dict(reserved=1)),
    (BAD_FLAGS, dict(depth_min=NAN)), (BAD_FLAGS, dict(depth_max=NAN)), (BAD_FLAGS, dict(mask_threshold=NAN)),
    (BAD_FLAGS, dict(tol_abs=-1e-3)), (BAD_FLAGS, dict(tol_abs=INF)), (BAD_FLAGS, dict(tol_rel=NAN)), (BAD_FLAGS, dict(tol_rel=INF)),
    (WORKSPACE, dict(workspace_bytes=16)), (WORKSPACE, dict(workspace=FAKE + 8)),
])
def test_filter_views_refuses_before_it_touches_the_device(want, kw):
    from gaussiananything_amd import _lib
    assert _lib.lib().ga_pc_filter_views(ctypes.byref(_filter_args(**kw)), None) == want
    assert _lib.lib().ga_pc_filter_views(None, None) == NULL_ARG


@pytest.mark.parametrize("want,kw", [
    (NULL_ARG, dict(points=None)), (NULL_ARG, dict(out_points=None)), (NULL_ARG, dict(kept_rows=None)), (NULL_ARG, dict(count=None)),
    (NULL_ARG, dict(workspace=None)), (NULL_ARG, dict(colors=FAKE)), (NULL_ARG, dict(out_normals=FAKE)), (NULL_ARG, dict(source=FAKE)),
    (NULL_ARG, dict(out_source=FAKE)), (NULL_ARG, dict(view_counts=FAKE, num_views=2, view_pixels=64)),
    (BAD_SHAPE, dict(rows=0)), (BAD_SHAPE, dict(rows=(1 << 30) + 1)), (BAD_SHAPE, dict(capacity=0)),
    (BAD_SHAPE, dict(table_slots=100)), (BAD_SHAPE, dict(table_slots=96)), (BAD_SHAPE, dict(table_slots=64)),
    (BAD_SHAPE, dict(table_slots=-128)), (BAD_SHAPE, dict(table_slots=1 << 32)),
    (BAD_SHAPE, dict(view_counts=FAKE, source=FAKE, out_source=FAKE, num_views=0, view_pixels=64)),
    (BAD_SHAPE, dict(view_counts=FAKE, source=FAKE, out_source=FAKE, num_views=2, view_pixels=0)),
    (BAD_FLAGS, dict(keep=2)), (BAD_FLAGS, dict(keep=-1)), (BAD_FLAGS, dict(flags=2)), (BAD_FLAGS, dict(flags=-1)),
    (BAD_FLAGS, dict(voxel_size=0.0)), (BAD_FLAGS, dict(voxel_size=-0.1)), (BAD_FLAGS, dict(voxel_size=INF)), (BAD_FLAGS, dict(voxel_size=NAN)),
    (BAD_FLAGS, dict(origin=(ctypes.c_float * 3)(0, NAN, 0))), (BAD_FLAGS, dict(origin=(ctypes.c_float * 3)(INF, 0, 0))),
    (WORKSPACE, dict(workspace_bytes=16)), (WORKSPACE, dict(workspace=FAKE + 4)),
    (WORKSPACE, dict(table_slots=1024)),                                             # a larger table than the default one was sized for
])
def test_voxel_thin_refuses_before_it_touches_the_device(want, kw):
    from gaussiananything_amd import _lib
    assert _lib.lib().ga_pc_voxel_thin(ctypes.byref(_voxel_args(**kw)), None) == want
    assert _lib.lib().ga_pc_voxel_thin(None, None) == NULL_ARG


def test_workspace_sizes():
    from gaussiananything_amd import _lib
    L = _lib.lib()
    for rows in (0, -1, (1 << 30) + 1):
        assert L.ga_pc_filter_views_workspace_bytes(rows) == 0 and L.ga_pc_voxel_thin_workspace_bytes(rows, 0) == 0
    for rows in (1, 1023, 1024, 1025, 266241):
        bands = ref.plan(rows)[0]
        compact = (bands + 1 + 3) // 4 * 16 + (rows + 15) // 16 * 16
        assert L.ga_pc_filter_views_workspace_bytes(rows) == compact
        slots = 1
        while slots < 2 * rows:
            slots *= 2
        table = lambda s: compact + (rows * 4 + 15) // 16 * 16 + (s * 20 + 15) // 16 * 16
        assert L.ga_pc_voxel_thin_workspace_bytes(rows, 0) == table(slots) == L.ga_pc_voxel_thin_workspace_bytes(rows, slots)
        assert L.ga_pc_voxel_thin_workspace_bytes(rows, 4 * slots) == table(4 * slots)
        for bad in (slots - 1, rows if rows & (rows - 1) == 0 else 3 * slots, -slots):
            assert L.ga_pc_voxel_thin_workspace_bytes(rows, bad) == 0, (rows, bad)


def test_front_ends_refuse():
    from gaussiananything_amd import pointcloud as pc
    pts, depth, cam = torch.zeros(10, 3), torch.ones(2, 8, 8), torch.zeros(2, 21)
    for bad, kw in ((ValueError, dict(depth_kind="x")), (ValueError, dict(window=2)), (ValueError, dict(tolerance=(-1.0, 0.0))),
                    (ValueError, dict(tolerance=(0.0, float("inf")))), (ValueError, dict(min_support=-1)), (ValueError, dict(max_conflicts=-1)),
                    (ValueError, dict(depth_range=(1.0, 1.0))), (ValueError, dict(mask_threshold=float("nan"))),
                    (RuntimeError, dict())):                                         # a CPU cloud: no fallback
        with pytest.raises(bad):
            pc.filter_view_consistency(pts, depth, cam, **kw)
    with pytest.raises(ValueError):
        pc.filter_view_consistency(torch.zeros(10, 2), depth, cam)
    with pytest.raises(ValueError):
        pc.filter_view_consistency(pts, torch.ones(2, 3, 8, 8), cam)
    with pytest.raises(ValueError):
        pc.filter_view_consistency(pts, depth, torch.zeros(3, 21))
    with pytest.raises(TypeError):
        pc.filter_view_consistency(pts.long(), depth, cam)
    for bad, args, kw in ((ValueError, (pts, 0.0), {}), (ValueError, (pts, float("inf")), {}), (ValueError, (pts, 0.1), dict(keep="mean")),
                          (ValueError, (pts, 0.1), dict(origin=(0, 0))), (ValueError, (pts, 0.1), dict(origin=(0, float("nan"), 0))),
                          (ValueError, (pts, 0.1), dict(colors=torch.zeros(9, 3))), (ValueError, (pts, 0.1), dict(view_pixels=64)),
                          (ValueError, (torch.zeros(0, 3), 0.1), {}), (RuntimeError, (pts, 0.1), {})):
        with pytest.raises(bad):
            pc.voxel_thin(*args, **kw)
    assert issubclass(pc.FilteredCloud, pc.UnprojectedCloud)


def test_from_rgbd_refuses_bad_keywords():
    from gaussiananything_amd import fitting
    d, cv, t = torch.ones(2, 1, 8, 8), torch.eye(4).repeat(2, 1, 1), torch.zeros(2, 3, 8, 8)
    with pytest.raises(TypeError, match="consistency"):
        fitting.SurfelFitter.from_rgbd(d, cv, cv, 0.5, t, consistency="yes")
    with pytest.raises(ValueError, match="voxel_size"):
        fitting.SurfelFitter.from_rgbd(d, cv, cv, 0.5, t, voxel_size=0.0)


# ---- the voxel restatement ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cloud():
    rng = np.random.default_rng(11)
    p = rng.uniform(-0.35, 0.35, size=(5000, 3)).astype(F)
    p[100:140] = p[60:100]                                   # duplicated points
    p[200:230] = (np.round(p[200:230] / F(0.1)) * F(0.1)).astype(F)   # on cell faces
    p[300], p[301], p[302], p[303] = (np.nan, 0, 0), (0, np.inf, 0), (0, 0, -np.inf), (0, 2e5, 0)
    return p


@pytest.mark.parametrize("keep", [ref.VOXEL_FIRST, ref.VOXEL_CENTER])
def test_voxel_restatement_properties(cloud, keep):
    vs, origin = 0.1, (0.013, -0.02, 0.0)
    out = ref.voxel_thin_f32(cloud, vs, origin, keep)
    ok, key, rank = ref.voxel_cells(cloud, vs, origin, keep)
    assert out["dropped"] == 4 and not ok[300:304].any() and ok.sum() == 4996
    n = out["count"]
    assert n == len(np.unique(key[ok])) and 200 < n < 600                          # one kept row per distinct cell
    kept = out["kept_rows"][:n]
    assert (np.diff(kept) > 0).all()                                                 # ascending input order
    for r in kept:                                                                   # each its cell's minimum rank, by brute force
        same = np.flatnonzero(ok & (key == key[r]))
        assert rank[r] == rank[same].min() and out["multiplicity"][list(kept).index(r)] == len(same)
    assert out["multiplicity"][:n].sum() == 5000 - out["dropped"]
    again = ref.voxel_thin_f32(out["points"][:n], vs, origin, keep)                  # thinning again on the same grid changes nothing
    assert again["count"] == n and np.array_equal(again["kept_rows"][:n], np.arange(n)) and (again["multiplicity"][:n] == 1).all()
    assert np.array_equal(again["points"][:n].view(np.uint32), out["points"][:n].view(np.uint32))
    if keep == ref.VOXEL_FIRST:
        assert not np.isin(np.arange(100, 140), kept).any()                          # of two equal points the lower row wins
    else:
        dup = np.isin(np.arange(100, 140), kept)
        assert not dup.any()


def test_voxel_restatement_faces_and_signs():
    """a point exactly on a face belongs to the cell above it; negative coordinates floor downwards"""
    p = np.array([[0.0, 0.0, 0.0], [-0.0, 0.25, 0.5], [-1e-9, 0.0, 0.0], [0.5, 0.5, 0.5], [-0.5, -0.5, -0.5], [-0.5000001, 0, 0]], F)
    ok, key, _ = ref.voxel_cells(p, 0.5)
    i = np.stack([(key >> 42) & 0x1fffff, (key >> 21) & 0x1fffff, key & 0x1fffff], 1) - (1 << 20)
    assert ok.all() and i.tolist() == [[0, 0, 0], [0, 0, 1], [-1, 0, 0], [1, 1, 1], [-1, -1, -1], [-2, 0, 0]]
    edge = np.array([[ref.MAX_INDEX + 0.5, 0, 0], [ref.MAX_INDEX + 1.0, 0, 0], [-ref.MAX_INDEX - 0.0, 0, 0], [-ref.MAX_INDEX - 0.5, 0, 0]], F)
    assert ref.voxel_cells(edge, 1.0)[0].tolist() == [True, False, True, False]


# ---- the filter on the analytic scene ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene():
    """two spheres, 8 views of 64 x 64 on a ring, 3 % of the surface pixels turned into floaters; the cloud of all views"""
    cam = ref.ring_cameras(8)
    clean = ref.raycast_z(cam, 64, 64)
    depth, floater = ref.add_floaters(clean, 0.03, seed=5)
    cloud = uref.unproject_f32(depth, cam)
    n = cloud["count"]
    return dict(cam=cam, depth=depth, points=cloud["points"][:n], source=cloud["source"][:n], floater=floater.reshape(-1)[cloud["source"][:n]])


def _rates(scene, **kw):
    out = ref.filter_views_f32(scene["points"], scene["depth"], scene["cam"], source=scene["source"], **kw)
    f = scene["floater"]
    return out["keep"][~f].mean(), out["keep"][f].mean(), out


def test_filter_restatement_meets_the_bars_on_the_analytic_scene(scene):
    """window 1, tolerance (0, 1 %), min_support 1, max_conflicts 0: at least 98 % of the true points stay, at most 3 % of the floaters"""
    f = scene["floater"]
    assert 0.025 < f.mean() < 0.035 and len(f) > 8000
    true_kept, floaters_kept, out = _rates(scene, window=1, tol_abs=0.0, tol_rel=0.01, min_support=1, max_conflicts=0)
    print(f"analytic scene: {len(f)} points, {int(f.sum())} floaters; kept {true_kept:.4f} of the true points, {floaters_kept:.4f} of the floaters")
    assert true_kept >= 0.98
    assert floaters_kept <= 0.03
    carved = _rates(scene, window=1, tol_abs=0.0, tol_rel=0.01, min_support=1, max_conflicts=0, carve=True)
    print(f"with carve: kept {carved[0]:.4f} of the true points, {carved[1]:.4f} of the floaters")
    assert carved[1] <= floaters_kept and carved[0] <= true_kept
    # every kind of answer a view can give occurs
    seen = set(np.unique(out["classes"]).tolist())
    assert {ref.SKIPPED_OWN, ref.SUPPORT, ref.CONFLICT, ref.OCCLUDED, ref.UNDECIDED} <= seen


def test_window_is_what_keeps_grazing_points(scene):
    narrow = _rates(scene, window=0, tol_abs=0.0, tol_rel=0.01, min_support=1, max_conflicts=0)[0]
    wide = _rates(scene, window=1, tol_abs=0.0, tol_rel=0.01, min_support=1, max_conflicts=0)[0]
    print(f"window 0 keeps {narrow:.4f} of the true points, window 1 {wide:.4f}")
    assert narrow < wide


def test_filter_restatement_rule(scene):
    """the keep rule on the votes, in_count, a foreign cloud (every view votes) and saturation of the stored votes"""
    pts, depth, cam, src = scene["points"][:3000], scene["depth"], scene["cam"], scene["source"][:3000]
    s, c, _ = ref.votes_f32(pts, depth, cam, source=src)
    for ms, mc in ((0, 0), (1, 0), (2, 1), (3, 0)):
        out = ref.filter_views_f32(pts, depth, cam, source=src, min_support=ms, max_conflicts=mc)
        assert np.array_equal(out["keep"], (s >= ms) & (c <= mc)) and out["count"] == out["keep"].sum()
        assert out["view_counts"].sum() == out["count"]
    short = ref.filter_views_f32(pts, depth, cam, source=src, in_count=1000, min_support=0)
    assert short["count"] <= 1000 and not short["keep"][1000:].any() and not short["support"][1000:].any()
    assert ref.filter_views_f32(pts, depth, cam, source=src, in_count=-5, min_support=0)["count"] == 0
    foreign = ref.votes_f32(pts, depth, cam)
    assert (foreign[0] >= s).all() and (foreign[0] > s).any()                      # the own view supports its own points
    many = np.repeat(cam[:1], 300, 0), np.repeat(depth[:1], 300, 0)
    sat = ref.filter_views_f32(pts[:50], many[1], many[0], min_support=1)
    assert sat["support"].max() == 255 and sat["support"].dtype == np.uint8
