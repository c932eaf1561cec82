"""The restatement of the registration kernels (tests/_align_ref.py) against an independent float64 reference -- weighted means,
``np.linalg.svd``, determinant correction, Umeyama scale -- and against known transforms in an ICP scene; and the argument validation
of the Python front ends.  No GPU: the device is compared with the restatement bit for bit in tests/test_align_gpu.py."""
import math

import numpy as np
import pytest
import torch

from tests import _align_bounds as bounds
from tests import _align_ref as ref

F = np.float32


def _split(tf):
    tf = np.asarray(tf, np.float64)
    return tf[1:10].reshape(3, 3), tf[10:13], tf[0]


def _sums(x, y, w):
    G = ref.groups_of(len(x))
    return ref.tree_sums(ref.terms(x, y, w, ref.dist2_f32(x, y), G), G)


def test_well_conditioned_sets_against_svd():
    worst = dict(R=0.0, T=0.0, s=0.0)
    for x, y, w, scale in ref.well_conditioned_problems():
        out = ref.align_points(x[None], y[None], w[None], estimate_scale=scale)
        assert out["status"][0] == ref.RUNNING
        R, T, s = _split(out["transform"][0])
        R0, T0, s0 = ref.kabsch_f64(x, y, w, scale)
        worst["R"] = max(worst["R"], float(np.abs(R - R0).max()))
        worst["T"] = max(worst["T"], float(np.abs(T - T0).max()))
        worst["s"] = max(worst["s"], abs(float(s) - s0))
        assert abs(np.linalg.det(R) - 1.0) < 1e-6                                   # a proper rotation, never a reflection
        assert scale or s == 1.0
    print("worst differences from the SVD solution:", worst)
    assert worst["R"] <= bounds.R_BOUND and worst["T"] <= bounds.T_BOUND and worst["s"] <= bounds.S_BOUND, worst


def test_rmse_is_of_the_pairs_as_given():
    for x, y, w, scale in ref.well_conditioned_problems()[::7]:
        out = ref.align_points(x[None], y[None], w[None], estimate_scale=scale)
        w64 = w.astype(np.float64)
        want = math.sqrt(float((w64 * ((x.astype(np.float64) - y.astype(np.float64)) ** 2).sum(1)).sum() / w64.sum()))
        assert abs(float(out["rmse"][0]) - want) <= 4e-7 * want      # fp32 dist2 (three roundings, 2^-24 each) and the fp32 result


def test_planar_and_collinear_sets_by_residual():
    """the rotation is not unique there: the weighted residual of our solution against the SVD solution's.  The float64 solve is held
    to residual * (1 + 1e-6) + 1e-12 * sum(w |y|^2).  The fp32-rounded transform the device returns cannot meet that -- the SVD
    solution rounded to fp32 does not either -- so it is held to the same limit widened by what rounding 13 numbers to fp32 can move
    each transformed point, e_i = 2^-24 * sqrt(3) * (2 s |x_i|_1 + max|T|), through the triangle inequality of the weighted norm."""
    for x, y, w, scale in ref.degenerate_problems():
        exact, _, ok = ref.solve(_sums(x, y, w), scale, rounded=False)
        assert ok and exact is not None
        R0, T0, s0 = ref.kabsch_f64(x, y, w, scale)
        theirs = ref.residual_f64(x, y, w, R0, T0, s0)
        w64 = w.astype(np.float64)
        limit = theirs * (1 + 1e-6) + 1e-12 * float((w64 * (y.astype(np.float64) ** 2).sum(1)).sum())
        assert ref.residual_f64(x, y, w, *_split(exact)) <= limit
        R, T, s = _split(ref.align_points(x[None], y[None], w[None], estimate_scale=scale)["transform"][0])
        e = 2.0 ** -24 * math.sqrt(3) * (2 * abs(s) * np.abs(x.astype(np.float64)).sum(1) + np.abs(T).max())
        assert ref.residual_f64(x, y, w, R, T, s) <= (math.sqrt(limit) + math.sqrt(float((w64 * e * e).sum()))) ** 2
        assert abs(np.linalg.det(R) - 1.0) < 1e-6


def test_degenerate_inputs():
    x = np.random.default_rng(1).normal(size=(1, 9, 3)).astype(F)
    out = ref.align_points(x, x + F(1), np.zeros((1, 9), F))
    assert out["status"][0] == ref.DEGENERATE and np.array_equal(out["transform"][0], ref.IDENTITY) and out["rmse"][0] == 0
    same = np.tile(x[:, :1], (1, 9, 1))
    assert ref.align_points(same, x, estimate_scale=True)["status"][0] == ref.DEGENERATE
    out = ref.align_points(same, x, estimate_scale=False)                     # coincident X without scale: a pure translation
    assert out["status"][0] == ref.RUNNING
    assert np.allclose(ref.apply_transform(same[0], out["transform"][0]).mean(0), x[0].mean(0), atol=1e-6)


# ---- the ICP scene: a bumpy ellipsoid, X a random subset of it moved by a known transform ------------------------------------------------
# Point-to-point ICP on a sampled surface has local minima one sample spacing off the truth (rmse 1e-2 here; about a quarter of random
# axes at these angles end there, in the restatement as in any implementation).  The seeds below are scenes whose basin holds the truth:
# what is tested is the arithmetic of the passes, not the width of ICP's basin.
ICP_CASES = [  # n, m, angle, translation, scale, noise, seed
    (300, 1000, 0.15, 0.03, 1.0, 0.0, 101),
    (300, 1000, 0.30, 0.05, 1.1, 0.0, 101),
    (300, 1000, 0.20, 0.04, 1.0, 0.003, 103),
    (700, 1500, 0.30, 0.05, 1.0, 0.0, 103),
    (700, 1500, 0.15, 0.03, 1.05, 0.0, 104),
    (700, 1500, 0.25, 0.05, 1.0, 0.003, 106),
]
# Noise-free, the final matches are the true pairs and the solve is Kabsch on exact data up to the fp32 rounding of X: a coordinate of
# magnitude <= 0.5 moves by <= 2^-25, which over the thinnest extent of the target (0.3) is an angle, or a relative scale, of at most
# 2^-25 / 0.15 = 2e-7 with every rounding conspiring; the fp32 rounding of the result adds 2^-24 (times s <= 1.1 for the scale).
R_ICP_BOUND = 2.0e-7 + 2.0 ** -24
S_ICP_BOUND = 2.0e-7 + 1.1 * 2.0 ** -24


def _scene(n, m, angle, translation, scale, noise, seed):
    rng = np.random.default_rng(seed)
    y = ref.bumpy_ellipsoid(m)
    R = ref.rotation(rng.normal(size=3), angle)
    d = rng.normal(size=3)
    T = translation * d / np.linalg.norm(d)
    sub = y[rng.choice(m, n, replace=False)].astype(np.float64) + noise * rng.normal(size=(n, 3))
    return ref.moved(sub, R, T, scale), y, R, T, scale


@pytest.mark.parametrize("case", range(len(ICP_CASES)))
def test_icp_restatement_recovers_the_known_transform(case):
    n, m, angle, translation, scale, noise, seed = ICP_CASES[case]
    x, y, R0, T0, s0 = _scene(n, m, angle, translation, scale, noise, seed)
    out = ref.icp(x[None], y[None], max_iterations=60, relative_rmse_thr=1e-6, estimate_scale=scale != 1.0)
    R, T, s = _split(out["transform"][0])
    its, rmse = int(out["iterations"][0]), float(out["rmse"][0])
    print(f"case {case}: status {out['status'][0]}, {its} iterations, rmse {rmse:.3e}, R error {np.abs(R - R0).max():.2e}, "
          f"s error {abs(s - s0):.2e}")
    assert out["status"][0] == ref.CONVERGED and its < 60
    assert np.array_equal(out["history"][0, its, :13], out["transform"][0]) and out["history"][0, its, 13] == out["rmse"][0]
    assert np.array_equal(out["history"][0, its:], np.tile(out["history"][0, its], (61 - its, 1)))
    assert np.array_equal(out["xt"][0], ref.apply_transform(x, out["transform"][0]))
    if noise == 0.0:
        assert np.abs(R - R0).max() <= R_ICP_BOUND and abs(s - s0) <= S_ICP_BOUND
    else:
        # the rmse of isotropic Gaussian noise of deviation sigma is sigma * sqrt(3); the nearest match and the fit can only lower
        # it, and its sampling deviation over 3n coordinates is 1 / sqrt(6n) < 2.4 %
        assert 0.8 * noise * math.sqrt(3) <= rmse <= 1.1 * noise * math.sqrt(3)
        assert np.abs(R - R0).max() <= 10 * noise


def test_icp_gate_on_partial_overlap():
    rng = np.random.default_rng(9)
    y = ref.bumpy_ellipsoid(1500)
    half = np.flatnonzero(y[:, 0] > 0)
    R0 = ref.rotation(rng.normal(size=3), 0.1)
    d = rng.normal(size=3)
    T0 = 0.02 * d / np.linalg.norm(d)
    inliers = ref.moved(y[rng.choice(half, 500, replace=False)], R0, T0, 1.0)
    d = rng.normal(size=(50, 3))
    outliers = (d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.8, 1.2, size=(50, 1))).astype(F)
    x = np.concatenate([inliers, outliers])
    gated = ref.icp(x[None], y[None], max_iterations=60, max_distance=0.08)
    free = ref.icp(x[None], y[None], max_iterations=60)
    err = lambda o: float(np.abs(_split(o["transform"][0])[0] - R0).max())
    print(f"gated: {int(gated['iterations'][0])} iterations, R error {err(gated):.2e}; ungated: R error {err(free):.2e}")
    assert gated["status"][0] == ref.CONVERGED
    assert int((gated["dist2"][0] <= F(0.08) * F(0.08)).sum()) == 500 and bool((gated["dist2"][0, :500] <= F(0.08) * F(0.08)).all())
    assert err(gated) <= R_ICP_BOUND
    assert err(free) > 1e-3 and err(free) > err(gated)


def test_frozen_cloud_in_a_batch():
    """a cloud that starts aligned converges at once, its neighbour goes on; lengths differ"""
    x1, y, *_ = _scene(300, 1000, 0.3, 0.05, 1.0, 0.0, 3)
    x0 = y[:300].copy()
    out = ref.icp(np.stack([x0, x1]), np.stack([y, y]), x_lengths=[200, 300], max_iterations=30)
    assert out["status"].tolist() == [ref.CONVERGED, ref.CONVERGED]
    assert out["iterations"][0] == 1 and out["iterations"][1] > 3 and out["rmse"][0] == 0
    assert (out["idx"][0, 200:] == -1).all() and np.array_equal(out["idx"][0, :200], np.arange(200))


# ---- the front ends' argument validation: before the device check, so CPU tensors do -----------------------------------------------------
def test_front_end_validation():
    from gaussiananything_amd import mesh, pointcloud as pc
    X, Y = torch.zeros(2, 5, 3), torch.zeros(2, 7, 3)
    with pytest.raises(NotImplementedError):
        pc.corresponding_points_alignment(X, X, allow_reflection=True)
    with pytest.raises(NotImplementedError):
        pc.iterative_closest_point(X, Y, allow_reflection=True)
    for kw in (dict(max_iterations=-1), dict(relative_rmse_thr=-1e-3), dict(relative_rmse_thr=float("nan")),
               dict(max_correspondence_distance=0.0), dict(max_correspondence_distance=float("inf"))):
        with pytest.raises(ValueError):
            pc.iterative_closest_point(X, Y, **kw)
    with pytest.raises(ValueError):
        pc.iterative_closest_point(torch.zeros(5, 3), Y)
    with pytest.raises(ValueError):
        pc.corresponding_points_alignment(torch.zeros(2, 5, 2), X)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pc.iterative_closest_point(X, Y)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pc.corresponding_points_alignment(X, X)
    with pytest.raises(ValueError):
        mesh.mesh_cloud_distance(torch.zeros(3, 3), torch.zeros(1, 3, dtype=torch.int64), torch.zeros(4, 3), align="affine")
    assert pc.SimilarityTransform._fields == ("R", "T", "s")
    assert pc.ICPSolution._fields[:5] == ("converged", "rmse", "Xt", "RTs", "t_history")


def test_apply_similarity_transform_matches_the_restatement():
    from gaussiananything_amd import pointcloud as pc
    rng = np.random.default_rng(5)
    x = rng.normal(size=(2, 40, 3)).astype(F)
    tf = np.stack([ref.pack(ref.rotation(rng.normal(size=3), 0.7), rng.normal(size=3), 1.3), ref.IDENTITY])
    got = pc.apply_similarity_transform(torch.from_numpy(x), torch.from_numpy(tf)).numpy()
    want = np.stack([ref.apply_transform(x[b], tf[b]) for b in range(2)])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    t = pc.SimilarityTransform(torch.from_numpy(tf[:, 1:10].reshape(2, 3, 3)), torch.from_numpy(tf[:, 10:]), torch.from_numpy(tf[:, 0]))
    assert np.array_equal(pc.apply_similarity_transform(torch.from_numpy(x), t).numpy().view(np.uint32), want.view(np.uint32))


# ---- the C entry points: everything the host can see is turned away before anything touches the device -------------------------------
GA_ERR_NULL_ARG, GA_ERR_BAD_SHAPE, GA_ERR_WORKSPACE, GA_ERR_BAD_FLAGS = -1, -2, -3, -5


def _lib():
    from gaussiananything_amd import _lib
    return _lib, _lib.lib()


def test_host_validation_rejects_before_any_launch():
    """Fake, non-NULL device addresses: a call that got past validation would fault; every one here must be turned away."""
    import ctypes
    _l, L = _lib()
    P = 0x1000   # never dereferenced
    BIG = (1 << 31) // 3 + 1

    def icp(B=2, N=10, M=20, K=5, scale=0, reserved=0, thr=1e-6, gate=0.0, ws_bytes=1 << 20, **ptr):
        q = dict(x=P, y=P, transform=P, rmse=P, status=P, iterations=P, xt=P, idx=P, dist2=P, workspace=P)
        q.update(ptr)
        a = _l.GaIcpArgs(B, N, M, K, scale, reserved, thr, gate, q["x"], q["y"], None, None, None, None, q["transform"], q["rmse"],
                         q["status"], q["iterations"], None, q["xt"], q["idx"], q["dist2"], q["workspace"], ws_bytes)
        return L.ga_pc_icp(ctypes.byref(a), None)

    def align(B=2, N=10, scale=0, reserved=0, ws_bytes=1 << 20, **ptr):
        q = dict(x=P, y=P, transform=P, rmse=P, status=P, workspace=P)
        q.update(ptr)
        a = _l.GaAlignArgs(B, N, scale, reserved, q["x"], q["y"], None, None, q["transform"], q["rmse"], q["status"], q["workspace"],
                           ws_bytes)
        return L.ga_pc_align_points(ctypes.byref(a), None)

    assert L.ga_pc_icp(None, None) == GA_ERR_NULL_ARG and L.ga_pc_align_points(None, None) == GA_ERR_NULL_ARG
    for name in ("x", "y", "transform", "rmse", "status", "iterations", "xt", "idx", "dist2", "workspace"):
        assert icp(**{name: None}) == GA_ERR_NULL_ARG, name
    for name in ("x", "y", "transform", "rmse", "status", "workspace"):
        assert align(**{name: None}) == GA_ERR_NULL_ARG, name
    for kw in (dict(B=0), dict(B=65536), dict(N=0), dict(N=-1), dict(M=0), dict(N=BIG), dict(M=BIG), dict(K=-1), dict(K=10001)):
        assert icp(**kw) == GA_ERR_BAD_SHAPE, kw
    for kw in (dict(B=0), dict(B=65536), dict(N=0), dict(N=BIG)):
        assert align(**kw) == GA_ERR_BAD_SHAPE, kw
    for kw in (dict(scale=2), dict(scale=-1), dict(reserved=1), dict(thr=-1.0), dict(thr=float("nan")), dict(thr=float("inf")),
               dict(gate=-0.1), dict(gate=float("nan")), dict(gate=float("inf"))):
        assert icp(**kw) == GA_ERR_BAD_FLAGS, kw
    assert align(scale=2) == GA_ERR_BAD_FLAGS and align(reserved=3) == GA_ERR_BAD_FLAGS
    need = int(L.ga_pc_align_workspace_bytes(2, 10))
    assert icp(ws_bytes=need - 1) == GA_ERR_WORKSPACE and align(ws_bytes=need - 1) == GA_ERR_WORKSPACE


def test_plan_and_workspace_are_host_only():
    import ctypes
    _l, L = _lib()
    pl = _l.GaAlignPlan()
    assert L.ga_pc_align_plan(100, 100, None) == GA_ERR_NULL_ARG
    for bad in ((0, 100), (100, 0), ((1 << 31) // 3 + 1, 100)):
        assert L.ga_pc_align_plan(*bad, ctypes.byref(pl)) == GA_ERR_BAD_SHAPE, bad
    for N in (1, 256, 257, 100000):
        assert L.ga_pc_align_plan(N, 5000, ctypes.byref(pl)) == 0
        assert (pl.threads, pl.tile, pl.grid_x, pl.sweeps, pl.terms) == (ref.THREADS, ref.TILE, ref.groups_of(N), ref.SWEEPS, ref.TERMS)
        assert pl.sweeps == _l.GA_PC_ALIGN_SWEEPS and pl.terms == _l.GA_PC_ALIGN_TERMS
        for B in (1, 7):
            ws = int(L.ga_pc_align_workspace_bytes(B, N))
            assert ws % 16 == 0 and ws >= (B * pl.grid_x * pl.terms + B) * 8
    assert L.ga_pc_align_workspace_bytes(0, 10) == 0 and L.ga_pc_align_workspace_bytes(1, 0) == 0
