"""CPU tests of the normal estimation and the surfel initialiser (include/ga_pointcloud.h, csrc/pc_normals.hip): the float32
restatement the GPU tests hold the kernels to bit for bit (tests/_normals_ref.py) against float64, the rules the header states (sign,
viewpoint, invalid rows, frame, scale), the PLY round trip, and everything the host refuses before a launch.

Bars.  ``BAR_NORMAL`` and ``BAR_LAMBDA`` are 4 x the largest value the final restatement (5 sweeps) reaches on the three test clouds
at K = 8 and K = 16; the margin covers another libm or numpy build.  Measured:
    sin(angle to the float64 normal) * (lam1 - lam0) / lam2   largest 1.761e-7 (sphere, K = 16)   ->  BAR_NORMAL 7.044e-7
    |eigenvalue - float64 eigenvalue| / lam2                  largest 2.827e-7 (sphere, K = 16)   ->  BAR_LAMBDA 1.1308e-6
Nothing here is pinned to Open3D or pytorch3d: neither is on the machine, the definitions are the project's own."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import _normals_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GA_ERR_NULL_ARG, GA_ERR_BAD_SHAPE = -1, -2
F = np.float32
BAR_NORMAL, BAR_LAMBDA = ref.BAR_NORMAL, ref.BAR_LAMBDA


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def restated():
    """(cloud name, K) -> (points, dist2, idx, normal, tangent, eigenvalues): computed once, shared, left unchanged"""
    out = {}
    for name, p in ref.clouds().items():
        for K in (8, 16):
            d2, idx = ref.self_knn(p, K)
            out[name, K] = (p, d2, idx) + ref.normals_f32(p, idx)
    return out


# ---- 1, 2: the restatement against float64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [8, 16])
@pytest.mark.parametrize("name", ["sphere", "plane", "cube"])
def test_restated_normals_against_float64_eigh(restated, name, K):
    """every point, no exclusions: sin(angle between the two normals) * gap <= BAR_NORMAL with gap = (lam1 - lam0) / lam2 in float64
    (largest measured value 1.761e-7, bar 4 x that: the module docstring)"""
    p, _, idx, normal, tangent, _ = restated[name, K]
    n64, lam64, v64 = ref.normals_f64(p, idx)
    crit = ref.sin_times_gap(normal, n64, lam64)
    # the tangent by the same criterion with its own gap, (lam2 - lam1) / lam2
    tsin = np.linalg.norm(np.cross(tangent.astype(np.float64), v64[:, :, 2]), axis=1)
    tcrit = tsin * (lam64[:, 2] - lam64[:, 1]) / lam64[:, 2]
    print(f"tangents {name} K {K}: largest sin * gap {tcrit.max():.3e}")
    print(f"normals {name} K {K}: largest sin * gap {crit.max():.3e} (bar {BAR_NORMAL:.3e}), smallest gap "
          f"{((lam64[:, 1] - lam64[:, 0]) / lam64[:, 2]).min():.2e}")
    assert crit.shape == (2048,) and np.isfinite(crit).all()
    assert (crit <= BAR_NORMAL).all(), float(crit.max())
    assert np.abs(np.linalg.norm(normal.astype(np.float64), axis=1) - 1).max() <= 2 * 2.0 ** -23
    assert np.abs(np.linalg.norm(tangent.astype(np.float64), axis=1) - 1).max() <= 2 * 2.0 ** -23
    assert (tcrit <= BAR_NORMAL).all(), float(tcrit.max())


@pytest.mark.parametrize("K", [8, 16])
@pytest.mark.parametrize("name", ["sphere", "plane", "cube"])
def test_restated_eigenvalues_are_ascending_and_near_float64(restated, name, K):
    """each eigenvalue within BAR_LAMBDA of the float64 one, relative to lam2 (largest measured value 2.827e-7, bar 4 x that)"""
    p, _, idx, _, _, eig = restated[name, K]
    _, lam64, _ = ref.normals_f64(p, idx)
    assert eig.dtype == F and (np.diff(eig, axis=1) >= 0).all()
    err = np.abs(eig.astype(np.float64) - lam64) / lam64[:, 2:3]
    print(f"eigenvalues {name} K {K}: largest |error| / lam2 {err.max():.3e} (bar {BAR_LAMBDA:.3e})")
    assert (err <= BAR_LAMBDA).all(), float(err.max())


def test_the_sweep_count_is_the_converged_one_plus_one(restated):
    """what GA_PC_NORMALS_SWEEPS in the header says: after 4 sweeps the off-diagonal is gone and the normals no longer change"""
    from gaussiananything_amd import _lib
    assert ref.SWEEPS == _lib.GA_PC_NORMALS_SWEEPS == 5
    for (name, K), (p, _, idx, normal, _, _) in restated.items():
        offs = []
        ref.jacobi_f32(ref.covariance_f32(p, idx, len(p), K)[1], ref.SWEEPS - 1, trace_off=offs)
        assert offs[-1] <= 1e-14, (name, K, offs)
        assert np.array_equal(_bits(ref.normals_f32(p, idx, sweeps=ref.SWEEPS - 1)[0]), _bits(normal)), (name, K)


# ---- 3: points exactly on a plane ----------------------------------------------------------------------------------------------------------
def _dyadic_plane():
    """a 16 x 16 grid x, y in k/16 on z = x/2 + y/4: every coordinate, centroid (K = 8) and centred product is exact in float32"""
    g = np.arange(16, dtype=np.float64) / 16
    x, y = (a.ravel() for a in np.meshgrid(g, g, indexing="ij"))
    return np.stack([x, y, x / 2 + y / 4], 1).astype(F), np.array([0.5, 0.25, -1.0]) / np.linalg.norm([0.5, 0.25, -1.0])


def test_points_exactly_on_a_plane_give_its_normal():
    p, want = _dyadic_plane()
    assert np.array_equal(p.astype(np.float64)[:, 2], p.astype(np.float64)[:, 0] / 2 + p.astype(np.float64)[:, 1] / 4)
    _, idx = ref.self_knn(p, 8)
    normal, tangent, eig = ref.normals_f32(p, idx)
    sin = np.linalg.norm(np.cross(normal.astype(np.float64), want), axis=1)
    print(f"exact plane: largest sin {sin.max():.3e} (bar {BAR_NORMAL:.3e}), largest |lam0| / lam2 {np.abs(eig[:, 0] / eig[:, 2]).max():.3e}")
    assert (sin <= BAR_NORMAL).all(), float(sin.max())
    assert (np.abs((tangent.astype(np.float64) * want).sum(1)) <= BAR_NORMAL).all()   # the tangent lies in the plane


# ---- 4: sign and viewpoint ----------------------------------------------------------------------------------------------------------------
def test_sign_rule_and_viewpoint_flip(restated):
    p, _, idx, normal, tangent, _ = restated["sphere", 16]
    for v in (normal, tangent):     # the component of largest magnitude is positive
        big = np.take_along_axis(v, np.abs(v).argmax(1)[:, None], 1)
        assert (big > 0).all()
    # the first among equal magnitudes decides
    x, y, z = ref._unit_with_default_sign([np.array([-1, 1, 0, 0], F), np.array([1, -1, -2, 0], F), np.array([1, 1, 2, -3], F)])
    got = np.stack([x, y, z], 1)
    assert (np.sign(got) == np.array([[1, -1, -1], [1, -1, 1], [0, 1, -1], [0, 0, 1]])).all()
    # towards a viewpoint: the centre of the sphere sees every normal pointing inwards, a far point on +z splits them by hemisphere
    inward = ref.normals_f32(p, idx, viewpoint=(0.0, 0.0, 0.0))[0]
    assert ((inward * p).sum(1) < 0).all()
    assert np.array_equal(np.abs(inward), np.abs(normal)) and (inward != normal).any()
    outside = ref.normals_f32(p, idx, viewpoint=(0.0, 0.0, 10.0))[0]
    d = np.array([0, 0, 10], F) - p
    assert ((outside * d).sum(1) > 0).all()
    # a dot product of exactly 0 keeps the default sign: points in z = 0 have the normal (0, 0, 1) exactly, a viewpoint in their plane
    # gives (dx * 0 + dy * 0) + 0 * 1 = 0; one below the plane turns every normal
    g = np.arange(8, dtype=np.float64) / 8
    flat = np.stack([a.ravel() for a in np.meshgrid(g, g, indexing="ij")] + [np.zeros(64)], 1).astype(F)
    _, fidx = ref.self_knn(flat, 8)
    base = ref.normals_f32(flat, fidx)[0]
    assert np.array_equal(base, np.tile(np.array([0, 0, 1], F), (64, 1)))
    in_plane = ref.normals_f32(flat, fidx, viewpoint=(5.0, 5.0, 0.0))[0]
    assert np.array_equal(_bits(in_plane), _bits(base))
    below = ref.normals_f32(flat, fidx, viewpoint=(0.25, 0.25, -1.0))[0]
    assert np.array_equal(below, -base)


# ---- 5: invalid rows ----------------------------------------------------------------------------------------------------------------------
def test_invalid_rows():
    rng = np.random.default_rng(3)
    p = rng.uniform(-0.5, 0.5, size=(300, 3)).astype(F)
    inv_n, inv_t = np.array(ref.INVALID_NORMAL, F), np.array(ref.INVALID_TANGENT, F)

    def invalid(normal, tangent, eig, rows):
        return (np.array_equal(_bits(normal[rows]), _bits(np.tile(inv_n, (len(normal[rows]), 1)))) and
                np.array_equal(_bits(tangent[rows]), _bits(np.tile(inv_t, (len(normal[rows]), 1)))) and not _bits(eig[rows]).any())

    # rows past the length
    _, idx = ref.self_knn(p[:37], 16)
    padded = np.zeros((300, 16), np.int64)
    padded[:37] = idx
    normal, tangent, eig = ref.normals_f32(p, padded, n=37, K=16)
    assert invalid(normal, tangent, eig, slice(37, None)) and eig[:37, 2].all()
    # m = min(K, n) < 3: nothing is valid
    padded = np.zeros((300, 8), np.int64)
    padded[:2, :2] = ref.self_knn(p[:2], 8)[1]
    assert invalid(*ref.normals_f32(p, padded, n=2, K=8), slice(None))
    # 40 copies of one point beside 260 distinct ones: the 16 nearest of a copy are copies, the covariance trace is exactly 0
    q = ref.cloud_with_copies()
    _, idx = ref.self_knn(q, 16)
    normal, tangent, eig = ref.normals_f32(q, idx)
    assert invalid(normal, tangent, eig, slice(100, 140))
    rest = np.r_[0:100, 140:300]
    # (the trace is EXACTLY 0 because the partial sums k * x of the copied point are exact -- its coordinates are dyadic; copies of a
    # point whose partial sums round leave a rounding-level covariance instead: such a row counts as valid, and stays finite and unit)
    r = q.copy()
    r[100:140] = p[100]
    rn, rt, re = ref.normals_f32(r, ref.self_knn(r, 16)[1])
    assert np.isfinite(rn).all() and np.isfinite(rt).all() and np.isfinite(re).all()
    assert np.abs(np.linalg.norm(rn.astype(np.float64), axis=1) - 1).max() < 1e-6 and (re[100:140, 2] < 1e-12).all()
    assert eig[rest, 2].all() and np.abs(np.linalg.norm(normal[rest].astype(np.float64), axis=1) - 1).max() < 1e-6
    # the surfel initialiser gives such rows opacity 0, scale 1e-4, the identity rotation, grey
    d2, _ = ref.self_knn(q, 16)
    g = ref.surfel_init_f32(q, normal, tangent, d2, eigenvalues=eig, colors=np.full((300, 3), 0.25, F))
    want = np.concatenate([q[100:140], np.tile(np.array([0, 1e-4, 1e-4, 1, 0, 0, 0, 0.5, 0.5, 0.5], F), (40, 1))], 1)
    assert np.array_equal(_bits(g[100:140]), _bits(want))
    assert (g[rest, 3] == F(0.1)).all() and (g[rest, 10:13] == F(0.25)).all()
    short = ref.surfel_init_f32(q, normal, tangent, d2, n=3, eigenvalues=eig)        # min(K, n) < 4
    assert not short[:, 3].any() and (short[:, 6] == 1).all()


# ---- 6: the surfel initialiser ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("given_normals", [False, True])
def test_surfel_init_restatement(restated, given_normals):
    """The rasterizer's quaternion -> matrix formula (csrc/surfel_preprocess.hip:51-55, restated in numpy) gives back the frame: third
    column = n and first column orthogonal to n within 1e-5 absolute -- a few products of unit-bounded fp32 numbers are about 10 ulp,
    1.2e-6, the bar has an 8 x margin; w >= 0; the scale is the formula bit for bit; to_raw takes the result as it is."""
    from gaussiananything_amd import fitting
    p, d2, _, normal, tangent, eig = restated["sphere", 16]
    n_in = (p / np.linalg.norm(p, axis=1, keepdims=True)).astype(F) * F(3) if given_normals else normal   # radial, not unit
    colors = np.random.default_rng(1).uniform(0.05, 0.95, size=p.shape).astype(F)
    g, branch = ref.surfel_init_f32(p, n_in, tangent, d2, eigenvalues=eig, colors=colors, opacity=0.1, scale_factor=1.5,
                                    return_branch=True)
    assert g.dtype == F and g.shape == (2048, 13) and np.isfinite(g).all()
    assert set(branch.tolist()) == {0, 1, 2, 3}       # every one of Shepperd's branches is taken on the sphere
    unit = n_in.astype(np.float64) / np.linalg.norm(n_in.astype(np.float64), axis=1, keepdims=True)
    tu, tv, nn = ref.rasterizer_frame(g[:, 6:10])
    print(f"surfel init (given normals {given_normals}): |nn - n| {np.abs(nn - unit).max():.2e}, |tu . n| {np.abs((tu * unit).sum(1)).max():.2e}")
    assert np.abs(nn - unit).max() <= 1e-5
    assert np.abs((tu.astype(np.float64) * unit).sum(1)).max() <= 1e-5 and np.abs((tv.astype(np.float64) * unit).sum(1)).max() <= 1e-5
    assert (g[:, 6] >= 0).all()
    assert np.abs(np.linalg.norm(g[:, 6:10].astype(np.float64), axis=1) - 1).max() <= 2 * 2.0 ** -23
    s = F(1.5) * np.sqrt(np.maximum(((d2[:, 1] + d2[:, 2]) + d2[:, 3]) / F(3), F(1e-7)))
    assert s.dtype == F and np.array_equal(_bits(g[:, 4]), _bits(s)) and np.array_equal(_bits(g[:, 5]), _bits(s))
    assert np.array_equal(g[:, 0:3], p) and (g[:, 3] == F(0.1)).all() and np.array_equal(g[:, 10:13], colors)
    grey = ref.surfel_init_f32(p, n_in, tangent, d2)
    assert (grey[:, 10:13] == F(0.5)).all() and np.array_equal(_bits(grey[:, :10]), _bits(ref.surfel_init_f32(p, n_in, tangent, d2, scale_factor=1.0)[:, :10]))
    t = torch.from_numpy(g)
    raw = fitting.to_raw(t)                               # accepted: no zero quaternion, [N,13]
    assert torch.equal(raw[:, 0:3], t[:, 0:3]) and torch.equal(raw[:, 6:10], t[:, 6:10]) and bool(torch.isfinite(raw).all())
    if not given_normals:     # the disc's first axis is the direction of largest spread: the PCA tangent itself, up to rounding
        assert np.abs(np.abs((tu.astype(np.float64) * tangent).sum(1)) - 1).max() <= 1e-5
    # the floor of the scale: a cloud whose three nearest others are at distance 0 (the point is still valid if its list spreads)
    d0 = d2.copy()
    d0[:, 1:4] = 0
    assert (ref.surfel_init_f32(p, n_in, tangent, d0)[:, 4] == np.sqrt(F(1e-7))).all()


# ---- 7: the oriented PLY --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_colors", [False, True])
def test_oriented_ply_round_trip(tmp_path, restated, with_colors):
    from gaussiananything_amd import io_formats
    p, _, _, normal, _, _ = restated["cube", 8]
    rgb = np.random.default_rng(2).integers(0, 256, size=(len(p), 3)).astype(np.uint8) if with_colors else None
    path = tmp_path / "oriented.ply"
    io_formats.save_oriented_points_ply(path, p, normal, rgb)
    head = path.read_bytes().split(b"end_header\n")[0].decode("ascii").splitlines()
    props = [l.split()[1:] for l in head if l.startswith("property")]
    want = [["float", k] for k in ("x", "y", "z", "nx", "ny", "nz")] + ([["uchar", k] for k in ("red", "green", "blue")] if with_colors else [])
    assert head[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 2048"] and props == want
    xyz, nrm, col = io_formats.load_oriented_points_ply(path)
    assert np.array_equal(_bits(xyz), _bits(p)) and np.array_equal(_bits(nrm), _bits(normal))
    assert (col is None) if not with_colors else np.array_equal(col, rgb)
    assert np.array_equal(io_formats.load_points_ply(path), p)         # a plain PLY reader finds the positions
    if with_colors:     # float colours are scaled and rounded like every other writer here
        io_formats.save_oriented_points_ply(path, p, normal, rgb.astype(np.float64) / 255.0)
        assert np.array_equal(io_formats.load_oriented_points_ply(path)[2], rgb)
    with pytest.raises(ValueError):
        io_formats.save_oriented_points_ply(path, p, normal[:5])
    io_formats.save_points_ply(path, p)
    with pytest.raises(ValueError):
        io_formats.load_oriented_points_ply(path)


# ---- 8: refusals ----------------------------------------------------------------------------------------------------------------------------
def _lib():
    from gaussiananything_amd import _lib
    return _lib, _lib.lib()


def test_host_validation_rejects_before_any_launch():
    """Fake, non-NULL device addresses: a call that got past validation would fault; every one here must be turned away."""
    _l, L = _lib()
    P = 0x1000   # never dereferenced

    def normals(B=2, N=10, k=8, points=P, idx=P, normal=P):
        a = _l.GaNormalsArgs(B, N, k, 0, points, None, idx, None, normal, None, None)
        return L.ga_pc_normals(ctypes.byref(a), None)

    def init(B=2, N=10, k=8, points=P, normal=P, tangent=P, dist2=P, out=P):
        a = _l.GaSurfelInitArgs(B, N, k, 0.1, 1.0, 0, points, normal, tangent, dist2, None, None, None, out)
        return L.ga_pc_surfel_init(ctypes.byref(a), None)

    assert L.ga_pc_normals(None, None) == GA_ERR_NULL_ARG and L.ga_pc_surfel_init(None, None) == GA_ERR_NULL_ARG
    for kw in (dict(points=None), dict(idx=None), dict(normal=None)):
        assert normals(**kw) == GA_ERR_NULL_ARG, kw
    for kw in (dict(points=None), dict(normal=None), dict(tangent=None), dict(dist2=None), dict(out=None)):
        assert init(**kw) == GA_ERR_NULL_ARG, kw
    shapes = (dict(B=0), dict(B=65536), dict(N=0), dict(N=-1), dict(k=33), dict(k=-1), dict(N=(1 << 31) // 3 + 1, k=3),
              dict(N=1 << 26, k=32), dict(N=1 << 27, k=16))
    for kw in shapes + (dict(k=2), dict(k=0)):
        assert normals(**kw) == GA_ERR_BAD_SHAPE, kw
    for kw in shapes + (dict(k=3), dict(k=0)):
        assert init(**kw) == GA_ERR_BAD_SHAPE, kw


def test_normals_plan_is_host_only():
    _l, L = _lib()
    pl = _l.GaNormalsPlan()
    assert L.ga_pc_normals_plan(100, 8, None) == GA_ERR_NULL_ARG
    for bad in ((0, 8), (100, 2), (100, 33), (1 << 26, 32), ((1 << 31) // 3 + 1, 3)):
        assert L.ga_pc_normals_plan(*bad, ctypes.byref(pl)) == GA_ERR_BAD_SHAPE, bad
    for n in (1, 255, 256, 257, 100000):
        assert L.ga_pc_normals_plan(n, 16, ctypes.byref(pl)) == 0
        assert pl.threads > 0 and pl.threads % 64 == 0 and pl.grid_x == -(-n // pl.threads) and pl.grid_y == 1
        assert pl.sweeps == _l.GA_PC_NORMALS_SWEEPS
    from gaussiananything_amd import pointcloud
    d = pointcloud.normals_plan(4096, 16)
    assert set(d) == {"threads", "grid_x", "grid_y", "sweeps"} and d["grid_x"] * d["threads"] >= 4096
    with pytest.raises(RuntimeError):
        pointcloud.normals_plan(4096, 2)


def test_ctypes_mirrors_have_the_layout_of_the_header(tmp_path):
    from gaussiananything_amd import _lib as _l
    mirrors = [_l.GaNormalsArgs, _l.GaNormalsPlan, _l.GaSurfelInitArgs]
    consts = ("GA_PC_NORMALS_SWEEPS", "GA_PC_NORMALS_MIN_K", "GA_PC_SURFEL_MIN_K", "GA_PC_SURFEL_FLOATS", "GA_PC_KNN_MAX_K")
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "ga_pointcloud.h"', "int main(void) {"]
    lines += [f'  printf("{c} %d\\n", {c});' for c in consts]
    for cls in mirrors:
        lines.append(f'  printf("{cls.__name__} %zu\\n", sizeof({cls.__name__}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cls.__name__}.{fname} %zu\\n", offsetof({cls.__name__}, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for c in consts:
        assert int(got[c]) == getattr(_l, c), c
    for cls in mirrors:
        assert int(got[cls.__name__]) == ctypes.sizeof(cls), cls.__name__
        for fname, _ in cls._fields_:
            assert int(got[f"{cls.__name__}.{fname}"]) == getattr(cls, fname).offset, (cls.__name__, fname)


def test_front_ends_validate_on_the_host():
    from gaussiananything_amd import fitting, pointcloud
    from gaussiananything_amd.fitting import SurfelFitter
    a = torch.zeros(1, 10, 3)
    for K in (2, 0, 33):
        with pytest.raises(ValueError, match="32"):
            pointcloud.estimate_normals(a, K=K)
    for K in (3, 33):
        with pytest.raises(ValueError, match="32"):
            fitting.surfels_from_points(a, K=K)
    with pytest.raises(RuntimeError, match="GPU"):     # GPU only, no fallback
        pointcloud.estimate_normals(a, K=8)
    with pytest.raises(RuntimeError, match="GPU"):
        fitting.surfels_from_points(a[0])
    with pytest.raises(RuntimeError, match="GPU"):
        SurfelFitter.from_points(a[0], torch.zeros(2, 4, 4), torch.zeros(2, 4, 4), 0.5, torch.zeros(2, 3, 32, 32))
    for bad in (torch.zeros(10, 3), torch.zeros(1, 10, 2), torch.zeros(1, 0, 3), np.zeros((1, 10, 3), F)):
        with pytest.raises(ValueError):
            pointcloud.estimate_normals(bad)
    for bad in (torch.zeros(2, 10, 3), torch.zeros(10, 4), torch.zeros(10)):
        with pytest.raises(ValueError):
            fitting.surfels_from_points(bad)
    with pytest.raises(TypeError):
        fitting.surfels_from_points(np.zeros((10, 3), F))
    with pytest.raises(ValueError):
        fitting.surfels_from_points(a, colors=torch.zeros(1, 9, 3, 1))
    with pytest.raises(ValueError):
        fitting.surfels_from_points(a, opacity=1.5)
    with pytest.raises(ValueError):
        fitting.surfels_from_points(a, scale_factor=0.0)
