"""CPU tests of the restatement of the mesh-input operations (tests/_mesh_ops_ref.py) -- against float64, against the statistics a sampler
owes, and against itself -- and of ``io_formats.load_obj``.  The GPU tests then hold the kernels to this restatement bit for bit."""
import functools

import numpy as np
import pytest

from tests import _mesh_bounds as bounds
from tests import _mesh_ops_ref as ref

F32 = np.float32
EPS = float(np.finfo(F32).eps)


@functools.lru_cache(maxsize=None)
def zoo():
    """name -> (vertices, faces): every mesh of the zoo"""
    z = {f"icosphere{s}": ref.icosphere(s) for s in range(4)}
    z["square"] = ref.unit_square()
    z["pair"] = ref.pair_1_3()
    z["soup"] = ref.soup()
    z["spliced"] = ref.spliced_soup()[:2]
    z["ties"] = ref.tie_mesh_and_queries()[:2]
    return z


@functools.lru_cache(maxsize=None)
def distance_queries(name):
    """the query set of a zoo mesh: the seven region queries of each of (at most 96 of) its valid faces, and the tie queries on 'ties'"""
    v, f = zoo()[name]
    good = f[ref.triangles(v, f)["w"] > 0][:96]
    q = ref.region_queries(v, good, offset=0.02 if name != "icosphere3" else 0.005, height=0.01)
    if name == "ties":
        q = np.concatenate([ref.tie_mesh_and_queries()[2], q])
    return q


@pytest.mark.parametrize("name", ["icosphere0", "icosphere2", "square", "soup", "spliced"])
def test_barycentric_weights_and_points(name):
    v, f = zoo()[name]
    s = ref.sample(v, f, 4000, seed=11)
    b = s["bary"].astype(np.float64)
    assert (s["bary"] >= 0).all() and (s["face"] >= 0).all()
    assert np.abs(b.sum(1) - 1.0).max() <= 4 * EPS
    tri = v[f[s["face"]]].astype(np.float64)                       # [S,3,3]
    extent = np.abs(v).max()
    exact = (b[:, :, None] * tri).sum(1)
    assert np.abs(s["points"] - exact).max() <= 4 * EPS * extent   # three products and two sums of magnitudes <= extent
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    off_plane = np.abs(((s["points"] - tri[:, 0]) * n).sum(1))
    assert off_plane.max() <= 8 * EPS * extent
    assert np.abs((s["normals"].astype(np.float64) * n).sum(1) - 1.0).max() <= 1e-5
    # inside the face: the float64 distance of the point to its own triangle is rounding only
    for k in range(0, 4000, 500):
        d, _, _ = ref.point_distance64(s["points"][k:k + 1], v, f[s["face"][k:k + 1]])
        assert d[0] <= (8 * EPS * extent) ** 2


def test_face_shares_of_the_1_to_3_pair():
    v, f = zoo()["pair"]
    S = 40000
    face = ref.sample(v, f, S, seed=5)["face"]
    for k, share in ((0, 0.25), (1, 0.75)):
        sd = (share * (1 - share) / S) ** 0.5
        assert abs((face == k).mean() - share) <= 4 * sd


def test_chi_square_on_the_icosphere():
    """face counts against areas on the 1280-face icosphere: 64 000 samples (50 expected per face), chi-square with 1279 degrees of
    freedom.  The bound is its 0.9999 quantile by Wilson-Hilferty, k (1 - 2/(9k) + z sqrt(2/(9k)))^3 with z = 3.719: 1475.7."""
    v, f = zoo()["icosphere3"]
    S = 64000
    face = ref.sample(v, f, S, seed=3)["face"]
    w = ref.triangles(v, f)["w"].astype(np.float64)
    expected = S * w / w.sum()
    counts = np.bincount(face, minlength=f.shape[0])
    chi2 = ((counts - expected) ** 2 / expected).sum()
    k = f.shape[0] - 1
    quantile = k * (1 - 2 / (9 * k) + 3.719 * (2 / (9 * k)) ** 0.5) ** 3
    assert quantile == pytest.approx(1475.7, abs=0.1)
    assert chi2 <= quantile, chi2


def test_weight_zero_faces_are_never_drawn():
    v, f, dead = ref.spliced_soup()
    assert dead.sum() >= 10 and (ref.triangles(v, f)["w"][dead] == 0).all() and (ref.triangles(v, f)["w"][~dead] > 0).all()
    for seed in (0, 1, 2):
        face = ref.sample(v, f, 20000, seed=seed)["face"]
        assert not dead[face].any()
    # every face but one dead: all samples on the live one, wherever it stands in its group
    v2, f2 = ref.strip(600)
    for live in (0, 255, 256, 599):
        g = np.zeros_like(f2)
        g[live] = f2[live]
        assert (ref.sample(v2, g, 500, seed=live)["face"] == live).all()
    # nothing to draw from
    s = ref.sample(v2, np.zeros_like(f2), 16, seed=0)
    assert (s["face"] == -1).all() and not s["points"].any() and not s["bary"].any()


def test_query_set_covers_every_region_and_the_ties():
    """a condition on the INPUTS of the distance tests: each of the seven regions wins somewhere, and both kinds of tie are there"""
    for name in ("soup", "spliced", "ties"):
        v, f = zoo()[name]
        r = ref.point_distance(distance_queries(name), v, f)
        assert (r["face"] >= 0).all()
        won = np.bincount(r["region"], minlength=7)
        assert (won > 0).all(), (name, dict(zip(ref.REGIONS, won.tolist())))
    v, f, q, ties = ref.tie_mesh_and_queries()
    d, _ = ref.pair_dist2(q, v, f)
    r = ref.point_distance(q, v, f)
    for row, faces in enumerate(ties):
        assert all(d[row, k].tobytes() == d[row].min().tobytes() for k in faces), (row, d[row])
        assert r["face"][row] == min(faces)          # the lowest face among equals
    assert f[ties[0][0]].tolist() != f[ties[0][1]].tolist() and len(set(f[ties[0][0]]) & set(f[ties[0][1]])) == 2   # a shared edge
    assert f[ties[1][0]].tolist() == f[ties[1][1]].tolist()                                                     # a duplicate


def measured_error(name):
    """the largest |dist2 - dist2_64| / (dist2_64 + extent^2 eps) of a zoo mesh over its query set, and the same between the float64
    distances of the two chosen faces where the choices differ"""
    v, f = zoo()[name]
    q = distance_queries(name)
    got = ref.point_distance(q, v, f)
    want, face64, all64 = ref.point_distance64(q, v, f)
    scale = want + float(np.abs(v).max()) ** 2 * EPS
    err = np.abs(got["dist2"].astype(np.float64) - want) / scale
    other = got["face"] != face64
    swap = np.abs(all64[np.arange(q.shape[0]), got["face"]] - want) / scale
    return float(err.max()), float(swap[other].max()) if other.any() else 0.0


def test_restatement_against_float64():
    assert set(bounds.MEASURED) == set(zoo())
    for name in zoo():
        err, swap = measured_error(name)
        print(f"{name}: {err:.3e} (faces differ: {swap:.3e})")
        assert err <= bounds.DIST2_REL_BOUND, (name, err)
        assert swap <= bounds.DIST2_REL_BOUND, (name, swap)


def test_padding_and_no_valid_triangle():
    v, f = zoo()["soup"]
    q = distance_queries("soup")[:20]
    r = ref.point_distance(q, v, f, count=13)
    full = ref.point_distance(q, v, f)
    assert (r["face"][13:] == -1).all() and not r["dist2"][13:].any() and not r["closest"][13:].any() and not r["bary"][13:].any()
    assert np.array_equal(r["dist2"][:13], full["dist2"][:13]) and np.array_equal(r["face"][:13], full["face"][:13])
    none = ref.point_distance(q, v, np.zeros_like(f))
    assert np.isposinf(none["dist2"]).all() and (none["face"] == -1).all() and not none["closest"].any()


def test_load_obj_round_trips_write_obj(tmp_path):
    from gaussiananything_amd import io_formats, mesh
    v, f = zoo()["icosphere1"]
    c = np.random.default_rng(0).uniform(0, 1, v.shape).astype(F32)
    path = str(tmp_path / "ico.obj")
    mesh.write_obj(path, v, c, f)
    v2, f2, c2 = io_formats.load_obj(path)
    assert np.array_equal(f2, f) and f2.dtype == np.int32
    assert np.abs(v2 - v).max() <= 1e-6 and np.abs(c2 - c).max() <= 1e-5
    io_formats.save_obj(v, f, c, path)                 # z mirrored, winding reversed: read back as written
    v3, f3, c3 = io_formats.load_obj(path)
    assert np.array_equal(f3, f[:, ::-1]) and np.abs(v3 - v * np.asarray([1, 1, -1], F32)).max() <= 1e-6
    assert np.abs(c3 - c).max() <= 1 / 255


def test_load_obj_reads_quads_slashes_and_negative_indices(tmp_path):
    from gaussiananything_amd import io_formats
    path = tmp_path / "hand.obj"
    path.write_text("# a square, a pentagon fan and friends\n"
                    "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0.5 0.5\nvn 0 0 1\n"
                    "f 1 2 3 4\n"
                    "v 2 0 0\n"
                    "f 2/1 5/1 3/1\n"
                    "f -1//1 -3//1 -4//1\n"
                    "f 1/1/1 2/1/1 5/1/1 3/1/1 4/1/1\n"
                    "g tail\nf 1 2 3\n")
    v, f, c = io_formats.load_obj(str(path))
    assert c is None and v.shape == (5, 3) and v.dtype == F32
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [1, 4, 2], [4, 2, 1], [0, 1, 4], [0, 4, 2], [0, 2, 3], [0, 1, 2]]
    with pytest.raises(ValueError):
        bad = tmp_path / "bad.obj"
        bad.write_text("v 0 0 0\nf 1 2 3\n")
        io_formats.load_obj(str(bad))


def test_ctypes_mirrors_have_the_layout_of_the_header(tmp_path):
    """one compiled check of the sizes, every field offset and the constants of include/ga_mesh.h against gaussiananything_amd/_lib.py,
    and of the restatement's constants"""
    import ctypes
    import os
    import subprocess
    from gaussiananything_amd import _lib as _l
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mirrors = [_l.GaMeshSampleArgs, _l.GaMeshSamplePlan, _l.GaMeshPointDistanceArgs, _l.GaMeshPointDistancePlan]
    consts = ("GA_MESH_THREADS", "GA_MESH_PHILOX_STREAM", "GA_MESH_MAX_FACES", "GA_MESH_MAX_ROWS", "GA_MESH_AREA_FACES")
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "ga_mesh.h"', "int main(void) {"]
    lines += [f'  printf("{c} %lld\\n", (long long)({c}));' for c in consts]
    for cls in mirrors:
        lines.append(f'  printf("{cls.__name__} %zu\\n", sizeof({cls.__name__}));')
        lines += [f'  printf("{cls.__name__}.{n} %zu\\n", offsetof({cls.__name__}, {n}));' for n, _ in cls._fields_]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for c in consts[:-1]:
        assert int(got[c]) == getattr(_l, c), c
    assert int(got["GA_MESH_AREA_FACES"]) == ref.FACES_PER_GROUP and int(got["GA_MESH_PHILOX_STREAM"]) == ref.PHILOX_STREAM
    for cls in mirrors:
        assert int(got[cls.__name__]) == ctypes.sizeof(cls), cls.__name__
        for n, _ in cls._fields_:
            assert int(got[f"{cls.__name__}.{n}"]) == getattr(cls, n).offset, (cls.__name__, n)


def test_plans_and_host_refusals():
    """the plans (host only) and the refusals that come before anything touches a device, with fake addresses"""
    import ctypes
    from gaussiananything_amd import _lib as _l
    from gaussiananything_amd import mesh
    L = _l.lib()
    sp = mesh.mesh_sample_plan(65537, 10)
    assert (sp["faces_per_group"], sp["sums_per_trip"], sp["num_groups"]) == (256, 256, 257) and sp["workspace_bytes"] % 16 == 0
    assert sp["workspace_bytes"] >= 8 * (257 + 1 + 65537)
    for n, f in ((1, 1), (257, 257), (4096, 1000000), (100000, 20480)):
        dp = mesh.point_mesh_distance_plan(n, f)
        tiles = -(-f // dp["tile"])
        assert dp["num_chunks"] == -(-tiles // dp["tiles_per_chunk"]) <= 1024
        assert dp["workspace_bytes"] == 64 * f + 8 * dp["num_chunks"] * n
    assert mesh.point_mesh_distance_plan(4096, 1000000)["num_chunks"] >= 32       # few queries, many faces: the grid is split
    for bad in ((0, 1), (1, 0), (_l.GA_MESH_MAX_FACES + 1, 1)):
        assert L.ga_mesh_sample_plan(bad[0], bad[1], ctypes.byref(_l.GaMeshSamplePlan())) == -2
        assert L.ga_mesh_point_distance_plan(bad[1], bad[0], ctypes.byref(_l.GaMeshPointDistancePlan())) == -2
    assert L.ga_mesh_sample_plan(1, 1, None) == -1 and L.ga_mesh_sample(None, None) == -1 and L.ga_mesh_point_distance(None, None) == -1
    fake = 1 << 20
    sample = lambda **kw: _l.GaMeshSampleArgs(**dict(dict(num_vertices=3, num_faces=1, num_samples=4, vertices=fake, faces=fake,  # noqa: E731
                                                          points=fake, face=fake, bary=fake, workspace=fake, workspace_bytes=1 << 12), **kw))
    dist = lambda **kw: _l.GaMeshPointDistanceArgs(**dict(dict(num_points=4, num_vertices=3, num_faces=1, points=fake, vertices=fake,  # noqa: E731
                                                               faces=fake, dist2=fake, face=fake, closest=fake, bary=fake, workspace=fake,
                                                               workspace_bytes=1 << 12), **kw))
    for kw, code in ((dict(num_faces=0), -2), (dict(num_vertices=0), -2), (dict(num_samples=-1), -2), (dict(reserved=2), -5),
                     (dict(points=None), -1), (dict(colors=fake), -1), (dict(vertex_colors=fake), -1), (dict(workspace_bytes=8), -3),
                     (dict(workspace=fake + 8), -3)):
        assert L.ga_mesh_sample(ctypes.byref(sample(**kw)), None) == code, kw
    for kw, code in ((dict(num_points=0), -2), (dict(num_faces=-3), -2), (dict(num_vertices=0), -2), (dict(reserved=1), -5),
                     (dict(dist2=None), -1), (dict(bary=None), -1), (dict(workspace_bytes=64), -3), (dict(workspace=fake + 4), -3)):
        assert L.ga_mesh_point_distance(ctypes.byref(dist(**kw)), None) == code, kw
