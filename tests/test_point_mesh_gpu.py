"""GPU tests of ``ga_mesh_point_distance`` (include/ga_mesh.h, csrc/mesh_ops.hip) and of what is built on it.

The raw C-ABI call is compared with the numpy restatement (tests/_mesh_ops_ref.py) for EQUALITY, bit for bit: squared distance, face,
closest point and barycentric weights, padding rows included.  Every raw call poisons its outputs first and checks guard words behind
each of them and behind the workspace.  Tile and chunk sizes come from ``ga_mesh_point_distance_plan``."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _mesh_bounds as bounds
from tests import _mesh_ops_ref as ref
from tests.test_mesh_sample_gpu import GUARD_WORD, _guarded, _same, _take

pytestmark = pytest.mark.gpu

F32 = np.float32


def plan(n, f):
    from gaussiananything_amd import mesh
    return mesh.point_mesh_distance_plan(n, f)


def raw_distance(device, points, vertices, faces, count=None):
    """one guarded ``ga_mesh_point_distance`` call -> dict of numpy outputs"""
    from gaussiananything_amd import _lib
    L = _lib.lib()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)   # noqa: E731
    p, v, f = dev(np.asarray(points, F32)), dev(np.asarray(vertices, F32)), dev(np.asarray(faces, np.int32))
    N = p.shape[0]
    cnt = torch.tensor([count], dtype=torch.int32, device=device) if count is not None else None
    dist2, face, closest, bary = _guarded(N, device), _guarded(N, device), _guarded(3 * N, device), _guarded(3 * N, device)
    ws_bytes = plan(N, f.shape[0])["workspace_bytes"]
    assert ws_bytes % 8 == 0
    ws = _guarded(ws_bytes // 4, device)
    args = _lib.GaMeshPointDistanceArgs(N, v.shape[0], f.shape[0], 0, p.data_ptr(), cnt.data_ptr() if cnt is not None else None,
                                        v.data_ptr(), f.data_ptr(), dist2.data_ptr(), face.data_ptr(), closest.data_ptr(),
                                        bary.data_ptr(), ws.data_ptr(), ws_bytes)
    with torch.cuda.device(device):
        _lib.check(L.ga_mesh_point_distance(ctypes.byref(args), ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)),
                   "ga_mesh_point_distance")
        torch.cuda.synchronize()
    assert bool((ws[ws_bytes // 4:] == GUARD_WORD).all()), "guard words behind the workspace overwritten"
    assert np.array_equal(p.cpu().numpy().view(np.uint32), np.asarray(points, F32).view(np.uint32)), "the queries were written to"
    return dict(dist2=_take(dist2, N, (N,)), face=_take(face, N, (N,), torch.int32), closest=_take(closest, 3 * N, (N, 3)),
                bary=_take(bary, 3 * N, (N, 3)))


def _check(got, want):
    assert np.array_equal(got["face"], want["face"]), f"faces differ at {np.nonzero(got['face'] != want['face'])[0][:8].tolist()}"
    for k in ("dist2", "closest", "bary"):
        _same(got[k], want[k], k)


def _queries(vertices, faces, n, seed=0):
    """n queries: the region queries of the first valid faces, then seeded points around the mesh's box"""
    good = faces[ref.triangles(vertices, faces)["w"] > 0]
    q = ref.region_queries(vertices, good[:max(1, n // 7)])[:n]
    lo, hi = vertices.min(0) - 0.2, vertices.max(0) + 0.2
    rest = np.random.default_rng(seed).uniform(lo, hi, (n - q.shape[0], 3)).astype(F32)
    return np.concatenate([q, rest])


def _soup_of(num_faces):
    return ref.soup(num_faces, seed=3)


@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("faces", ["one", "tile-1", "tile+1"])
def test_distance_bits(gpu_device, n, faces):
    tile = plan(1, 1)["tile"]
    F = {"one": 1, "tile-1": tile - 1, "tile+1": tile + 1}[faces]
    if faces == "tile+1":                        # at these sizes a chunk is one tile: the last face is also one beyond a chunk
        assert plan(n, F)["tiles_per_chunk"] == 1 and plan(n, F)["num_chunks"] == 2
    v, f = _soup_of(F)
    q = _queries(v, f, n, seed=n)
    _check(raw_distance(gpu_device, q, v, f), ref.point_distance(q, v, f))


def test_one_face_beyond_a_chunk_of_several_tiles(gpu_device):
    """the smallest mesh whose plan has chunks of at least two tiles and whose last chunk holds ONE face; the query sits on that face"""
    tile = plan(1, 1)["tile"]
    for tiles in range(3, 1 << 14):
        pl = plan(1, (tiles - 1) * tile + 1)
        if pl["tiles_per_chunk"] >= 2 and (tiles - 1) % pl["tiles_per_chunk"] == 0:
            break
    else:
        pytest.fail("no such plan below 2^14 tiles")
    F = (tiles - 1) * tile + 1
    assert pl["num_chunks"] == (tiles - 1) // pl["tiles_per_chunk"] + 1
    v, f = ref.strip(F)
    q = np.concatenate([ref.region_queries(v, f[-1:])[6:], ref.region_queries(v, f[:1])[6:]])   # above the last and the first face
    want = ref.point_distance(q, v, f)
    assert want["face"].tolist() == [F - 1, 0]
    _check(raw_distance(gpu_device, q, v, f), want)


@pytest.mark.parametrize("name", ["soup", "spliced", "ties"])
def test_regions_ties_and_spliced_soup(gpu_device, name):
    from tests.test_mesh_ops_cpu import distance_queries, zoo
    v, f = zoo()[name]
    q = distance_queries(name)
    want = ref.point_distance(q, v, f)
    assert (np.bincount(want["region"], minlength=7) > 0).all()
    _check(raw_distance(gpu_device, q, v, f), want)


def test_device_count_pads_the_rest(gpu_device):
    from tests.test_mesh_ops_cpu import distance_queries, zoo
    v, f = zoo()["spliced"]
    q = distance_queries("spliced")[:600]
    for count in (0, 1, 256, 257, 599, 600, 100000, -5):
        got = raw_distance(gpu_device, q, v, f, count=count)
        want = ref.point_distance(q, v, f, count=count)
        live = max(0, min(600, count))
        assert (got["face"][live:] == -1).all() and not got["dist2"][live:].view(np.uint32).any()
        _check(got, want)


def test_no_valid_triangle(gpu_device):
    v, f = _soup_of(300)
    q = _queries(v, f, 300)
    dead = np.zeros_like(f)
    dead[5] = (0, 1, 10 ** 6)
    got = raw_distance(gpu_device, q, v, dead)
    assert np.isposinf(got["dist2"]).all() and (got["face"] == -1).all()
    assert not got["closest"].view(np.uint32).any() and not got["bary"].view(np.uint32).any()
    q[3, 1] = np.nan                                   # a NaN query among live triangles: +inf / -1 too
    got = raw_distance(gpu_device, q, v, f)
    assert np.isposinf(got["dist2"][3]) and got["face"][3] == -1 and (got["face"][np.arange(300) != 3] >= 0).all()


def test_front_end_on_an_untrimmed_cloud(gpu_device):
    import collections
    from gaussiananything_amd import mesh
    from tests.test_mesh_ops_cpu import distance_queries, zoo
    v, f = zoo()["soup"]
    q = distance_queries("soup")
    tv, tf, tq = (torch.from_numpy(a).to(gpu_device) for a in (v, f, q))
    want = ref.point_distance(q, v, f, count=100)
    cloud = collections.namedtuple("Cloud", "points count")(tq, torch.tensor([100], dtype=torch.int32, device=gpu_device))
    r = mesh.point_mesh_distance(cloud, tv, tf)
    assert r.face.dtype == torch.int64
    _check(dict(dist2=r.dist2.cpu().numpy(), face=r.face.cpu().numpy().astype(np.int32), closest=r.closest.cpu().numpy(),
                bary=r.bary.cpu().numpy()), want)
    with pytest.raises(RuntimeError):
        mesh.point_mesh_distance(tq.cpu(), tv.cpu(), tf.cpu())


def test_gradients_against_float64_autograd(gpu_device):
    """``differentiable=True``: the gradients with respect to points and vertices against autograd through a float64 torch brute force
    (closest point by the same region test, minimum over the faces).  Queries: the region set of the soup, ties removed (there are none
    in a soup: asserted).  Tolerance: the relative bound of tests/_mesh_bounds.py on dist2, scaled by the extent -- the gradient is
    2 (p - closest), a length where dist2 is a length squared."""
    from gaussiananything_amd import mesh
    from tests.test_mesh_ops_cpu import distance_queries, zoo
    v, f = zoo()["soup"]
    q = distance_queries("soup")
    d, _ = ref.pair_dist2(q, v, f)
    two = np.sort(d, axis=1)[:, :2]
    keep = two[:, 0] != two[:, 1]
    assert keep.all()
    tv = torch.from_numpy(v).to(gpu_device).requires_grad_(True)
    tq = torch.from_numpy(q).to(gpu_device).requires_grad_(True)
    tf = torch.from_numpy(f).to(gpu_device)
    r = mesh.point_mesh_distance(tq, tv, tf, differentiable=True)
    weight = torch.linspace(0.5, 1.5, q.shape[0], device=gpu_device)
    (r.dist2 * weight).sum().backward()
    plain = mesh.point_mesh_distance(tq, tv, tf)
    assert not plain.dist2.requires_grad
    # the torch expression moves the nearest point by at most delta = 8 eps extent (three products, two sums, against the kernel's
    # a + ab v + ac w), so dist2 by at most 2 dist delta + delta^2, plus the rounding of its own three squares
    extent = float(np.abs(v).max())
    delta = 8 * float(np.finfo(F32).eps) * extent
    slack = 2 * plain.dist2.sqrt() * delta + delta ** 2 + 4 * float(np.finfo(F32).eps) * plain.dist2
    assert bool(((r.dist2.detach() - plain.dist2).abs() <= slack).all())

    v64 = torch.from_numpy(v).double().requires_grad_(True)
    q64 = torch.from_numpy(q).double().requires_grad_(True)
    d64 = _dist2_torch64(q64, v64, torch.from_numpy(f).long())
    (d64 * weight.cpu().double()).sum().backward()
    tol = bounds.DIST2_REL_BOUND * extent
    assert float((tq.grad.cpu().double() - q64.grad).abs().max()) <= tol
    assert float((tv.grad.cpu().double() - v64.grad).abs().max()) <= tol


def _dist2_torch64(p, v, f):
    """float64 brute force in torch, differentiable: min over faces of the squared distance to the closest point (Ericson 5.1.5)"""
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    p = p[:, None, :]
    ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
    dot = lambda x, y: (x * y).sum(-1)   # noqa: E731
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    safe = lambda x: torch.where(x == 0, torch.ones_like(x), x)   # noqa: E731
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    pts = [a.expand_as(ap), b.expand_as(ap), a + (d1 / safe(d1 - d3))[..., None] * ab, c.expand_as(ap),
           a + (d2 / safe(d2 - d6))[..., None] * ac, b + ((d4 - d3) / safe((d4 - d3) + (d5 - d6)))[..., None] * (c - b)]
    den = safe(va + vb + vc)
    closest = a + ab * (vb / den)[..., None] + ac * (vc / den)[..., None]
    for cond, pt in zip(reversed(conds), reversed(pts)):
        closest = torch.where(cond[..., None], pt, closest)
    return ((p - closest) ** 2).sum(-1).min(dim=1).values


def test_mesh_cloud_distance_on_the_icosphere(gpu_device):
    """the 1280-face icosphere against points ON the unit sphere: every point lies within the largest sagitta of the inscribed mesh
    (the sphere's radius minus the smallest distance of a face's plane from the centre), so completeness stays below it, the F-score
    is 1 at a threshold above it and 0 at threshold 0"""
    from gaussiananything_amd import mesh
    v, f = ref.icosphere(3)
    tri = v[f].astype(np.float64)
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    sagitta = float(1.0 - np.abs((tri[:, 0] * n).sum(1)).min())
    assert 0 < sagitta < 0.01
    pts = np.random.default_rng(8).normal(size=(20000, 3))
    pts = (pts / np.linalg.norm(pts, axis=1, keepdims=True)).astype(F32)
    tv, tf, tp = (torch.from_numpy(a).to(gpu_device) for a in (v, f, pts))
    out = mesh.mesh_cloud_distance(tv, tf, tp, num_samples=20000, threshold=sagitta + 0.1, seed=4)
    assert all(t.device.type == "cuda" and t.dim() == 0 for t in out.values())
    assert 0 < float(out["completeness"]) < sagitta + 1e-6
    assert 0 < float(out["accuracy"]) < 0.1                      # 20 000 points on the sphere: every sample has one nearby
    assert float(out["fscore"]) == 1.0 and float(out["precision"]) == 1.0 and float(out["recall"]) == 1.0
    zero = mesh.mesh_cloud_distance(tv, tf, tp, num_samples=20000, threshold=0.0, seed=4)
    assert float(zero["fscore"]) == 0.0
    assert set(mesh.mesh_cloud_distance(tv, tf, tp, num_samples=1000)) == {"accuracy", "completeness"}
