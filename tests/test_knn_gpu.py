"""GPU tests of ``ga_pc_knn`` / ``ga_pc_knn_backward`` (include/ga_pointcloud.h, csrc/pointcloud.hip) and of what is built on them.

The forward kernel is compared with the numpy float32 restatement (tests/_knn_ref.py) for EQUALITY -- indices with
``np.array_equal``, distances bit for bit -- and with the float64 brute force on dyadic lattice clouds; the backward kernel with the
contract's float32 loop, bit for bit on both outputs.  Shapes are taken from ``ga_pc_knn_plan`` (T = queries per workgroup, L =
targets per LDS tile), so the cases sit on the kernel's boundaries without knowing its constants.  Every raw call poisons its outputs
first and checks guard words behind each of them."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _knn_ref as kref
from tests import _pointcloud_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 64            # int32 words behind every buffer
GUARD_WORD = 0x5A5A5A5A
POISON = -77


def _guarded(n_words, device):
    t = torch.full((n_words + GUARD,), GUARD_WORD, dtype=torch.int32, device=device)
    t[:n_words] = POISON
    return t


def _guards_intact(t, n_words):
    return bool((t[n_words:] == GUARD_WORD).all())


def _plan(nq=1000, nt=1000, K=1):
    from gaussiananything_amd import pointcloud
    return pointcloud.knn_plan(nq, nt, K)


def _TL():
    pl = _plan()
    return pl["threads"], pl["tile"]


def _slot_classes():
    return sorted({_plan(K=k)["k_slots"] for k in range(1, 33)})


def _dev(a, dtype, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype) if a is not None else None


def raw_knn(query, target, K, qlen=None, tlen=None, device="cuda:0"):
    """ga_pc_knn on a padded numpy batch through the C-ABI -> (dist2 [B,Nq,K] float32, idx [B,Nq,K] int32)"""
    from gaussiananything_amd import _lib
    B, Nq, _ = query.shape
    Nt = target.shape[1]
    q, t = _dev(query, torch.float32, device), _dev(target, torch.float32, device)
    ql = torch.tensor(qlen, dtype=torch.int32, device=device) if qlen is not None else None
    tl = torch.tensor(tlen, dtype=torch.int32, device=device) if tlen is not None else None
    n = B * Nq * K
    od, oi = _guarded(n, device), _guarded(n, device)
    args = _lib.GaKnnArgs(B, Nq, Nt, K, q.data_ptr(), t.data_ptr(), ql.data_ptr() if ql is not None else None,
                          tl.data_ptr() if tl is not None else None, od.data_ptr(), oi.data_ptr())
    with torch.cuda.device(device):
        _lib.check(_lib.lib().ga_pc_knn(ctypes.byref(args), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "ga_pc_knn")
        torch.cuda.synchronize()
    assert _guards_intact(od, n) and _guards_intact(oi, n)
    idx = oi[:n].reshape(B, Nq, K).cpu().numpy()
    assert not (idx == POISON).any()   # every slot written
    return od[:n].view(torch.float32).reshape(B, Nq, K).cpu().numpy(), idx


def raw_knn_backward(query, target, idx, grad, qlen=None, tlen=None, device="cuda:0", want_query=True, want_target=True):
    """ga_pc_knn_backward through the C-ABI -> (grad_query [B,Nq,3] or None, grad_target [B,Nt,3] or None)"""
    from gaussiananything_amd import _lib
    B, Nq, _ = query.shape
    Nt = target.shape[1]
    K = idx.shape[2]
    q, t = _dev(query, torch.float32, device), _dev(target, torch.float32, device)
    ix, g = _dev(idx, torch.int32, device), _dev(grad, torch.float32, device)
    ql = torch.tensor(qlen, dtype=torch.int32, device=device) if qlen is not None else None
    tl = torch.tensor(tlen, dtype=torch.int32, device=device) if tlen is not None else None
    gq = _guarded(B * Nq * 3, device) if want_query else None
    gt = _guarded(B * Nt * 3, device) if want_target else None
    args = _lib.GaKnnBackwardArgs(B, Nq, Nt, K, q.data_ptr(), t.data_ptr(), ql.data_ptr() if ql is not None else None,
                                  tl.data_ptr() if tl is not None else None, ix.data_ptr(), g.data_ptr(),
                                  gq.data_ptr() if want_query else None, gt.data_ptr() if want_target else None)
    with torch.cuda.device(device):
        _lib.check(_lib.lib().ga_pc_knn_backward(ctypes.byref(args), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                   "ga_pc_knn_backward")
        torch.cuda.synchronize()
    out = []
    for buf, n in ((gq, B * Nq * 3), (gt, B * Nt * 3)):
        if buf is None:
            out.append(None)
            continue
        assert _guards_intact(buf, n)
        assert not (buf[:n] == POISON).any()   # every element written (POISON as a float is a NaN pattern no sum produces)
        out.append(buf[:n].view(torch.float32).reshape(B, n // (3 * B), 3).cpu().numpy())
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_forward(d, i, q, t, qlen, tlen, K, want=None):
    """(d, i) of the kernel against the padded float32 restatement, bit for bit, zero padding of both kinds included"""
    wd, wi = want if want is not None else kref.knn_padded(q, t, qlen, tlen, K)
    assert np.array_equal(i, wi)
    assert np.array_equal(_bits(d), _bits(wd))
    for b in range(q.shape[0]):
        m = min(K, tlen[b])
        assert not i[b, :, m:].any() and not _bits(d[b, :, m:]).any()          # slots past min(K, target length)
        assert not i[b, qlen[b]:].any() and not _bits(d[b, qlen[b]:]).any()    # queries past the query length


# ---------------------------------------------------------------------------------------------------------------- forward

SLOT_KS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32]   # every class s and s/2 + 1, and 3, 5, 17, 31 (checked against the plan below)
BOUNDARY_LABELS = ["1,1", "T-1,L-1", "T,L", "T+1,L+1", "1,2L+3", "2T+1,1"]
LATTICE_CASES = [("65", "63", 20, 32), ("T+1", "2L+1", 700, 17), ("300", "L+1", 1, 8)]


def _resolve(label):
    T, L = _TL()
    return int(eval(label.replace("2L", "2*L").replace("2T", "2*T"), {"T": T, "L": L}))


def _slot_ks_from_the_plan():
    return sorted({s for s in _slot_classes()} | {s // 2 + 1 for s in _slot_classes()} | {3, 5, 17, 31})


@pytest.fixture(scope="module")
def slot_case():
    """(T + 1, 2L + 1), B = 2, cloud 1 shortened on both sides; the reference lists for K = 32 once -- every K is a prefix of them"""
    T, L = _TL()
    nq, nt = T + 1, 2 * L + 1
    q, t = ref.uniform_cloud((2, nq), seed=nq), ref.uniform_cloud((2, nt), seed=nt + 1)
    qlen, tlen = [nq, nq // 2 + 1], [nt, (2 * nt) // 3 + 1]
    return q, t, qlen, tlen, kref.knn_padded(q, t, qlen, tlen, 32)


def test_the_cases_reach_every_instance_and_straddle_the_tiles(gpu_device):
    classes = _slot_classes()
    assert classes[0] == 1 and classes[-1] == 32
    assert _slot_ks_from_the_plan() == SLOT_KS                      # the parametrisation below is the issue's list for THIS plan
    assert {_plan(K=k)["k_slots"] for k in SLOT_KS} == set(classes)   # every instance the library is built with is launched
    T, L = _TL()
    for k in (1, 8, 32):   # the boundaries do not move with K or the shape
        assert (_plan(K=k)["threads"], _plan(K=k)["tile"]) == (T, L) and _plan(5 * T, 3, k)["threads"] == T
    shapes = [tuple(_resolve(p) for p in l.split(",")) for l in BOUNDARY_LABELS]
    assert {(T - 1, L - 1), (T, L), (T + 1, L + 1)} <= set(shapes)
    assert _plan(T, L)["grid_x"] == 1 and _plan(T + 1, L)["grid_x"] == 2 and _plan(2 * T + 1, 1)["grid_x"] == 3
    assert any(nt > 2 * L for _, nt in shapes) and any(nt < 8 for _, nt in shapes)   # three tiles; fewer targets than K


@pytest.mark.parametrize("K", SLOT_KS)
def test_knn_matches_the_fp32_restatement_in_every_slot_class(gpu_device, slot_case, K):
    q, t, qlen, tlen, (wd, wi) = slot_case
    d, i = raw_knn(q, t, K, qlen, tlen, device=gpu_device)
    _check_forward(d, i, q, t, qlen, tlen, K, want=(wd[:, :, :K], wi[:, :, :K]))


@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("label", BOUNDARY_LABELS)
def test_knn_at_the_workgroup_and_tile_boundaries(gpu_device, label, K):
    nq, nt = (_resolve(p) for p in label.split(","))
    q, t = ref.uniform_cloud((2, nq), seed=nq + 10), ref.uniform_cloud((2, nt), seed=nt + 11)
    qlen, tlen = [nq, nq // 2 + 1], [nt, (2 * nt) // 3 + 1]
    d, i = raw_knn(q, t, K, qlen, tlen, device=gpu_device)
    _check_forward(d, i, q, t, qlen, tlen, K)
    if (nq, nt, K) == (1, 1, 8):   # one valid slot, seven zero pairs
        assert np.array_equal(_bits(d[0, 0]), _bits(np.r_[kref.knn_f32(q[0], t[0], 1)[0][0], np.zeros(7, np.float32)]))
        assert np.array_equal(i[0, 0], np.zeros(8))
    d2, i2 = raw_knn(q, t, K, device=gpu_device)   # NULL lengths = full lengths
    d3, i3 = raw_knn(q, t, K, [nq, nq], [nt, nt], device=gpu_device)
    assert np.array_equal(i2, i3) and np.array_equal(_bits(d2), _bits(d3))
    _check_forward(d2, i2, q, t, [nq, nq], [nt, nt], K)


def test_knn_with_as_many_targets_as_slots_sorts_the_cloud(gpu_device):
    T, _ = _TL()
    q, t = ref.uniform_cloud((1, T + 1), seed=5), ref.uniform_cloud((1, 32), seed=6)
    d, i = raw_knn(q, t, 32, device=gpu_device)
    _check_forward(d, i, q, t, [T + 1], [32], 32)
    assert all(np.array_equal(np.sort(row), np.arange(32)) for row in i[0])   # every list is a permutation of the cloud
    assert (np.diff(d[0], axis=1) >= 0).all()


@pytest.mark.parametrize("nq_label,nt_label,distinct,K", LATTICE_CASES)
def test_knn_on_lattice_clouds_keeps_the_lower_index(gpu_device, nq_label, nt_label, distinct, K):
    nq, nt = _resolve(nq_label), _resolve(nt_label)
    q = ref.lattice_cloud(nq, seed=nq + 2)
    t = ref.lattice_cloud(nt, seed=nt + 3, distinct=distinct)   # duplicated targets: equal distances at different indices
    d, i = raw_knn(q[None], t[None], K, device=gpu_device)
    d32, i32 = kref.knn_f32(q, t, K)
    d64, i64 = kref.knn_f64(q, t, K)
    assert np.array_equal(i[0], i64) and np.array_equal(d[0].astype(np.float64), d64)
    assert np.array_equal(i[0], i32) and np.array_equal(_bits(d[0]), _bits(d32))
    if distinct == 1:
        assert np.array_equal(i[0], np.tile(np.arange(K), (nq, 1)))


# --------------------------------------------------------------------------------------------------------------- backward

def _check_backward(q, t, K, qlen, tlen, device, seed=5):
    """indices from the forward kernel, weights U(-1, 1); both outputs against the contract's float32 loop, bit for bit"""
    B = q.shape[0]
    _, idx = raw_knn(q, t, K, qlen, tlen, device=device)
    w = np.random.default_rng(seed).uniform(-1, 1, size=idx.shape).astype(np.float32)
    gq, gt = raw_knn_backward(q, t, idx, w, qlen, tlen, device=device)
    for b in range(B):
        nq_b = qlen[b] if qlen is not None else q.shape[1]
        nt_b = tlen[b] if tlen is not None else t.shape[1]
        wq, wt = kref.knn_backward_f32(q[b], t[b], idx[b], w[b], nq_b, nt_b)
        assert np.array_equal(_bits(gq[b]), _bits(wq)) and np.array_equal(_bits(gt[b]), _bits(wt))
        assert not _bits(gq[b, nq_b:]).any() and not _bits(gt[b, nt_b:]).any()   # rows past the lengths: exactly +0
    return idx, w, gq, gt


def test_knn_backward_on_uniform_clouds(gpu_device):
    q, t = ref.uniform_cloud((1, 300), seed=43), ref.uniform_cloud((1, 1025), seed=143)
    idx, _, _, gt = _check_backward(q, t, 16, None, None, gpu_device)
    unselected = np.setdiff1d(np.arange(1025), idx[0].ravel())
    assert len(unselected) and not _bits(gt[0, unselected]).any()   # targets nobody selected: exactly 0


def test_knn_backward_across_the_workgroup_and_tile_boundaries_with_one_neighbour(gpu_device):
    T, L = _TL()
    q, t = ref.uniform_cloud((1, T + 1), seed=44), ref.uniform_cloud((1, L + 1), seed=144)
    _check_backward(q, t, 1, None, None, gpu_device)


def test_knn_backward_with_lengths(gpu_device):
    q, t = ref.uniform_cloud((2, 65), seed=45), ref.uniform_cloud((2, 63), seed=145)
    _check_backward(q, t, 32, [65, 33], [63, 20], gpu_device)   # cloud 1: fewer targets than K -- slots 20 .. 31 are padding


def test_knn_backward_when_every_query_selects_the_same_targets(gpu_device):
    """one lattice point repeated: every list reads 0, 1, 2, 3, so targets 0 .. 3 each sum a term from every one of the 2T + 1 queries
    (4 (2T + 1) entries: several staging tiles) in ascending order, and every other target receives exactly 0"""
    T, _ = _TL()
    nq = 2 * T + 1
    q = ref.lattice_cloud(nq, seed=7)
    t = ref.lattice_cloud(40, seed=8, distinct=1)
    idx, w, gq, gt = _check_backward(q[None], t[None], 4, None, None, gpu_device)
    assert np.array_equal(idx[0], np.tile(np.arange(4), (nq, 1)))
    assert gt[0, :4].all() and not _bits(gt[0, 4:]).any()


def test_knn_backward_outputs_are_optional_and_independent(gpu_device):
    q, t = ref.uniform_cloud((2, 130), seed=46), ref.uniform_cloud((2, 300), seed=146)
    qlen, tlen = [130, 70], [300, 201]
    idx, w, gq, gt = _check_backward(q, t, 5, qlen, tlen, gpu_device)
    only_t = raw_knn_backward(q, t, idx, w, qlen, tlen, device=gpu_device, want_query=False)
    only_q = raw_knn_backward(q, t, idx, w, qlen, tlen, device=gpu_device, want_target=False)
    assert only_t[0] is None and np.array_equal(_bits(only_t[1]), _bits(gt))
    assert only_q[1] is None and np.array_equal(_bits(only_q[0]), _bits(gq))


# -------------------------------------------------------------------------------------------------------------- front ends

def test_knn_points_front_end(gpu_device):
    from gaussiananything_amd.pointcloud import knn_gather, knn_points
    p1, p2 = ref.uniform_cloud((2, 70), seed=1), ref.uniform_cloud((2, 90), seed=2)
    a, b = torch.from_numpy(p1).to(gpu_device), torch.from_numpy(p2).to(gpu_device)
    l1, l2 = [70, 3], [90, 5]
    out = knn_points(a, b, lengths1=torch.tensor(l1), lengths2=torch.tensor(l2), K=7, return_nn=True, version=0, return_sorted=False)
    assert out._fields == ("dists", "idx", "knn")
    assert out.dists.dtype == torch.float32 and out.idx.dtype == torch.int64 and out.knn.dtype == torch.float32
    assert out.dists.shape == (2, 70, 7) and out.idx.shape == (2, 70, 7) and out.knn.shape == (2, 70, 7, 3)
    wd, wi = kref.knn_padded(p1, p2, l1, l2, 7)
    assert np.array_equal(out.idx.cpu().numpy(), wi) and np.array_equal(_bits(out.dists.cpu().numpy()), _bits(wd))
    assert torch.equal(out.knn, knn_gather(b, out.idx, torch.tensor(l2)))
    knn = out.knn.cpu().numpy()
    assert np.array_equal(knn[0], p2[0][wi[0]])
    assert np.array_equal(knn[1, :3, :5], p2[1][wi[1, :3, :5]]) and not knn[1, :, 5:].any()   # zero fill where k >= lengths2
    assert np.array_equal(knn[1, 3:, :5], np.broadcast_to(p2[1, 0], (67, 5, 3)))              # padded rows: index 0, as pytorch3d
    plain = knn_points(a, b, K=1)
    assert plain.knn is None and plain.dists.shape == (2, 70, 1) and not plain.dists.requires_grad
    wd1, wi1 = ref.nearest_f32(p1[0], p2[0])
    assert np.array_equal(plain.idx[0, :, 0].cpu().numpy(), wi1) and np.array_equal(plain.dists[0, :, 0].cpu().numpy(), wd1)
    with pytest.raises(ValueError):
        knn_points(a, b[:1], K=2)
    with pytest.raises(ValueError):
        knn_points(a, b, lengths2=[90, 91], K=2)
    with pytest.raises(ValueError, match="32"):
        knn_points(a, b, K=33)


def test_knn_points_carries_the_gradient(gpu_device):
    from gaussiananything_amd.pointcloud import knn_points
    p1, p2 = ref.uniform_cloud((2, 130), seed=47), ref.uniform_cloud((2, 300), seed=147)
    l1, l2 = [130, 70], [300, 201]
    a = torch.from_numpy(p1).to(gpu_device).requires_grad_(True)
    b = torch.from_numpy(p2).to(gpu_device).requires_grad_(True)
    w = np.random.default_rng(5).uniform(-1, 1, size=(2, 130, 6)).astype(np.float32)
    out = knn_points(a, b, lengths1=l1, lengths2=l2, K=6)
    assert out.dists.requires_grad and not out.idx.requires_grad
    (out.dists * torch.from_numpy(w).to(gpu_device)).sum().backward()
    idx = out.idx.cpu().numpy()
    assert np.array_equal(idx, kref.knn_padded(p1, p2, l1, l2, 6)[1])
    for bb in range(2):
        gq64, gt64, (mq, aq), (mt, at) = kref.knn_backward_f64(p1[bb], p2[bb], idx[bb], w[bb], l1[bb], l2[bb])
        eq = np.abs(a.grad[bb].double().cpu().numpy() - gq64)
        et = np.abs(b.grad[bb].double().cpu().numpy() - gt64)
        bq, bt = kref.grad_bound(mq, aq), kref.grad_bound(mt, at)
        print(f"cloud {bb}: worst error / bound: query {np.max(eq[mq > 0] / bq[mq > 0]):.3f}, target {np.max(et[mt > 0] / bt[mt > 0]):.3f}")
        assert (eq <= bq).all() and (et <= bt).all()   # the bound is 0 where nothing is summed: those must be exactly 0
    only = knn_points(a.detach(), b, K=3)   # one side only
    ga, = torch.autograd.grad(only.dists.sum(), [b])
    assert ga.shape == b.shape and not a.detach().requires_grad


CHAMFER_INPUTS = {"300x257": ((300, 41), (257, 141), None, None), "1500x1700 with lengths": ((1500, 44), (1700, 144), [900], [1201])}


@pytest.fixture(scope="module")
def chamfer_batch():
    x = np.stack([ref.uniform_cloud((1500,), seed=21), ref.uniform_cloud((1500,), seed=22)])
    y = np.stack([ref.uniform_cloud((1700,), seed=23), ref.uniform_cloud((1700,), seed=24)])
    return x, y, [1500, 900], [1700, 1201]


@pytest.mark.parametrize("batch_reduction", ["mean", "sum", None])
@pytest.mark.parametrize("point_reduction", ["mean", "sum"])
def test_differentiable_chamfer_has_the_bits_of_the_forward_only_loss(gpu_device, chamfer_batch, point_reduction, batch_reduction):
    from gaussiananything_amd.pointcloud import chamfer_distance
    x, y, xl, yl = chamfer_batch
    xt, yt = torch.from_numpy(x).to(gpu_device), torch.from_numpy(y).to(gpu_device)
    kw = dict(batch_reduction=batch_reduction, point_reduction=point_reduction)
    plain, _ = chamfer_distance(xt, yt, xl, yl, **kw)
    xg, yg = xt.clone().requires_grad_(True), yt.clone().requires_grad_(True)
    diff, normals = chamfer_distance(xg, yg, xl, yl, differentiable=True, **kw)
    assert normals is None and diff.requires_grad and not plain.requires_grad
    assert torch.equal(diff.detach(), plain) and diff.shape == plain.shape
    with pytest.raises(RuntimeError):
        chamfer_distance(xg, yg, xl, yl, **kw)   # the default stays forward only
    # single_directional: the x -> y half, with either setting
    half_plain, _ = chamfer_distance(xt, yt, xl, yl, single_directional=True, **kw)
    half_diff, _ = chamfer_distance(xg, yg, xl, yl, single_directional=True, differentiable=True, **kw)
    other, _ = chamfer_distance(yt, xt, yl, xl, single_directional=True, **kw)
    assert torch.equal(half_plain, half_diff.detach()) and torch.equal(half_plain + other, plain)
    from gaussiananything_amd.pointcloud import nearest_points
    d = nearest_points(xt, yt, xl, yl)[0].sum(1)
    d = d / torch.tensor(xl, device=d.device).float() if point_reduction == "mean" else d
    d = d if batch_reduction is None else d.sum() / 2 if batch_reduction == "mean" else d.sum()
    assert torch.equal(half_plain, d)


@pytest.mark.parametrize("point_reduction,batch_reduction", [("mean", "mean"), ("sum", "sum")])
@pytest.mark.parametrize("case", list(CHAMFER_INPUTS))
def test_differentiable_chamfer_gradients_against_float64_autograd(gpu_device, case, point_reduction, batch_reduction):
    """Reference: torch float64 autograd on the CPU of the dense formulation (the minimum over the full distance matrix).  Tolerance
    per component (m + 8) * 2^-24 * sum|term| over the m terms a point's gradient sums: three roundings per term and one per addition
    as for the kNN gradient, the others for the reductions' weights (the division by the length and by the batch on the way back)."""
    from gaussiananything_amd.pointcloud import chamfer_distance
    (nx, sx), (ny, sy), xl, yl = CHAMFER_INPUTS[case]
    x, y = ref.uniform_cloud((nx,), seed=sx), ref.uniform_cloud((ny,), seed=sy)
    lx, ly = (xl or [nx])[0], (yl or [ny])[0]
    # precondition, on the references alone: fp32 and float64 select the same neighbours, so the two argmins differentiate one function
    ixy32, ixy64 = ref.nearest_f32(x[:lx], y[:ly])[1], ref.nearest_f64(x[:lx], y[:ly])[1]
    iyx32, iyx64 = ref.nearest_f32(y[:ly], x[:lx])[1], ref.nearest_f64(y[:ly], x[:lx])[1]
    assert np.array_equal(ixy32, ixy64) and np.array_equal(iyx32, iyx64)
    # float64 autograd of the dense formulation
    x64 = torch.from_numpy(x[:lx]).double().requires_grad_(True)
    y64 = torch.from_numpy(y[:ly]).double().requires_grad_(True)
    dm = (x64[:, None, :] - y64[None, :, :]).square().sum(-1)
    cx, cy = dm.min(1).values.sum(), dm.min(0).values.sum()
    wx, wy = (1.0 / lx, 1.0 / ly) if point_reduction == "mean" else (1.0, 1.0)   # B = 1: the batch reduction changes nothing
    want_loss = cx * wx + cy * wy
    want_loss.backward()
    # m and sum|term| per component, float64: x_i sums its own x -> y term and one y -> x term per y that selected it (y likewise)
    X, Y = x[:lx].astype(np.float64), y[:ly].astype(np.float64)
    txy = np.abs(2 * wx * (X - Y[ixy64]))                 # [lx,3]: the term of pair (i, nearest(i)), on both of its ends
    tyx = np.abs(2 * wy * (Y - X[iyx64]))                 # [ly,3]
    mx, ax = np.ones((lx, 3)), txy.copy()
    my, ay = np.ones((ly, 3)), tyx.copy()
    np.add.at(mx, iyx64, 1)
    np.add.at(ax, iyx64, tyx)
    np.add.at(my, ixy64, 1)
    np.add.at(ay, ixy64, txy)
    xg = torch.from_numpy(x[None]).to(gpu_device).requires_grad_(True)
    yg = torch.from_numpy(y[None]).to(gpu_device).requires_grad_(True)
    loss, _ = chamfer_distance(xg, yg, xl, yl, batch_reduction=batch_reduction, point_reduction=point_reduction, differentiable=True)
    loss.backward()
    assert float(loss.detach()) == pytest.approx(float(want_loss.detach()), rel=1e-5)
    gx, gy = xg.grad[0].double().cpu().numpy(), yg.grad[0].double().cpu().numpy()
    ex, ey = np.abs(gx[:lx] - x64.grad.numpy()), np.abs(gy[:ly] - y64.grad.numpy())
    bx, by = (mx + 8) * 2.0 ** -24 * ax, (my + 8) * 2.0 ** -24 * ay
    print(f"chamfer gradient {case} {point_reduction}/{batch_reduction}: worst error / bound x {np.max(ex / bx):.3f}, y {np.max(ey / by):.3f}; "
          f"fan-in up to {int(mx.max())}, {int(my.max())}")
    assert (ex <= bx).all() and (ey <= by).all()
    assert not gx[lx:].any() and not gy[ly:].any()   # padded rows: exactly 0


def _outliers_f64(p, nb, ratio):
    """float64 restatement for one cloud -> (m, threshold)"""
    P = np.asarray(p, np.float64)
    d = np.sqrt(((P[:, None, :] - P[None, :, :]) ** 2).sum(-1))
    m = np.sort(d, axis=1)[:, 1:nb + 1].mean(1)   # column 0 is the point itself
    return m, m.mean() + ratio * m.std()


@pytest.fixture(scope="module")
def scan_with_outliers():
    """cloud 0: 600 uniform points and 6 strays at radius >= 3, scattered through the array; cloud 1: 400 and 4, padded to 606"""
    rng = np.random.default_rng(12)

    def cloud(n, k, seed):
        p = ref.uniform_cloud((n + k,), seed=seed)
        where = np.sort(rng.choice(n + k, size=k, replace=False))
        v = rng.normal(size=(k, 3))
        p[where] = (v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(3.0, 4.0, size=(k, 1))).astype(np.float32)
        return p, where

    p0, w0 = cloud(600, 6, 51)
    p1, w1 = cloud(400, 4, 52)
    pts = np.zeros((2, 606, 3), np.float32)
    pts[0], pts[1, :404] = p0, p1
    return pts, [606, 404], [w0, w1]


def test_remove_statistical_outliers(gpu_device, scan_with_outliers):
    from gaussiananything_amd.pointcloud import remove_statistical_outliers
    pts, lengths, strays = scan_with_outliers
    want = np.zeros((2, 606), bool)
    for b in range(2):   # on the restatement alone: the strays, exactly, and no m_i near the threshold
        m, thr = _outliers_f64(pts[b, :lengths[b]], 20, 2.0)
        assert np.min(np.abs(m - thr) / thr) > 1e-3
        want[b, :lengths[b]] = m <= thr
        assert np.array_equal(np.flatnonzero(~want[b, :lengths[b]]), strays[b])
    out, new_len, keep = remove_statistical_outliers(torch.from_numpy(pts).to(gpu_device), lengths, nb_neighbors=20, std_ratio=2.0)
    assert keep.dtype == torch.bool and np.array_equal(keep.cpu().numpy(), want)
    assert new_len.tolist() == [600, 400] and out.shape == (2, 606, 3) and out.dtype == torch.float32
    out = out.cpu().numpy()
    for b in range(2):
        assert np.array_equal(out[b, :new_len[b]], pts[b][want[b]])   # original order
        assert not out[b, new_len[b]:].any()                          # zero pad
    alone, alone_len, alone_keep = remove_statistical_outliers(torch.from_numpy(pts[1:, :404]).to(gpu_device))   # the defaults; no lengths
    assert alone_len.tolist() == [400] and np.array_equal(alone_keep[0].cpu().numpy(), want[1, :404])            # clouds are independent
    assert np.array_equal(alone[0, :400].cpu().numpy(), out[1, :400])
    with pytest.raises(ValueError):
        remove_statistical_outliers(torch.from_numpy(pts).to(gpu_device), [606, 20], nb_neighbors=20)   # fewer than nb + 1 points
    with pytest.raises(ValueError):
        remove_statistical_outliers(torch.from_numpy(pts).to(gpu_device), lengths, nb_neighbors=32)


def test_cloud_to_condition_with_the_outlier_filter_equals_its_parts(gpu_device):
    from gaussiananything_amd import cascade
    from gaussiananything_amd.pointcloud import remove_statistical_outliers, sample_farthest_points
    rng = np.random.default_rng(4)
    cloud = rng.uniform(-0.5, 0.5, size=(1, 2000, 3)).astype(np.float32)   # past the +-0.45 box: the clip acts
    v = rng.normal(size=(5, 3))
    cloud[0, [3, 500, 501, 1200, 1999]] = (v / np.linalg.norm(v, axis=1, keepdims=True) * 3.5).astype(np.float32)
    points = torch.from_numpy(cloud).to(gpu_device)
    got = cascade.cloud_to_condition(points, 768, outlier_neighbors=20)
    kept, new_len, keep = remove_statistical_outliers(points, None, 20, 2.0)
    assert new_len.tolist() == [1995] and not keep[0, [3, 500, 501, 1200, 1999]].any()
    want = sample_farthest_points(kept, lengths=new_len, K=768)[0].clip(-0.45, 0.45)
    assert torch.equal(got, want) and got.shape == (1, 768, 3) and float(got.abs().max()) == pytest.approx(0.45)
    # without the filter: today's path -- FPS starts at index 0 and takes the farthest point next, which is a stray
    plain = cascade.cloud_to_condition(points, 768)
    assert torch.equal(plain, sample_farthest_points(points, K=768)[0].clip(-0.45, 0.45))
    assert torch.equal(plain, cascade.cloud_to_condition(points, 768, outlier_neighbors=None, outlier_std_ratio=0.1))
    idx = ref.fps_f32(cloud[0], 768, 0)
    assert np.array_equal(plain[0].cpu().numpy(), np.clip(cloud[0, idx], -0.45, 0.45)) and idx[1] in (3, 500, 501, 1200, 1999)
    with pytest.raises(ValueError):   # "too small" applies to what the filter leaves
        cascade.cloud_to_condition(points[:, :770], 768, outlier_neighbors=20, outlier_std_ratio=0.0)
