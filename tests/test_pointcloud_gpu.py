"""GPU tests of the point-cloud kernels (include/ga_pointcloud.h, csrc/pointcloud.hip) and of what is built on them.

FPS and nearest point are compared with the numpy float32 restatement of the arithmetic contract (tests/_pointcloud_ref.py) for
EQUALITY -- index lists with ``np.array_equal``, distances and gathered points bit for bit -- and with the float64 brute force on
dyadic lattice clouds.  Every raw call poisons its outputs first and checks guard words behind each output and the workspace."""
import ctypes

import numpy as np
import pytest
import torch

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


def _plan(N):
    from gaussiananything_amd import pointcloud
    return pointcloud.fps_plan(N)


def _na():
    """the largest N the plan sends to the register-resident variant"""
    lo, hi = 1, 1 << 24
    assert _plan(lo)["variant"] == "register" and _plan(hi)["variant"] == "streaming"
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if _plan(mid)["variant"] == "register" else (lo, mid)
    return lo


def _resolve_n(label):
    return {"Na-1": _na() - 1, "Na": _na(), "Na+1": _na() + 1}.get(label) or int(label)


def raw_fps(points, K, lengths=None, starts=None, device="cuda:0", want_points=True):
    """ga_pc_fps on a padded numpy batch through the C-ABI, with poisoned outputs and guard words -> (idx [B,K] int32, points [B,K,3])"""
    from gaussiananything_amd import _lib
    L = _lib.lib()
    B, N, _ = points.shape
    p = torch.from_numpy(np.ascontiguousarray(points)).to(device)
    ln = torch.tensor(lengths, dtype=torch.int32, device=device) if lengths is not None else None
    st = torch.tensor(starts, dtype=torch.int32, device=device) if starts is not None else None
    oi = _guarded(B * K, device)
    op = _guarded(B * K * 3, device) if want_points else None
    nbytes = int(L.ga_pc_fps_workspace_bytes(B, N, K))
    assert nbytes % 4 == 0 and (nbytes > 0) == (_plan(N)["variant"] == "streaming")
    ws = _guarded(nbytes // 4, device)
    args = _lib.GaFpsArgs(B, N, K, p.data_ptr(), ln.data_ptr() if ln is not None else None, st.data_ptr() if st is not None else None,
                          oi.data_ptr(), op.data_ptr() if want_points else None, ws.data_ptr(), nbytes)
    with torch.cuda.device(device):
        _lib.check(L.ga_pc_fps(ctypes.byref(args), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "ga_pc_fps")
        torch.cuda.synchronize()
    assert _guards_intact(oi, B * K) and _guards_intact(ws, nbytes // 4)
    idx = oi[:B * K].reshape(B, K).cpu().numpy()
    assert not (idx == POISON).any()   # every slot written
    if not want_points:
        return idx, None
    assert _guards_intact(op, B * K * 3)
    return idx, op[:B * K * 3].view(torch.float32).reshape(B, K, 3).cpu().numpy()


_full_order = {}


def full_order(N):
    """the seeded U(-0.45, 0.45) cloud of N points and its complete FPS order from index 0 (every K is a prefix of it); computed once"""
    if N not in _full_order:
        p = ref.uniform_cloud((N,), seed=1000 + N)
        _full_order[N] = (p, ref.fps_f32(p, N, 0))
    return _full_order[N]


N_LABELS = ["1", "2", "63", "64", "65", "1023", "1025", "5000", "Na-1", "Na", "Na+1"]


def test_the_cases_straddle_the_variant_boundary_and_reach_every_instance(gpu_device):
    na = _na()
    assert _plan(na)["variant"] == "register" and _plan(na + 1)["variant"] == "streaming"
    ns = [_resolve_n(l) for l in N_LABELS] + [100, 4096]   # + the duplicate-point clouds below
    assert {na - 1, na, na + 1} <= set(ns)
    reached = {(pl["variant"], pl["threads"], pl["points_per_lane"] if pl["variant"] == "register" else 0) for pl in map(_plan, ns)}
    # one wave, four waves, sixteen waves, and the streaming kernel
    assert {t for v, t, _ in reached if v == "register"} == {64, 256, 1024} and any(v == "streaming" for v, _, _ in reached)


# K = 768 where N allows (the boundary sizes are far above it, asserted in the test)
NK_LABELS = [(n, k) for n in N_LABELS for k in ("1", "17", "N", "N+5", "768") if k != "768" or n.startswith("Na") or int(n) >= 768]


@pytest.mark.parametrize("n_label,k_label", NK_LABELS)
def test_fps_matches_the_fp32_restatement(gpu_device, n_label, k_label):
    N = _resolve_n(n_label)
    K = {"N": N, "N+5": N + 5}.get(k_label) or int(k_label)
    assert k_label != "768" or N >= 768
    p, order = full_order(N)
    idx, pts = raw_fps(p[None], K, device=gpu_device)
    m = min(K, N)
    assert np.array_equal(idx[0, :m], order[:m])
    assert np.array_equal(idx[0, m:], np.full(K - m, -1))
    assert np.array_equal(pts[0, :m].view(np.uint32), p[order[:m]].view(np.uint32))   # the gathered inputs, bit for bit
    assert np.array_equal(pts[0, m:].view(np.uint32), np.zeros((K - m, 3), np.uint32))


@pytest.mark.parametrize("n_label", N_LABELS)
def test_fps_batch_with_lengths_and_starts(gpu_device, n_label):
    N = _resolve_n(n_label)
    lengths, starts = [N, N // 2 + 1, 1], [0, N // 3, 0]
    K = min(N + 5, 773)   # past the shorter clouds always, past the longest when it is small: -1 / zero padding in every case
    p0, order0 = full_order(N)
    p = np.stack([p0, ref.uniform_cloud((N,), seed=7 + N), ref.uniform_cloud((N,), seed=8 + N)])
    want_idx, want_pts = ref.fps_padded(p[1:], lengths[1:], K, starts[1:])
    m0 = min(K, N)
    idx, pts = raw_fps(p, K, lengths, starts, device=gpu_device)
    assert np.array_equal(idx[0, :m0], order0[:m0]) and np.array_equal(idx[0, m0:], np.full(K - m0, -1))
    assert np.array_equal(idx[1:], want_idx) and np.array_equal(pts[1:].view(np.uint32), want_pts.view(np.uint32))
    assert idx[1, 0] == N // 3 and np.array_equal(idx[2], [0] + [-1] * (K - 1))
    idx_only, none = raw_fps(p, K, lengths, starts, device=gpu_device, want_points=False)   # out_points may be NULL
    assert none is None and np.array_equal(idx_only, idx)


def test_fps_lattice_cloud_with_duplicates(gpu_device):
    """4096 lattice points drawn from 2048 sites (more than half are duplicates): distances are exact and tie in almost every iteration"""
    p = ref.lattice_cloud(4096, seed=5, distinct=2048)
    assert len(np.unique(p, axis=0)) <= 2048
    want32, want64 = ref.fps_f32(p, 512), ref.fps_f64(p, 512)
    assert np.array_equal(want32, want64)
    idx, pts = raw_fps(p[None], 512, device=gpu_device)
    assert np.array_equal(idx[0], want64) and np.array_equal(pts[0], p[want64])


def test_fps_one_point_repeated(gpu_device):
    p = np.tile(np.array([[0.25, -0.125, 0.375]], np.float32), (100, 1))
    idx, pts = raw_fps(p[None], 10, device=gpu_device)
    assert np.array_equal(idx[0], np.zeros(10, np.int32)) and np.array_equal(pts[0], p[:10])


def test_sample_farthest_points_front_end(gpu_device):
    """pytorch3d's signature: (points [B,K,3], idx [B,K] int64); lengths, fixed and random starts; non-contiguous fp16 input is cast"""
    import random
    from gaussiananything_amd.pointcloud import sample_farthest_points
    p = ref.uniform_cloud((2, 300), seed=3)
    t = torch.from_numpy(p).to(gpu_device)
    pts, idx = sample_farthest_points(t, K=40)
    want_idx, want_pts = ref.fps_padded(p, [300, 300], 40, [0, 0])
    assert idx.dtype == torch.int64 and idx.shape == (2, 40) and pts.shape == (2, 40, 3)
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(pts.cpu().numpy(), want_pts)
    pts, idx = sample_farthest_points(t, lengths=torch.tensor([300, 20]), K=40, start_idx=[5, 19])
    want_idx, want_pts = ref.fps_padded(p, [300, 20], 40, [5, 19])
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(pts.cpu().numpy(), want_pts)
    random.seed(11)
    starts = [random.randint(0, 299), random.randint(0, 19)]
    random.seed(11)
    pts, idx = sample_farthest_points(t, lengths=[300, 20], K=8, random_start_point=True)
    assert np.array_equal(idx.cpu().numpy(), ref.fps_padded(p, [300, 20], 8, starts)[0])
    half = torch.from_numpy(p).to(gpu_device).half().transpose(0, 1).contiguous().transpose(0, 1)   # not contiguous, not fp32
    pts, idx = sample_farthest_points(half, K=12)
    assert np.array_equal(idx.cpu().numpy(), ref.fps_padded(half.float().cpu().numpy(), [300, 300], 12, [0, 0])[0])
    for bad in (dict(lengths=[300, 0]), dict(lengths=[301, 1]), dict(lengths=[300]), dict(start_idx=[0, 300]), dict(K=0)):
        with pytest.raises(ValueError):
            sample_farthest_points(t, **{"K": 4, **bad})


def raw_nearest(query, target, qlen=None, tlen=None, device="cuda:0"):
    from gaussiananything_amd import _lib
    B, Nq, _ = query.shape
    Nt = target.shape[1]
    q = torch.from_numpy(np.ascontiguousarray(query)).to(device)
    t = torch.from_numpy(np.ascontiguousarray(target)).to(device)
    ql = torch.tensor(qlen, dtype=torch.int32, device=device) if qlen is not None else None
    tl = torch.tensor(tlen, dtype=torch.int32, device=device) if tlen is not None else None
    od, oi = _guarded(B * Nq, device), _guarded(B * Nq, device)
    args = _lib.GaNearestArgs(B, Nq, Nt, q.data_ptr(), t.data_ptr(), ql.data_ptr() if ql is not None else None,
                              tl.data_ptr() if tl is not None else None, od.data_ptr(), oi.data_ptr())
    with torch.cuda.device(device):
        _lib.check(_lib.lib().ga_pc_nearest(ctypes.byref(args), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "ga_pc_nearest")
        torch.cuda.synchronize()
    assert _guards_intact(od, B * Nq) and _guards_intact(oi, B * Nq)
    idx = oi[:B * Nq].reshape(B, Nq).cpu().numpy()
    assert not (idx == POISON).any()
    return od[:B * Nq].view(torch.float32).reshape(B, Nq).cpu().numpy(), idx


# the kernel walks targets in tiles of 1024: 2049 = two tiles and one, 1025 / 1023 sit on either side of one tile
NEAREST_SHAPES = [(1, 1), (65, 63), (1000, 1), (1, 1000), (1537, 2049), (300, 1025), (257, 1023), (256, 1024)]


@pytest.mark.parametrize("nq,nt", NEAREST_SHAPES)
def test_nearest_matches_the_fp32_restatement(gpu_device, nq, nt):
    """B = 2 with lengths: cloud 0 full, cloud 1 shortened on both sides"""
    q, t = ref.uniform_cloud((2, nq), seed=nq), ref.uniform_cloud((2, nt), seed=nt + 1)
    qlen, tlen = [nq, nq // 2 + 1], [nt, (2 * nt) // 3 + 1]
    d, i = raw_nearest(q, t, qlen, tlen, device=gpu_device)
    for b in range(2):
        wd, wi = ref.nearest_f32(q[b, :qlen[b]], t[b, :tlen[b]])
        assert np.array_equal(i[b, :qlen[b]], wi)
        assert np.array_equal(d[b, :qlen[b]].view(np.uint32), wd.view(np.uint32))
        assert np.array_equal(i[b, qlen[b]:], np.full(nq - qlen[b], -1)) and not d[b, qlen[b]:].any()
    d2, i2 = raw_nearest(q, t, device=gpu_device)   # NULL lengths = all
    wd, wi = ref.nearest_f32(q[1], t[1])
    assert np.array_equal(i2[1], wi) and np.array_equal(d2[1].view(np.uint32), wd.view(np.uint32))


@pytest.mark.parametrize("nq,nt,distinct", [(65, 63, 20), (1537, 2049, 700), (300, 1025, 1)])
def test_nearest_on_lattice_clouds_takes_the_lowest_index(gpu_device, nq, nt, distinct):
    q = ref.lattice_cloud(nq, seed=nq + 2)
    t = ref.lattice_cloud(nt, seed=nt + 3, distinct=distinct)   # duplicated targets: equal distances at different indices
    d, i = raw_nearest(q[None], t[None], device=gpu_device)
    d64, i64 = ref.nearest_f64(q, t)
    d32, i32 = ref.nearest_f32(q, t)
    assert np.array_equal(i[0], i64) and np.array_equal(d[0].astype(np.float64), d64)
    assert np.array_equal(i[0], i32) and np.array_equal(d[0], d32)


def test_nearest_points_front_end(gpu_device):
    from gaussiananything_amd.pointcloud import nearest_points
    x, y = ref.uniform_cloud((2, 70), seed=1), ref.uniform_cloud((2, 90), seed=2)
    d, i = nearest_points(torch.from_numpy(x).to(gpu_device), torch.from_numpy(y).to(gpu_device), x_lengths=[70, 3], y_lengths=[90, 50])
    assert d.dtype == torch.float32 and i.dtype == torch.int64
    wd, wi = ref.nearest_f32(x[1, :3], y[1, :50])
    assert np.array_equal(i[1, :3].cpu().numpy(), wi) and np.array_equal(d[1, :3].cpu().numpy(), wd)
    assert i[1, 3:].eq(-1).all() and d[1, 3:].eq(0).all()
    with pytest.raises(ValueError):
        nearest_points(torch.from_numpy(x).to(gpu_device), torch.from_numpy(y).to(gpu_device), y_lengths=[90, 91])


@pytest.fixture(scope="module")
def chamfer_clouds():
    x = np.stack([ref.uniform_cloud((1500,), seed=21), ref.uniform_cloud((1500,), seed=22)])
    y = np.stack([ref.uniform_cloud((1700,), seed=23), ref.uniform_cloud((1700,), seed=24)])
    xl, yl = [1500, 900], [1700, 1201]
    per = {pr: np.array([ref.chamfer_f64(x[b, :xl[b]], y[b, :yl[b]], pr) for b in range(2)]) for pr in ("mean", "sum")}
    return x, y, xl, yl, per


@pytest.mark.parametrize("batch_reduction", ["mean", "sum", None])
@pytest.mark.parametrize("point_reduction", ["mean", "sum"])
def test_chamfer_against_float64_brute_force(gpu_device, chamfer_clouds, point_reduction, batch_reduction):
    """relative error <= 1e-5: the fp32 distances carry a few ulps each (2^-24 relative), and the fp32 summation of <= 2^11 terms adds
    a few ulps times log2 N"""
    from gaussiananything_amd.pointcloud import chamfer_distance
    x, y, xl, yl, per = chamfer_clouds
    loss, normals = chamfer_distance(torch.from_numpy(x).to(gpu_device), torch.from_numpy(y).to(gpu_device), xl, yl,
                                     batch_reduction=batch_reduction, point_reduction=point_reduction)
    assert normals is None
    want = per[point_reduction]
    want = want.mean() if batch_reduction == "mean" else want.sum() if batch_reduction == "sum" else want
    got = loss.double().cpu().numpy()
    assert got.shape == np.shape(want)
    rel = np.max(np.abs(got - want) / np.abs(want))
    print(f"chamfer {point_reduction}/{batch_reduction}: relative error {rel:.3e}")
    assert rel <= 1e-5


def test_chamfer_of_a_permuted_cloud_is_zero(gpu_device):
    from gaussiananything_amd.pointcloud import chamfer_distance
    x = torch.from_numpy(ref.uniform_cloud((1, 1500), seed=31)).to(gpu_device)
    perm = torch.randperm(1500, generator=torch.Generator().manual_seed(0)).to(gpu_device)
    for pr in ("mean", "sum"):
        loss, _ = chamfer_distance(x, x[:, perm], point_reduction=pr)
        assert float(loss) == 0.0
    with pytest.raises(RuntimeError):
        chamfer_distance(x.clone().requires_grad_(True), x)


def test_from_point_cloud_equals_its_parts(gpu_device):
    """stage 2 -> decode on a user's 5000-point cloud, on the small golden models: the driver must give exactly what the pieces give
    when called by hand on ``cloud_to_condition``'s output, and the query cloud must be the clipped FPS subset of the input."""
    from gaussiananything_amd import cascade, synthetic
    from gaussiananything_amd.decode import SurfelDecoder
    from gaussiananything_amd.dit import DiT_I23D_PCD_PixelArt_noclip_clay_stage2
    z2 = torch.load(synthetic.fixture_path("dit_ref_stage2.pt"))
    m2 = DiT_I23D_PCD_PixelArt_noclip_clay_stage2(**dict(z2["kwargs"], use_pe_cond=True))
    m2.load_state_dict(z2["state_dict"])
    zd = torch.load(synthetic.fixture_path("decode_ref.pt"))
    cfg = zd["config"]
    dec = SurfelDecoder(embed_dim=cfg["D"], depth=cfg["depth"], num_heads=cfg["heads"], tokens=cfg["tokens"],
                        ldm_z_channels=cfg["z_channels"])
    dec.load_state_dict(zd["state_dict"])
    m2.to(gpu_device)
    dec.to(gpu_device)
    ctx = torch.load(synthetic.fixture_path("dit_ref_stage1.pt"))["context"]
    cond = {k: v[:1].to(gpu_device) for k, v in ctx.items()}
    uc = {k: torch.zeros_like(v) for k, v in cond.items()}
    L = cfg["tokens"]
    cloud = np.random.default_rng(4).uniform(-0.5, 0.5, size=(1, 5000, 3)).astype(np.float32)   # past the +-0.45 box: the clip acts
    points = torch.from_numpy(cloud).to(gpu_device)
    out = cascade.from_point_cloud(m2, dec, cond, uc, points, num_steps=6, sampling_method="euler", seed=3)
    fps = cascade.cloud_to_condition(points, L)
    want_idx = ref.fps_f32(cloud[0], L, 0)
    assert fps.shape == (1, L, 3)
    assert np.array_equal(fps[0].cpu().numpy(), np.clip(cloud[0, want_idx], -0.45, 0.45))
    assert float(fps.abs().max()) == pytest.approx(0.45)
    c2 = dict(cond, **{"fps-xyz": fps / 0.45})
    lat = cascade.sample(m2, c2, dict(c2), (L, 10), 1, 4.0, 3, 6, "euler")
    want = dec.decode(lat, fps)
    assert torch.equal(out["query_pcd_xyz"], fps) and torch.equal(out["gaussians_upsampled_3"], want["gaussians_upsampled_3"])
    assert "renders" not in out
    same = cascade.cloud_to_condition(fps * 1.5, L)   # N == num_points: order kept, clipped
    assert torch.equal(same, (fps * 1.5).clip(-0.45, 0.45))


def test_export_fps_points(gpu_device, tmp_path):
    from gaussiananything_amd import io_formats
    rng = np.random.default_rng(9)
    g = rng.uniform(-0.4, 0.4, size=(1, 3000, 13)).astype(np.float32)
    g[0, :, 3] = rng.uniform(0.2, 1.0, size=3000)
    low = rng.choice(3000, size=700, replace=False)
    g[0, low, 3] = rng.uniform(0.0, 0.0049, size=700)
    g[0, low[0], 3] = 0.005   # the threshold itself stays (the reference masks ``opacity < 0.005``)
    keep = np.ones(3000, bool)
    keep[low[1:]] = False
    kept = g[0, keep, :3]
    path = tmp_path / "fps-256.ply"
    pts = io_formats.export_fps_points(torch.from_numpy(g).to(gpu_device), str(path), K=256)
    want = kept[ref.fps_f32(kept, 256, 0)]
    back = io_formats.load_points_ply(str(path))
    assert np.array_equal(pts, want) and np.array_equal(back, want)
    dropped = {tuple(r) for r in g[0, ~keep, :3]}
    pts_all = io_formats.export_fps_points(g, str(tmp_path / "all.ply"), K=len(kept))   # every survivor, from a host array
    assert len({tuple(r) for r in pts_all}) == len(kept) and not ({tuple(r) for r in pts_all} & dropped)
    assert {tuple(r) for r in pts_all} == {tuple(r) for r in kept}
