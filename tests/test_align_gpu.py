"""GPU tests of ``ga_pc_align_points`` and ``ga_pc_icp`` (include/ga_pointcloud.h, csrc/pc_align.hip) and of what is built on them.

Every raw C-ABI call is compared with the restatement (tests/_align_ref.py) for EQUALITY, bit for bit: transform, rmse, status,
iterations, history, Xt, idx and dist2.  Every raw call poisons its outputs first, checks guard words behind each of them and behind
the workspace, and that its inputs are unchanged.  The front ends follow."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _align_ref as ref

pytestmark = pytest.mark.gpu

F = np.float32
GUARD = 64            # int32 words behind every buffer
GUARD_WORD = 0x5A5A5A5A
POISON = -77          # as a float: a NaN pattern no arithmetic here produces


@pytest.fixture(scope="module")
def device(gpu_device):
    return gpu_device


def _guarded(n_words, device):
    t = torch.full((n_words + GUARD,), GUARD_WORD, dtype=torch.int32, device=device)
    t[:n_words] = POISON
    return t


def _take(buf, n, shape, dtype=torch.float32):
    assert bool((buf[n:] == GUARD_WORD).all()), "guard words overwritten"
    assert not bool((buf[:n] == POISON).any()), "an output element was not written"
    return buf[:n].view(dtype).reshape(shape).cpu().numpy()


def _same(got, want, what):
    a, b = np.ascontiguousarray(got, F).view(np.uint32), np.ascontiguousarray(want, F).view(np.uint32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = a != b
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ in bits, first at {np.argwhere(bad)[0].tolist()}: " \
                          f"{got[tuple(np.argwhere(bad)[0])]!r} != {want[tuple(np.argwhere(bad)[0])]!r}"


class Raw:
    """one bound ``ga_pc_align_points`` (``y`` has the rows of ``x``, ``icp=False``) or ``ga_pc_icp`` call: device copies of the inputs,
    guarded outputs and workspace; ``enqueue`` launches on a stream, ``outputs`` reads back after the checks"""

    def __init__(self, device, x, y, icp=True, weights=None, x_lengths=None, y_lengths=None, init_transform=None, max_iterations=4,
                 relative_rmse_thr=1e-6, estimate_scale=False, max_distance=0.0, history=True):
        from gaussiananything_amd import _lib
        self._lib, self.L, self.device, self.icp = _lib, _lib.lib(), device, icp
        self.B, self.N, _ = x.shape
        self.M, self.K = y.shape[1], max_iterations
        i32 = lambda a: None if a is None else np.asarray(a, np.int32)
        self.host = dict(x=np.asarray(x, F), y=np.asarray(y, F), weights=None if weights is None else np.asarray(weights, F),
                         x_lengths=i32(x_lengths), y_lengths=i32(y_lengths),
                         init=None if init_transform is None else np.asarray(init_transform, F))
        self.inp = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) if v is not None else None for k, v in self.host.items()}
        B, N, K = self.B, self.N, self.K
        self.out = dict(transform=_guarded(B * 13, device), rmse=_guarded(B, device), status=_guarded(B, device))
        if icp:
            self.out.update(iterations=_guarded(B, device), history=_guarded(B * (K + 1) * 14, device) if history else None,
                            xt=_guarded(B * N * 3, device), idx=_guarded(B * N, device), dist2=_guarded(B * N, device))
        self.ws_bytes = int(self.L.ga_pc_align_workspace_bytes(B, N))
        assert self.ws_bytes >= (B * ref.groups_of(N) * ref.TERMS + B) * 8 and self.ws_bytes % 16 == 0
        self.ws = _guarded(self.ws_bytes // 4, device)
        p = lambda t: t.data_ptr() if t is not None else None
        i, o = self.inp, self.out
        if icp:
            self.args = _lib.GaIcpArgs(B, N, self.M, K, int(estimate_scale), 0, relative_rmse_thr, max_distance, p(i["x"]), p(i["y"]),
                                       p(i["weights"]), p(i["x_lengths"]), p(i["y_lengths"]), p(i["init"]), p(o["transform"]),
                                       p(o["rmse"]), p(o["status"]), p(o["iterations"]), p(o["history"]), p(o["xt"]), p(o["idx"]),
                                       p(o["dist2"]), p(self.ws), self.ws_bytes)
            self.call, self.name = self.L.ga_pc_icp, "ga_pc_icp"
        else:
            self.args = _lib.GaAlignArgs(B, N, int(estimate_scale), 0, p(i["x"]), p(i["y"]), p(i["weights"]), p(i["x_lengths"]),
                                         p(o["transform"]), p(o["rmse"]), p(o["status"]), p(self.ws), self.ws_bytes)
            self.call, self.name = self.L.ga_pc_align_points, "ga_pc_align_points"

    def enqueue(self, stream):
        self._lib.check(self.call(ctypes.byref(self.args), ctypes.c_void_p(stream.cuda_stream)), self.name)

    def outputs(self):
        B, N, K, o = self.B, self.N, self.K, self.out
        assert bool((self.ws[self.ws_bytes // 4:] == GUARD_WORD).all()), "guard words behind the workspace overwritten"
        out = dict(transform=_take(o["transform"], B * 13, (B, 13)), rmse=_take(o["rmse"], B, (B,)),
                   status=_take(o["status"], B, (B,), torch.int32))
        if self.icp:
            out.update(iterations=_take(o["iterations"], B, (B,), torch.int32), xt=_take(o["xt"], B * N * 3, (B, N, 3)),
                       idx=_take(o["idx"], B * N, (B, N), torch.int32), dist2=_take(o["dist2"], B * N, (B, N)))
            if o["history"] is not None:
                out["history"] = _take(o["history"], B * (K + 1) * 14, (B, K + 1, 14))
        for k, v in self.host.items():                       # the inputs are left alone
            if v is not None:
                assert np.array_equal(self.inp[k].cpu().numpy().view(np.uint8), np.ascontiguousarray(v).view(np.uint8)), k
        return out


def _run(device, x, y, **kw):
    with torch.cuda.device(device):
        r = Raw(device, x, y, **kw)
        r.enqueue(torch.cuda.current_stream())
        torch.cuda.synchronize()
        return r.outputs()


def _equal(got, want):
    for k in ("status", "iterations", "idx"):
        if k in got:
            assert np.array_equal(got[k], want[k]), (k, got[k][..., :8], want[k][..., :8])
    for k in ("transform", "rmse", "history", "xt", "dist2"):
        if k in got:
            _same(got[k], want[k], k)


def _pairs(B, N, seed, noise=0.01):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, N, 3)).astype(F)
    y = np.stack([(rng.uniform(0.5, 2.0) * x[b].astype(np.float64) @ ref.rotation(rng.normal(size=3), rng.uniform(0, 3)) + rng.normal(size=3)
                   + noise * rng.normal(size=(N, 3))).astype(F) for b in range(B)])
    w = rng.uniform(0.1, 1.0, size=(B, N)).astype(F)
    w[rng.uniform(size=(B, N)) < 0.2] = 0
    return x, y, w


def _scene(B, N, M, seed, angle=0.2, translation=0.04, scale=1.0):
    """B clouds of N points of the bumpy ellipsoid of M points (with replacement when N > M), each moved by its own transform"""
    rng = np.random.default_rng(seed)
    y = ref.bumpy_ellipsoid(M)
    xs = []
    for _ in range(B):
        d = rng.normal(size=3)
        xs.append(ref.moved(y[rng.choice(M, N, replace=N > M)], ref.rotation(rng.normal(size=3), angle),
                            translation * d / np.linalg.norm(d), scale))
    return np.stack(xs), np.tile(y[None], (B, 1, 1))


SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 700)   # around a wave, around a workgroup, three workgroups with a ragged last


@pytest.mark.parametrize("N", SIZES)
def test_align_points_bits(device, N):
    x, y, w = _pairs(2, N, N)
    for scale in (False, True):
        _equal(_run(device, x, y, icp=False, weights=w, estimate_scale=scale), ref.align_points(x, y, w, estimate_scale=scale))
    _equal(_run(device, x, y, icp=False), ref.align_points(x, y))


def test_align_points_lengths_and_degenerate(device):
    x, y, w = _pairs(3, 300, 11)
    lengths = [300, 2, 257]
    w[1, :2] = (0.25, 0.75)                                        # the cloud of two points: both weigh (one alone has no extent)
    w[2] = 0                                                       # all-zero weights: DEGENERATE, the identity
    got = _run(device, x, y, icp=False, weights=w, x_lengths=lengths, estimate_scale=True)
    want = ref.align_points(x, y, w, lengths, estimate_scale=True)
    assert want["status"].tolist() == [ref.RUNNING, ref.RUNNING, ref.DEGENERATE]
    _equal(got, want)
    assert got["status"].tolist() == [ref.RUNNING, ref.RUNNING, ref.DEGENERATE] and np.array_equal(got["transform"][2], ref.IDENTITY)
    same = np.tile(x[:, :1], (1, 300, 1))                         # coincident X: DEGENERATE when the scale is wanted
    got = _run(device, same, y, icp=False, estimate_scale=True)
    _equal(got, ref.align_points(same, y, estimate_scale=True))
    assert (got["status"] == ref.DEGENERATE).all()
    got = _run(device, same, y, icp=False)
    _equal(got, ref.align_points(same, y))
    assert (got["status"] == ref.RUNNING).all()


@pytest.mark.parametrize("N", SIZES)
def test_icp_bits_over_query_sizes(device, N):
    x, y = _scene(1, N, 1025, 40 + N)
    for scale in (False, True):
        _equal(_run(device, x, y, max_iterations=3, estimate_scale=scale), ref.icp(x, y, max_iterations=3, estimate_scale=scale))


@pytest.mark.parametrize("M", (1, ref.TILE - 1, ref.TILE, ref.TILE + 1, 2 * ref.TILE + 52))
def test_icp_bits_over_target_sizes(device, M):
    x, y = _scene(1, 257, M, 60 + M % 7)
    _equal(_run(device, x, y, max_iterations=3), ref.icp(x, y, max_iterations=3))


def test_icp_batch_lengths_weights_gate_init(device):
    x, y = _scene(3, 300, 1100, 5, scale=1.05)
    xl, yl = [300, 2, 129], [1100, 1024, 700]
    rng = np.random.default_rng(6)
    w = rng.uniform(0.1, 1.0, size=(3, 300)).astype(F)
    w[rng.uniform(size=(3, 300)) < 0.2] = 0
    init = np.stack([ref.pack(ref.rotation(rng.normal(size=3), 0.05), 0.01 * rng.normal(size=3), 1.02) for _ in range(3)])
    kw = dict(x_lengths=xl, y_lengths=yl, weights=w, init_transform=init, max_iterations=6, estimate_scale=True, max_distance=0.06)
    got = _run(device, x, y, **kw)
    _equal(got, ref.icp(x, y, **kw))
    assert (got["idx"][1, 2:] == -1).all() and (got["dist2"][1, 2:] == 0).all() and (got["xt"][1, 2:] == 0).all()
    _same(got["history"][:, 0, :13], init, "history row 0 is the initial transform")
    kw.update(estimate_scale=False, max_distance=0.0)
    got = _run(device, x, y, history=False, **kw)                      # no history buffer: everything else as with one
    assert "history" not in got
    _equal(got, ref.icp(x, y, **kw))


def test_icp_degenerate_keeps_the_transform(device):
    x, y = _scene(2, 100, 500, 8)
    init = np.stack([ref.pack(ref.rotation([1, 2, 3], 0.1), [0.01, 0.02, 0.03], 1.0)] * 2)
    w = np.ones((2, 100), F)
    w[0] = 0                                                       # no weight at all
    got = _run(device, x, y, weights=w, init_transform=init, max_iterations=5)
    _equal(got, ref.icp(x, y, weights=w, init_transform=init, max_iterations=5))
    assert got["status"][0] == ref.DEGENERATE and got["iterations"][0] == 0 and got["status"][1] != ref.DEGENERATE
    _same(got["transform"][0], init[0], "a degenerate cloud keeps its transform")
    far = x + F(10)                                                # everything beyond the gate
    got = _run(device, far, y, max_iterations=5, max_distance=0.05)
    _equal(got, ref.icp(far, y, max_iterations=5, max_distance=0.05))
    assert (got["status"] == ref.DEGENERATE).all() and np.array_equal(got["transform"], np.tile(ref.IDENTITY, (2, 1)))
    same = np.tile(x[:, :1], (1, 100, 1))                         # coincident X: no extent for the scale
    got = _run(device, same, y, max_iterations=5, estimate_scale=True)
    _equal(got, ref.icp(same, y, max_iterations=5, estimate_scale=True))
    assert (got["status"] == ref.DEGENERATE).all()


def test_icp_frozen_clouds(device):
    """one cloud starts aligned and converges after one update; its neighbour goes on"""
    x, y = _scene(2, 300, 1000, 3, angle=0.3, translation=0.05)
    x[0] = y[0, :300]
    got = _run(device, x, y, max_iterations=30)
    _equal(got, ref.icp(x, y, max_iterations=30))
    its = got["iterations"]
    assert got["status"].tolist() == [ref.CONVERGED, ref.CONVERGED] and its[0] == 1 and its[1] > 3
    for b in range(2):
        _same(got["history"][b, its[b]:], np.tile(got["history"][b, its[b]], (31 - its[b], 1)), "later history rows repeat")
        _same(got["history"][b, its[b], :13], got["transform"][b], "the last row holds the returned transform")
        assert got["rmse"][b].view(np.uint32) == got["history"][b, its[b], 13].view(np.uint32)
    assert not np.array_equal(got["history"][1, 1], got["history"][1, 2])


def test_icp_matches_are_ga_pc_nearest(device):
    from gaussiananything_amd import pointcloud as pc
    x, y = _scene(2, 700, 2100, 9)
    xl, yl = [700, 513], [2100, 1500]
    got = _run(device, x, y, x_lengths=xl, y_lengths=yl, max_iterations=4)
    d2, idx = pc.nearest_points(torch.from_numpy(got["xt"]).to(device), torch.from_numpy(y).to(device), xl, yl)
    assert np.array_equal(idx.cpu().numpy(), got["idx"])
    _same(d2.cpu().numpy(), got["dist2"], "dist2")


def test_icp_in_a_graph(device):
    from gaussiananything_amd import pointcloud as pc
    x, y = _scene(2, 300, 1000, 12)
    x2, _ = _scene(2, 300, 1000, 13, angle=0.1)
    with torch.cuda.device(device):
        X, Y = torch.from_numpy(x).to(device), torch.from_numpy(y).to(device)
        pc.iterative_closest_point(X, Y, max_iterations=5, return_history=True)          # warm-up outside the capture
        torch.cuda.synchronize()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            with torch.cuda.graph(graph, stream=stream):
                sol = pc.iterative_closest_point(X, Y, max_iterations=5, return_history=True)
        X.copy_(torch.from_numpy(x2).to(device))
        graph.replay()
        torch.cuda.synchronize()
    want = ref.icp(x2, y, max_iterations=5)
    got = dict(transform=torch.cat([sol.RTs.s[:, None], sol.RTs.R.reshape(2, 9), sol.RTs.T], 1).cpu().numpy(), rmse=sol.rmse.cpu().numpy(),
               iterations=sol.iterations.cpu().numpy(), history=sol.history.cpu().numpy(), xt=sol.Xt.cpu().numpy(),
               idx=sol.idx.cpu().numpy(), dist2=sol.dist2.cpu().numpy())
    _equal(got, want)
    assert np.array_equal(sol.converged.cpu().numpy(), want["status"] == ref.CONVERGED)


def test_front_ends(device):
    from gaussiananything_amd import pointcloud as pc
    x, y = _scene(2, 300, 1000, 21, scale=1.1)
    X, Y = torch.from_numpy(x).to(device), torch.from_numpy(y).to(device)
    with pytest.raises(NotImplementedError):
        pc.iterative_closest_point(X, Y, allow_reflection=True)
    with pytest.raises(NotImplementedError):
        pc.corresponding_points_alignment(X, X, allow_reflection=True)
    sol = pc.iterative_closest_point(X.requires_grad_(True), Y, max_iterations=40, estimate_scale=True, return_history=True)
    assert sol._fields[:5] == ("converged", "rmse", "Xt", "RTs", "t_history") and sol.RTs._fields == ("R", "T", "s")
    assert sol.converged.dtype == torch.bool and sol.converged.device.type == "cuda" and bool(sol.converged.all())
    assert not sol.Xt.requires_grad and sol.idx.dtype == torch.int64 and len(sol.t_history) == 41
    want = ref.icp(x, y, max_iterations=40, estimate_scale=True)
    _same(sol.Xt.cpu().numpy(), want["xt"], "Xt")
    assert np.array_equal(sol.iterations.cpu().numpy(), want["iterations"])
    _same(pc.apply_similarity_transform(X, sol.RTs).cpu().numpy(), sol.Xt.cpu().numpy(), "apply_similarity_transform(X, RTs) == Xt")
    again = pc.iterative_closest_point(X, Y, init_transform=sol.RTs, max_iterations=3, estimate_scale=True)
    _same(again.RTs.R.cpu().numpy(), sol.RTs.R.cpu().numpy(), "restarting from the solution stays there")
    # corresponding points: the matches ICP found give its transform back
    pairs = torch.gather(Y, 1, sol.idx[:, :, None].expand(-1, -1, 3))
    t, rmse, status = pc.corresponding_points_alignment(X, pairs, estimate_scale=True, return_status=True)
    wantp = ref.align_points(x, y[np.arange(2)[:, None], want["idx"]], estimate_scale=True)
    _same(torch.cat([t.s[:, None], t.R.reshape(2, 9), t.T], 1).cpu().numpy(), wantp["transform"], "transform")
    _same(rmse.cpu().numpy(), wantp["rmse"], "rmse")
    assert status.tolist() == [0, 0]
    _same(t.R.cpu().numpy(), sol.RTs.R.cpu().numpy(), "the solve of the final matches is the ICP transform")
    assert pc.align_plan(700, 1000) == dict(threads=ref.THREADS, tile=ref.TILE, grid_x=3, solve_threads=64, sweeps=ref.SWEEPS,
                                            terms=ref.TERMS)


def _icosphere(level):
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v), np.array(f, np.int64)


def test_mesh_cloud_distance_align(device):
    from gaussiananything_amd import mesh
    v, f = _icosphere(3)                                                            # 1 280 faces
    v = (v * np.array([0.4, 0.25, 0.15]) * (1 + 0.1 * np.sin(5 * v[:, [1, 2, 0]]))).astype(F)
    V, Fc = torch.from_numpy(v).to(device), torch.from_numpy(f).to(device)
    cloud = mesh.sample_points_from_mesh(V, Fc, 2000, seed=5)
    R = torch.from_numpy(ref.rotation([1.0, -2.0, 0.5], 0.1).astype(F)).to(device)
    moved = cloud @ R + torch.tensor([0.02, -0.01, 0.015], device=device)
    plain = mesh.mesh_cloud_distance(V, Fc, moved, num_samples=4000, threshold=0.01)
    none = mesh.mesh_cloud_distance(V, Fc, moved, num_samples=4000, threshold=0.01, align=None)
    assert set(plain) == set(none) and all(torch.equal(plain[k], none[k]) for k in plain)
    rigid = mesh.mesh_cloud_distance(V, Fc, moved, num_samples=4000, threshold=0.01, align="rigid")
    print("accuracy", float(plain["accuracy"]), "->", float(rigid["accuracy"]), "completeness", float(plain["completeness"]), "->",
          float(rigid["completeness"]))
    assert float(rigid["accuracy"]) < float(plain["accuracy"]) and float(rigid["completeness"]) < float(plain["completeness"])
    assert rigid["transform"].R.shape == (1, 3, 3) and rigid["points"].shape == moved.shape and float(rigid["transform"].s[0]) == 1.0
    sim = mesh.mesh_cloud_distance(V, Fc, moved, num_samples=4000, align="similarity")
    assert float(sim["accuracy"]) < float(plain["accuracy"])
