"""View mini-batches selected on the device (include/ga_fit.h: ga_fit_select_views; fitting.SurfelFitter(batch_views=...)).

Kernel level: the batch buffers bit for bit against numpy indexing of the pool, through the C ABI, on both kernel paths (16 bytes per
lane / one element per lane), with and without mask and normal, for every position of the device counter including one past the table;
the buffers sit between guard words that must survive.

Fitter level: the YARDSTICK is the loop a user writes without mini-batches -- a V = 2 fitter driven by ``set_views(pool[S[t]])`` and
``step(1)`` -- run twice, the second time with every raw element moved by one float32 ulp.  The gathered bytes are identical, so only the
floating-point atomics of ``ga_surfel_backward`` separate the mini-batch fitter from that loop; it gets 4 x the spread of the two runs,
the bar tests/test_fit_gpu.py holds the fitter to.  Figures of the last run: profiles/fit_minibatch_parity.txt."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_fit_gpu import _fitter, _group_rel, _scene, _ulp_twin

pytestmark = pytest.mark.gpu

P = 5
GUARD = 64                     # elements before and after every batch buffer (256 bytes: the buffer itself stays 16-byte aligned)
SENTINEL = 0x7FC0BEEF          # a NaN with a payload, as int32 bits
SHAPES = [(1, 1), (5, 7), (8, 8), (12, 6), (33, 33), (40, 40)]


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _bit_patterns(rng, shape):
    """int32 words that, read as float32, are NaNs with payloads, +-inf, +-0, denormals and ordinary values, mixed"""
    w = rng.integers(-2 ** 31, 2 ** 31, size=shape, dtype=np.int64).astype(np.int32)
    special = np.array([0x7FC00001, 0x7F800123, -0x00400000, 0x7F800000, -0x00800000, -0x80000000, 0x00000001, 0x007FFFFF,
                        -0x7FFFFFFF, 0, 0x3F800000], dtype=np.int64).astype(np.int32)
    pick = rng.integers(0, 4, size=shape)
    w = np.where(pick == 0, special[rng.integers(0, len(special), size=shape)], w)
    return w


def _schedule(T, B):
    """rows that all differ, values in [0, P); with B >= 2 row 2 names view 3 twice"""
    s = (2 * np.arange(T)[:, None] + 1 + 3 * np.arange(B)[None, :]) % P
    if B >= 2:
        s[2, :2] = 3
    s = s.astype(np.int32)
    assert len({tuple(r) for r in s.tolist()}) == T and s.min() >= 0 and s.max() < P       # nothing out of range goes to the device
    return s


class _Select:
    """pools and guarded batch buffers on the device, one GaFitSelectArgs over them"""

    def __init__(self, dev, H, W, B, sched, with_mask, with_normal, u8=False, shift=0, seed=0):
        from gaussiananything_amd import _lib
        self.lib, self.L, self.dev, self.B, self.H, self.W = _lib, _lib.lib(), dev, B, H, W
        rng = np.random.default_rng(seed)
        T = sched.shape[0]
        planes = {"view": (16,), "proj": (16,), "targets": (3, H, W)}
        if with_mask:
            planes["mask"] = (1, H, W)
        if with_normal:
            planes["normal"] = (3, H, W)
        self.names = list(planes)
        self.pool_np, self.pool, self.flat, self.batch = {}, {}, {}, {}
        for k, shape in planes.items():
            if k == "targets" and u8:
                host = rng.integers(0, 256, size=(P,) + shape).astype(np.uint8)
                host.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)      # all 256 values, in the first views of the pool
                dtype = torch.uint8
            else:
                host = _bit_patterns(rng, (P,) + shape)
                dtype = torch.int32
            self.pool_np[k] = host
            # shift: the pool starts `shift` elements into its allocation, which takes a 16-byte aligned base pointer away
            store = torch.zeros(host.size + shift, dtype=dtype, device=dev)
            store[shift:].copy_(torch.from_numpy(host.reshape(-1)))
            self.pool[k] = store[shift:]
            n = B * int(np.prod(shape))
            self.flat[k] = torch.full((GUARD + shift + n + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
            self.batch[k] = self.flat[k][GUARD + shift:GUARD + shift + n]
        self.sched_np = sched
        self.sched = torch.from_numpy(sched).to(dev)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.selected = torch.full((B + 2,), -7, dtype=torch.int32, device=dev)
        ptr = lambda d, k: d[k].data_ptr() if k in d else None
        self.args = _lib.GaFitSelectArgs(P, B, H, W, T, _lib.GA_FIT_SELECT_U8_TARGETS if u8 else 0, self.sched.data_ptr(),
                                         self.counter.data_ptr(), ptr(self.pool, "view"), ptr(self.pool, "proj"), ptr(self.pool, "targets"),
                                         ptr(self.pool, "mask"), ptr(self.pool, "normal"), ptr(self.batch, "view"), ptr(self.batch, "proj"),
                                         ptr(self.batch, "targets"), ptr(self.batch, "mask"), ptr(self.batch, "normal"),
                                         self.selected[1:].data_ptr())
        self.u8 = u8

    def run(self):
        self.lib.check(self.L.ga_fit_select_views(ctypes.byref(self.args), _stream(self.dev)), "ga_fit_select_views")

    def expected(self, k, row):
        src = self.pool_np[k][row]                                  # numpy indexing: [B, ...]
        if k == "targets" and self.u8:
            return (src.astype(np.float32) / np.float32(255)).view(np.int32).reshape(-1)
        return src.reshape(-1)

    def check(self, row, what):
        torch.cuda.synchronize()
        row = np.asarray(row)
        for k in self.names:
            flat = self.flat[k].cpu().numpy()
            n = self.batch[k].numel()
            lo = flat.size - GUARD - n
            want = self.expected(k, row)
            got = flat[lo:lo + n]
            bad = got != want
            assert not bad.any(), f"{what}: {k}: {int(bad.sum())} of {n} words differ, first at {int(np.argmax(bad))}"
            assert (flat[:lo] == np.int32(SENTINEL)).all() and (flat[lo + n:] == np.int32(SENTINEL)).all(), f"{what}: {k}: a guard word was written"
        sel = self.selected.cpu().numpy()
        assert np.array_equal(sel[1:1 + self.B], row) and sel[0] == -7 and sel[-1] == -7, (what, sel, row)


@pytest.mark.parametrize("extras", ((False, False), (True, True)), ids=("bare", "mask+normal"))
@pytest.mark.parametrize("B", (1, 2, 5))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_select_is_numpy_indexing_bit_for_bit(gpu_device, shape, B, extras):
    H, W = shape
    T = 5
    sched = _schedule(T, B)
    k = _Select(gpu_device, H, W, B, sched, *extras, seed=100 * H + B)
    for c in (0, 2, T - 1, T + 3):
        k.counter.fill_(c)
        for f in k.flat.values():
            f.fill_(SENTINEL)
        k.run()
        k.check(sched[min(c, T - 1)], f"{H}x{W} B={B} counter={c}")
        assert int(k.counter.cpu()) == c                             # read, never written


@pytest.mark.parametrize("only", ("mask", "normal"))
def test_select_with_one_of_mask_and_normal(gpu_device, only):
    sched = _schedule(5, 2)
    for H, W in ((5, 7), (8, 8)):
        k = _Select(gpu_device, H, W, 2, sched, only == "mask", only == "normal", seed=7)
        k.counter.fill_(2)
        k.run()
        k.check(sched[2], f"{only} only, {H}x{W}")


@pytest.mark.parametrize("shape", ((8, 8), (40, 40)), ids=("8x8", "40x40"))
def test_select_from_pools_offset_by_one_element(gpu_device, shape):
    """base pointers that are not 16-byte aligned although H*W % 4 == 0: the one-element path"""
    sched = _schedule(5, 2)
    k = _Select(gpu_device, *shape, 2, sched, True, True, shift=1, seed=11)
    assert all(t.data_ptr() % 16 == 4 for t in k.pool.values() if t.dtype == torch.int32) and k.batch["targets"].data_ptr() % 16 == 4
    for c in (1, 2):
        k.counter.fill_(c)
        k.run()
        k.check(sched[c], f"offset pools, counter={c}")


@pytest.mark.parametrize("shape,shift", (((16, 16), 0), ((5, 7), 0), ((33, 33), 0), ((16, 16), 1)), ids=("vector", "scalar", "scalar-1089", "unaligned"))
def test_select_uint8_targets(gpu_device, shape, shift):
    """(float)u / 255.0f is numpy's u.astype(float32) / float32(255), bit for bit, for all 256 values"""
    sched = _schedule(5, 2)
    k = _Select(gpu_device, *shape, 2, sched, True, False, u8=True, shift=shift, seed=13)
    assert set(k.pool_np["targets"][:3].reshape(-1).tolist()) == set(range(256))
    sched = sched.copy()
    sched[0], sched[3] = (0, 0), (1, 2)                               # the views that hold all 256 values, one of them twice
    k.sched.copy_(torch.from_numpy(sched))
    for c in (0, 3):
        k.counter.fill_(c)
        k.run()
        k.check(sched[c], f"uint8 {shape} counter={c}")


def test_select_status_codes(gpu_device):
    from gaussiananything_amd import _lib
    L = _lib.lib()
    k = _Select(gpu_device, 8, 8, 2, _schedule(5, 2), True, True)
    s = _stream(gpu_device)

    def rc(**change):
        a = _lib.GaFitSelectArgs()
        ctypes.memmove(ctypes.byref(a), ctypes.byref(k.args), ctypes.sizeof(a))
        for name, value in change.items():
            setattr(a, name, value)
        return L.ga_fit_select_views(ctypes.byref(a), s)

    assert L.ga_fit_select_views(None, s) == -1
    for name in ("schedule", "counter", "pool_view", "pool_proj", "pool_targets", "view", "proj", "targets", "mask", "pool_mask", "normal",
                 "pool_normal"):
        assert rc(**{name: None}) == -1, name
    for change in (dict(pool_views=0), dict(batch_views=0), dict(height=0), dict(width=0), dict(max_steps=0), dict(batch_views=P + 1),
                   dict(height=1 << 16, width=1 << 15)):
        assert rc(**change) == -2, change
    assert rc(flags=2) == -5
    assert rc(selected=None) == 0 and rc() == 0
    torch.cuda.synchronize()


def test_graph_replay_selects_another_row_every_time(gpu_device):
    """select + advance captured once and replayed six times on a table whose rows all differ: after replay t the batch buffers are
    pool[schedule[t]].  A counter frozen into the graph would gather row 0 six times."""
    from gaussiananything_amd import _lib
    T, B = 6, 2
    sched = np.array([[0, 1], [1, 2], [2, 3], [3, 3], [4, 0], [2, 4]], np.int32)
    k = _Select(gpu_device, 8, 8, B, sched, True, True, seed=21)
    history = torch.zeros(T, 8, dtype=torch.float32, device=gpu_device)
    adv = _lib.GaFitAdvanceArgs(1, T, k.counter.data_ptr(), None, None, None, None, history.data_ptr(), 0.0, 0, None, None)

    def iteration():
        s = _stream(gpu_device)
        _lib.check(k.L.ga_fit_select_views(ctypes.byref(k.args), s), "ga_fit_select_views")
        _lib.check(k.L.ga_fit_advance(ctypes.byref(adv), s), "ga_fit_advance")

    iteration()
    k.check(sched[0], "eager")
    k.counter.zero_()
    side = torch.cuda.Stream(device=gpu_device)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            iteration()
    torch.cuda.synchronize()
    for t in range(T):
        graph.replay()
        k.check(sched[t], f"replay {t}")
        assert int(k.counter.cpu()) == min(t + 1, T - 1)


# ---- the fitter ------------------------------------------------------------------------------------------------------------------------
POOL, BATCH, STEPS = 6, 2, 6


def _record(lines):
    for line in lines:
        print("fit minibatch parity:", line)


def _sub(sc, idx):
    """the scene restricted to the pool views ``idx``"""
    idx = torch.as_tensor(np.asarray(idx), dtype=torch.long, device=sc["cv"].device)
    return dict(sc, **{k: sc[k][idx].contiguous() for k in ("cv", "cvp", "cp", "targets", "mask")})


@pytest.fixture(scope="module")
def pool(gpu_device):
    return _scene(gpu_device, n=1000, views=POOL)


@pytest.fixture(scope="module")
def schedule():
    from gaussiananything_amd import fitting
    S = fitting.view_schedule(64, POOL, BATCH, seed=1)
    assert len({tuple(r) for r in S[:STEPS].tolist()}) > 1
    return S


def _set_views_loop(pool, S, twin=False):
    """the loop a user writes without mini-batches: a V = 2 fitter, set_views(pool[S[t]]) and step(1)"""
    f = _fitter(_sub(pool, S[0].numpy()))
    if twin:
        raw0 = f.raw.clone()
        f.load_state_dict({"raw": _ulp_twin(raw0), "m": torch.zeros_like(raw0), "v": torch.zeros_like(raw0), "steps": 0,
                           "history": torch.zeros(0, 8, device=raw0.device)})
    for t in range(STEPS):
        v = _sub(pool, S[t].numpy())
        f.set_views(v["cv"], v["cvp"], v["targets"], mask=v["mask"])
        f.step(1)
    return f


@pytest.fixture(scope="module")
def yardstick(pool, schedule):
    a, b = _set_views_loop(pool, schedule), _set_views_loop(pool, schedule, twin=True)
    return {"loop": a, "raw": _group_rel(b.raw, a.raw), "raw_grad": _group_rel(b.raw_grad, a.raw_grad)}


@pytest.fixture(scope="module")
def minibatch(pool, schedule):
    f = _fitter(pool, batch_views=BATCH, view_schedule=schedule)
    graph = f._graph
    f.step(STEPS)
    return f, graph


def test_minibatch_fitter_against_the_set_views_loop(minibatch, yardstick, schedule):
    f, graph = minibatch
    loop = yardstick["loop"]
    assert f._graph is graph and f.steps == loop.steps == STEPS
    for what, x, y in (("raw", f.raw, loop.raw), ("raw_grad", f.raw_grad, loop.raw_grad)):
        got = _group_rel(x, y)
        _record([f"{what} {k}: mini-batch vs set_views loop {got[k]:.3e}, loop vs its ulp twin {yardstick[what][k]:.3e}" for k in got])
        for k in got:
            assert yardstick[what][k] > 0, (what, k)
            assert got[k] <= 4 * yardstick[what][k], (what, k, got[k], yardstick[what][k])
    h, hl = f.loss_history()["loss"], loop.loss_history()["loss"]
    _record([f"loss history mini-batch {h.tolist()}", f"loss history set_views loop {hl.tolist()}"])
    assert len(h) == STEPS and np.allclose(h, hl, rtol=1e-4)
    assert len(set(h.tolist())) == STEPS
    assert torch.equal(f.last_views().cpu(), schedule[STEPS - 1])
    assert f.last_views().dtype == torch.int32 and tuple(f.last_views().shape) == (BATCH,)


def test_the_whole_pool_with_the_identity_schedule_is_the_full_batch_fitter(pool, yardstick):
    sc = _sub(pool, [0, 1])
    ident = torch.arange(2, dtype=torch.int32).repeat(64, 1)
    full, mb = _fitter(sc), _fitter(sc, batch_views=2, view_schedule=ident)
    full.step(STEPS)
    mb.step(STEPS)
    for what, x, y in (("raw", mb.raw, full.raw), ("raw_grad", mb.raw_grad, full.raw_grad)):
        got = _group_rel(x, y)
        _record([f"identity schedule, {what} {k}: {got[k]:.3e} (bar 4 x {yardstick[what][k]:.3e})" for k in got])
        for k in got:
            assert got[k] <= 4 * yardstick[what][k], (what, k, got[k], yardstick[what][k])
    assert np.allclose(mb.loss_history()["loss"], full.loss_history()["loss"], rtol=1e-4)
    assert torch.equal(mb.last_views().cpu(), ident[0])


def test_a_redone_stretch_draws_the_same_rows(pool, schedule, minibatch):
    """capacity far too small: whatever the warm-up on row 0 grows it to, the run ends on the ample run's losses -- a redo that drew
    other rows would not"""
    small = _fitter(pool, batch_views=BATCH, view_schedule=schedule, capacity=64)
    small.step(STEPS)
    assert small.capacity > 64 and small.steps == STEPS
    h, ha = small.loss_history()["loss"], minibatch[0].loss_history()["loss"]
    assert np.allclose(h, ha, rtol=1e-6), (h, ha)
    assert torch.equal(small.last_views().cpu(), schedule[STEPS - 1])


def test_a_uint8_pool_against_its_float_pool(pool, schedule):
    u8 = (pool["targets"] * 255).round().clamp(0, 255).to(torch.uint8)
    as_float = torch.from_numpy(u8.cpu().numpy().astype(np.float32) / np.float32(255)).to(u8.device)
    a = _fitter(dict(pool, targets=u8), batch_views=BATCH, view_schedule=schedule)
    b = _fitter(dict(pool, targets=as_float), batch_views=BATCH, view_schedule=schedule)
    a.step(1)
    b.step(1)
    assert torch.equal(a._targets.view(torch.int32), b._targets.view(torch.int32))
    assert torch.equal(a._targets.view(torch.int32), as_float[schedule[0].long().to(u8.device)].view(torch.int32))
    a.step(STEPS - 1)
    b.step(STEPS - 1)
    assert np.allclose(a.loss_history()["loss"], b.loss_history()["loss"], rtol=1e-4)
    with pytest.raises(TypeError, match="uint8"):
        a.set_views(pool["cv"], pool["cvp"], as_float, mask=pool["mask"])
    a.set_views(pool["cv"], pool["cvp"], u8, mask=pool["mask"])


def test_density_control_on_mini_batches(pool, schedule):
    """a round due after iteration 3 (a threshold of 0: every surfel that was seen is cloned or split): N changes, the history has its
    six rows, the views still follow the schedule"""
    cfg = dict(extent=1.0, start=3, every=3, stop=3, grad_threshold=0.0, min_opacity=0.0, max_screen_size=0, opacity_reset_every=0)
    f = _fitter(pool, batch_views=BATCH, view_schedule=schedule, densify=cfg)
    f.step(STEPS)
    assert [e[0] for e in f.densify_log] == [3] and f.num_points != 1000 and f.densify_log[0][2] == f.num_points
    h = f.loss_history()["loss"]
    assert f.steps == STEPS and len(h) == STEPS and np.isfinite(h).all() and (h > 0).all() and len(set(h.tolist())) == STEPS
    assert torch.equal(f.last_views().cpu(), schedule[STEPS - 1])
    assert tuple(f.raw.shape) == (f.num_points, 13)


def test_the_pool_and_the_table_are_replaced_without_a_new_capture(pool, schedule):
    f = _fitter(pool, batch_views=BATCH, view_schedule=schedule)
    graph = f._graph
    f.step(2)
    other = schedule.flip(0).contiguous()
    f.set_view_schedule(other)
    f.set_views(pool["cv"].flip(0).contiguous(), pool["cvp"].flip(0).contiguous(), pool["targets"].flip(0).contiguous(),
                mask=pool["mask"].flip(0).contiguous())
    f.step(1)
    assert f._graph is graph and torch.equal(f.last_views().cpu(), other[2])
    assert torch.equal(f._targets, pool["targets"].flip(0)[other[2].long().to(f.device)])
    bad = other.clone()
    bad[0, 0] = POOL
    with pytest.raises(ValueError, match="outside"):
        f.set_view_schedule(bad)
    with pytest.raises(ValueError, match=r"cam_view must be \[6, 4, 4\]"):          # the pool keeps its P
        f.set_views(pool["cv"][:2], pool["cvp"][:2], pool["targets"][:2], mask=pool["mask"][:2])
    with pytest.raises(RuntimeError, match="without batch_views"):
        _fitter(_sub(pool, [0, 1])).last_views()
