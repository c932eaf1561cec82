"""Adaptive density control on the device (include/ga_densify.h, gaussiananything_amd/fitting.py).

Kernel level: ``ga_fit_accumulate``, ``ga_densify`` and ``ga_fit_reset_opacity`` against the float32 restatement of
tests/_densify_ref.py, bit for bit.  The restatement is fed the kernel's own ``noise_out`` and the activated arrays the kernel read, so
``exp``, ``log``, ``sin`` and ``cos`` are outside the comparison; ``noise_out`` itself is held to the float64 Philox + Box-Muller of
tests/_sde_ref.py within 1e-5 absolute, the bar tests/test_sde_gpu.py uses for this same transform.

Fitter level: the parity scene of tests/test_fit_gpu.py (1000 surfels, 2 views, 64 x 64).  Exact surfel counts across a whole ``step`` are
not asserted: the floating-point atomics of ``ga_surfel_backward`` move the statistics at rounding level and a threshold decision may
flip; what a round did is compared with the restatement on the statistics read back just before it."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import _densify_ref as ref
from tests.test_densify_cpu import PARAMS, PATTERNS, pattern_stats
from tests.test_fit_gpu import _fitter, _mixed, _raw, _same_bits, _scene, _stream

pytestmark = pytest.mark.gpu

F = np.float32
POISON_F, POISON_I = 0x7FC12345, -7            # a NaN with a payload; no kernel here produces either
BIG_N = ref.THREADS * ref.BLOCK_ROWS + 1       # one block sum more than the scan's workgroup has lanes: its loop takes a second trip
NS = (1, 63, 64, 65, 255, 256, 257, 1000)


def _poisoned(dev, *shape):
    return torch.full(shape, POISON_F, dtype=torch.int32, device=dev).view(torch.float32)


def _activate(dev, raw):
    """ga_fit_activate on raw (numpy [N,13]) -> dict of numpy arrays"""
    from gaussiananything_amd import _lib
    n = raw.shape[0]
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)    # noqa: E731
    t = {"means": z(n, 3), "opacities": z(n), "colors": z(n, 3), "scales": z(n, 2), "rotations": z(n, 4), "inv_norm": z(n)}
    r = torch.from_numpy(raw).to(dev)
    a = _lib.GaFitActivateArgs(n, 0, r.data_ptr(), t["means"].data_ptr(), t["opacities"].data_ptr(), t["colors"].data_ptr(),
                               t["scales"].data_ptr(), t["rotations"].data_ptr(), t["inv_norm"].data_ptr())
    _lib.check(_lib.lib().ga_fit_activate(ctypes.byref(a), _stream(dev)), "ga_fit_activate")
    return {k: x.cpu().numpy() for k, x in t.items()}


def _densify(dev, raw, m, v, act, stats, *, seed=0, round_=0, flags=0, **params):
    """ga_densify through the C-ABI on poisoned outputs -> dict of host arrays: the WHOLE 2 N rows of raw / m / v / parent, counts,
    noise"""
    from gaussiananything_amd import _lib
    L, n = _lib.lib(), raw.shape[0]
    p = dict(PARAMS)
    p.update(params)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)    # noqa: E731
    ins = [up(x) for x in (raw, m, v, act["opacities"], act["scales"], act["rotations"], *stats)]
    out_raw, out_m, out_v = (_poisoned(dev, 2 * n, 13) for _ in range(3))
    parent = torch.full((2 * n,), POISON_I, dtype=torch.int32, device=dev)
    noise = _poisoned(dev, n, 4)
    counts = torch.full((8,), -1, dtype=torch.int64, device=dev)
    ws = torch.zeros(int(L.ga_densify_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    a = _lib.GaDensifyArgs()
    a.num_points, a.flags, a.round, a.seed = n, flags, round_, seed
    a.grad_threshold, a.min_opacity, a.percent_dense, a.extent = p["grad_threshold"], p["min_opacity"], p["percent_dense"], p["extent"]
    a.max_screen_size = p.get("max_screen_size", 0)
    (a.raw, a.m, a.v, a.opacities, a.scales, a.rotations, a.grad_accum, a.denom, a.max_radius) = (t.data_ptr() for t in ins)
    a.out_raw, a.out_m, a.out_v, a.parent = out_raw.data_ptr(), out_m.data_ptr(), out_v.data_ptr(), parent.data_ptr()
    a.noise_out, a.out_counts, a.workspace, a.workspace_bytes = noise.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel()
    _lib.check(L.ga_densify(ctypes.byref(a), _stream(dev)), "ga_densify")
    return {"raw": out_raw.cpu().numpy(), "m": out_m.cpu().numpy(), "v": out_v.cpu().numpy(), "parent": parent.cpu().numpy(),
            "counts": counts.cpu().tolist(), "noise": noise.cpu().numpy()}


def _check_round(got, want, n, seed, round_, flags=0):
    """every requirement of the issue on one ga_densify call; returns the worst |noise - float64 restatement|"""
    c, na = got["counts"], want["N_after"]
    assert c == [na, want["kept"], want["cloned"], want["split"], want["pruned"], n, round_, flags], c
    assert np.array_equal(got["parent"][:na], want["parent"]) and (got["parent"][na:] == POISON_I).all()
    for k in ("raw", "m", "v"):
        _same_bits(got[k][:na], want[k], k)
        assert (got[k][na:].view(np.int32) == POISON_F).all(), f"{k}: a row past N' was written"
    worst = float(np.abs(got["noise"].astype(np.float64) - ref.expected_noise(want["codes"], seed, round_)).max())
    assert worst <= 1e-5, worst
    assert not got["noise"][want["codes"] != ref.SPLIT].any()
    return worst


def _case(dev, pattern, n, seed):
    code, opa, scales, stats = pattern_stats(pattern, n, seed)
    raw, m, v = _raw(n, seed + 1), _mixed(np.random.default_rng(seed + 2), (n, 13)), np.abs(_mixed(np.random.default_rng(seed + 3), (n, 13)))
    act = _activate(dev, raw)
    act["opacities"], act["scales"] = opa, scales
    return code, raw, m, v, act, stats


# ---- ga_fit_accumulate ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_views", (1, 3))
@pytest.mark.parametrize("n", (1, 63, 65, 257, 1000))
def test_accumulate_bit_equal_to_the_restatement(gpu_device, n, num_views):
    """three successive calls on changing gradients (exact zeros, 1e-20, 1e+4) and radii; surfels seen by no view, by some, by all:
    the three statistics bit-equal after every call, and untouched where no view sees the surfel"""
    from gaussiananything_amd import _lib, synthetic
    dev, V = gpu_device, num_views
    rng = np.random.default_rng(900 + n + V)
    cams = synthetic.eval_cameras(4)
    view = cams["cam_view"][:V].reshape(V, 16).float().contiguous()
    means = rng.uniform(-0.5, 0.5, size=(n, 3)).astype(F)
    acc, den, rad = rng.uniform(0, 1, n).astype(F), rng.integers(0, 5, n).astype(np.int32), rng.integers(0, 30, n).astype(np.int32)
    d = {"view": view.to(dev), "means": torch.from_numpy(means).to(dev), "g": torch.zeros(n, 3, device=dev),
         "radii": torch.zeros(V, n, dtype=torch.int32, device=dev), "acc": torch.from_numpy(acc).to(dev),
         "den": torch.from_numpy(den).to(dev), "rad": torch.from_numpy(rad).to(dev)}
    a = _lib.GaFitAccumulateArgs(n, V, float(cams["tanfov"]), 0, d["g"].data_ptr(), d["means"].data_ptr(), d["radii"].data_ptr(),
                                 d["view"].data_ptr(), d["acc"].data_ptr(), d["den"].data_ptr(), d["rad"].data_ptr())
    for call in range(3):
        g = _mixed(rng, (n, 3))
        radii = rng.integers(0, 60, size=(V, n)).astype(np.int32)
        radii[:, call::3] = 0                                                   # seen by no view
        radii[rng.integers(0, V, size=n), np.arange(n)] *= rng.integers(0, 2, size=n).astype(np.int32)     # ... or by some
        hidden = (radii == 0).all(0)
        d["g"].copy_(torch.from_numpy(g)); d["radii"].copy_(torch.from_numpy(radii))
        _lib.check(_lib.lib().ga_fit_accumulate(ctypes.byref(a), _stream(dev)), "ga_fit_accumulate")
        before = (acc, den, rad)
        acc, den, rad = ref.accumulate(g, means, radii, view.numpy(), F(cams["tanfov"]), acc, den, rad)
        for name, got, want, was in zip(("grad_accum", "denom", "max_radius"), (d["acc"], d["den"], d["rad"]), (acc, den, rad), before):
            got = got.cpu().numpy()
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (name, call)
            assert np.array_equal(got[hidden].view(np.int32), was[hidden].view(np.int32)), (name, call)
        assert (den[~hidden] == before[1][~hidden] + 1).all()


# ---- ga_densify ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", NS)
def test_densify_bit_equal_to_the_restatement(gpu_device, n, pattern):
    seed, round_ = 0xC0FFEE00 + n, 3
    code, raw, m, v, act, stats = _case(gpu_device, pattern, n, 100 + n)
    got = _densify(gpu_device, raw, m, v, act, stats, seed=seed, round_=round_)
    want = ref.densify(raw, m, v, act, stats, got["noise"], **PARAMS)
    assert np.array_equal(want["codes"], code)
    worst = _check_round(got, want, n, seed, round_)
    print(f"densify parity: N={n} {pattern}: N' {want['N_after']}, worst |normal - float64| {worst:.3e}")
    if pattern == "none":                          # bit-identical to the input, m and v included
        for k, x in (("raw", raw), ("m", m), ("v", v)):
            _same_bits(got[k][:n], x, k)
    if pattern == "all_pruned":                    # N' = 0 and nothing at all was written
        assert got["counts"][0] == 0 and (got["raw"].view(np.int32) == POISON_F).all() and (got["parent"] == POISON_I).all()


@pytest.mark.parametrize("pattern", ("mix", "none"))
def test_densify_more_block_sums_than_scan_lanes(gpu_device, pattern):
    """N = lanes x rows per block + 1: the one workgroup that scans the block sums loops a second time"""
    from gaussiananything_amd import _lib
    assert int(_lib.lib().ga_densify_workspace_bytes(BIG_N)) // 16 == ref.THREADS + 1
    code, raw, m, v, act, stats = _case(gpu_device, pattern, BIG_N, 7)
    got = _densify(gpu_device, raw, m, v, act, stats, seed=5, round_=1)
    want = ref.densify(raw, m, v, act, stats, got["noise"], **PARAMS)
    worst = _check_round(got, want, BIG_N, 5, 1)
    print(f"densify parity: N={BIG_N} {pattern}: N' {want['N_after']}, worst |normal - float64| {worst:.3e}")


def test_same_seed_same_bits_another_round_moves_only_split_children(gpu_device):
    n = 1000
    code, raw, m, v, act, stats = _case(gpu_device, "mix", n, 300)
    a = _densify(gpu_device, raw, m, v, act, stats, seed=11, round_=4)
    b = _densify(gpu_device, raw, m, v, act, stats, seed=11, round_=4)
    c = _densify(gpu_device, raw, m, v, act, stats, seed=11, round_=5)
    for k in ("raw", "m", "v", "parent", "noise"):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
    na = a["counts"][0]
    assert a["counts"][:6] == c["counts"][:6] and np.array_equal(a["parent"], c["parent"])
    for k in ("m", "v"):
        assert np.array_equal(a[k].view(np.int32), c[k].view(np.int32)), k
    differ = (a["raw"][:na].view(np.int32) != c["raw"][:na].view(np.int32))
    child = code[a["parent"][:na]] == ref.SPLIT
    assert child.any() and not differ[~child].any() and not differ[:, 3:].any()
    assert differ[child][:, 0:3].any(axis=1).all()                 # every split child moved


def _raw_for(code, seed):
    """raw parameters whose activation realises the codes under PARAMS (opacity 0.5 / 0.01, scales 0.01 / 0.1)"""
    raw = _raw(len(code), seed)
    raw[:, 3] = np.where(code == ref.PRUNED, math.log(0.01 / 0.99), 0.0)
    raw[:, 4:6] = np.where(code == ref.SPLIT, math.log(0.1), math.log(0.01))[:, None]
    return raw


def test_max_points_returns_the_prune_only_round(gpu_device):
    from gaussiananything_amd import fitting
    dev, n = gpu_device, 1000
    code, _, _, stats = pattern_stats("mix", n, 400)
    raw, m, v = _raw_for(code, 401), _mixed(np.random.default_rng(402), (n, 13)), np.abs(_mixed(np.random.default_rng(403), (n, 13)))
    act = _activate(dev, raw)
    full = ref.densify(raw, m, v, act, stats, np.zeros((n, 4), F), **PARAMS)
    assert np.array_equal(full["codes"], code) and full["N_after"] > n
    dv = [torch.from_numpy(x).to(dev) for x in (raw, m, v, *stats)]
    for limit, flags in ((full["N_after"], 0), (full["N_after"] - 1, ref.PRUNE_ONLY)):
        r, mm, vv, parent, counts = fitting.densify_and_prune(*dv, max_points=limit, seed=3, round=2, return_noise=True, **PARAMS)
        want = ref.densify(raw, m, v, act, stats, counts["noise"].cpu().numpy(), flags=flags, **PARAMS)
        assert counts["prune_only"] == bool(flags) and counts["N_before"] == n
        assert [counts[k] for k in ("N_after", "kept", "cloned", "split", "pruned")] == [want[k] for k in ("N_after", "kept", "cloned", "split", "pruned")]
        assert r.shape == (want["N_after"], 13) and np.array_equal(parent.cpu().numpy(), want["parent"])
        for k, x in (("raw", r), ("m", mm), ("v", vv)):
            _same_bits(x, want[k], f"{k}, max_points {limit}")
        if flags:
            assert counts["cloned"] == counts["split"] == 0 and counts["N_after"] == n - counts["pruned"] <= limit
    # every surfel pruned: empty tensors, no error
    r, mm, vv, parent, counts = fitting.densify_and_prune(*dv, **dict(PARAMS, min_opacity=1.0))
    assert counts["N_after"] == 0 and r.shape == (0, 13) and parent.shape == (0,)


@pytest.mark.parametrize("n", (1, 257, 1000))
def test_reset_opacity_bit_equal(gpu_device, n):
    from gaussiananything_amd import fitting
    raw, m, v = _raw(n, 500 + n), _mixed(np.random.default_rng(501), (n, 13)), np.abs(_mixed(np.random.default_rng(502), (n, 13)))
    raw[:, 3] -= 3.0                                   # both sides of logit(0.01) = -4.595
    d = [torch.from_numpy(x.copy()).to(gpu_device) for x in (raw, m, v)]
    out = fitting.reset_opacity(*d)
    assert out is d[0]
    want = ref.reset_opacity(raw, m, v)
    keep = [k for k in range(13) if k != 3]
    for k, got, w, was in zip(("raw", "m", "v"), d, want, (raw, m, v)):
        _same_bits(got, w, k)
        assert np.array_equal(got.cpu().numpy()[:, keep].view(np.int32), was[:, keep].view(np.int32)), k
    fitting.reset_opacity(*d, cap=0.5)
    assert float(d[0][:, 3].max()) <= 0.0


# ---- the fitter ------------------------------------------------------------------------------------------------------------------------
NOTHING = dict(extent=1.0, grad_threshold=float("inf"), min_opacity=0.0, max_screen_size=0)


@pytest.fixture(scope="module")
def scene(gpu_device):
    return _scene(gpu_device)


def _restated_tallies(f, cfg, max_screen_size=0):
    """the restatement's classification on the fitter's own statistics and activated values, read back now"""
    s = f.densify_stats()
    g = f.gaussians()[0].cpu().numpy()
    codes = ref.classify(g[:, 3], g[:, 4:6], s["grad_accum"].cpu().numpy(), s["denom"].cpu().numpy(), s["max_radius"].cpu().numpy(),
                         grad_threshold=cfg["grad_threshold"], min_opacity=cfg["min_opacity"], percent_dense=cfg["percent_dense"],
                         extent=cfg["extent"], max_screen_size=max_screen_size)
    return tuple(int((codes == k).sum()) for k in (ref.CLONE, ref.SPLIT, ref.PRUNED))


@pytest.fixture(scope="module")
def config(scene):
    """thresholds at which the restatement selects some of each kind on this scene: read off a probe fitter's statistics after five
    iterations (the median average gradient, the median larger scale, the 10 % quantile of the opacities)"""
    f = _fitter(scene, densify=dict(NOTHING))
    f.step(5)
    s = f.densify_stats()
    g = f.gaussians()[0]
    avg = (s["grad_accum"] / s["denom"].clamp_min(1).float())
    return dict(extent=1.0, start=10, every=10, stop=40, grad_threshold=float(avg[s["denom"] > 0].median()),
                percent_dense=float(g[:, 4:6].max(dim=1).values.median()), min_opacity=float(g[:, 3].quantile(0.1)), seed=9)


def _consistent(log, n0):
    prev = n0
    for step, before, after, cloned, split, pruned in log:
        assert before == prev and after == before - pruned + cloned + split, (step, before, after, cloned, split, pruned)
        prev = after
    return prev


def test_a_round_that_selects_nothing_changes_nothing(scene):
    f = _fitter(scene, densify=dict(NOTHING))
    f.step(3)
    before = [t.clone() for t in (f.raw, f._m, f._v)]
    entry = f.densify_now()
    assert entry == (3, 1000, 1000, 0, 0, 0) and f.densify_log == [entry] and f.num_points == 1000
    for was, now, k in zip(before, (f.raw, f._m, f._v), "raw m v".split()):
        _same_bits(now, was, k)
    assert not f.densify_stats()["denom"].any()
    f.step(2)
    h = f.loss_history()["loss"]
    assert f.steps == 5 and len(h) == 5 and np.isfinite(h).all() and not torch.equal(f.raw, before[0])


def test_rounds_during_a_fit(gpu_device, scene, config):
    from gaussiananything_amd.gs_surfel import GaussianRenderer2DGS
    f = _fitter(scene, densify=config)
    f.step(5)
    want = _restated_tallies(f, config)
    assert min(want) > 0, want                                  # some of each kind
    entry = f.densify_now()
    assert entry[0] == 5 and entry[1] == 1000 and entry[3:] == want, (entry, want)
    f.step(45)
    n = _consistent(f.densify_log, 1000)
    assert [e[0] for e in f.densify_log] == [5, 10, 20, 30, 40] and n == f.num_points != 1000
    print("densify parity: N per round", [(e[0], e[2]) for e in f.densify_log])
    g = f.gaussians()
    assert tuple(g.shape) == (1, f.num_points, 13) and bool(torch.isfinite(g).all())
    assert tuple(f.raw.shape) == tuple(f.raw_grad.shape) == (f.num_points, 13)
    with torch.no_grad():
        pred = GaussianRenderer2DGS(scene["size"], 3, {}).render(g, scene["cv"][None], scene["cvp"][None], scene["cp"][None], scene["tanfov"])
    assert bool(torch.isfinite(pred["image"]).all())
    h = f.loss_history()
    assert f.steps == 50 and all(len(x) == 50 and np.isfinite(x).all() for x in h.values())


def test_growth_through_a_small_workspace(scene, config):
    """capacity far too small: every capture after a round goes through the grow-and-retry path"""
    f = _fitter(scene, densify=config, capacity=64)
    f.step(50)
    assert f.steps == 50 and f.capacity > 64 and len(f.densify_log) == 4
    assert _consistent(f.densify_log, 1000) == f.num_points
    h = f.loss_history()["loss"]
    assert len(h) == 50 and np.isfinite(h).all()


def test_opacity_reset(scene):
    """after the reset every activated opacity is at most 0.01; one Adam step later at most sigmoid(logit(0.01) + d), d the largest
    step Adam can take from zeroed moments: m' = (1 - b1) g and v' = (1 - b2) g^2 give |m' / (sqrt(v') / sbc2)| = (1 - b1) / sqrt(1 - b2)
    * sbc2 whatever g is, times the opacity step size of the table's row"""
    cfg = dict(NOTHING, start=0, stop=10, every=100, opacity_reset_every=5)
    f = _fitter(scene, densify=cfg)
    f.step(4)
    assert float(f.gaussians()[0, :, 3].max()) > 0.5
    f.step(1)
    assert f.densify_log == []
    cap = math.log(0.01 / 0.99)
    top = float(f.gaussians()[0, :, 3].max())
    assert top <= 0.01 * (1 + 1e-5), top
    assert float(f.raw[:, 3].max()) == float(F(cap)) and not f._m[:, 3].any() and not f._v[:, 3].any()
    row = f._table[5].cpu().numpy().astype(np.float64)
    d = row[1] * (0.1 / math.sqrt(0.001)) * row[5] * (1 + 1e-4)
    f.step(1)
    top = float(f.gaussians()[0, :, 3].max())
    assert 0.0 < top <= 1.0 / (1.0 + math.exp(-(cap + d))) * (1 + 1e-5), (top, d)
    assert bool((f.raw[:, 3] != float(F(cap))).any())


def test_state_dict_of_another_n(scene, config):
    a = _fitter(scene, densify=config)
    a.step(5)
    a.densify_now()
    a.step(3)
    state = a.state_dict()
    assert state["N"] == a.num_points != 1000 and state["round"] == 1 and bool(state["denom"].any())
    b = _fitter(scene, densify=config).load_state_dict(state)
    assert b.num_points == a.num_points and b.steps == a.steps == 8
    for k, x, y in (("raw", a.raw, b.raw), ("m", a._m, b._m), ("v", a._v, b._v)):
        _same_bits(y, x, f"loaded {k}")
    ea, eb = a.densify_now(), b.densify_now()
    assert ea == eb and ea[2] != ea[1]
    for k, x, y in (("raw", a.raw, b.raw), ("m", a._m, b._m), ("v", a._v, b._v)):
        _same_bits(y, x, f"{k} after a round on both")
    b.step(2)
    assert b.steps == 10 and np.isfinite(b.loss_history()["loss"]).all()
