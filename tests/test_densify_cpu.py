"""Adaptive density control without a device: the soundness of the restatement the GPU tests compare the kernels with
(tests/_densify_ref.py restates include/ga_densify.h) and the host-side checks of gaussiananything_amd.fitting."""
import math

import numpy as np
import pytest
import torch

from tests import _densify_ref as ref
from tests import _fit_ref as fit
from tests import _sde_ref as sde

F = np.float32
PARAMS = dict(grad_threshold=2e-4, min_opacity=0.05, percent_dense=0.01, extent=2.0)


def _raw(n, seed):
    rng = np.random.default_rng(seed)
    raw = rng.standard_normal((n, 13)).astype(F)
    raw[:, 4:6] = raw[:, 4:6] - 3.0
    return raw


# ---- geometry of a split -----------------------------------------------------------------------------------------------------------
def test_split_children_lie_in_the_parents_plane():
    """|(child - parent) . n| <= 8 ulp of |child - parent| + 4 ulp of |parent| (the offset is a sum of two in-plane vectors rounded
    three times, added to the parent with two more roundings), n the third column of the oracle's rotation (oracle/surfel_autograd.py:
    quat_to_rot, float64) of the same quaternion"""
    from oracle.surfel_autograd import quat_to_rot
    n = 500
    raw = _raw(n, 1)
    act = fit.activate(raw)
    xi = np.random.default_rng(2).standard_normal((n, 4)).astype(F)
    kids = ref.children(raw, act["scales"], act["rotations"], xi).astype(np.float64)
    normal = quat_to_rot(torch.from_numpy(act["rotations"]).double())[:, :, 2].numpy()
    eps = float(np.finfo(F).eps)
    for child in range(2):
        d = kids[:, child, 0:3] - raw[:, 0:3].astype(np.float64)
        off = np.abs((d * normal).sum(1))
        bar = 8 * eps * np.linalg.norm(d, axis=1) + 4 * eps * np.linalg.norm(raw[:, 0:3].astype(np.float64), axis=1)
        assert (off <= bar).all(), float((off / bar).max())
        assert (np.linalg.norm(d, axis=1) > 0).all()


def test_split_offsets_in_the_tangent_frame():
    """the offset of a child, expressed in (tu, tv), is (s0 xa, s1 xb) within fp32 rounding; scales are divided by 1.6, the rest is
    the parent's"""
    n = 500
    raw = _raw(n, 3)
    act = fit.activate(raw)
    xi = np.random.default_rng(4).standard_normal((n, 4)).astype(F)
    kids = ref.children(raw, act["scales"], act["rotations"], xi)
    tu, tv = (t.astype(np.float64) for t in ref.tangents(act["rotations"]))
    s = act["scales"].astype(np.float64)
    eps = float(np.finfo(F).eps)
    # fp32 tangents: every component carries a few roundings (normalisation, three products, two sums), so the frame is orthonormal
    # within 16 eps, and an offset read back in that frame within 16 eps of its size plus the roundings of the two sums at |parent|
    assert max(np.abs((tu * tu).sum(1) - 1).max(), np.abs((tv * tv).sum(1) - 1).max(), np.abs((tu * tv).sum(1)).max()) < 16 * eps
    for child in range(2):
        d = kids[:, child, 0:3].astype(np.float64) - raw[:, 0:3].astype(np.float64)
        want = np.stack([s[:, 0] * xi[:, 2 * child], s[:, 1] * xi[:, 2 * child + 1]], 1)
        got = np.stack([(d * tu).sum(1), (d * tv).sum(1)], 1)
        bar = (16 * eps * np.abs(want).sum(1) + 8 * eps * np.linalg.norm(raw[:, 0:3].astype(np.float64), axis=1))[:, None]
        assert (np.abs(got - want) <= bar).all()
        assert np.array_equal(kids[:, child, 6:], raw[:, 6:]) and np.array_equal(kids[:, child, 3], raw[:, 3])
        ratio = np.exp(kids[:, child, 4:6].astype(np.float64)) / np.exp(raw[:, 4:6].astype(np.float64))
        assert np.abs(ratio - 1 / 1.6).max() < 1e-6
    assert float(ref.LOG_1P6) == float(F(math.log(1.6)))


# ---- classification ----------------------------------------------------------------------------------------------------------------
def _classify(opa, s0, s1, acc, den, rad, **kw):
    p = dict(PARAMS)
    p.update(kw)
    one = lambda x, t: np.asarray([x], t)   # noqa: E731
    return int(ref.classify(one(opa, F), np.asarray([[s0, s1]], F), one(acc, F), one(den, np.int32), one(rad, np.int32), **p)[0])


def test_classification_hits_every_branch():
    K, C, S, P = ref.KEPT, ref.CLONE, ref.SPLIT, ref.PRUNED
    thr, pd_ext = F(2e-4), F(0.01) * F(2.0)
    assert _classify(0.5, 0.01, 0.005, 1.0, 0, 0) == K                           # denom == 0: avg is 0 whatever was accumulated
    assert _classify(0.5, 0.01, 0.005, float("nan"), 3, 0) == K                  # a NaN average counts as 0
    assert _classify(0.5, 0.01, 0.005, float("nan"), 3, 0, grad_threshold=0.0) == C      # ... and 0 >= 0
    assert _classify(0.5, 0.01, 0.005, 3 * float(thr), 3, 0) == C                # avg exactly at the threshold: >=
    assert _classify(0.5, 0.01, 0.005, 3 * float(np.nextafter(thr, F(0))), 3, 0) == K
    assert _classify(0.5, float(pd_ext), 0.001, 1.0, 1, 0) == C                  # smax exactly percent_dense * extent: <= is a clone
    assert _classify(0.5, 0.001, float(np.nextafter(pd_ext, F(1))), 1.0, 1, 0) == S      # (the larger scale is the second one)
    assert _classify(0.05, 0.01, 0.01, 1.0, 1, 0) == C                           # opacity exactly min_opacity: < does not prune
    assert _classify(float(np.nextafter(F(0.05), F(0))), 0.01, 0.01, 1.0, 1, 0) == P     # pruned, not cloned first
    assert _classify(0.5, 5.0, 5.0, 0.0, 1, 1000) == K                           # max_screen_size = 0: no pruning by size at all
    assert _classify(0.5, 0.01, 0.01, 0.0, 1, 20, max_screen_size=20) == K       # radius exactly max_screen_size: > does not prune
    assert _classify(0.5, 0.01, 0.01, 1.0, 1, 21, max_screen_size=20) == P
    big = F(0.1) * F(2.0)
    assert _classify(0.5, float(big), 0.01, 0.0, 1, 0, max_screen_size=20) == K  # smax exactly 0.1 extent: > does not prune
    assert _classify(0.5, float(np.nextafter(big, F(1))), 0.01, 1.0, 1, 0, max_screen_size=20) == P
    assert _classify(0.5, 0.5, 0.5, 1.0, 1, 0, flags=ref.PRUNE_ONLY) == K        # prune only: split and clone are kept
    assert _classify(0.01, 0.5, 0.5, 1.0, 1, 0, flags=ref.PRUNE_ONLY) == P
    assert _classify(0.5, 0.01, 0.005, 1.0, 1, 0, grad_threshold=float("inf")) == K


PATTERNS = ("none", "all_pruned", "all_cloned", "all_split", "first", "last", "mix")


def pattern_stats(pattern, n, seed):
    """statistics and activated values that realise a pattern under ``PARAMS``: -> (act overrides, stats); used by the GPU tests too.
    opacity 0.5 and scales 0.01 keep a surfel, accum >= threshold selects it, a scale of 0.1 makes it a split, opacity 0.01 prunes"""
    rng = np.random.default_rng(seed)
    code = {"none": np.zeros(n, int), "all_pruned": np.full(n, ref.PRUNED), "all_cloned": np.full(n, ref.CLONE),
            "all_split": np.full(n, ref.SPLIT), "mix": rng.integers(0, 4, size=n)}.get(pattern)
    if pattern == "first":
        code = np.zeros(n, int); code[0] = ref.SPLIT
    if pattern == "last":
        code = np.zeros(n, int); code[-1] = ref.CLONE
    opa = np.where(code == ref.PRUNED, 0.01, 0.5).astype(F)
    scales = np.where((code == ref.SPLIT)[:, None], 0.1, 0.01).astype(F) * rng.uniform(0.5, 1.0, size=(n, 2)).astype(F)
    scales[:, 0] = np.where(code == ref.SPLIT, 0.1, scales[:, 0])
    denom = rng.integers(1, 5, size=n).astype(np.int32)
    acc = np.where((code == ref.CLONE) | (code == ref.SPLIT), 1e-3, 1e-5).astype(F) * denom.astype(F)
    acc[code == ref.PRUNED] = 1.0                      # selected as well: pruning wins
    return code.astype(np.int32), opa, scales, (acc, denom, np.zeros(n, np.int32))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", (1, 65, 257))
def test_counts_parent_map_and_row_order(pattern, n):
    code, opa, scales, stats = pattern_stats(pattern, n, 10 + n)
    raw, m, v = _raw(n, 20 + n), _raw(n, 30 + n), np.abs(_raw(n, 40 + n))
    act = fit.activate(raw)
    act["opacities"], act["scales"] = opa, scales
    xi = np.random.default_rng(5).standard_normal((n, 4)).astype(F)
    out = ref.densify(raw, m, v, act, stats, xi, **PARAMS)
    assert np.array_equal(out["codes"], code)
    emitted = np.asarray([1, 2, 2, 0])[code]
    assert out["N_after"] == emitted.sum() == n - out["pruned"] + out["cloned"] + out["split"]
    assert out["kept"] + out["cloned"] + out["split"] + out["pruned"] == n
    assert np.array_equal(out["parent"], np.repeat(np.arange(n), emitted))       # ascending, a parent's rows adjacent
    first = np.concatenate([[0], np.cumsum(emitted)[:-1]])
    for i in range(n):
        at = first[i]
        if code[i] in (ref.KEPT, ref.CLONE):
            assert np.array_equal(out["raw"][at], raw[i]) and np.array_equal(out["m"][at], m[i]) and np.array_equal(out["v"][at], v[i])
        if code[i] == ref.CLONE:
            assert np.array_equal(out["raw"][at + 1], raw[i]) and not out["m"][at + 1].any() and not out["v"][at + 1].any()
        if code[i] == ref.SPLIT:
            assert not out["m"][at:at + 2].any() and not out["v"][at:at + 2].any()
            assert not np.array_equal(out["raw"][at, 0:3], out["raw"][at + 1, 0:3])
            assert np.array_equal(out["raw"][at:at + 2, 6:], np.stack([raw[i, 6:]] * 2))
    if pattern == "none":
        assert np.array_equal(out["raw"], raw) and np.array_equal(out["m"], m) and np.array_equal(out["v"], v)
    if pattern == "all_pruned":
        assert out["N_after"] == 0 and out["raw"].shape == (0, 13)


def test_normals_are_philox_blocks_of_this_kernels_counter():
    """the vectorised blocks against the integer Philox, one parent at a time; the round and the seed reach the counter and the key"""
    seed, rnd, n = 0x0123456789ABCDEF, 7, 40
    got = ref.normals(seed, rnd, n)
    for i in (0, 1, 17, n - 1):
        w = np.asarray([sde.philox_int((i, rnd, ref.STREAM, 0), (seed & sde.MASK, seed >> 32))], dtype=np.uint32)
        assert np.array_equal(got[i], sde.normals64(w))
    assert not np.array_equal(got, ref.normals(seed, rnd + 1, n)) and not np.array_equal(got, ref.normals(seed + 1, rnd, n))
    big = ref.normals(3, 0, 20000)
    assert abs(big.mean()) < 0.02 and abs(big.std() - 1) < 0.02
    codes = np.asarray([ref.KEPT, ref.SPLIT, ref.CLONE, ref.PRUNED, ref.SPLIT])
    e = ref.expected_noise(codes, seed, rnd)
    assert not e[[0, 2, 3]].any() and np.array_equal(e[[1, 4]], ref.normals(seed, rnd, 5)[[1, 4]])


def test_accumulate_restatement():
    """hand-made: a surfel seen by no view keeps its three words; one seen by views 0 and 2 averages their depths"""
    view = np.zeros((3, 16), F)
    view[:, 10] = 1.0
    view[:, 14] = [1.0, 5.0, 3.0]
    means = np.asarray([[0, 0, 1], [0, 0, 1]], F)
    g = np.asarray([[3, 4, 0], [3, 4, 0]], F)
    radii = np.asarray([[0, 2], [0, 0], [0, 9]], np.int32)
    acc, den, rad = ref.accumulate(g, means, radii, view, 0.5, np.asarray([7, 7], F), np.asarray([1, 1], np.int32), np.asarray([4, 4], np.int32))
    assert acc.tolist() == [7.0, 7.0 + 5.0 * 3.0 * 0.5] and den.tolist() == [1, 2] and rad.tolist() == [4, 9]


def test_reset_opacity_restatement():
    raw, m, v = _raw(50, 6), _raw(50, 7), _raw(50, 8)
    raw[:, 3] *= 6
    r, mm, vv = ref.reset_opacity(raw, m, v)
    cap = F(math.log(0.01 / 0.99))
    assert (r[:, 3] <= cap).all() and (r[:, 3] == np.minimum(raw[:, 3], cap)).all() and (raw[:, 3] > cap).any() and (raw[:, 3] < cap).any()
    keep = [k for k in range(13) if k != 3]
    assert np.array_equal(r[:, keep], raw[:, keep]) and np.array_equal(mm[:, keep], m[:, keep]) and np.array_equal(vv[:, keep], v[:, keep])
    assert not mm[:, 3].any() and not vv[:, 3].any()


# ---- host-side validation: raises before anything is enqueued (no device is needed to get there) -----------------------------------
def test_config_validation():
    from gaussiananything_amd.fitting import DensifyConfig, _as_config
    c = DensifyConfig(extent=1.5)
    assert (c.start, c.stop, c.every, c.grad_threshold, c.min_opacity, c.percent_dense) == (500, 15000, 100, 2e-4, 0.05, 0.01)
    assert (c.max_screen_size, c.screen_size_from, c.opacity_reset_every, c.max_points, c.seed) == (20, 3000, 3000, None, 0)
    assert _as_config(None) is None and _as_config(c) is c and _as_config({"extent": 2, "every": 10}).every == 10
    assert DensifyConfig(extent=1.0, grad_threshold=float("inf"), min_opacity=0, max_screen_size=0).grad_threshold == math.inf
    with pytest.raises(TypeError):
        DensifyConfig()                                          # extent is required
    with pytest.raises(ValueError, match="extent"):
        _as_config({"every": 10})
    with pytest.raises(ValueError, match="unknown"):
        _as_config({"extent": 1.0, "evry": 10})
    with pytest.raises(TypeError):
        _as_config(3)
    bad = dict(extent=(0.0, -1.0, float("inf"), float("nan"), "1"), start=(-1, 1.5, True), stop=(-1, 2.5), every=(0, -3, 1.0),
               grad_threshold=(-1e-4, float("nan"), None), min_opacity=(-0.1, 1.1, float("nan")), percent_dense=(-1.0, float("inf")),
               max_screen_size=(-1, float("inf"), float("nan")), screen_size_from=(-1, 0.5), opacity_reset_every=(-1, 2.5),
               max_points=(0, -5, 1.5), seed=(-1, 1 << 64, 0.5))
    for name, values in bad.items():
        for value in values:
            kw = {"extent": 1.0, name: value}
            with pytest.raises(ValueError, match=name):
                DensifyConfig(**kw)
    with pytest.raises(ValueError, match="stop"):
        DensifyConfig(extent=1.0, start=100, stop=50)


def test_argument_validation_without_a_device():
    from gaussiananything_amd import fitting
    n = 8
    raw, m, v = (torch.zeros(n, 13) for _ in range(3))
    stats = (torch.zeros(n), torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32))
    ok = dict(PARAMS)
    for name, value in (("grad_threshold", -1.0), ("min_opacity", 2.0), ("percent_dense", float("nan")), ("extent", 0.0),
                        ("max_screen_size", -1), ("seed", -1), ("max_points", 0), ("round", -1), ("round", 1 << 32)):
        with pytest.raises(ValueError, match=name):
            fitting.densify_and_prune(raw, m, v, *stats, **dict(ok, **{name: value}))
    with pytest.raises(ValueError, match="no CPU path"):
        fitting.densify_and_prune(raw, m, v, *stats, **ok)
    with pytest.raises(TypeError, match="raw"):
        fitting.densify_and_prune(raw.double(), m, v, *stats, **ok)
    with pytest.raises(ValueError, match="cap"):
        fitting.reset_opacity(raw, m, v, cap=1.0)
    with pytest.raises(ValueError, match="no CPU path"):
        fitting.reset_opacity(raw, m, v)
    with pytest.raises(TypeError):
        fitting.reset_opacity(raw, m.double(), v)
