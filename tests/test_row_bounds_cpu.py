"""CPU test of the row-kernel test (tests/test_row_instances_gpu.py): a torch fp32 / bf16 emulation of the ROUNDING MODEL the bounds of
tests/_bounds.py ("Row kernels") describe -- not a port of a kernel: the orders of summation are torch's -- on every case of
tests/_row_cases.py.

* the emulation stays within the bound on every element of every case (and the branch-reach assertions of the case file hold: the
  reference asserts them);
* every seeded mutation -- what a subtly wrong kernel would do -- exceeds the bound on at least one element of every case that claims
  to catch it (MUST_CATCH).  This is the standing proof that the GPU test fails on such a kernel;
* a removed softplus threshold is documented as outside the test's reach: log1pf(expf(x)) agrees with x beyond 20 to ~1e-9 relative."""
import math

import pytest
import torch

from tests import _row_cases as rc

F32 = torch.float32


def _bf(x):
    return x.to(torch.bfloat16).to(F32)


def _f(z):
    return {n: t.to(F32) for n, t in z.items()}


def _silu(v):
    return v / (1.0 + torch.exp(-v))


def _c(v):
    return torch.tensor(v, dtype=F32)


# ------------------------------------------------------------------------------------------------------------------- emulations
def emu_rmsnorm_modulate(c, z, mutate=None):
    f = _f(z)
    M, D, rpb, first = c["M"], c["D"], c["rpb"], c["first"]
    x = f["x"].clone()
    if first is not None:
        lo = {"bias_from_next": first + 1, "bias_whole_workgroup": first // 4 * 4}.get(mutate, first)
        x[lo:] = x[lo:] + f["row_bias"]
    xs = x[:, :D - 4] if mutate == "drop_last_float4" else x
    eps = _c(1e-6 if mutate == "eps" else 1e-5)
    rs = torch.rsqrt((xs * xs).sum(-1, keepdim=True) / D + eps)
    y = x * rs * f["weight"]
    if c["mod"] != "none":
        b = torch.arange(M) // rpb
        if mutate == "neighbour_batch":                                 # the last row of a batch item reads the next item's modulation
            b = torch.where((torch.arange(M) + 1) % rpb == 0, (b + 1).clamp(max=int(b.max())), b)
        sc, sh = f["table"][b, 1], f["table"][b, 0]
        y = y * (sc if mutate == "no_one_plus" else 1.0 + sc) + sh
    return {"out": _bf(y), "x": x}


def _layernorm32(x, D, eps, mutate):
    xs = x[:, :D - 4] if mutate == "drop_last_float4" else x
    mean = xs.sum(-1, keepdim=True) / D
    e = x - mean
    return e * torch.rsqrt((e * e).sum(-1, keepdim=True) / D + eps)


def emu_layernorm_modulate(c, z, mutate=None):
    f = _f(z)
    eps = c["eps"]
    if mutate == "eps":
        eps = 1e-6 if eps == 1e-5 else 1e-5
    y = _layernorm32(f["x"], c["D"], _c(eps), mutate)
    if c["affine"]:
        y = y * f["weight"] + f["bias"]
    if c["mod"]:
        r = torch.arange(c["M"])
        if mutate == "neighbour_batch":
            r = (r + 1).clamp(max=c["M"] - 1)
        sc, sh = f["table"][r, 1], f["table"][r, 0]
        y = y * (sc if mutate == "no_one_plus" else 1.0 + sc) + sh
    return {"out": _bf(y)}


def emu_small_linear(c, z, mutate=None):
    f = _f(z)
    x = f["x"]
    if c["act_in"] == 1:
        x = _silu(x)
    elif c["act_in"] == 2:
        j = torch.arange(128, dtype=F32)
        fr = torch.exp(_c(-9.210340371976184) * j / (256.0 if mutate == "freq_256" else 128.0))
        arg = x.view(-1, 1) * fr
        halves = [torch.cos(arg), torch.sin(arg)]
        x = torch.cat(halves[::-1] if mutate == "swap_sin_cos" else halves, 1)
    v = (x if mutate == "no_bf16_input" else _bf(x)) @ f["W"].T
    if c["bias"]:
        v = v + f["bias"]
    if c["act_out"]:
        v = _silu(v)
    if c["add"]:
        v = v + f["add"]
    return {"y": v}


def emu_shift_bias(c, z, mutate=None):
    f = _f(z)
    v = f["shift"] @ f["W"].T
    return {"out": v + f["bias"] if c["bias"] else v}


def emu_tiny_mlp_silu(c, z, mutate=None):
    f = _f(z)
    s = f["b1"] + f["x"] @ f["w1"].T
    if mutate == "erf_gelu":
        h = torch.nn.functional.gelu(s)
    else:
        h = 0.5 * s * (1.0 + torch.tanh(_c(0.7978845608028654) * (s + _c(0.044715) * s * s * s)))
    return {"out": _bf(_silu(f["b2"] + h @ f["w2"].T))}


def emu_assemble_tokens(c, z, mutate=None):
    P, D, sf, f = c["P"], c["D"], c["src_f"], c["f"]
    p = torch.arange(P)
    sr = (p // sf) * (1 + sf) + 1 + p % sf if sf else p
    return {"out": torch.cat([z["src"][sr].view(P, 1, D), z["latent_embedding"].expand(P, f, D)], 1).reshape(P * (1 + f), D).to(F32)}


def emu_tiny_attention(c, z, mutate=None):
    """tile by tile as the kernel forms them: G = 16 / S whole groups, a block-diagonal mask, exp2 of the log2-scaled difference, the
    NORMALISED probabilities rounded to bf16 into the P V product"""
    S, groups, H = c["S"], c["groups"], c["heads"]
    G = 16 // S
    qkv = z["qkv"].to(F32).reshape(groups * S, 3, H, 64)
    out = torch.empty(groups * S, H, 64)
    log2e = _c(1.4426950408889634)
    for t0 in range(0, groups, G):
        nrow = min(G, groups - t0) * S
        rows = torch.arange(t0 * S, t0 * S + nrow)
        key = torch.arange(nrow)
        if mutate == "pad_key" and nrow < G * S:                        # one padding key (a re-read of the last valid row) admitted
            rows, key = torch.cat([rows, rows[-1:]]), torch.cat([key, key[-1:]])
        q, k, v = qkv[rows[:nrow], 0], qkv[rows, 1], qkv[rows, 2]
        span = G * S if mutate == "mask_tile" else S
        ok = (torch.arange(nrow)[:, None] // span) == (key[None, :] // span)
        for h in range(H):
            p = (q[:, h] @ k[:, h].T) * 0.125
            p = torch.where(ok, p, _c(-1e30))
            e = torch.where(ok, torch.exp2((p - p.amax(-1, keepdim=True)) * log2e), _c(0.0))
            out[rows[:nrow], h] = _bf(e * (1.0 / e.sum(-1, keepdim=True))) @ v[:, h]
    return {"out": _bf(out.reshape(groups * S, H * 64))}


def emu_surfel_head(c, z, mutate=None):
    f = _f(z)
    D, mode = c["D"], c["mode"]
    xr, p = rc.sh_rows(c)
    if mutate == "token_row":
        xr = xr - 1                                                     # p (1 + f) + j instead of p (1 + f) + 1 + j
    x = f["x"][xr]
    if mode == 1:
        y = _layernorm32(x, D, _c(1e-6 if mutate == "eps" else 1e-5), mutate) * f["ln_weight"] + f["ln_bias"]
    else:
        y = _silu(x)
    pre = y @ f["w"].T + f["b"]
    if mode == 0:
        pos = torch.tanh(pre[:, :3]) * _c(0.225) * _c(0.7) + f["anchor"]
    else:
        pos = torch.tanh(pre[:, :3]) * _c(0.225) + f["anchor"][p, :3]
        pre = pre + f["base_pre"][p]
    g = torch.empty_like(pre)
    g[:, :3] = pos
    g[:, 3] = 1.0 / (1.0 + torch.exp(-pre[:, 3]))
    sp = torch.log1p(torch.exp(pre[:, 4:6]))
    g[:, 4:6] = (sp if mutate == "no_softplus_threshold" else torch.where(pre[:, 4:6] > 20.0, pre[:, 4:6], sp)) * _c(0.0045) / _c(0.6931471805599453)
    n = torch.sqrt((pre[:, 6:10] ** 2).sum(-1, keepdim=True))
    g[:, 6:10] = pre[:, 6:10] * (1.0 / (n if mutate == "no_normalize_clamp" else n.clamp_min(1e-12)))
    g[:, 10:] = 0.5 * torch.tanh(pre[:, 10:]) + 0.5
    return {"gaussians": g, "pre_out": pre}


EMULATE = {"rmsnorm_modulate": emu_rmsnorm_modulate, "small_linear": emu_small_linear, "shift_bias": emu_shift_bias,
           "layernorm_modulate": emu_layernorm_modulate, "tiny_mlp_silu": emu_tiny_mlp_silu, "assemble_tokens": emu_assemble_tokens,
           "tiny_attention": emu_tiny_attention, "surfel_head": emu_surfel_head}

_cache = {}


def _prepared(case):
    if case["name"] not in _cache:
        if len(_cache) > 64:
            _cache.clear()
        z = rc.inputs(case)
        _cache[case["name"]] = (z, rc.reference(case, z))
    return _cache[case["name"]]


def _ratio(case, mutate=None):
    z, ref = _prepared(case)
    got = EMULATE[case["kernel"]](case, z, mutate)
    return {n: rc.worst_ratio(got[n], *ref[n]) for n in ref}


@pytest.mark.parametrize("case", rc.ALL, ids=[c["name"] for c in rc.ALL])
def test_the_emulated_rounding_model_stays_within_the_bound(case):
    r = _ratio(case)
    print(f"{case['name']}: worst err/bound " + ", ".join(f"{n} {v:.3f}" for n, v in r.items()))
    assert max(r.values()) <= 1.0, (case["name"], r)


# (kernel, mutation) -> the cases that must catch it.  A mutation is claimed only where it changes what the kernel computes: a bias
# that starts one row late needs a row that gets it, a workgroup-wide bias needs `first` inside a 4-row workgroup, a dropped float4
# needs the families that put energy there, eps needs the low-energy rows, a key of the neighbouring group needs a tile with two groups,
# a padding key needs a ragged tile whose uniform weights it dilutes (S = 1 re-reads the only key of its group: nothing changes).
# An unrounded input moves a sum by ~ sqrt(K) 2^-9 |x w| while the accumulation bound grows as K^2 u |x w|: claimed up to K = 264.
MUST_CATCH = {
    ("rmsnorm_modulate", "eps"): lambda c: c["family"] == "low",
    ("rmsnorm_modulate", "drop_last_float4"): lambda c: c["family"] in ("plain", "big"),
    ("rmsnorm_modulate", "neighbour_batch"): lambda c: c["mod"] != "none",
    ("rmsnorm_modulate", "no_one_plus"): lambda c: c["mod"] != "none",
    ("rmsnorm_modulate", "bias_from_next"): lambda c: c["first"] is not None and c["first"] < c["M"],
    ("rmsnorm_modulate", "bias_whole_workgroup"): lambda c: c["first"] is not None and c["first"] % 4 != 0 and c["first"] < c["M"],
    ("layernorm_modulate", "eps"): lambda c: c["family"] == "low",
    ("layernorm_modulate", "drop_last_float4"): lambda c: c["family"] in ("plain", "big"),
    ("layernorm_modulate", "neighbour_batch"): lambda c: c["mod"] == 1,
    ("layernorm_modulate", "no_one_plus"): lambda c: c["mod"] == 1,
    ("small_linear", "no_bf16_input"): lambda c: c["act_in"] != 2 and 256 <= c["K"] <= 264 and c["N"] >= 6,
    ("small_linear", "swap_sin_cos"): lambda c: c["act_in"] == 2,
    ("small_linear", "freq_256"): lambda c: c["act_in"] == 2,
    ("tiny_attention", "pad_key"): lambda c: rc.ta_ragged(c) and c["family"] == "flat" and c["S"] > 1,
    ("tiny_attention", "mask_tile"): lambda c: c["S"] <= 8 and c["groups"] >= 2,
    ("tiny_mlp_silu", "erf_gelu"): lambda c: c["Ch"] >= 10 and c["D"] >= 70,
    ("surfel_head", "eps"): lambda c: c["family"] == "low",
    ("surfel_head", "drop_last_float4"): lambda c: c["mode"] == 1 and c["family"] == "plain",
    ("surfel_head", "no_normalize_clamp"): lambda c: c["family"] == "tail",
    ("surfel_head", "token_row"): lambda c: c["mode"] == 1,
}


@pytest.mark.parametrize("key", list(MUST_CATCH), ids=[f"{k}-{m}" for k, m in MUST_CATCH])
def test_every_seeded_mutation_exceeds_the_bound(key):
    kernel, mutate = key
    claimed = [c for c in rc.CASES[kernel] if MUST_CATCH[key](c)]
    assert claimed, f"no case claims {key}"
    for c in claimed:
        r = _ratio(c, mutate)
        print(f"{mutate:22s} {c['name']}: worst err/bound " + ", ".join(f"{n} {v:.3g}" for n, v in r.items()))
        assert max(r.values()) > 1.0, (mutate, c["name"], r)


def test_a_removed_softplus_threshold_is_outside_the_reach_of_the_test():
    """log1pf(expf(x)) agrees with x to ~1e-9 relative beyond the threshold of 20, far inside any fp32 bound: the tail cases reach the
    branch (the case file asserts pre > 20 on a scale channel), so a WRONG branch body would show, but not its absence"""
    for c in rc.CASES["surfel_head"]:
        if c["family"] == "tail":
            r = _ratio(c, "no_softplus_threshold")
            assert max(r.values()) <= 1.0, (c["name"], r)
    assert math.log1p(math.exp(21.0)) - 21.0 < 1e-9


def test_plain_rows_do_not_see_a_wrong_epsilon():
    """why the low-energy family exists: on O(1) rows eps 1e-5 against 1e-6 stays inside the bound"""
    c = next(c for c in rc.CASES["rmsnorm_modulate"] if c["family"] == "plain")
    assert max(_ratio(c, "eps").values()) <= 1.0
