"""CPU test of the head / tail kernel test (tests/test_headtail_instances_gpu.py), in the pattern of tests/test_row_bounds_cpu.py: a
torch fp32 / bf16 emulation of each kernel's arithmetic -- not a port: the orders of summation are torch's -- on every case of
tests/_headtail_cases.py.

* the emulation stays within the bound on every element of every case (and the reach assertions of the case file hold);
* every seeded mutation -- what a subtly wrong kernel would do -- exceeds the bound on at least one element of every case that claims
  to catch it (MUST_CATCH).  This is the standing proof that the GPU test fails on such a kernel."""
import pytest
import torch

from tests import _headtail_cases as hc

F32 = torch.float32


def _bf(x):
    return x.to(torch.bfloat16).to(F32)


def _f(z):
    return {n: t.to(F32) for n, t in z.items() if torch.is_tensor(t)}


def _silu(v):
    return v / (1.0 + torch.exp(-v))


def _c(v):
    return torch.tensor(v, dtype=F32)


# ------------------------------------------------------------------------------------------------------------------- emulations
def _pe(xyz, mutate):
    M = xyz.shape[0]
    pe = torch.zeros(M, 63)
    pe[:, :3] = xyz
    for k in range(10):
        arg = (xyz[:, [2, 1, 0]] if mutate == "axis_order" else xyz) * float(1 << (k + 1 if mutate == "k_off_by_one" else k))
        s, c = torch.sin(arg), torch.cos(arg)
        if mutate == "swap_sin_cos":
            s, c = c, s
        pe[:, 3 + 6 * k:6 + 6 * k], pe[:, 6 + 6 * k:9 + 6 * k] = s, c
    return pe


def emu_stream(c, z, f, mutate):
    stage2, _, C, _ = hc.forward_shape(c)
    M, D = c["B"] * c["L"], c["D"]
    x = _bf(f["x"]).clone()
    if mutate == "drop_channel_15" and C == 16:
        x[:, 15] = 0
    acc = f["b1"] + x @ _bf(f["w1"]).T
    h = 0.5 * acc * (1.0 + torch.tanh(_c(0.7978845608028654) * (acc + _c(0.044715) * acc * acc * acc)))
    h = h if mutate == "h_not_rounded" else _bf(h)
    r = torch.zeros(M, D)
    if stage2:
        r = f["bx"] + _bf(_pe(f["xyz"], mutate)) @ _bf(f["wx"]).T
    if mutate == "drop_last_column_tile":                               # what was never written: zeros here
        n0 = (D - 1) // 128 * 128
        h[:, n0:], r[:, n0:] = 0, 0
    if mutate == "drop_ragged_tokens" and M % 8:
        h[M - M % 8:], r[M - M % 8:] = 0, 0
    return r + (h + f["b2"])


def emu_gates(c, z, f, x, mutate):
    D, B, L, depth = c["D"], c["B"], c["L"], c["depth"]
    t = f["tb2"] + f["pooled"]
    t0 = _bf(_silu(t)) @ f["adaln_w"].T + f["adaln_b"]
    mod = f["tables"].view(depth, 1, 6, D) + t0.view(1, B, 6, D)        # [blk][b][row][d]
    if mutate == "swap_block_batch":
        mod = mod.transpose(0, 1)
    b = torch.arange(B * L) // L
    rows = (5, 2) if mutate == "swap_rows_2_5" else (2, 5)
    for blk in range(depth):
        x = x + mod[blk, b, rows[0]] * f["proj_b"][blk]
        x = x + mod[blk, b, rows[1]] * f["fc2_b"][blk]
    return x


def emu_final_rows(c, z, f, x, mutate):
    D, B, L = c["D"], c["B"], c["L"]
    t = f["tb2"] + f["pooled"]
    if "fmod_w" in f:
        v = _bf(_silu(t)) @ f["fmod_w"].T + f["fmod_b"]
        sh, sc = v[:, :D], v[:, D:]
    else:
        sh, sc = f["table"][0] + t, f["table"][1] + t
    if mutate == "swap_shift_scale":
        sh, sc = sc, sh
    b = torch.arange(B * L) // L
    if mutate == "neighbour_modulation":
        b = (b + 1) % B
    v = x if mutate == "unpivoted" else x - x[:, :1]
    keep = slice(0, ((D - 1) // 256 * 256 if D > 256 else D - 4)) if mutate == "stats_drop_last_chunk" else slice(0, D)
    mean = v[:, keep].sum(-1, keepdim=True) / D
    var = (v * v)[:, keep].sum(-1, keepdim=True) / D - mean * mean
    rs = torch.rsqrt(var.clamp_min(0.0) + _c(1e-5 if mutate == "eps" else 1e-6))
    y = (v - mean) * rs * (1.0 + sc[b]) + sh[b]
    return y if mutate == "input_not_rounded" else _bf(y)


def emu_forward(c, z, mutate=None):
    f = _f(z)
    k, D, B, L = c["kernel"], c["D"], c["B"], c["L"]
    M = B * L
    x = emu_stream(c, z, f, mutate)
    if k == "gates":
        x = emu_gates(c, z, f, x, mutate)
    y = emu_final_rows(c, z, f, x, mutate)
    if k in ("embed", "gates"):
        return {"y": y + f["final_b"][torch.arange(D) % 16]}
    W = f["final_w"] if mutate == "weight_not_rounded" else _bf(f["final_w"])
    keep = slice(0, ((D - 1) // 256 * 256 if D > 256 else D - 4)) if mutate == "dot_drop_last_chunk" else slice(0, D)
    out = y[:, keep] @ W[:, keep].T + f["final_b"]
    if k == "final":
        return {"out": out}
    half = M // 2 if c["cfg"] else M
    if c["cfg"]:
        cnd, unc = out[:half], out[half:]
        if mutate == "wrong_twin":
            unc = unc.roll(1, 0)
        v = (cnd if mutate == "cfg_from_c" else unc) + _c(c["s"]) * (cnd - unc)
        v = torch.cat([v, v])
    else:
        v = out
    if c["mode"] == "velocity":
        if mutate == "one_half_only" and c["cfg"]:
            v = torch.cat([v[:half], torch.zeros_like(v[half:])])
        return {"velocity": v}
    y = f["x"] + f["dt"] * v
    if mutate == "one_half_only" and c["cfg"]:
        y = torch.cat([y[:half], f["x"][half:]])
    res = {"state": y}
    if c["mode"] == "euler":
        traj = torch.full((z["slices"], M * c["Cout"]), hc.TRAJ_FILL)
        traj[z["counter"] + (0 if mutate == "slice_counter" else 1)] = y.reshape(-1)
        res["traj"] = traj
    return res


def emu_pooled(c, z, mutate=None):
    f = _f(z)
    x, K = f["x"], c["ctx"]
    mean = x.sum(-1, keepdim=True) / K
    if mutate == "one_pass_variance":
        var = (x * x).sum(-1, keepdim=True) / K - mean * mean
    else:
        var = ((x - mean) ** 2).sum(-1, keepdim=True) / K
    y = (x - mean) * torch.rsqrt(var.clamp_min(0.0) + _c(1e-5)) * f["ln_w"] + (0.0 if mutate == "drop_ln_bias" else f["ln_b"])
    out = _bf(y) @ f["W"].T + (0.0 if mutate == "drop_bias" else f["b"])
    return {"scratch": y, "out": out}


def emu_ctxnorm(c, z, mutate=None):
    f = _f(z)
    x, K = f["x"], c["ctx"]
    if mutate == "subtract_mean":
        x = x - x.sum(-1, keepdim=True) / K
    rs = torch.rsqrt((x * x).sum(-1, keepdim=True) / K + _c(1e-6 if mutate == "eps" else 1e-5))
    return {"scratch": _bf(x * rs * f["w"][0 if mutate == "first_block_weight" else -1])}


def emu_advance(c, z, mutate=None):
    n, cnt = c["grid_len"], c["counter"]
    k = cnt + 1 if mutate == "no_clamp" else min(cnt + 1, n - 1)
    kd = min(cnt, n - 1) if mutate == "dt_before_increment" else k
    pad = torch.cat([z["t_grid"], torch.full((64,), -5.0, dtype=hc.F64)]), torch.cat([z["dt_grid"], torch.full((64,), -5.0, dtype=hc.F64)])
    return {"timesteps": pad[0][k].expand(c["batch"]).clone().view(1, -1), "dt": pad[1][kd].view(1, 1),
            "counter": torch.tensor([[float(cnt + 1)]], dtype=hc.F64)}


EMULATE = {"embed": emu_forward, "final": emu_forward, "step": emu_forward, "gates": emu_forward, "pooled": emu_pooled,
           "ctxnorm": emu_ctxnorm, "advance": emu_advance}

_cache = {}


def _prepared(case):
    if case["name"] not in _cache:
        if len(_cache) > 32:
            _cache.clear()
        z = hc.inputs(case)
        _cache[case["name"]] = (z, hc.reference(case, z))
    return _cache[case["name"]]


def _ratio(case, mutate=None):
    z, ref = _prepared(case)
    got = EMULATE[case["kernel"]](case, z, mutate)
    return {n: hc.worst_ratio(got[n], *ref[n]) for n in ref}


@pytest.mark.parametrize("case", hc.ALL, ids=[c["name"] for c in hc.ALL])
def test_the_emulated_rounding_model_stays_within_the_bound(case):
    r = _ratio(case)
    print(f"{case['name']}: worst err/bound " + ", ".join(f"{n} {v:.3f}" for n, v in r.items()))
    assert max(r.values()) <= 1.0, (case["name"], r)


# (kernel, mutation) -> the cases that must catch it.  A mutation is claimed only where it changes what the kernel computes: a dropped
# column tile or chunk needs what it drops to matter (every row is normalised over all columns, so one dropped tile moves the whole row;
# the dot product needs the non-zero weights of the last float4, which every final case plants), ragged tokens need M % 8 != 0, channel
# 15 needs C = 16, the positional-encoding mutations need stage 2, the unpivoted variance needs the common offset, eps the low-variance
# rows, the neighbour's modulation more than one batch item, the CFG mutations a CFG case (with cfg_scale 1 the guided velocity u + (c - u)
# is c whatever u is: the wrong twin is claimed where the scale is 4; c + s (c - u) differs from it by c - u at either scale), one half
# only and the wrong slice the Euler update.  pooled: the mean of a correct two-pass kernel may carry gamma(D) |offset| in the worst order
# of summation, the one-pass variance loses u offset^2: their ratio is offset / (D spread) -- 31 and 10 at 64 and 192 columns, 2 at 1024,
# so the one-pass variance is claimed up to 192 columns.
MUST_CATCH = {
    ("embed", "drop_last_column_tile"): lambda c: True,
    ("embed", "drop_ragged_tokens"): lambda c: c["B"] * c["L"] % 8 != 0,
    ("embed", "swap_sin_cos"): lambda c: c["stage"] == 2,
    ("embed", "k_off_by_one"): lambda c: c["stage"] == 2,
    ("embed", "axis_order"): lambda c: c["stage"] == 2,
    ("embed", "drop_channel_15"): lambda c: c["C"] == 16,
    ("embed", "h_not_rounded"): lambda c: c["family"] != "big" or c["stage"] == 1,
    ("final", "stats_drop_last_chunk"): lambda c: c["family"] in ("plain", "big"),
    ("final", "dot_drop_last_chunk"): lambda c: True,
    ("final", "unpivoted"): lambda c: c["family"] == "offset",
    ("final", "eps"): lambda c: c["family"] == "low",
    ("final", "neighbour_modulation"): lambda c: c["B"] > 1,
    ("final", "swap_shift_scale"): lambda c: True,
    ("final", "weight_not_rounded"): lambda c: True,
    ("final", "input_not_rounded"): lambda c: True,
    ("step", "wrong_twin"): lambda c: c["cfg"] == 1 and c["s"] != 1.0,
    ("step", "cfg_from_c"): lambda c: c["cfg"] == 1,
    ("step", "one_half_only"): lambda c: c["cfg"] == 1,
    ("step", "slice_counter"): lambda c: c["mode"] == "euler",
    ("pooled", "one_pass_variance"): lambda c: c["family"] == "offset" and c["ctx"] <= 192,
    ("pooled", "drop_bias"): lambda c: True,
    ("pooled", "drop_ln_bias"): lambda c: True,
    ("ctxnorm", "subtract_mean"): lambda c: c["T"] > 1 or c["family"] != "low",
    ("ctxnorm", "eps"): lambda c: c["family"] == "low",
    ("ctxnorm", "first_block_weight"): lambda c: c["depth"] > 1,
    ("advance", "no_clamp"): lambda c: c["counter"] + 1 > c["grid_len"] - 1,
    ("advance", "dt_before_increment"): lambda c: c["counter"] + 1 <= c["grid_len"] - 1,
    ("gates", "swap_block_batch"): lambda c: True,
    ("gates", "swap_rows_2_5"): lambda c: True,
}


@pytest.mark.parametrize("key", list(MUST_CATCH), ids=[f"{k}-{m}" for k, m in MUST_CATCH])
def test_every_seeded_mutation_exceeds_the_bound(key):
    kernel, mutate = key
    claimed = [c for c in hc.CASES[kernel] if MUST_CATCH[key](c)]
    assert claimed, f"no case claims {key}"
    for c in claimed:
        r = _ratio(c, mutate)
        print(f"{mutate:24s} {c['name']}: worst err/bound " + ", ".join(f"{n} {v:.3g}" for n, v in r.items()))
        assert max(r.values()) > 1.0, (mutate, c["name"], r)


def test_the_case_list_covers_what_the_issue_names():
    lds = {hc.final_weight_in_lds(c) for c in hc.CASES["final"]}
    assert lds == {True, False}
    assert max(c["Cout"] * c["D"] * 4 for c in hc.CASES["final"] if hc.final_weight_in_lds(c)) == hc.LDS_LIMIT
    assert min(c["Cout"] * c["D"] * 4 for c in hc.CASES["final"] if not hc.final_weight_in_lds(c)) == 65536
    assert any(c["D"] == 2048 and hc.final_weight_in_lds(c) for c in hc.CASES["final"])
    assert any(c["D"] == 2048 and not hc.final_weight_in_lds(c) for c in hc.CASES["final"])
    assert {(c["B"], c["L"]) for c in hc.CASES["step"] if c["cfg"]} >= {(2, 3), (4, 5)}
    assert {c["batch"] for c in hc.CASES["pooled"]} == {1, 3, 16} and {c["ctx"] for c in hc.CASES["pooled"]} == {64, 192, 1024}
    assert {c["B"] * c["T"] for c in hc.CASES["ctxnorm"]} == {1, 5, 154} and any(c["depth"] == 2 for c in hc.CASES["ctxnorm"])
    assert {c["batch"] for c in hc.CASES["advance"]} == {1, 16, 64}
