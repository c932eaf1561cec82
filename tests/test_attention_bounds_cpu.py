"""CPU test of the attention test (tests/test_attention_instances_gpu.py): a torch fp32 / bf16 emulation of the ROUNDING MODEL the
bound of tests/_bounds.py describes -- not a port of a kernel: 64-key tiles, key groups, tiles per stage and the lazy threshold are
parameters -- on a reduced copy of every input family of tests/_attention_cases.py.

* the emulation stays within the bound on every element, for 1, 2, 3 key groups, two tiles per stage, lazy on and off, for every
  operand path (q read, q with its norm, q projected inside, K normalised inside, the other head dims);
* every seeded mutation -- what a subtly wrong kernel would do -- exceeds the bound on at least one element of each family that claims
  to catch it (MUST_CATCH).  This is the standing proof that the GPU test fails on such a kernel."""
import math

import pytest
import torch

from tests import _attention_cases as ac
from tests import _bounds as bd

C32 = torch.tensor(0.125, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)
EPS32 = torch.tensor(1e-5, dtype=torch.float32)


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def _pairs(t, B, H, d):
    return t.permute(0, 2, 1, 3).reshape(B * H, t.shape[1], d)


def _normed32(x, w, d):
    ss = (x * x).sum(-1, keepdim=True)
    return _bf(x * (torch.rsqrt(ss / d + EPS32) * w))


def operands_fp32(case, z):
    """the MFMA operands as an fp32 evaluation produces them (the orders of summation are torch's, not a kernel's)"""
    c = case
    B, H, Lq, d, norm = c["B"], c["H"], c["Lq"], c["d"], c["norm"]
    f = {n: t.float() for n, t in z.items()}
    wq = f["wq"] if "q" in norm else None
    kh = _normed32(f["k"], f["wk"], d) if "k" in norm else f["k"]
    cs = 1.0
    if c["kind"] == "fwd":
        if c["qp"]:
            K = c["qp"]["K"]
            y = (f["A"] @ f["W"].T).view(B, Lq, H, 64)
            if c["qp"]["row_ss"]:
                y = y * torch.rsqrt(f["row_ss"].sum(-1) * (1.0 / K) + EPS32).view(B, Lq, 1, 1)
            if wq is not None:
                y = y * (torch.rsqrt((y * y).sum(-1, keepdim=True) * (1.0 / 64) + EPS32) * wq)
            qh = _bf(_bf(y) * C32)
        elif wq is not None:
            q = f["q"]
            qh = _bf((q * wq) * (C32 * torch.rsqrt((q * q).sum(-1, keepdim=True) * (1.0 / 64) + EPS32)))
        else:
            qh = _bf(f["q"] * C32)
    elif c["kind"] == "hdv":
        qh = _normed32(f["q"], wq, d) if wq is not None else f["q"]
        cs = float(torch.rsqrt(torch.tensor(float(d), dtype=torch.float32)) * torch.tensor(1.4426950408889634, dtype=torch.float32))
    else:
        qh = _bf(f["q"] * (torch.rsqrt(torch.tensor(float(d), dtype=torch.float32)) * torch.tensor(1.4426950408889634, dtype=torch.float32)))
    return _pairs(qh, B, H, d), _pairs(kh, B, H, d), _pairs(f["v"], B, H, d), cs


def emulate(qh, kh, v, cs=1.0, lazy=8.0, ks=1, tps=1, mutate=None):
    """fp32 attention over [P, L, d] operands with the rounding points of the model: fp32 scores, exp2, the fp32 row sum of the unrounded
    P, bf16 P into the P V product, one (max, sum, O) state per key group merged at the end, o (1 / l), bf16 store.  lazy > 0: the
    reference moves only when a row of a 16-row block exceeds it by more than `lazy` (the scale is folded into qh: cs = 1);
    lazy = 0: the running maximum, the scale cs inside the exponent."""
    P, Lq, d = qh.shape
    Lk = kh.shape[1]
    T = (Lk + 63) // 64
    if mutate == "q_shift":
        qh = torch.roll(qh, 1, 1)
    if mutate == "drop_last" and Lk > 1:          # the clamp of the ragged tile one key short: key Lk - 1 read from row Lk - 2
        kh = kh.clone()
        kh[:, Lk - 1] = kh[:, Lk - 2]
    if mutate == "swap_v" and Lk > 1:
        v = v.clone()
        v[:, [Lk - 2, Lk - 1]] = v[:, [Lk - 1, Lk - 2]]
    pad = (-Lq) % 16
    if pad:
        qh = torch.cat([qh, qh[:, -1:].expand(P, pad, d)], 1)
    R = qh.shape[1]
    states = []
    for g in range(ks):
        m = torch.zeros(P, R) if lazy > 0 else torch.full((P, R), -1e30)
        l, o, first, any_tile = torch.zeros(P, R), torch.zeros(P, R, v.shape[2]), True, False
        for tile in range(T):
            if (tile // tps) % ks != g or (mutate == "skip_tile" and tile == 1):
                continue
            any_tile = True
            lo, hi = tile * 64, min(tile * 64 + 64, Lk)
            s = qh @ kh[:, lo:hi].transpose(1, 2)
            if mutate == "mask_extra" and hi == Lk:
                s[:, :, -1] = -1e30
            if lazy > 0:
                s = s - m[..., None]
                tmax = s.amax(-1)
                move = (tmax > lazy).view(P, R // 16, 16).any(-1, keepdim=True).expand(P, R // 16, 16).reshape(P, R)
                if first:
                    delta, alpha = tmax, torch.zeros(P, R)
                else:
                    delta = torch.where(move, tmax.clamp_min(0), torch.zeros(P, R))
                    alpha = torch.exp2(-delta)
                    if mutate == "no_rescale":
                        alpha = torch.ones(P, R)
                m = m + delta
                s = s - delta[..., None]
                p = torch.exp2(s)
            else:
                m_new = torch.maximum(m, s.amax(-1) * cs)
                alpha = torch.exp2(m - m_new)
                if mutate == "no_rescale":
                    alpha = torch.ones(P, R)
                m = m_new
                p = torch.exp2(s * cs - m_new[..., None])
            l = l * alpha + p.sum(-1)
            o = o * alpha[..., None] + _bf(p) @ v[:, lo:hi]
            first = False
        states.append((m if any_tile else torch.full((P, R), -1e30), l, o))
    m_all = torch.stack([s[0] for s in states]).amax(0)
    l, o = torch.zeros(P, R), torch.zeros(P, R, v.shape[2])
    for g, (m, lg, og) in enumerate(states):
        w = torch.exp2((states[0][0] if mutate == "merge_ref" and g > 0 else m) - m_all)
        l, o = l + w * lg, o + w[..., None] * og
    return _bf(o * (1.0 / l)[..., None])[:, :Lq]


# operand paths (kind, d, norm, qp) x walk parameters (key groups, tiles per stage): what the instances of the two files combine
PATHS = {"fwd": ("fwd", 64, "", None), "fwd_nq": ("fwd", 64, "q", None), "fwd_knorm": ("fwd", 64, "k", None), "fwd_nqk": ("fwd", 64, "qk", None),
         "fwd_qp": ("fwd", 64, "q", dict(K=192, tiled=False, row_ss=True)), "hdv_nq": ("hdv", 72, "q", None), "hdv_nqk": ("hdv", 40, "qk", None),
         "hdv": ("hdv", 96, "", None), "hd": ("hd", 56, "", None)}
WALKS = {"fwd": [(3, 1), (2, 1), (1, 2)], "fwd_nq": [(3, 1), (1, 2)], "fwd_knorm": [(1, 1)], "fwd_nqk": [(1, 1)], "fwd_qp": [(3, 1)],
         "hdv_nq": [(1, 1), (2, 1)], "hdv_nqk": [(2, 1)], "hdv": [(2, 1)], "hd": [(1, 1)]}


def _case(path, family):
    kind, d, norm, qp = PATHS[path]
    Lk = 456 if family in ("ascending", "descending", "under_lazy") else 200
    return ac.A(f"cpu_{path}_{family}", kind, 2, 2, 64, Lk, family, d=d, norm=norm, qp=qp)


_cache = {}


def _prepared(path, family):
    if (path, family) not in _cache:
        _cache.clear()                      # (one case at a time: the parametrisation is ordered by case)
        c = _case(path, family)
        z = ac.inputs(c)
        o = ac.operands(c, z)
        _cache[(path, family)] = (c, o, operands_fp32(c, z))
    return _cache[(path, family)]


def _ratio(path, family, ks, tps, mutate=None):
    c, o, (qh, kh, v, cs) = _prepared(path, family)
    lazy = 8.0 if c["kind"] == "fwd" else 0.0
    ref, bound, dom = bd.attention(o["qh"], o["dq"], o["kh"], o["dk"], o["v"], c=o["c"], n_acc=o["n_acc"], rel_c=o["rel_c"], lazy=o["lazy"], groups=ks)
    got = emulate(qh, kh, v, cs=cs, lazy=lazy, ks=ks, tps=tps, mutate=mutate).double()
    r = (got - ref).abs() / bound
    return torch.where(torch.isfinite(r), r, torch.full_like(r, math.inf)), ref, bound


@pytest.mark.parametrize("family", ac.FAMILIES)
@pytest.mark.parametrize("path", list(PATHS))
def test_the_emulated_rounding_model_stays_within_the_bound(path, family):
    for ks, tps in WALKS[path]:
        r, ref, bound = _ratio(path, family, ks, tps)
        print(f"{path} {family} ks={ks} tps={tps}: worst err/bound {float(r.max()):.3f}, median bound {float(bound.median()):.3g}, "
              f"median |out| {float(ref.abs().median()):.3g}")
        assert float(r.max()) <= 1.0, (path, family, ks, tps, float(r.max()))


# mutation -> the families that must catch it (flat data is allowed not to see a missing rescale: its rows never move their reference)
MUST_CATCH = {
    "drop_last": ("planted8", "planted14", "fewhot"),
    "mask_extra": ("planted8", "planted14", "fewhot"),
    "swap_v": ("planted8", "planted14", "fewhot"),
    "skip_tile": ("planted8", "planted14", "fewhot", "flat"),
    "no_rescale": ("ascending", "under_lazy", "planted8", "planted14"),
    "merge_ref": ("ascending", "descending", "under_lazy", "planted14"),
    "q_shift": ("planted8", "planted14", "flat"),
}
MUTATION_WALKS = [("fwd_nq", 3, 1), ("fwd", 1, 2), ("fwd", 2, 1), ("hdv_nq", 2, 1), ("fwd_qp", 3, 1)]


@pytest.mark.parametrize("family", sorted({f for fs in MUST_CATCH.values() for f in fs}))
def test_every_seeded_mutation_exceeds_the_bound(family):
    for path, ks, tps in MUTATION_WALKS:
        for mutate, families in MUST_CATCH.items():
            if family not in families or (mutate == "merge_ref" and ks == 1):
                continue
            r, _, _ = _ratio(path, family, ks, tps, mutate)
            print(f"{mutate:10s} {family:10s} {path} ks={ks} tps={tps}: worst err/bound {float(r.max()):.3g}, {int((r > 1).sum())} elements over")
            assert float(r.max()) > 1.0, (mutate, family, path, ks, tps, float(r.max()))


def test_flat_data_does_not_see_a_missing_rescale():
    """why the designed families exist: on randn inputs the rescale branch can be deleted without moving one output over its bound"""
    r, _, _ = _ratio("fwd_nq", "flat", 3, 1, "no_rescale")
    print(f"no_rescale on flat data: worst err/bound {float(r.max()):.3f}")
    assert float(r.max()) <= 1.0
