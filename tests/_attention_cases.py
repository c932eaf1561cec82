"""The attention case table: shapes, norms, q-projection settings and INPUT FAMILIES of ga_attention_bf16 / ga_attention_hd_bf16 calls
that together reach every kernel instance the two dispatchers can launch (tests/test_attention_plan.py checks that on the CPU through
ga_attention_plan / ga_attention_hd_plan); tests/test_attention_instances_gpu.py runs each case on the GPU against a float64 reference
with the error model of tests/_bounds.py, tests/test_attention_bounds_cpu.py proves on the CPU that the model and the families
together catch a subtly wrong kernel.

A case is a dict: name, kind ("fwd": head dim 64, ga_attention_bf16 | "hdv": ga_attention_hd_bf16 with V^T | "hd": with v row-major),
B, H, Lq, Lk, d, norm (which per-head RMSNorms run INSIDE the kernel: "", "q", "k", "qk"), qp (fwd: None or dict(K, tiled, row_ss):
the q projection inside the workgroup), family (below).

Input families (seeded, every tensor bf16-exact).  A softmax over flat random scores averages hundreds of V rows: a dropped key, a
wrong mask or merge weight moves nothing visibly.  So the keys are DESIGNED from the effective queries qe (the queries after whatever
norm / projection the kernel applies, in float64; score_ij = qe_i . ke_j / sqrt(d) nats):
  flat        randn everywhere
  planted8 /  query i of pair p = (batch, head) has ONE dominant key pi_p(i), parallel to qe_i with score 8 / 14 over a background of
  planted14   small keys: out_i ~ v[pi(i)].  pi_p(i) = Lk - 1 - (i P + p) mod Lk: across the P pairs every key is dominant for some
              query (when (Lq - 1) P >= Lk), and the last query of every pair is moved to key Lk - 1
  fewhot      five keys (fewer for few tiles) with top scores within 1 nat in different 64-key tiles -- the first two tiles, the
              middle, the last two: different key groups and both halves of a two-tile stage; positions move with the pair
  ascending   (rank-1 scores s_ij = a_i t_j, all queries of a pair nearly parallel) the tile level t rises by 6.2 nats = 8.9 log2
              units per tile: the lazy softmax must rescale in every tile, for every key group stride
  descending  the mirror image: no rescale after the first tile
  under_lazy  a staircase 0, +5.2, +5.3 (7.5 and 7.65 log2 units: P up to 2^7.65 on an unchanged reference), then +11.0 (crosses),
              repeated
  zero_q      flat with all-zero query rows (first, middle, last): RMSNorm(0) = 0, uniform softmax
  equal       every key of a pair identical: all scores equal
  negative    every score near -30 nats
With K normalised inside the kernel the key magnitudes are gone: there the raw q is scaled to reach the target scores ("k"), and with
both norms inside ("qk") the scores are what unit-RMS vectors give (|s| <= ~8 w^2): the ramp families still run, at that scale."""
import math
import zlib

import torch

FAKE_PTR = 1 << 20
FAMILIES = ("flat", "planted8", "planted14", "fewhot", "ascending", "descending", "under_lazy", "zero_q", "equal", "negative")
RANK1 = ("fewhot", "ascending", "descending", "under_lazy", "equal", "negative")
EPS = 9.99999974737875163555145263671875e-06     # 1e-5f


def A(name, kind, B, H, Lq, Lk, family, d=64, norm="", qp=None):
    assert family in FAMILIES and kind in ("fwd", "hdv", "hd")
    return dict(name=name, kind=kind, B=B, H=H, Lq=Lq, Lk=Lk, d=d, norm=norm, qp=qp, family=family)


CASES = []

# ---- ga_attention_bf16.  The instance follows W = ceil(Lq / 128) heads batch: <4,3,false> for W <= 128 (the only one that can project q
# itself), <8,2,false> up to 512, <8,1,false> (two tiles per stage) beyond, <8,1,true> whenever K is normalised inside.
# Key axis: 1 key; < 64; 64; one full + ragged tile; tile counts that leave a key group (or half a stage) empty; 768 and 1369.
# Query axis: 1; < 16; not a multiple of the workgroup's rows.
_FWD = {
    # <4,3>: 1, 2, 4, 5, 7 tiles
    "w4k3": (lambda Lq: (2, 3), [(1, 1, "flat", ""), (5, 37, "planted8", "q"), (100, 64, "planted14", ""), (70, 100, "zero_q", "q"),
                                 (130, 256, "fewhot", ""), (64, 200, "planted14", "q"), (48, 448, "ascending", ""),
                                 (48, 448, "descending", "q"), (100, 400, "under_lazy", ""), (33, 300, "equal", ""),
                                 (33, 300, "negative", "q"), (100, 300, "flat", "q"), (40, 448, "ascending", "q"),
                                 (60, 130, "fewhot", "q"), (768, 1369, "planted8", "q"), (768, 768, "planted14", "")]),
    # <8,2>: 1 and 3 tiles (the second group idle / one tile each side), 4, 7, ragged
    "w8k2": (lambda Lq: (9, 16), [(1, 1, "flat", ""), (5, 37, "planted8", "q"), (100, 64, "planted14", ""), (70, 100, "zero_q", "q"),
                                  (130, 192, "fewhot", ""), (64, 137, "planted14", "q"), (48, 448, "ascending", ""),
                                  (48, 448, "descending", "q"), (100, 400, "under_lazy", ""), (33, 300, "equal", ""),
                                  (33, 300, "negative", "q"), (20, 448, "ascending", "q"), (100, 300, "flat", "q")]),
    # <8,1,false>: two tiles per stage -- odd tile counts leave half a stage empty (1, 3, 7), even ones do not (2, 4)
    "w8k1": (lambda Lq: (33, 16), [(1, 1, "flat", ""), (5, 37, "planted8", "q"), (100, 64, "planted14", ""), (70, 100, "zero_q", "q"),
                                   (30, 192, "fewhot", ""), (64, 137, "planted14", "q"), (20, 320, "ascending", ""),
                                   (20, 320, "descending", "q"), (40, 300, "under_lazy", ""), (33, 256, "equal", ""),
                                   (33, 300, "negative", "q"), (16, 384, "ascending", "q"), (50, 256, "fewhot", "q"),
                                   (17, 128, "flat", "q")]),
    # <8,1,true>: K normalised while it is staged
    "knorm": (lambda Lq: (2, 3), [(1, 1, "flat", "qk"), (5, 37, "planted8", "qk"), (100, 64, "planted14", "k"), (70, 100, "zero_q", "qk"),
                                  (130, 256, "fewhot", "k"), (64, 200, "planted14", "qk"), (48, 448, "ascending", "k"),
                                  (48, 448, "descending", "k"), (100, 400, "under_lazy", "k"), (33, 300, "equal", "qk"),
                                  (33, 300, "negative", "k"), (100, 300, "flat", "qk"), (140, 448, "ascending", "qk")]),
}
for _inst, (_bh, _rows) in _FWD.items():
    for _Lq, _Lk, _fam, _norm in _rows:
        _B, _H = _bh(_Lq)
        if _Lq * _Lk >= 768 * 768:
            _B, _H = (1, 16) if _Lk == 1369 else (1, 2)
        CASES.append(A(f"fwd_{_inst}_{_Lq}x{_Lk}_{_fam}" + (f"_n{_norm}" if _norm else ""), "fwd", _B, _H, _Lq, _Lk, _fam, norm=_norm))
# the released sizes on the larger grids: a CFG pair's self-attention (<8,2>), CFG batch 6 (<8,1>: the real size), 1369 image tokens
CASES += [A("fwd_w8k2_768x768_planted14_nq", "fwd", 2, 16, 768, 768, "planted14", norm="q"),
          A("fwd_w8k2_768x1369_planted8_nq", "fwd", 2, 16, 768, 1369, "planted8", norm="q"),
          A("fwd_w8k1_768x768_planted14_nq", "fwd", 6, 16, 768, 768, "planted14", norm="q"),
          A("fwd_w8k1_700x1369_flat", "fwd", 6, 16, 700, 1369, "flat"),
          A("fwd_knorm_768x768_planted8_nqk", "fwd", 2, 16, 768, 768, "planted8", norm="qk")]
# <4,3> with the q projection inside: qp_k = 64 (one K-slice: two key groups have none), 192 (one each), 1024; both weight layouts;
# with and without the folded row scale; with and without the per-head norm
for _K, _tiled, _rss, _norm, _Lq, _Lk, _fam in [(64, False, False, "q", 70, 100, "planted8"), (64, True, True, "", 5, 37, "flat"),
                                               (192, False, True, "q", 100, 300, "planted14"), (192, True, False, "q", 130, 256, "fewhot"),
                                               (192, True, True, "q", 48, 448, "ascending"), (192, False, False, "", 48, 448, "descending"),
                                               (256, True, True, "q", 100, 400, "under_lazy"), (256, False, True, "q", 33, 64, "zero_q"),
                                               (128, True, False, "q", 1, 1, "equal"), (128, False, True, "", 33, 300, "negative"),
                                               (1024, True, True, "q", 200, 137, "planted14"), (1024, False, False, "q", 64, 200, "planted8")]:
    CASES.append(A(f"fwd_qp{_K}{'t' if _tiled else 'r'}{'s' if _rss else ''}_{_Lq}x{_Lk}_{_fam}" + (f"_n{_norm}" if _norm else ""), "fwd",
                   2, 3, _Lq, _Lk, _fam, norm=_norm, qp=dict(K=_K, tiled=_tiled, row_ss=_rss)))
CASES.append(A("fwd_qp1024ts_768x1369_planted8_nq", "fwd", 1, 16, 768, 1369, "planted8", norm="q", qp=dict(K=1024, tiled=True, row_ss=True)))

# ---- ga_attention_hd_bf16, the V^T variant: HD16 = 1 .. 8 (d = 8 .. 128, 16 h - 8 and 16 h alternating), both product configurations
# (3: eight waves x 16 queries for >= 160 128-query workgroups; 4: two key groups of four waves below), the norms inside: none, q, q and k.
# Geometries and families rotate with HD16 so that each configuration sees every one of them.
_HDV_GEO = [(1, 1), (5, 37), (100, 64), (70, 100), (130, 192), (64, 137), (48, 448), (33, 300)]
_HDV_FAM = {"": ("flat", "planted14", "fewhot", "ascending", "under_lazy", "equal", "negative", "planted8"),
            "q": ("planted8", "zero_q", "descending", "planted14", "ascending", "flat", "fewhot", "under_lazy"),
            "qk": ("planted14", "flat", "zero_q", "planted8", "fewhot", "ascending", "equal", "descending")}
for _h in range(1, 9):
    _d = 16 * _h - (8 if _h % 2 else 0)
    for _ci, (_cfg, _B, _H) in enumerate(((3, 4, 40), (4, 2, 3))):
        for _ni, _norm in enumerate(("", "q", "qk")):
            _Lq, _Lk = _HDV_GEO[(_h + 3 * _ci + _ni) % 8]
            _fam = _HDV_FAM[_norm][(_h + 5 * _ci) % 8]
            if _fam in ("ascending", "descending", "under_lazy") and _Lk < 300:
                _Lq, _Lk = 48, 448
            if _fam == "fewhot" and _Lk < 130:
                _Lq, _Lk = 130, 192
            CASES.append(A(f"hdv{_h}_c{_cfg}_d{_d}_{_Lq}x{_Lk}_{_fam}" + (f"_n{_norm}" if _norm else ""), "hdv", _B, _H, _Lq, _Lk, _fam, d=_d, norm=_norm))
CASES += [A("hdv5_c3_d72_768x768_planted14_nqk", "hdv", 2, 16, 768, 768, "planted14", d=72, norm="qk"),
          A("hdv5_c4_d72_768x1369_planted8_nq", "hdv", 1, 16, 768, 1369, "planted8", d=72, norm="q"),
          A("hdv4_c4_d64_1x1_flat", "hdv", 1, 1, 1, 1, "flat", d=64), A("hdv6_c3_d96_5x37_planted8_nq", "hdv", 9, 20, 5, 37, "planted8", d=96, norm="q")]
# ---- ga_attention_hd_bf16 with v row-major: attention_hd_kernel<32 | 64 | 96 | 128>
for _d, _rows in ((24, [(1, 1, "flat"), (70, 100, "planted8"), (48, 448, "ascending")]),
                  (56, [(5, 37, "planted14"), (130, 192, "fewhot"), (48, 448, "under_lazy")]),
                  (72, [(100, 64, "zero_q"), (64, 137, "planted14"), (48, 448, "descending"), (768, 768, "planted8")]),
                  (128, [(33, 300, "equal"), (33, 300, "negative"), (70, 200, "planted8"), (50, 130, "flat")])):
    for _Lq, _Lk, _fam in _rows:
        CASES.append(A(f"hd{(_d + 31) // 32 * 32}_d{_d}_{_Lq}x{_Lk}_{_fam}", "hd", *((2, 16) if _Lq == 768 else (2, 3)), _Lq, _Lk, _fam, d=_d))

assert len({c["name"] for c in CASES}) == len(CASES)


def reduced(case, Lq=64, Lk=200, B=2, H=2):
    """a small copy of a case (same kind, norms, family) for the CPU emulation"""
    return dict(case, name=case["name"] + "_reduced", B=B, H=H, Lq=Lq, Lk=Lk)


# ------------------------------------------------------------------------------------------------------------------------- inputs
def _bf(x):
    return x.to(torch.bfloat16).to(torch.float64)


def _rms(x, w):
    return x * w * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS)


def planted_map(case):
    """[P, Lq] dominant key of every query, P = pairs the map varies over (batch x heads; batch alone when q is projected inside: the
    rows of A are shared by the heads)"""
    B, H, Lq, Lk = case["B"], case["H"], case["Lq"], case["Lk"]
    P = B if case["qp"] else B * H
    i, p = torch.arange(Lq)[None], torch.arange(P)[:, None]
    pi = (Lk - 1 - (i * P + p) % Lk) % Lk
    pi[:, Lq - 1] = Lk - 1
    return pi if not case["qp"] else pi[:, None].expand(B, H, Lq).reshape(B * H, Lq)


def _levels(family, T):
    """score level (nats) of each of the T key tiles"""
    if family == "ascending":
        return [6.2 * min(t, 6) for t in range(T)]
    if family == "descending":
        return [6.2 * (6 - min(t, 6)) for t in range(T)]
    lv, cur = [], 0.0
    for t in range(T):                      # under_lazy
        lv.append(min(cur, 38.0))
        cur += (5.2, 0.1, 5.7)[t % 3]
    return lv


def _targets(case, g):
    """[P, Lk] target scores t_j (nats) of the rank-1 families"""
    B, H, Lk, fam = case["B"], case["H"], case["Lk"], case["family"]
    P, T = B * H, (case["Lk"] + 63) // 64
    j = torch.arange(Lk)
    if fam == "equal":
        return torch.full((P, Lk), 2.0, dtype=torch.float64)
    if fam == "negative":
        return -30.0 - 2.0 * torch.rand(P, Lk, generator=g, dtype=torch.float64)
    if fam == "fewhot":
        t = 0.3 * torch.randn(P, Lk, generator=g, dtype=torch.float64)
        tiles = torch.tensor(sorted({0, min(1, T - 1), T // 2, max(T - 2, 0), T - 1}))
        n, p = torch.arange(len(tiles))[None], torch.arange(P)[:, None]
        lo = tiles[None] * 64
        cnt = torch.minimum(lo + 64, torch.tensor(Lk)) - lo
        t.scatter_(1, lo + (17 * n + 5 * p + 3) % cnt, (10.0 - torch.tensor((0.0, 0.3, 0.7, 1.0, 0.5), dtype=torch.float64)[:len(tiles)])[None].expand(P, -1))
        t[:, Lk - 1] = t[:, Lk - 1].clamp_min(9.2)                   # the last key is hot in every pair
        return t
    lv = torch.tensor(_levels(fam, T), dtype=torch.float64)[j // 64]
    t = (lv - 3.0 - 0.5 * torch.rand(P, Lk, generator=g, dtype=torch.float64))
    tile, p = torch.arange(T)[None], torch.arange(P)[:, None]         # one key per tile exactly at the level, its place moves with the pair
    lo = tile * 64
    cnt = torch.minimum(lo + 64, torch.tensor(Lk)) - lo
    t.scatter_(1, lo + (17 * tile + 5 * p) % cnt, lv[lo].expand(P, T))
    return t


def inputs(case):
    """seeded CPU tensors of a case, float64 holding bf16-exact values (the fp32 operands exact fp32): q [B, Lq, H, d] (or A [B Lq, K],
    W [H 64, K], row_ss [B Lq, tiles]), k, v [B, Lk, H, d], wq, wk [d]"""
    c = case
    B, H, Lq, Lk, d, fam, norm, qp = c["B"], c["H"], c["Lq"], c["Lk"], c["d"], c["family"], c["norm"], c["qp"]
    g = torch.Generator().manual_seed(zlib.crc32(c["name"].encode()))
    rn = lambda *s: torch.randn(*s, generator=g).double()          # noqa: E731
    z = dict(wq=(1 + 0.2 * rn(d)).float().double(), wk=(1 + 0.2 * rn(d)).float().double())
    wq = z["wq"] if "q" in norm else None
    rank1 = fam in RANK1
    pi = planted_map(c) if fam.startswith("planted") else None
    # ---- queries: random (prototypes shared by the queries with the same dominant key) or nearly parallel within a pair
    if qp:
        K = qp["K"]
        if rank1:
            a0 = rn(B, 1, K)
            Araw = (0.8 + 0.2 * torch.rand(B, Lq, 1, generator=g, dtype=torch.float64)) * a0 + 0.02 * rn(B, Lq, K)
        elif pi is not None:
            Araw = torch.gather(rn(B, Lk, K), 1, pi.view(B, H, Lq)[:, 0, :, None].expand(B, Lq, K))
        else:
            Araw = rn(B, Lq, K)
        if fam == "zero_q":
            Araw[:, [0, Lq // 2, Lq - 1]] = 0
        z["A"] = _bf(Araw).reshape(B * Lq, K)
        z["W"] = _bf(rn(H * 64, K) / math.sqrt(K))
        qe = (z["A"] @ z["W"].T).view(B, Lq, H, 64)
        if qp["row_ss"]:
            tiles = (K // 64 + 3) // 4 * 4
            z["row_ss"] = torch.zeros(B * Lq, tiles, dtype=torch.float64)
            z["row_ss"][:, :K // 64] = (torch.rand(B * Lq, K // 64, generator=g) * 128).double()
            qe = qe * torch.rsqrt(z["row_ss"].sum(-1) / K + EPS).view(B, Lq, 1, 1)
    else:
        if rank1:
            qraw = (0.8 + 0.2 * torch.rand(B, Lq, H, 1, generator=g, dtype=torch.float64)) * rn(B, 1, H, d) + 0.02 * rn(B, Lq, H, d)
        elif pi is not None:
            qraw = torch.gather(rn(B, H, Lk, d), 2, pi.view(B, H, Lq, 1).expand(B, H, Lq, d)).permute(0, 2, 1, 3)
        else:
            qraw = rn(B, Lq, H, d)
        if fam == "zero_q":
            qraw[:, [0, Lq // 2, Lq - 1]] = 0
        qe = z["q"] = _bf(qraw.contiguous())
    if wq is not None:
        qe = _rms(qe, wq)
    qe = qe.permute(0, 2, 1, 3)                                            # [B, H, Lq, d] effective queries, score = qe . ke / sqrt(d)
    # ---- keys
    knorm = "k" in norm
    sd = math.sqrt(d)
    if fam in ("flat", "zero_q"):
        kd = rn(B, H, Lk, d)
    elif pi is not None:
        beta = 8.0 if fam == "planted8" else 14.0
        kd = (rn(B, H, Lk, d) if knorm else 0.3 * rn(B, H, Lk, d))
        n2 = qe.pow(2).sum(-1, keepdim=True).clamp_min(1e-30)
        idx = pi.view(B, H, Lq, 1).expand(B, H, Lq, d)
        kd.scatter_(2, idx, qe if knorm else beta * sd * qe / n2)
    else:
        t = _targets(c, g).view(B, H, Lk, 1)
        u = qe[:, :, :1]                                                   # the pair's prototype direction
        n2 = u.pow(2).sum(-1, keepdim=True).clamp_min(1e-30)
        if fam == "equal":
            kd = (2.0 * sd * u / n2).expand(B, H, Lk, d).clone()
        elif knorm:
            cj = (t / 40.0).clamp(-1, 1)
            uh = u / n2.sqrt()
            nz = rn(B, H, Lk, d)
            nz = nz - (nz * uh).sum(-1, keepdim=True) * uh
            kd = cj * uh + (1 - cj * cj).sqrt() * nz / nz.norm(dim=-1, keepdim=True).clamp_min(1e-30)
        else:
            kd = t * sd * u / n2 + (0.0 if fam == "equal" else 0.05) * rn(B, H, Lk, d)
    if knorm:
        kd = kd / z["wk"]                                                  # the kernel's norm multiplies the weight back in
    z["k"] = _bf(kd.permute(0, 2, 1, 3).contiguous())
    if knorm and "q" not in norm and "q" in z and fam not in ("flat", "zero_q"):
        # key magnitudes are normalised away: scale the raw queries so that the top score reaches the family's level
        ke = _rms(z["k"], z["wk"]).permute(0, 2, 1, 3)
        top = (z["q"].permute(0, 2, 1, 3) @ ke.transpose(-1, -2) / sd).abs().amax(-1, keepdim=True).clamp_min(1e-3)       # [B, H, Lq, 1]
        want = {"planted8": 8.0, "planted14": 14.0, "fewhot": 10.0, "equal": 2.0, "negative": 30.0}.get(fam, 38.0)
        if rank1:
            top = top[:, :, :1]
        z["q"] = _bf(z["q"] * (want / top).permute(0, 2, 1, 3))
    z["v"] = _bf(rn(B, Lk, H, d))
    return z


# ------------------------------------------------------------------------------------------------------------------- the library
def make_args(case, ptr=None, strides=None):
    """GaAttentionArgs / GaAttentionHdArgs of a case.  ptr(name) -> device pointer of the named operand (None: FAKE_PTR everywhere, for
    plan queries); strides: q_stride / k_stride / v_stride / vt_ld / out_stride / qp_lda overrides (elements)."""
    from gaussiananything_amd import dit_ops as ops
    c = case
    P = ptr or (lambda name: FAKE_PTR)
    B, H, Lq, Lk, d = c["B"], c["H"], c["Lq"], c["Lk"], c["d"]
    s = dict(q_stride=H * d, k_stride=H * d, v_stride=H * d, vt_ld=(Lk + 63) // 64 * 64, out_stride=H * d, qp_lda=c["qp"]["K"] if c["qp"] else 0)
    s.update(strides or {})
    wq = P("wq") if "q" in c["norm"] else None
    wk = P("wk") if "k" in c["norm"] else None
    if c["kind"] == "fwd":
        a = ops.GaAttentionArgs(B, H, Lq, Lk, None if c["qp"] else P("q"), P("k"), P("vt"), s["q_stride"], s["k_stride"], s["vt_ld"], wq, wk,
                                P("out"), s["out_stride"])
        if c["qp"]:
            K = c["qp"]["K"]
            a.qp_a, a.qp_w, a.qp_lda, a.qp_k, a.qp_w_tiled = P("A"), P("W"), s["qp_lda"], K, 1 if c["qp"]["tiled"] else 0
            if c["qp"]["row_ss"]:
                a.qp_row_ss, a.qp_row_ss_tiles, a.qp_row_ss_dim, a.qp_row_ss_eps = P("row_ss"), (K // 64 + 3) // 4 * 4, K, 1e-5
        return a
    if c["kind"] == "hdv":
        return ops.GaAttentionHdArgs(B, H, Lq, Lk, d, P("q"), P("k"), None, s["q_stride"], s["k_stride"], 0, P("out"), s["out_stride"],
                                     P("vt"), s["vt_ld"], wq, wk)
    return ops.GaAttentionHdArgs(B, H, Lq, Lk, d, P("q"), P("k"), P("v"), s["q_stride"], s["k_stride"], s["v_stride"], P("out"),
                                 s["out_stride"], None, 0, None, None)


def plan_of(case, ptr=None, strides=None):
    """(plan, its cell key) of a case"""
    from gaussiananything_amd import dit_ops as ops
    a = make_args(case, ptr, strides)
    p = ops.attention_plan(a) if case["kind"] == "fwd" else ops.attention_hd_plan(a)
    return p, cell(p)


def cell(p):
    """the kernel instance of a plan: ("fwd", NW, KS, KNORM, TPS) | ("hdv", HD16, config) | ("hd", HDP)"""
    if hasattr(p, "knorm"):
        return ("fwd", p.nw, p.ks, p.knorm, p.tps)
    return ("hdv", p.hd16, p.config) if p.family == 1 else ("hd", p.hdp)


def describe(p):
    if hasattr(p, "knorm"):
        return (f"attention_fwd_kernel<{p.nw},{p.ks},{'true' if p.knorm else 'false'}> tps={p.tps} q/wg={p.queries_per_wg} "
                f"qproj={p.fuses_q} grid={p.grid_x}x{p.grid_y}x{p.grid_z} lds={p.lds_bytes}")
    if p.family == 1:
        return (f"attention_hdv_kernel<{p.hd16},{p.qf},{p.nw},{p.ks}> config={p.config}{' (forced)' if p.forced else ''} "
                f"q/wg={p.queries_per_wg} grid={p.grid_x}x{p.grid_y} lds={p.lds_bytes}")
    return f"attention_hd_kernel<{p.hdp}> q/wg=64 grid={p.grid_x}x{p.grid_y}x{p.grid_z} lds={p.lds_bytes}"


def key_place(p, key):
    """(tile, key group) that walks key index `key` under plan p"""
    tile = key // 64
    tps = p.tps if hasattr(p, "tps") else 1
    return tile, (tile // tps) % p.ks


# ----------------------------------------------------------------------------------------------------------- reference and bound
def operands(case, z, dev=None):
    """the kernel's MFMA operands mirrored in float64 and the parameters of the bound: dict(qh, dq, kh, dk [P, L, d], v [P, Lk, d],
    c, n_acc, rel_c, lazy) -- tests/_bounds.py, 'Attention'.  z: inputs(case) (moved to `dev`)."""
    from tests import _bounds as bd
    c = case
    B, H, Lq, Lk, d, norm = c["B"], c["H"], c["Lq"], c["Lk"], c["d"], c["norm"]
    z = {n: (t.to(dev) if dev is not None else t) for n, t in z.items()}
    wq = z["wq"] if "q" in norm else None
    pairs = lambda t: t.permute(0, 2, 1, 3).reshape(B * H, t.shape[1], d)          # noqa: E731  [B, L, H, d] -> [B H, L, d]
    k = pairs(z["k"])
    o = dict(v=pairs(z["v"]), rel_c=0.0, c=1.0)
    if "k" in norm:
        o["kh"], o["dk"] = bd.attn_rows_normed(k, z["wk"], d)
    else:
        o["kh"], o["dk"] = k, torch.zeros_like(k)
    if c["kind"] == "fwd":
        if c["qp"]:
            K = c["qp"]["K"]
            T = z["row_ss"].sum(-1) if c["qp"]["row_ss"] else None
            qh, dq = bd.attn_q_proj(z["A"], z["W"].view(H, 64, K), T, K // 64, K, bd.EPS_F32, wq)
            qh, dq = (t.view(B, Lq, H, 64) for t in (qh, dq))
        else:
            qh, dq = bd.attn_q_fwd(z["q"], wq)
        o.update(qh=pairs(qh), dq=pairs(dq), n_acc=64, lazy=8.0)
    elif c["kind"] == "hdv":
        # q is read unrounded unless its norm runs inside; the scale is the fp32 product rsqrtf(d) log2 e inside the exponent's FMA
        qh, dq = bd.attn_rows_normed(z["q"], wq, d) if wq is not None else (z["q"], torch.zeros_like(z["q"]))
        o.update(qh=pairs(qh), dq=pairs(dq), n_acc=(d + 15) // 16 * 16, lazy=0.0, c=bd.LOG2E_F32 / math.sqrt(d),
                 rel_c=bd.RSQRT_REL + bd.gamma(1))
    else:
        qh, dq = bd.attn_q_hd(z["q"], d)
        o.update(qh=pairs(qh), dq=pairs(dq), n_acc=(d + 31) // 32 * 32, lazy=0.0)
    return o


def reference(case, z, groups, dev=None, budget=1 << 27):
    """(out [B, Lq, H d], bound, dominant key [B, H, Lq]) of a case in float64"""
    from tests import _bounds as bd
    o = operands(case, z, dev)
    B, H, Lq, d = case["B"], case["H"], case["Lq"], case["d"]
    out, bound, dom = bd.attention(o["qh"], o["dq"], o["kh"], o["dk"], o["v"], c=o["c"], n_acc=o["n_acc"], rel_c=o["rel_c"], lazy=o["lazy"],
                                   groups=groups, budget=budget)
    shape = lambda t: t.view(B, H, Lq, d).permute(0, 2, 1, 3).reshape(B, Lq, H * d)          # noqa: E731
    return shape(out), shape(bound), dom.view(B, H, Lq)


def assert_within_bound(name, got, ref, bound, dom, plan, heads, d):
    """element-wise |got - ref| <= bound on [B, Lq, H d] outputs; returns the worst err / bound.  The failure names the element, its
    (batch, head, query), the query's dominant key with the tile and key group that walk it, and the instance."""
    err = (got.double() - ref).abs()
    ratio = torch.where(torch.isfinite(err), err / bound.clamp_min(1e-300), torch.full_like(err, math.inf))
    worst = float(ratio.max())
    if not worst <= 1.0:
        flat = int(ratio.argmax())
        b, rest = divmod(flat, ratio.shape[1] * ratio.shape[2])
        i, col = divmod(rest, ratio.shape[2])
        h, e = divmod(col, d)
        key = int(dom[b, h, i])
        tile, group = key_place(plan, key)
        raise AssertionError(
            f"{name}: element (batch {b}, query {i}, column {col}) = head {h}, dim {e}: got {float(got[b, i, col])!r}, reference "
            f"{float(ref[b, i, col])!r}, |err| {float(err[b, i, col]):.4g} > bound {float(bound[b, i, col]):.4g} (x{worst:.3g}); the query's "
            f"dominant key is {key} (tile {tile}, key group {group}); workgroup row {i % plan.queries_per_wg} of query tile "
            f"{i // plan.queries_per_wg}; {describe(plan)}; {int((ratio > 1).sum())} of {ratio.numel()} elements over their bound")
    return worst
