"""The GEMM case table: shapes, epilogues and optional features of ga_gemm_bf16 calls that together reach every kernel instance the
dispatcher can launch (tests/test_gemm_plan.py checks that on the CPU through ga_gemm_plan) and run every optional feature on every
tile family that accepts it; tests/test_gemm_instances_gpu.py runs each case on the GPU against a float64 reference.

A case is a dict: name, M, N, K, epi (GA_GEMM_EPI_*), and the optional features
  rpb        rows_per_batch (gate rows, per-batch bias / emit_scale rows, V^T items); 0 = M
  gate       EPI 2: one gate row per batch item
  bias       None, "row" (bias[N]) or "batch" (one row per batch item, bias_stride > N)
  row_ss     EPI 0 / 1: number of partial sums of the folded RMSNorm row scale (0 = none)
  qk         EPI 0: per-head RMSNorm of the column groups [0, qk0) and [qk0, qk1)
  vt         EPI 0: columns >= vt are stored transposed (0 = none)
  emit       EPI 2: None, "plain" or "mod" (the folded pre-norm's emit_x / emit_ss, modulated or not)
  k_rows     EPI 2: only the first k_rows rows of A take part in the product (0 = all)
  splitk     ga_gemm_splitk_mode for the call (0 = no split-K scratch)
"""
EPI_BF16, EPI_GELU, EPI_RES, EPI_F32 = 0, 1, 2, 3
FAKE_PTR = 1 << 20        # plan queries on the CPU: any non-NULL pointer with the alignment the arguments need (256 bytes)


def C(name, M, N, K, epi, rpb=0, gate=False, bias="row", row_ss=0, qk=(0, 0), vt=0, emit=None, k_rows=0, splitk=0):
    if epi == EPI_F32 and bias == "row":
        bias = None
    return dict(name=name, M=M, N=N, K=K, epi=epi, rpb=rpb or M, gate=gate, bias=bias, row_ss=row_ss, qk=qk, vt=vt, emit=emit,
                k_rows=k_rows, splitk=splitk)


def ss_ld(tiles):
    """floats per row of the partial sums of squares (include/ga_dit.h: the tile count rounded up to a multiple of 4)"""
    return (tiles + 3) & ~3


CASES = []
_E = {EPI_BF16: "bf16", EPI_GELU: "gelu", EPI_RES: "res", EPI_F32: "f32"}

# ---- the general kernel (K / 64 with no ring: 1 here), 128 columns x 32 MT rows.  Four slots for grids of <= 256 workgroups, two
# above that and whenever more than 16 row partial sums are folded in (EPI 0 / 1).  MT follows the cost rule; M = tile * k +- 1 and
# N = 4 (mod 64) make every edge tile ragged.  The two-slot MT 1 .. 3 grids of EPI 2 / 3 need a grid of > 256 tile columns.
for e in (EPI_BF16, EPI_GELU, EPI_RES, EPI_F32):
    res = e == EPI_RES
    CASES += [C(f"general4_mt1_{_E[e]}", 31, 132, 64, e, gate=res, rpb=10 if res else 0),
              C(f"general4_mt2_{_E[e]}", 4097, 132, 64, e, gate=res, rpb=100 if res else 0),
              C(f"general4_mt3_{_E[e]}", 5567, 260, 64, e, gate=res, rpb=1000 if res else 0),
              C(f"general4_mt4_{_E[e]}", 6145, 388, 64, e, gate=res, rpb=1001 if res else 0)]
    if e in (EPI_BF16, EPI_GELU):
        CASES += [C(f"general2_mt1_{_E[e]}", 31, 132, 64, e, row_ss=17),
                  C(f"general2_mt2_{_E[e]}", 4097, 132, 64, e, row_ss=18),
                  C(f"general2_mt3_{_E[e]}", 5567, 260, 64, e, row_ss=19),
                  C(f"general2_mt4_{_E[e]}", 6145, 388, 64, e, row_ss=20)]
    else:
        CASES += [C(f"general2_mt1_{_E[e]}", 31, 32772, 64, e, gate=res, rpb=7 if res else 0),
                  C(f"general2_mt2_{_E[e]}", 33, 32772, 64, e, gate=res, rpb=16 if res else 0),
                  C(f"general2_mt3_{_E[e]}", 65, 32772, 64, e),
                  C(f"general2_mt4_{_E[e]}", 6145, 900, 64, e, gate=res, rpb=700 if res else 0)]

# ---- the ring kernels: four tiles x (four slots: K / 64 = 8 | four slots + two remainder tiles: 10 | three slots: 6), the smallest
# legal K of each ring.  Three-slot and remainder instances read up to 20 row partial sums.
_RING_SHAPES = {"192x128": (577, 4484), "96x128": (5183, 260), "96x64": (97, 5060), "64x64": (6143, 4)}
for k, ring in ((512, "ring4"), (640, "ring4r2"), (384, "ring3")):
    for tile, (M, N) in _RING_SHAPES.items():
        if tile == "192x128" and k == 512:
            M, N = 1, 32772          # (a 192 x 128 grid of 144+ workgroups at the K of the four-slot ring: the smallest is one row)
        for e in (EPI_BF16, EPI_GELU, EPI_RES, EPI_F32):
            if e == EPI_F32 and (k != 512 or tile == "96x128"):
                continue             # no fp32-store instance for K / 64 % 4 != 0; the 96 x 128 tile is never picked for it
            wide = k != 512 and e in (EPI_BF16, EPI_GELU)
            CASES.append(C(f"{ring}_{tile}_{_E[e]}", M, N, k, e, gate=e == EPI_RES, rpb=max(M // 3, 1) if e == EPI_RES else 0,
                           row_ss=(18 if wide else 8) if e in (EPI_BF16, EPI_GELU) and tile != "64x64" else 0))

# ---- split-K (ga_gemm_splitk_mode 1 ... 4): 192 x 128 x 4 | 96 x 128 x 2 | 96 x 128 x 4 | 192 x 128 x 2 (EPI 0 / 1 / 2)
CASES += [C("splitk1_192x128x4_res", 193, 132, 2048, EPI_RES, gate=True, rpb=144, bias="batch", splitk=1),
          C("splitk2_96x128x2_res", 97, 260, 1024, EPI_RES, gate=True, rpb=48, splitk=2),
          C("splitk3_96x128x4_res", 97, 132, 2048, EPI_RES, splitk=3),
          C("splitk4_192x128x2_bf16", 193, 384, 1024, EPI_BF16, rpb=144, bias="batch", row_ss=16, qk=(64, 128), vt=256, splitk=4),
          C("splitk4_192x128x2_gelu", 193, 132, 1024, EPI_GELU, rpb=144, bias="batch", row_ss=16, splitk=4),
          C("splitk4_192x128x2_res", 193, 256, 1024, EPI_RES, gate=True, rpb=144, emit="mod", splitk=4),
          C("splitk4_192x128x2_res_emit", 193, 256, 1024, EPI_RES, gate=True, rpb=48, emit="plain", splitk=4),
          C("splitk2_96x128x2_res_emit", 97, 256, 1024, EPI_RES, rpb=48, emit="mod", bias="batch", splitk=2),
          C("splitk3_96x128x4_res_emit", 97, 256, 2048, EPI_RES, gate=True, rpb=50, emit="plain", splitk=3),
          # more than 16 row partial sums at a K the split can take: the unsplit kernel serves it (the split instance reads 16)
          C("splitk4_wide_row_ss_gelu", 193, 256, 1024, EPI_GELU, row_ss=18, splitk=4)]

# ---- every optional feature on every tile family that accepts it (N % 64 == 0 where the feature needs it).  Per-batch operands on
# the ring tiles need one batch item per wave (rows_per_batch % 48, % 16 on 64 x 64): 144 / 80 rows, which split output tiles;
# k_rows off every tile boundary.
_FEATURE_SHAPES = {"general": (300, 256, 192), "192x128": (769, 4608, 512), "96x128": (2000, 1024, 512), "96x64": (1000, 1024, 512),
                   "64x64": (1000, 512, 512)}
# (q | k | v of D = N / 3 columns each: the per-head norm of q and of k, V^T behind them)
_QKV_SHAPES = {"general": (300, 384, 192), "192x128": (1000, 3456, 512), "96x128": (2600, 768, 512), "96x64": (1000, 1536, 512),
               "64x64": (1000, 384, 512)}
for tile, (M, N, K) in _FEATURE_SHAPES.items():
    rpb = 80 if tile == "64x64" else 144
    Mq, Nq, Kq = _QKV_SHAPES[tile]
    CASES += [C(f"feat_{tile}_qkv", Mq, Nq, Kq, EPI_BF16, rpb=rpb, bias="batch", row_ss=Kq // 64, qk=(Nq // 3, 2 * Nq // 3), vt=2 * Nq // 3),
              C(f"feat_{tile}_fc1", M, N, K, EPI_GELU, rpb=rpb, bias="batch", row_ss=K // 64),
              C(f"feat_{tile}_proj", M, N, K, EPI_RES, gate=True, rpb=rpb, emit="mod"),
              C(f"feat_{tile}_fc2", M, N, K, EPI_RES, gate=True, rpb=100, emit="plain", k_rows=M // 2 + 23),
              C(f"feat_{tile}_ca_out", M, N, K, EPI_RES, rpb=rpb, bias="batch", emit="mod", k_rows=M // 2 + 11),
              C(f"feat_{tile}_f32", M, N, K, EPI_F32, rpb=rpb, bias="batch")]
# more than 16 partial sums on the three-slot / remainder rings (K = 1152: 18 tiles) and the two-slot general kernel
CASES += [C("feat_192x128_wide_row_ss", 769, 4608, 1152, EPI_GELU, rpb=144, bias="batch", row_ss=18),
          C("feat_96x128_wide_row_ss", 1500, 1536, 1152, EPI_BF16, rpb=144, bias="batch", row_ss=18, qk=(512, 1024), vt=1024),
          C("feat_96x64_wide_row_ss", 1000, 1152, 1152, EPI_BF16, rpb=144, row_ss=20, qk=(64, 128)),
          C("feat_64x64_wide_row_ss", 1000, 512, 576, EPI_GELU, rpb=80, bias="batch", row_ss=17),
          C("feat_general_wide_row_ss", 300, 768, 512, EPI_BF16, rpb=100, bias="batch", row_ss=20, qk=(128, 256), vt=512)]

# ---- the shapes the released models run (768 tokens per item; batch 1, the CFG pair, CFG batch 4): DiT-B (768 wide, heads of 64),
# DiT-L (1024), XL (1152, heads of 72: no per-head norm in the GEMM); the folded modulated pre-norms of ga_dit_forward
for arch, D in (("B", 768), ("L", 1024), ("XL", 1152)):
    for B in (1, 2, 4):
        M = 768 * B
        qk = (D, 2 * D) if arch != "XL" else (0, 0)
        CASES += [C(f"{arch}_b{B}_qkv", M, 3 * D, D, EPI_BF16, rpb=768, bias="batch", row_ss=D // 64, qk=qk, vt=2 * D),
                  C(f"{arch}_b{B}_proj", M, D, D, EPI_RES, gate=True, rpb=768, emit="mod"),
                  C(f"{arch}_b{B}_fc1", M, 4 * D, D, EPI_GELU, rpb=768, bias="batch", row_ss=D // 64),
                  C(f"{arch}_b{B}_fc2", M, D, 4 * D, EPI_RES, gate=True, rpb=768, emit="plain")]
CASES += [C("L_b2_ca_out", 1536, 1024, 1024, EPI_RES, rpb=768, emit="mod", k_rows=768),
          C("XL_b2_ca_out", 1536, 1152, 1152, EPI_RES, rpb=768, emit="mod", k_rows=768)]

assert len({c["name"] for c in CASES}) == len(CASES)


def make_args(case, ptr=None, strides=None):
    """GaGemmArgs of a case.  ptr(name) -> device pointer of the named operand (None: FAKE_PTR everywhere, for plan queries);
    strides: lda / ldo / gate_stride / bias_stride / emit_ld / emit_scale_stride / vt_ld overrides (elements)."""
    from gaussiananything_amd import dit_ops as ops
    c = case
    P = ptr or (lambda name: FAKE_PTR)
    s = dict(lda=c["K"], ldo=c["vt"] or c["N"], gate_stride=c["N"], bias_stride=c["N"] + 4, emit_ld=c["N"], emit_scale_stride=c["N"],
             vt_ld=(c["rpb"] + 63) // 64 * 64)
    s.update(strides or {})
    a = ops.GaGemmArgs()
    a.M, a.N, a.K, a.epilogue = c["M"], c["N"], c["K"], c["epi"]
    a.A, a.lda, a.W, a.out, a.ldo = P("A"), s["lda"], P("W"), P("out"), s["ldo"]
    a.rows_per_batch = c["rpb"]
    if c["bias"]:
        a.bias = P("bias")
        if c["bias"] == "batch":
            a.bias_stride = s["bias_stride"]
    if c["gate"]:
        a.gate, a.gate_stride = P("gate"), s["gate_stride"]
    if c["vt"]:
        a.vt, a.vt_col0, a.vt_ld = P("vt"), c["vt"], s["vt_ld"]
    if c["qk"][1]:
        a.qk_cols0, a.qk_cols1 = c["qk"]
        a.qk_w0 = P("qk_w0") if c["qk"][0] else None
        a.qk_w1 = P("qk_w1") if c["qk"][1] > c["qk"][0] else None
    if c["row_ss"]:
        a.row_ss, a.row_ss_tiles, a.row_ss_dim, a.row_ss_eps = P("row_ss"), c["row_ss"], 64 * c["row_ss"], 1e-5
    if c["emit"]:
        a.emit_x, a.emit_ss, a.emit_ld = P("emit_x"), P("emit_ss"), s["emit_ld"]
        if c["emit"] == "mod":
            a.emit_w, a.emit_scale, a.emit_scale_stride = P("emit_w"), P("emit_scale"), s["emit_scale_stride"]
    a.k_rows = c["k_rows"]
    if c["splitk"]:
        a.splitk_ws, a.splitk_ws_bytes = P("splitk_ws"), int(ops.lib().ga_gemm_splitk_workspace_bytes(c["M"], c["N"]))
    return a


def plan_of(case, ptr=None, strides=None):
    """(GaGemmPlan, its cell key) of a case under its split-K mode"""
    from gaussiananything_amd import dit_ops as ops
    prev = ops.splitk_mode(case["splitk"] or -1)
    try:
        p = ops.gemm_plan(make_args(case, ptr, strides))
    finally:
        ops.splitk_mode(prev)
    return p, cell(p)


def cell(p):
    return (p.family, p.epilogue, p.tile_m, p.tile_n, p.waves, p.slots, p.rem, p.mt, p.splits)


def tile_family(p):
    from gaussiananything_amd import dit_ops as ops
    if p.family == ops.GEMM_FAMILY_GENERAL:
        return "general"
    return ("splitk_" if p.family == ops.GEMM_FAMILY_SPLITK else "") + f"{p.tile_m}x{p.tile_n}"


def describe(p):
    fam = {0: "general", 1: "ring", 2: "splitk"}[p.family]
    return (f"{fam} {p.tile_m}x{p.tile_n} epi{p.epilogue} waves={p.waves} slots={p.slots} rem={p.rem} mt={p.mt} splits={p.splits} "
            f"grid={p.grid_x}x{p.grid_y}x{p.grid_z} xmap={p.xmap} wt={p.wt}")
