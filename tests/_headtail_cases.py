"""Cases, inputs and float64 references of the kernels of csrc/dit_ops.hip that run only inside ga_dit_forward, ga_dit_cache_context_ws,
ga_dit_pooled_vector and ga_dit_sampler_advance: embed_tokens, final_layer (plain, velocity, fused Euler step, CFG twins),
layernorm_rows, ctx_rmsnorm, sampler_advance and the ModOut store of small_linear.  tests/test_headtail_instances_gpu.py runs every
case on the GPU, tests/test_headtail_bounds_cpu.py proves on the CPU that seeded kernel bugs land over the bounds.  Same shape as
tests/_row_cases.py: CASES, inputs(case), reference(case, z) -> {output: (ref, bound)}; reference ASSERTS that a case reaches the
branch it names.

THE PASS-THROUGH MODEL.  ga_dit_forward is embedding -> blocks -> final layer.  With adaLN_modulation, the blocks' scale_shift_table
and the cross-attention output projection zero, every block is the exact identity on the residual stream (zero gates, a zero
product); t_embedder.mlp[2].weight = 0 makes tvec[b] = fl(t_mlp2_b + pooled_vec[b]) known exactly, and x_embedder.fc2.weight = I
(exact in bf16) with a planted bias makes the stream that reaches the final layer fl(xres_pe + fl(h + b)) per element, nothing mixed
across columns.  The GPU test asserts the premise once per width (re-randomised block weights, bit-identical output).

  embed   the [M, Cout <= 16] output shows 16 columns of the stream per forward: final_w is swept over one-hot rows (final_b planted),
          so every column of every token is seen through LayerNorm + modulate + ONE bf16 rounding, which the reference MIRRORS
          (tests/_bounds.py: rounded_operand) -- an element is exact or one bf16 ulp off where its fp32 value lies on a rounding
          boundary.  h, the PE features and the in-kernel weight roundings are mirrored the same way.
  final   the embedding is switched to exact arithmetic: fc1 = 0 (h = gelu(0) = 0), xyz_embed rows one-hot over the three RAW
          coordinates (bf16-exact xyz, one exact product), so x[m][n] = fl(xyz[m][n % 3] w[n] + b[n]) is known to the bit and the bound
          is that of the final layer alone.  The weight rows are sparse: non-zeros in the first and last float4 and on both sides of
          every 256-column chunk boundary; the statistics involve every column.
  step    the same rows through GaDitSamplerStep: u + s (c - u) and y + dt v, one rounding per operation.
  gates   depth 3, adaLN_modulation with one non-zero weight per output row and a bias, block tables that differ per block, zero proj /
          fc2 weights with planted biases: the stream gains gate_msa[blk][b] bias_proj + gate_mlp[blk][b] bias_fc2 per block, which the
          one-hot final layer shows -- the (blk B + b) 6 D + n indexing and the table + y sum of ModOut for rows 2 and 5.  Rows 0, 1, 3
          and 4 of the modulation tables stay covered only by the folded-pre-norm tests (tests/test_dit_gpu.py): here they feed
          products with zero weights.

tanhf: the `big` embed family drives the argument of tanhf far beyond the grid behind TANHF_REL ([-32, 32]); tanh is 1 to less than an
ulp there, so the constant is applied as it stands (a tanhf that is not +-1 to 3 ulp on saturated arguments would show)."""
import math
import zlib

import torch

from tests import _bounds as bd
from tests._row_cases import F64, bf16, f32, worst_ratio  # noqa: F401  (worst_ratio: re-exported for the two test files)

EPS5 = bd.EPS_F32
EPS6 = bd.F32(1e-6)
CTX_TOKENS, CONTEXT_DIM = 8, 64
TRAJ_FILL = -777.0                                      # what the slices of a trajectory hold before the step (exact in fp32)
PE_EXTRA = (0, 2, 3, 5, 6, 8, 57, 62)


def _gen(case):
    return torch.Generator().manual_seed(zlib.crc32(case["name"].encode()))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F64)


def _rand(g, *shape):
    return torch.rand(*shape, generator=g, dtype=F64)


def _sign(g, *shape):
    return 1.0 - 2.0 * (torch.rand(*shape, generator=g, dtype=F64) < 0.5).to(F64)


def _case(kernel, family, **kw):
    name = kernel + "_" + "_".join(f"{k}{v}" for k, v in kw.items()) + "_" + family
    return dict(kw, kernel=kernel, family=family, name=name)


# =================================================================================================== the forward cases
def _embed_cases():
    rows = [(1, 64, 1, 1, 1, "plain", "none"), (1, 192, 1, 8, 3, "plain", "none"), (1, 320, 1, 13, 16, "plain", "none"),
            (1, 192, 3, 5, 16, "modulation", "none"), (1, 320, 3, 5, 10, "big", "none"), (1, 64, 1, 13, 10, "big", "none"),
            (2, 64, 1, 8, 3, "plain", "onehot"), (2, 192, 1, 13, 16, "plain", "onehot"), (2, 320, 3, 5, 10, "modulation", "onehot"),
            (2, 320, 1, 1, 1, "plain", "onehot"), (2, 192, 3, 5, 16, "plain", "dense"), (2, 320, 1, 13, 3, "big", "onehot")]
    out = [_case("embed", fam, stage=s, D=D, B=B, L=L, C=C, pe=pe) for s, D, B, L, C, fam, pe in rows]
    for axis, want in (("D", {64, 192, 320}), ("C", {1, 3, 10, 16}), ("stage", {1, 2})):
        assert {c[axis] for c in out} == want
    assert {c["B"] * c["L"] for c in out} == {1, 8, 13, 15} and all(c["B"] * c["L"] % 8 for c in out if c["C"] == 16)
    return out


FINAL_SHAPES = ((64, 3), (320, 10), (960, 16), (1024, 16), (2048, 3), (2048, 10))
LDS_LIMIT = 60 * 1024


def final_weight_in_lds(c):
    return c["Cout"] * c["D"] * 4 <= LDS_LIMIT


def _final_cases():
    assert 16 * 960 * 4 == LDS_LIMIT and 16 * 1024 * 4 > LDS_LIMIT and 3 * 2048 * 4 <= LDS_LIMIT < 10 * 2048 * 4
    fams = ("plain", "offset", "low", "big", "modulation")
    rows = [(64, 3, 1, 1, "plain"), (64, 3, 1, 5, "offset"), (320, 10, 3, 5, "low"), (320, 10, 1, 1, "big"), (960, 16, 3, 5, "modulation"),
            (960, 16, 1, 5, "plain"), (2048, 3, 3, 5, "offset"), (2048, 3, 1, 1, "low"), (2048, 3, 1, 5, "big"),
            (1024, 16, 3, 5, "plain"), (1024, 16, 1, 1, "offset"), (1024, 16, 3, 5, "modulation"), (2048, 10, 1, 5, "low"),
            (2048, 10, 1, 1, "big"), (2048, 10, 3, 5, "modulation")]
    out = [_case("final", fam, D=D, Cout=Cout, B=B, L=L, text=0) for D, Cout, B, L, fam in rows]
    for D, Cout, B, L, fam in ((64, 3, 3, 5, "modulation"), (320, 10, 1, 5, "offset")):
        out.append(_case("final", fam, D=D, Cout=Cout, B=B, L=L, text=1))
    assert {(c["D"], c["Cout"]) for c in out} == set(FINAL_SHAPES) and {c["B"] * c["L"] for c in out} == {1, 5, 15}
    for lds in (True, False):                                            # every family on both sides of the LDS limit
        assert {c["family"] for c in out if final_weight_in_lds(c) == lds and not c["text"]} == set(fams)
    return out


def _step_cases():
    rows = [("velocity", 0, 320, 10, 3, 5, 1.0, None), ("velocity", 1, 64, 3, 2, 3, 4.0, None), ("velocity", 1, 1024, 16, 4, 5, 1.0, None),
            ("euler", 0, 64, 3, 1, 5, 1.0, 0.125), ("euler", 1, 320, 10, 2, 3, 4.0, -0.0625), ("euler", 1, 64, 3, 4, 5, 4.0, 0.03),
            ("euler_notraj", 0, 1024, 16, 3, 5, 1.0, 0.3), ("euler_notraj", 1, 320, 10, 4, 5, 1.0, 0.01)]
    out = [_case("step", "modulation", mode=m, cfg=cfg, D=D, Cout=C, B=B, L=L, s=s, dt=dt) for m, cfg, D, C, B, L, s, dt in rows]
    assert {c["s"] for c in out if c["cfg"]} == {1.0, 4.0} and any(c["dt"] is not None and c["dt"] < 0 for c in out)
    return out


def _gates_cases():
    return [_case("gates", "plain", D=D, B=3, L=5, depth=3) for D in (64, 320)]


def forward_shape(c):
    """(stage2, depth, C, text) of the model a forward case runs"""
    k = c["kernel"]
    if k == "embed":
        return c["stage"] == 2, 1, c["C"], 0
    if k == "gates":
        return False, c["depth"], 3, 0
    return True, 1, c["Cout"], c.get("text", 0)


def _pe_selection(D):
    """the feature every row of the one-hot xyz_embed weight selects: n % 63, and PE_EXTRA on the rows behind the first 63"""
    sel = torch.arange(D) % 63
    n = min(len(PE_EXTRA), max(D - 63, 0))
    sel[63:63 + n] = torch.tensor(PE_EXTRA[:n])
    return sel


def _forward_inputs(c, g):
    k, fam, D, B, L = c["kernel"], c["family"], c["D"], c["B"], c["L"]
    stage2, depth, C, text = forward_shape(c)
    M = B * L
    z = dict(tb2=f32(0.3 * _randn(g, D)), timesteps=f32(0.3 + 0.1 * torch.arange(B, dtype=F64)))
    pooled = 0.5 * _randn(g, B, D)
    if fam == "modulation":
        pooled = pooled + 2.0 * (1 - 2 * (torch.arange(B, dtype=F64) % 2)).view(B, 1)
    z["pooled"] = f32(pooled)
    if text:
        z["fmod_w"], z["fmod_b"] = bf16(_randn(g, 2 * D, D) / math.sqrt(D)), f32(0.5 * _randn(g, 2 * D))
    else:
        z["table"] = f32(0.5 * _randn(g, 2, D))
    if k in ("embed", "gates"):
        x = _randn(g, M, C) * (1e2 if fam == "big" else 1.0)
        z["x"] = f32(x)
        z["w1"], z["b1"] = f32(_randn(g, D, C) / math.sqrt(C)), f32(0.5 * _randn(g, D))
        z["b2"] = f32(0.5 * _randn(g, D))
        z["final_b"] = f32(_randn(g, 16))
        if stage2:
            xyz = 2 * _rand(g, M, 3) - 1
            xyz.view(-1)[:3] = torch.tensor([0.0, 1.0, -1.0], dtype=F64)
            z["xyz"] = f32(xyz)
            if c["pe"] == "onehot":
                wx = torch.zeros(D, 63, dtype=F64)
                wx[torch.arange(D), _pe_selection(D)] = (0.5 + _rand(g, D)) * _sign(g, D)
            else:
                wx = _randn(g, D, 63) / math.sqrt(63.0)
            z["wx"], z["bx"] = f32(wx), f32(0.5 * _randn(g, D))
    else:
        # the exact stream: x[m][n] = fl(xyz[m][n % 3] w[n] + b2[n]) (fc1 = 0, bx = 0, one non-zero weight per xyz_embed row)
        sigma = {"low": 1e-3, "big": 1e4}.get(fam, 1.0)
        w = sigma * (0.5 + _rand(g, D)) * _sign(g, D)
        b2 = 0.5 * sigma * _randn(g, D)
        if fam in ("plain", "big"):                                      # half of a row's energy in its last float4
            w[-4:] = 1.2 * sigma * math.sqrt(D / 2.0) * _sign(g, 4)
        if fam == "offset":
            b2 = b2 + 2000.0 * math.sqrt(1.25)                            # 2000 x the spread (sqrt(E a^2 w^2 + 0.25) ~ 1.1)
        wx = torch.zeros(D, 63, dtype=F64)
        wx[torch.arange(D), torch.arange(D) % 3] = bf16(w)
        xyz = bf16((0.5 + _rand(g, M, 3)) * _sign(g, M, 3))               # |xyz| in [0.5, 1.5]: every row has a spread of the family's size
        z["xyz"], z["wx"], z["bx"], z["b2"] = xyz, wx, torch.zeros(D, dtype=F64), f32(b2)
        z["w1"], z["b1"] = torch.zeros(D, C, dtype=F64), torch.zeros(D, dtype=F64)
        z["x"] = f32(_randn(g, M, C))                                     # fc1 = 0: free to be the sampler state
        fw = torch.zeros(c["Cout"], D, dtype=F64)
        cols = sorted(set(range(4)) | set(range(D - 4, D)) | {e for q in range(256, D, 256) for e in (q - 1, q)})
        fw[:, cols] = _randn(g, c["Cout"], len(cols))
        z["final_w"], z["final_b"] = f32(fw), f32(_randn(g, c["Cout"]))
    if k == "step":
        half = B // 2
        if c["cfg"]:                                                      # both CFG halves hold the same state
            z["x"] = torch.cat([z["x"][:half * L], z["x"][:half * L]])
        if c["dt"] is not None:
            z["dt"] = f32(torch.tensor([c["dt"]], dtype=F64))
            z["counter"], z["slices"] = 2, 5
    if k == "gates":
        wa = torch.zeros(6 * D, D, dtype=F64)
        wa[torch.arange(6 * D), torch.randint(0, D, (6 * D,), generator=g)] = (0.5 + _rand(g, 6 * D)) * _sign(g, 6 * D)
        z["adaln_w"], z["adaln_b"] = bf16(wa), f32(0.5 * _randn(g, 6 * D))
        z["tables"] = f32(0.5 * _randn(g, depth, 6, D) + torch.arange(depth, dtype=F64).view(depth, 1, 1))
        z["proj_b"], z["fc2_b"] = f32(_randn(g, depth, D)), f32(_randn(g, depth, D))
    return z


def sweep_weight(D, s):
    """final_w of sweep s of an embed / gates case: output channel c shows column 16 s + c"""
    w = torch.zeros(16, D, dtype=F64)
    w[torch.arange(16), 16 * s + torch.arange(16)] = 1.0
    return w


def pe_features(xyz):
    """(ref, err) [M, 63] of [x, sin(2^k x), cos(2^k x)]_{k = 0..9}, index 3 + 6 k + {0..2 sin, 3..5 cos}: 2^k x is exact in fp32, so
    the only error is sinf's / cosf's own (SINF_REL, COSF_REL of tests/_bounds.py, measured on [0, 1024]; sin is odd and cos even, and
    |2^k x| <= 512 here).  The bf16 rounding that follows is 2^16 times coarser: the figure matters only on a rounding boundary."""
    M = xyz.shape[0]
    ref, err = torch.zeros(M, 63, dtype=F64), torch.zeros(M, 63, dtype=F64)
    ref[:, :3] = xyz
    for k in range(10):
        arg = xyz * float(1 << k)
        assert float(arg.abs().max()) <= 1024.0
        c, Pc, s, Ps = bd.sin_cos(arg, torch.zeros_like(arg))
        ref[:, 3 + 6 * k:6 + 6 * k], err[:, 3 + 6 * k:6 + 6 * k] = s, Ps
        ref[:, 6 + 6 * k:9 + 6 * k], err[:, 6 + 6 * k:9 + 6 * k] = c, Pc
    return ref, err


def tvec(z):
    """tvec[b] = fl(t_mlp2_b + pooled_vec[b]): the product with the zero weight is an exact zero"""
    return f32(z["tb2"] + z["pooled"])


def stream_reference(c, z):
    """(x, Px): the residual stream behind the token embedding, embed_tokens_kernel + the fc2 GEMM with the identity weight"""
    stage2, _, C, _ = forward_shape(c)
    xs, w1 = bd.bf16_round(z["x"]), bd.bf16_round(z["w1"])               # (autocast: both rounded in the kernel, exactly mirrored)
    acc, P = bd.sparse_dot(xs, torch.zeros_like(xs), w1, z["b1"])
    g, Pg = bd.gelu_tanh(acc, P)
    h, dh = bd.rounded_operand(g, Pg)
    v, Pv = bd.fl_add_sparse(h, dh, z["b2"])                              # the GEMM's epilogue: fl(acc + bias), acc = h exactly
    if not stage2:
        return v, Pv                                                     # xres starts at an exact zero
    fr, fe = pe_features(z["xyz"])
    spe, ds = bd.rounded_operand(fr, fe)
    r, Pr = bd.sparse_dot(spe, ds, bd.bf16_round(z["wx"]), z["bx"])
    return bd.fl_add_sparse(r, Pr, v, Pv)


def exact_stream(c, z):
    """the final / step cases: the stream known to the bit (asserted: every operation but the last is exact)"""
    x, Px = stream_reference(c, z)
    assert bool((z["w1"] == 0).all()) and bool((z["bx"] == 0).all()) and bool(((z["wx"] != 0).sum(-1) == 1).all())
    M, D = x.shape
    prod = z["xyz"][:, torch.arange(D) % 3] * z["wx"][torch.arange(D), torch.arange(D) % 3]
    assert bool((f32(prod) == prod).all()), "the one product of a column must be exact in fp32"
    s = prod + z["b2"]
    assert bool(((s - prod) == z["b2"]).all()) and bool(((s - z["b2"]) == prod).all()), "the float64 sum must be exact: one rounding to fp32"
    xe = f32(s)
    assert bool(((xe - x).abs() <= Px).all())
    return xe, torch.zeros_like(xe)


def gates_reference(c, z, x, Px):
    """the stream behind `depth` blocks whose proj / fc2 products are zero: x = fl(x + fl(gate bias)) twice per block, gate =
    fl(table[blk][row] + t0[b][row]), t0 = fl(bf16(silu(tvec)) W + bias) with one non-zero W per row"""
    D, B, L, depth = c["D"], c["B"], c["L"], c["depth"]
    sh, ds = bd.rounded_operand(*bd.silu(tvec(z), torch.zeros(B, D, dtype=F64)))
    t0, P0 = bd.sparse_dot(sh, ds, z["adaln_w"], z["adaln_b"])
    b = torch.arange(B * L) // L
    for blk in range(depth):
        for row, bias in ((2, z["proj_b"][blk]), (5, z["fc2_b"][blk])):
            gate, Pgate = bd.fl_add(z["tables"][blk, row], 0.0, t0[:, row * D:(row + 1) * D], P0[:, row * D:(row + 1) * D])
            gate, Pgate = gate[b], Pgate[b]
            xn = x + gate * bias
            Px = Px + Pgate * bias.abs() + bd.gamma(2) * (x.abs() + Px + (gate.abs() + Pgate) * bias.abs())
            x = xn
    return x, Px


def final_rows(c, z, x, Px):
    """(yh, dy): the bf16 operand of the final Linear, mirrored: bf16(fl(fl(fl(e rs) fl(1 + scale)) + shift))"""
    D, B, L = c["D"], c["B"], c["L"]
    t = tvec(z)
    if "fmod_w" in z:
        sh_, ds = bd.rounded_operand(*bd.silu(t, torch.zeros_like(t)))
        v, E = sh_ @ z["fmod_w"].T, ds @ z["fmod_w"].abs().T
        P = E + bd.accumulation(sh_.abs() @ z["fmod_w"].abs().T + E, D)
        v, P = bd.fl_add(v, P, z["fmod_b"])
        shift, Psh, scale, Psc = v[:, :D], P[:, :D], v[:, D:], P[:, D:]
    else:
        shift, scale = f32(z["table"][0] + t), f32(z["table"][1] + t)     # one rounding of exactly known operands: known to the bit
        Psh = Psc = torch.zeros_like(shift)
    b = torch.arange(B * L) // L
    e, De, r, rho = bd.pivoted_layernorm_stats(x, Px, EPS6)
    y, P = bd.fl_mul(e, De, r, r * rho)
    s1, Ps1 = bd.fl_add(scale[b], Psc[b], 1.0)
    y, P = bd.fl_mul(y, P, s1, Ps1)
    y, P = bd.fl_add(y, P, shift[b], Psh[b])
    return bd.rounded_operand(y, P)


def final_linear(yh, dy, w, bias):
    v, P = bd.sparse_dot(yh, dy, bd.bf16_round(w))
    return bd.fl_add(v, P, bias)


def _row_variance(x):
    return (x - x.mean(-1, keepdim=True)).pow(2).mean(-1)


def _forward_reference(c, z):
    k, fam, D, B, L = c["kernel"], c["family"], c["D"], c["B"], c["L"]
    M = B * L
    if k in ("embed", "gates"):
        x, Px = stream_reference(c, z)
        if k == "gates":
            x0 = x
            x, Px = gates_reference(c, z, x, Px)
            assert float((x - x0).abs().mean()) > 0.5, "the gated biases must move the stream by O(1)"
            t = z["tables"]
            assert float((t[1:] - t[:-1]).abs().min()) > 0 and bool((z["adaln_w"] != 0).sum(-1).eq(1).all())
        if fam == "big":
            assert float(z["x"].abs().max()) > 100 and bool((x > 50).any())
        if k == "embed" and c["pe"] == "onehot":
            assert set(PE_EXTRA[:max(0, min(8, D - 63))]) <= set(_pe_selection(D).tolist()) and float((z["xyz"].abs() * 512).max()) == 512.0
        yh, dy = final_rows(c, z, x, Px)
        ref = yh + z["final_b"][torch.arange(D) % 16]                     # sweep s, channel c shows column 16 s + c: fl(yh + bias[c])
        return {"y": (ref, dy + bd.U * (ref.abs() + dy))}
    x, Px = exact_stream(c, z)
    var, spread = _row_variance(x), _row_variance(x).sqrt()
    if fam == "low":
        assert bool(((var >= 0.1 * EPS6) & (var <= 10 * EPS6)).all()), (c["name"], "variance outside [0.1 eps, 10 eps]")
    if fam == "offset":
        ratio = x.mean(-1).abs() / spread
        assert bool(((ratio > 1000) & (ratio < 4000)).all()), (c["name"], "the common offset must be ~2000 x the spread")
    if fam == "big":
        assert float(x.abs().max()) > 1e4
    if fam in ("plain", "big"):
        tail = x[:, -4:].pow(2).sum(-1) / x.pow(2).sum(-1)
        assert bool((tail > 0.25).all()), (c["name"], "the last float4 must carry a large share of the row's energy")
    if fam == "modulation" and B > 1:
        assert float((z["pooled"][1:] - z["pooled"][:-1]).abs().mean()) > 2.0
    assert bool((z["final_w"][:, -4:] != 0).all()) and bool((z["final_w"][:, :4] != 0).all())
    yh, dy = final_rows(c, z, x, Px)
    out, P = final_linear(yh, dy, z["final_w"], z["final_b"])
    if k == "final":
        return {"out": (out, P)}
    # ---- the sampler step
    half = M // 2 if c["cfg"] else M
    if c["cfg"]:
        assert B % 2 == 0 and bool((z["x"][:half] == z["x"][half:]).all())
        assert float((z["pooled"][:B // 2] - z["pooled"][B // 2:]).abs().min()) > 0 and float((x[:half] - x[half:]).abs().mean()) > 0.1
        cnd, Pc, unc, Pu = out[:half], P[:half], out[half:], P[half:]
        d, Pd = bd.fl_add(cnd, Pc, -unc, Pu)
        m, Pm = bd.fl_mul(d, Pd, bd.F32(c["s"]))
        v, Pv = bd.fl_add(unc, Pu, m, Pm)
        v, Pv = torch.cat([v, v]), torch.cat([Pv, Pv])
    else:
        v, Pv = out, P
    if c["mode"] == "velocity":
        return {"velocity": (v, Pv)}
    p, Pp = bd.fl_mul(v, Pv, z["dt"])
    y, Py = bd.fl_add(z["x"], 0.0, p, Pp)
    res = {"state": (y, Py)}
    if c["mode"] == "euler":
        traj = torch.full((z["slices"], M * c["Cout"]), TRAJ_FILL, dtype=F64)
        Pt = torch.zeros_like(traj)
        traj[z["counter"] + 1], Pt[z["counter"] + 1] = y.reshape(-1), Py.reshape(-1)
        res["traj"] = (traj, Pt)
    return res


# =================================================================================================== pooled
def _pooled_cases():
    fams = ("plain", "offset", "low")
    out, i = [], 0
    for batch in (1, 3, 16):
        for ctx in (64, 192, 1024):
            out.append(_case("pooled", fams[(i + i // 3) % 3], batch=batch, ctx=ctx, D=(64, 192)[i % 2]))
            i += 1
    return out


def _pooled_inputs(c, g):
    B, K, D, fam = c["batch"], c["ctx"], c["D"], c["family"]
    x = _randn(g, B, K)
    if fam == "low":
        k = 10 ** (1.4 * _rand(g, B, 1) - 0.7)
        x = (x - x.mean(-1, keepdim=True)) / _row_variance(x).sqrt().view(B, 1) * (k * 1e-5).sqrt() + 0.01 * _randn(g, B, 1)
    elif fam == "offset":
        # the ratio of the final layer's offset family; at 1024 columns 100 x, the ratio of tests/_row_cases.py: the mean of a two-pass
        # kernel may carry gamma(D) |offset|, which at 2000 x and 1024 columns is a tenth of the spread -- a bound that sees little
        x = x + (2000.0 if K <= 192 else 100.0) * _sign(g, B, 1)
    else:
        x[:, -4:] *= max(1.0, math.sqrt(K / 4.0))
    return dict(x=f32(x), ln_w=f32(1 + 0.3 * _randn(g, K)), ln_b=f32(0.5 * _randn(g, K)), W=bf16(_randn(g, D, K) / math.sqrt(K)),
                b=f32(_randn(g, D)))


def _pooled_reference(c, z):
    """scratch = fl(fl(fl(e rs) w) + b) by the two-pass statistics of layernorm_rows_kernel; out = small_linear(scratch) (its bound)"""
    x, K = z["x"], c["ctx"]
    var = _row_variance(x)
    if c["family"] == "low":
        assert bool(((var >= 0.1 * EPS5) & (var <= 10 * EPS5)).all())
    if c["family"] == "offset":
        assert bool((x.mean(-1).abs() / var.sqrt() > (1000 if K <= 192 else 50)).all())
    e, De, r, rho = bd.layernorm_stats(x, EPS5)
    y, P = bd.fl_mul(e, De, r, r * rho)
    y, P = bd.fl_mul(y, P, z["ln_w"])
    y, P = bd.fl_add(y, P, z["ln_b"])
    xh, dq = bd.rounded_operand(y, P)
    v, E = xh @ z["W"].T, dq @ z["W"].abs().T
    Pv = E + bd.accumulation(xh.abs() @ z["W"].abs().T + E, K)
    v, Pv = bd.fl_add(v, Pv, z["b"])
    return {"scratch": (y, P), "out": (v, Pv)}


# =================================================================================================== ctxnorm
def _ctx_cases():
    fams = ("plain", "low", "big")
    out, i = [], 0
    for B, T in ((1, 1), (1, 5), (2, 77)):
        for ctx in (64, 192):
            out.append(_case("ctxnorm", fams[i % 3], B=B, T=T, ctx=ctx, depth=1))
            i += 1
    out.append(_case("ctxnorm", "low", B=1, T=5, ctx=192, depth=1))
    out.append(_case("ctxnorm", "big", B=2, T=77, ctx=64, depth=1))
    out.append(_case("ctxnorm", "plain", B=1, T=5, ctx=64, depth=2))
    assert {(c["family"], c["ctx"]) for c in out} >= {(f, k) for f in fams for k in (64, 192)}
    return out


def _ctx_inputs(c, g):
    rows, K, fam = c["B"] * c["T"], c["ctx"], c["family"]
    x = _randn(g, rows, K)
    if fam == "low":
        k = 10 ** (1.4 * _rand(g, rows, 1) - 0.7)
        x = x / x.pow(2).mean(-1, keepdim=True).sqrt() * (k * 1e-5).sqrt()
    else:
        x[:, -4:] *= max(1.0, math.sqrt(K / 4.0))
        x = x * (1e4 if fam == "big" else 1.5)
    return dict(x=bf16(x), w=f32(1 + 0.3 * _randn(g, c["depth"], K)))


def _ctx_reference(c, z):
    """scratch = bf16(fl(fl(x rs) w)) with the weight of the LAST block (the blocks share the scratch, in order)"""
    x = z["x"]
    if c["family"] == "low":
        ms = x.pow(2).mean(-1)
        assert bool(((ms >= 0.1 * EPS5) & (ms <= 10 * EPS5)).all())
    if c["depth"] > 1:
        assert float((z["w"][-1] - z["w"][0]).abs().mean()) > 0.1
    r, rho = bd.rms_rows(x, EPS5)
    y, P = bd.fl_mul(x, 0.0, r, r * rho)
    y, P = bd.fl_mul(y, P, z["w"][-1])
    return {"scratch": (y, bd.bf16_store(y, P))}


# =================================================================================================== advance
def _adv_cases():
    out = []
    for batch, n, counter in ((1, 9, 0), (16, 9, 4), (64, 9, 7), (16, 9, 8), (64, 9, 11), (1, 1, 0), (16, 1, 3), (64, 2, 0)):
        out.append(_case("advance", "plain", batch=batch, grid_len=n, counter=counter))
    n = 9
    assert {c["counter"] for c in out if c["grid_len"] == n} >= {0, 4, n - 2, n - 1} and any(c["grid_len"] == 1 for c in out)
    return out


def _adv_inputs(c, g):
    n = c["grid_len"]
    return dict(t_grid=f32(_rand(g, n)), dt_grid=f32(_randn(g, n)))


def _adv_reference(c, z):
    """timesteps[0:batch] = t_grid[k], dt = dt_grid[k], k = min(counter + 1, grid_len - 1); counter + 1 -- exact"""
    k = min(c["counter"] + 1, c["grid_len"] - 1)
    if c["counter"] + 1 > c["grid_len"] - 1:
        assert k == c["grid_len"] - 1
    t = z["t_grid"][k].expand(c["batch"]).clone().view(1, -1)
    zero = torch.zeros(1, 1, dtype=F64)
    return {"timesteps": (t, torch.zeros_like(t)), "dt": (z["dt_grid"][k].view(1, 1), zero),
            "counter": (torch.tensor([[float(c["counter"] + 1)]], dtype=F64), zero)}


# ===================================================================================================
_KERNELS = {"embed": (_embed_cases, _forward_inputs, _forward_reference), "final": (_final_cases, _forward_inputs, _forward_reference),
            "step": (_step_cases, _forward_inputs, _forward_reference), "gates": (_gates_cases, _forward_inputs, _forward_reference),
            "pooled": (_pooled_cases, _pooled_inputs, _pooled_reference), "ctxnorm": (_ctx_cases, _ctx_inputs, _ctx_reference),
            "advance": (_adv_cases, _adv_inputs, _adv_reference)}
CASES = {k: fns[0]() for k, fns in _KERNELS.items()}
ALL = [c for cs in CASES.values() for c in cs]
assert len({c["name"] for c in ALL}) == len(ALL)


def inputs(case):
    return _KERNELS[case["kernel"]][1](case, _gen(case))


def reference(case, z):
    """{output: (ref, bound)} float64; asserts that the case reaches what it names"""
    return _KERNELS[case["kernel"]][2](case, z)
