"""Cases, inputs and float64 references of the row kernels that have a C-ABI entry of their own: rmsnorm_modulate, small_linear and
shift_bias (csrc/dit_ops.hip) and the five kernels of csrc/decode_ops.hip.  tests/test_row_instances_gpu.py runs every case on the GPU,
tests/test_row_bounds_cpu.py proves on the CPU that seeded kernel bugs land over the bounds.

A case is a dict(kernel, name, family, shape parameters).  inputs(case) draws its tensors from a generator seeded by the name, as
float64 tensors that hold exactly the fp32 / bf16 values the kernel reads.  reference(case, z) returns {output name: (ref, bound)},
float64, by the error model of tests/_bounds.py ("Row kernels"), and ASSERTS that the case reaches the branch it names (the caps: a
low-energy row really has a mean square <= 10 eps, a tail case really has a pre-activation over the softplus threshold, ...).

Input families -- a structural mistake is an O(1) error on named elements:
  plain    O(1) rows; half of a row's energy sits in its last float4 (also in `big`), so a reduction that drops it is off by O(1)
  low      rows whose mean square (variance, for the LayerNorms, surfel_head mode 1 included) lies between 0.1 eps and 10 eps: eps decides the output
  big      rows at 1e4
  offset   (LayerNorms) rows with a common offset 100 x their spread: a one-pass variance would cancel
  modulation rows of neighbouring batch items differ by O(1) (+-2 alternating), so a row modulated with its neighbour's row is wrong by O(1)
  planted  (tiny attention) every group of a tile has (nearly) the SAME keys, one key dominates each query, V rows are distinct one-hot
           patterns with a group marker: a key of the neighbouring group let in takes half the weight
  flat     (tiny attention) zero queries: the uniform softmax weighs every admitted key alike, so one key too many or too few shows
  tail     (surfel head) weights scaled per channel so that the largest |pre-activation| of every channel is 28 (+28 on one softplus
           channel, -28 on the other): saturated tanh, softplus on both sides of its threshold, log1p(exp(pre)) of very negative pre; the
           quaternion channels have zero weights and bias, so every row of mode 0 and the rows of anchor 0 of mode 1 normalise an exact zero"""
import math
import zlib

import torch

from tests import _bounds as bd

F64 = torch.float64
EPS5 = bd.EPS_F32


def f32(t):
    return t.to(torch.float32).to(F64)


def bf16(t):
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def _gen(case):
    return torch.Generator().manual_seed(zlib.crc32(case["name"].encode()))


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F64)


def _rand(g, *shape):
    return torch.rand(*shape, generator=g, dtype=F64)


def _case(kernel, family, **kw):
    name = kernel + "_" + "_".join(f"{k}{v}" for k, v in kw.items()) + "_" + family
    return dict(kw, kernel=kernel, family=family, name=name.replace(" ", "").replace("(", "").replace(")", "").replace(",", "x"))


def _tail_gain(D):
    """plain and big rows carry half of their energy in the last float4, so a reduction that drops it is off by O(1)"""
    return max(1.0, math.sqrt(D / 4.0))


def _alternating_table(g, B, D):
    """a [B, 6, D] modulation table (row 0 shift, row 1 scale, as scale_shift_table) whose batch items differ by O(1)"""
    t = 0.5 * _randn(g, B, 6, D)
    t += 2.0 * (1 - 2 * (torch.arange(B, dtype=F64) % 2)).view(B, 1, 1)
    return f32(t)


# =================================================================================================== rmsnorm_modulate
def _rms_cases():
    rows = [(4, 1, "none", None, "plain"), (64, 3, "contig", 0, "low"), (260, 5, "table", 5, "plain"), (768, 3, "table", "M-1", "low"),
            (1152, 1, "contig", "M", "big"), (2048, 5, "table", 5, "big"), (768, 5, "contig", None, "low"), (260, 1, "none", 0, "low"),
            (2048, 3, "table", None, "low"), (4, 5, "contig", 5, "low")]
    out = []
    for D, rpb, mod, first, fam in rows:
        for M in (12, 13):
            fr = {"M-1": M - 1, "M": M}.get(first, first)
            out.append(_case("rmsnorm_modulate", fam, M=M, D=D, rpb=rpb, mod=mod, first=fr))
    return out


def _rms_inputs(c, g):
    M, D, rpb, fam = c["M"], c["D"], c["rpb"], c["family"]
    B = (M + rpb - 1) // rpb
    x = _randn(g, M, D)
    rb = _randn(g, D)
    if fam == "low":
        k = 10 ** (1.4 * _rand(g, M, 1) - 0.7)                          # mean square k eps, k in [0.2, 5]
        x = x / x.pow(2).mean(-1, keepdim=True).sqrt() * (k * 1e-5).sqrt()
        rb = rb * 0.5 * math.sqrt(1e-5)
    else:
        x[:, -4:] *= _tail_gain(D)
        x, rb = (x * 1e4, rb * 1e4) if fam == "big" else (x * 1.5, rb)
    z = dict(x=f32(x), weight=f32(1 + 0.3 * _randn(g, D)), row_bias=f32(rb))
    if c["mod"] != "none":
        z["table"] = _alternating_table(g, B, D)
    return z


def _modulate(y, P, scale, shift):
    """fl(fl(y_hat fl(1 + scale)) + shift)"""
    s1, Ps = bd.fl_add(scale, 0.0, 1.0)
    y, P = bd.fl_mul(y, P, s1, Ps)
    return bd.fl_add(y, P, shift)


def rms_x_after(c, z):
    """x as the kernel leaves it: fp32 x + row_bias on rows >= first (one rounding: exact in float64 arithmetic, then to fp32)"""
    x = z["x"].clone()
    if c["first"] is not None:
        x[c["first"]:] = f32(x[c["first"]:] + z["row_bias"])
    return x


def _rms_reference(c, z):
    M, rpb = c["M"], c["rpb"]
    x = rms_x_after(c, z)
    if c["family"] == "low":
        ms = x.pow(2).mean(-1)
        assert bool(((ms >= 0.1 * EPS5) & (ms <= 10 * EPS5)).all()), (c["name"], "low-energy rows outside [0.1 eps, 10 eps]")
    if c["first"] == 5:
        assert M > 8, "first = 5 must split the second 4-row workgroup"
    r, rho = bd.rms_rows(x, EPS5)
    y, P = bd.fl_mul(x, 0.0, r, r * rho)
    y, P = bd.fl_mul(y, P, z["weight"])
    if c["mod"] != "none":
        b = torch.arange(M) // rpb
        if rpb > 1:
            assert bool((z["table"][1:, :2] - z["table"][:-1, :2]).abs().mean() > 1.0), "neighbouring modulation rows must differ by O(1)"
        y, P = _modulate(y, P, z["table"][b, 1], z["table"][b, 0])
    return {"out": (y, bd.bf16_store(y, P)), "x": (x, torch.zeros_like(x))}


# =================================================================================================== small_linear
def _sl_cases():
    out = []
    i = 0
    for B in (1, 4, 16):
        for K in (8, 256, 520, 1024):
            for N in (1, 6, 384):
                out.append(_case("small_linear", "plain", B=B, K=K, N=N, act_in=i % 2, act_out=(i // 2) % 2, bias=int(i % 3 != 0), add=int(i % 5 < 2)))
                i += 1
    for m in range(16):                                                 # every combination at one mid shape
        out.append(_case("small_linear", "plain", B=4, K=264, N=10, act_in=m & 1, act_out=(m >> 1) & 1, bias=(m >> 2) & 1, add=(m >> 3) & 1))
    for N in (6, 384):                                                  # the timestep embedding formed in the kernel
        out.append(_case("small_linear", "timestep", B=5, K=256, N=N, act_in=2, act_out=int(N == 6), bias=1, add=int(N == 384)))
    return out


TIMESTEPS = (0.0, 1e-3, 0.5, 1.0, 1000.0)


def _sl_inputs(c, g):
    B, K, N = c["B"], c["K"], c["N"]
    x = f32(torch.tensor(TIMESTEPS, dtype=F64)) if c["act_in"] == 2 else f32(2 * _randn(g, B, K))
    return dict(x=x, W=bf16(2 * _randn(g, N, K) / math.sqrt(K)), bias=f32(_randn(g, N)), add=f32(_randn(g, B, N)))


def sl_operand(c, z):
    """(xh, dq): the bf16 operand of the product mirrored in float64 and what an element may deviate by (tests/_bounds.py, rounded_operand)"""
    x = z["x"]
    if c["act_in"] == 0:
        return bd.bf16_round(x), torch.zeros_like(x)
    if c["act_in"] == 1:
        return bd.rounded_operand(*bd.silu(x, torch.zeros_like(x)))
    arg, Pa = bd.sincos_arg(x.view(-1, 1), torch.arange(128, dtype=F64))
    cs, Pc, sn, Ps = bd.sin_cos(arg, Pa)
    return bd.rounded_operand(torch.cat([cs, sn], 1), torch.cat([Pc, Ps], 1))


def _sl_reference(c, z):
    K = c["K"]
    if c["act_in"] == 2:
        assert K == 256 and float(z["x"].max()) == 1000.0 and float(z["x"].min()) == 0.0
    xh, dq = sl_operand(c, z)
    W = z["W"]
    v = xh @ W.T
    E = dq @ W.abs().T
    P = E + bd.accumulation(xh.abs() @ W.abs().T + E, K)
    if c["bias"]:
        v, P = bd.fl_add(v, P, z["bias"])
    if c["act_out"]:
        v, P = bd.silu(v, P)
    if c["add"]:
        v, P = bd.fl_add(v, P, z["add"])
    return {"y": (v, P)}


# =================================================================================================== shift_bias
def _sb_cases():
    out = []
    Ks = (64, 1024, 4096)
    i = 0
    for batch in (1, 8, 9, 17):
        for N in (8, 520, 3072):
            out.append(_case("shift_bias", "plain", batch=batch, N=N, K=Ks[(i + i // 3) % 3], bias=i % 2))
            i += 1
    return out


def _sb_inputs(c, g):
    B, N, K = c["batch"], c["N"], c["K"]
    return dict(W=bf16(_randn(g, N, K) / math.sqrt(K)), shift=f32(_randn(g, B, K)), bias=f32(_randn(g, N)))


def _sb_reference(c, z):
    """out = fl(bias + sum_k fl(shift_k W_nk)): K products and K additions, gamma(2 K + 1) on the absolute sum"""
    K = c["K"]
    v = z["shift"] @ z["W"].T
    A = z["shift"].abs() @ z["W"].abs().T
    if c["bias"]:
        v, A = v + z["bias"], A + z["bias"].abs()
    return {"out": (v, bd.gamma(2 * K + 1) * A)}


# =================================================================================================== layernorm_modulate
def _ln_cases():
    out = []
    fams = ("plain", "low", "offset", "big")
    i = 0
    for D in (4, 132, 768, 2048):
        for affine in (0, 1):
            for mod in (0, 1):
                for M in (12, 13):
                    fam = fams[(i + i // 4) % 4]
                    # low-energy rows under both eps, the other families alternate
                    eps = (1e-5, 1e-6)[(i // 4) % 2] if fam == "low" else (1e-5, 1e-6)[i % 2]
                    out.append(_case("layernorm_modulate", fam, M=M, D=D, affine=affine, mod=mod, eps=eps))
                i += 1
    return out


def _ln_rows(g, M, D, fam, eps):
    x = _randn(g, M, D)
    if fam == "low":
        k = 10 ** (1.4 * _rand(g, M, 1) - 0.7)
        e = x - x.mean(-1, keepdim=True)
        return e / e.pow(2).mean(-1, keepdim=True).sqrt() * (k * eps).sqrt() + 0.3 * math.sqrt(eps)
    if fam == "offset":
        return 100.0 * (1 + _rand(g, M, 1)) + x
    x[:, -4:] *= _tail_gain(D)
    return 1e4 * x if fam == "big" else 1.5 * x + 0.3


def _ln_inputs(c, g):
    M, D = c["M"], c["D"]
    return dict(x=f32(_ln_rows(g, M, D, c["family"], c["eps"])), weight=f32(1 + 0.3 * _randn(g, D)), bias=f32(0.5 * _randn(g, D)),
                table=_alternating_table(g, M, D))


def _ln_reach(c, x, eps):
    var, mean = x.var(-1, unbiased=False), x.mean(-1)
    if c["family"] == "low":
        assert bool(((var >= 0.1 * eps) & (var <= 10 * eps)).all()), (c["name"], "low-energy rows outside [0.1 eps, 10 eps]")
    if c["family"] == "offset":
        assert bool((mean.abs() >= 50 * var.sqrt()).all()), (c["name"], "the common offset must dwarf the spread")


def _ln_reference(c, z):
    eps = bd.F32(c["eps"])
    _ln_reach(c, z["x"], eps)
    e, De, r, rho = bd.layernorm_stats(z["x"], eps)
    y, P = bd.fl_mul(e, De, r, r * rho)
    if c["affine"]:
        y, P = bd.fl_mul(y, P, z["weight"])
        y, P = bd.fl_add(y, P, z["bias"])
    if c["mod"]:
        y, P = _modulate(y, P, z["table"][:, 1], z["table"][:, 0])
    return {"out": (y, bd.bf16_store(y, P))}


# =================================================================================================== tiny_mlp_silu
def _mlp_cases():
    return [_case("tiny_mlp_silu", "plain", M=M, Cin=ci, Ch=ch, D=D) for ci, ch in ((1, 1), (10, 10), (16, 16), (3, 16)) for D in (1, 70, 128)
            for M in (8, 9)]


def _mlp_inputs(c, g):
    M, Cin, Ch, D = c["M"], c["Cin"], c["Ch"], c["D"]
    return dict(x=f32(1.5 * _randn(g, M, Cin)), w1=f32(1.5 * _randn(g, Ch, Cin) / math.sqrt(Cin)), b1=f32(0.5 * _randn(g, Ch)),
                w2=f32(1.5 * _randn(g, D, Ch) / math.sqrt(Ch)), b2=f32(0.5 * _randn(g, D)))


def _mlp_reference(c, z):
    """fc1: b1 + Cin multiply-adds in a chain, gamma(2 Cin) on the absolute sum; gelu_tanh; fc2 likewise over Ch with the errors of h; silu"""
    Cin, Ch = c["Cin"], c["Ch"]
    s1 = z["b1"] + z["x"] @ z["w1"].T
    P1 = bd.gamma(2 * Cin) * (z["b1"].abs() + z["x"].abs() @ z["w1"].abs().T)
    h, Ph = bd.gelu_tanh(s1, P1)
    s2 = z["b2"] + h @ z["w2"].T
    prop = Ph @ z["w2"].abs().T
    P2 = prop + bd.gamma(2 * Ch) * (z["b2"].abs() + h.abs() @ z["w2"].abs().T + prop)
    o, Po = bd.silu(s2, P2)
    return {"out": (o, bd.bf16_store(o, Po))}


# =================================================================================================== assemble_tokens
def _asm_cases():
    out = []
    for D in (4, 132, 1024):
        for src_f in (0, 3, 8):
            for f in (1, 4):
                for P in (24, 9):                                       # rows P (1 + f): 48 / 120 and 18 / 45
                    if src_f and P % src_f:
                        continue                                        # (P is a multiple of src_f: 8 only divides 24)
                    out.append(_case("assemble_tokens", "plain", P=P, D=D, src_f=src_f, f=f))
    return out


def _asm_inputs(c, g):
    P, D, sf, f = c["P"], c["D"], c["src_f"], c["f"]
    return dict(src=f32(_randn(g, P // sf * (1 + sf) if sf else P, D)), latent_embedding=f32(_randn(g, f, D)))


def _asm_reference(c, z):
    P, D, sf, f = c["P"], c["D"], c["src_f"], c["f"]
    p = torch.arange(P)
    sr = (p // sf) * (1 + sf) + 1 + p % sf if sf else p
    out = torch.empty(P, 1 + f, D, dtype=F64)
    out[:, 0] = z["src"][sr]
    out[:, 1:] = z["latent_embedding"]
    return {"out": (out.view(P * (1 + f), D), torch.zeros(P * (1 + f), D, dtype=F64))}


# =================================================================================================== tiny_attention
def _ta_cases():
    out = []
    for S in (1, 2, 3, 4, 5, 6, 7, 8, 9, 16):
        G = 16 // S
        for heads in (1, 3):
            fam = "planted" if heads == 1 else "flat"
            full = 2 * G if heads == 1 else G                           # groups % G == 0
            ragged = (1 if heads == 1 else 2 * G + max(1, G - 1)) if G > 1 else (1 if heads == 1 else 3)
            for groups in (full, ragged):
                out.append(_case("tiny_attention", fam, S=S, groups=groups, heads=heads))
            if G > 1:                                                   # and the other family on the other geometry
                out.append(_case("tiny_attention", "flat" if fam == "planted" else "planted", S=S, groups=G + 1, heads=heads))
    return out


def _ta_inputs(c, g):
    S, groups, H = c["S"], c["groups"], c["heads"]
    kbase = _randn(g, 1, S, H, 64)
    k = bf16(kbase + 0.05 * _randn(g, groups, S, H, 64))
    if c["family"] == "planted":
        perm = torch.stack([torch.randperm(S, generator=g) for _ in range(groups)])
        q = bf16(1.5 * k[torch.arange(groups)[:, None], perm])
    else:
        q = torch.zeros_like(k)
    v = torch.zeros(groups, S, H, 64, dtype=F64)
    row = torch.arange(groups * S).view(groups, S, 1)
    h = torch.arange(H).view(1, 1, H)
    v.scatter_(3, ((row * 5 + h) % 64).unsqueeze(-1), 1.0)               # a one-hot position of its own per row
    grp = torch.arange(groups).view(groups, 1, 1).expand(groups, S, H)
    v.scatter_add_(3, ((grp * 11 + 3) % 64).unsqueeze(-1), torch.full((groups, S, H, 1), 0.5, dtype=F64))      # the group's marker
    return dict(qkv=torch.stack([q, k, v], 2))                           # [groups, S, 3, H, 64]


def ta_pairs(c, z):
    """q, k, v as [groups x heads, S, 64]"""
    S, groups, H = c["S"], c["groups"], c["heads"]
    return tuple(z["qkv"][:, :, i].permute(0, 2, 1, 3).reshape(groups * H, S, 64) for i in range(3))


TA_SCALE = 0.125 * bd.LOG2E_F32          # p = fl(s 0.125) is exact; __expf multiplies by the fp32 log2 e


def _ta_reference(c, z):
    """the attention model of tests/_bounds.py with one key tile: scores in log2 units with c = 0.125 log2e_f32 applied after the
    product, rel_c the roundings of p - max and of the product with log2 e inside __expf, no lazy reference, one key group"""
    S, groups, H = c["S"], c["groups"], c["heads"]
    q, k, v = ta_pairs(c, z)
    zero = torch.zeros_like(q)
    out, bound, _ = bd.attention(q, zero, k, zero, v, c=TA_SCALE, n_acc=64, rel_c=bd.gamma(2), lazy=0.0, tiles=1, groups=1)
    if c["family"] == "planted" and S > 1:
        p = torch.softmax(0.125 * q @ k.transpose(1, 2), -1).amax(-1)
        assert float(p.median()) > 0.9, (c["name"], "one key must dominate")
    back = lambda t: t.view(groups, H, S, 64).permute(0, 2, 1, 3).reshape(groups * S, H * 64)        # noqa: E731
    return {"out": (back(out), back(bound))}


def ta_ragged(c):
    return c["groups"] % (16 // c["S"]) != 0


# =================================================================================================== surfel_head
SKIP_WEIGHT = bd.F32(0.7)
SCALE_FACTOR = bd.F32(bd.F32(0.0045) / bd.F32(0.6931471805599453))       # the kernel's fp32 constant scene_extent / softplus(0)
C225 = bd.F32(0.225)


def _sh_cases():
    out = []
    for D in (4, 128, 1028):
        for fam in ("plain", "tail"):
            for rows in (12, 9):
                out.append(_case("surfel_head", fam, rows=rows, D=D, mode=0, f=1))
                for f in (1, 3):
                    out.append(_case("surfel_head", fam, rows=rows, D=D, mode=1, f=f))
        for rows in (12, 9):                                             # the fixed 1e-5 of mode 1 decides these rows
            out.append(_case("surfel_head", "low", rows=rows, D=D, mode=1, f=3))
    return out


def sh_rows(c):
    """(x row, anchor index p) of every output row"""
    r = torch.arange(c["rows"])
    if c["mode"] == 0:
        return r, r
    p = r // c["f"]
    return p * (1 + c["f"]) + 1 + (r - p * c["f"]), p


def _sh_features(c, z):
    """(y, Py): the rows the 13 x D product reads -- LayerNorm with affine (mode 1) or silu (mode 0)"""
    xr, _ = sh_rows(c)
    x = z["x"][xr]
    if c["mode"] == 0:
        return bd.silu(x, torch.zeros_like(x))
    _ln_reach(c, x, EPS5)
    e, De, r, rho = bd.layernorm_stats(x, EPS5)
    y, P = bd.fl_mul(e, De, r, r * rho)
    y, P = bd.fl_mul(y, P, z["ln_weight"])
    return bd.fl_add(y, P, z["ln_bias"])


def _sh_inputs(c, g):
    rows, D, mode, f = c["rows"], c["D"], c["mode"], c["f"]
    np_ = rows // f
    nx = np_ * (1 + f) if mode else rows
    x = _ln_rows(g, nx, D, "low", 1e-5) if c["family"] == "low" else 1.5 * _randn(g, nx, D) + (0.3 if mode else 0.0)
    if mode == 1 and c["family"] == "plain":
        x[:, -4:] *= _tail_gain(D)
    z = dict(x=f32(x),
             ln_weight=f32(1 + 0.3 * _randn(g, D)), ln_bias=f32(0.3 * _randn(g, D)),
             anchor=f32(0.3 * _randn(g, np_, 13) if mode else 0.3 * _randn(g, rows, 3)), base_pre=f32(0.5 * _randn(g, np_, 13)))
    w, b = _randn(g, 13, D) / math.sqrt(D), 0.3 * _randn(g, 13)
    if c["family"] == "tail":
        y, _ = _sh_features(c, z)
        pre = y @ f32(w).T
        top = pre.abs().argmax(0)                                        # the row that ends at +-28, per channel
        scale = 28.0 / pre.abs().amax(0)
        scale[4] *= torch.sign(pre[top[4], 4])                           # ... at +28 on one softplus channel: over the threshold
        scale[5] *= -torch.sign(pre[top[5], 5])                          # ... at -28 on the other: log1p(exp(pre)) of a tiny exp
        w, b = w * scale[:, None], 0.3 * b
        w[6:10], b[6:10] = 0.0, 0.0
        z["base_pre"][0, 6:10] = 0.0
    z.update(w=f32(w), b=f32(b))
    return z


def _sh_reference(c, z):
    D, mode = c["D"], c["mode"]
    _, p = sh_rows(c)
    y, Py = _sh_features(c, z)
    w, b = z["w"], z["b"]
    prop = Py @ w.abs().T
    pre = y @ w.T + b                                                   # products, the sum of D terms, + b: gamma(2 D + 1)
    Pp = prop + bd.gamma(2 * D + 1) * (y.abs() @ w.abs().T + prop + b.abs())
    t, Pt = bd.tanh(pre[:, :3], Pp[:, :3])
    pos, Ppos = bd.fl_mul(t, Pt, C225)
    if mode == 0:
        pos, Ppos = bd.fl_mul(pos, Ppos, SKIP_WEIGHT)
        pos, Ppos = bd.fl_add(pos, Ppos, z["anchor"])
    else:
        pos, Ppos = bd.fl_add(pos, Ppos, z["anchor"][p, :3])
        pre, Pp = bd.fl_add(pre, Pp, z["base_pre"][p])
    assert float((pre.abs() + Pp).max()) <= bd.MATH_ARG_MAX, (c["name"], "a pre-activation outside the measured range of tanhf / expf")
    if c["family"] == "tail":
        assert bool((pre[:, 4:6] > 20).any()) and bool((pre[:, 4:6] < -10).any()), (c["name"], "softplus must see both tails")
        assert bool((pre[:, [0, 1, 2, 10, 11, 12]].abs() > 15).any()), (c["name"], "tanh must saturate")
        zq = (pre[:, 6:10] == 0).all(-1)
        assert bool(zq.any()) and bool((Pp[:, 6:10][zq] == 0).all()), (c["name"], "a row must normalise an exact zero quaternion")
        assert mode == 0 or not bool(zq.all()), (c["name"], "mode 1 keeps rows with a quaternion")
    g, Pg = torch.empty_like(pre), torch.empty_like(pre)
    g[:, :3], Pg[:, :3] = pos, Ppos
    g[:, 3], Pg[:, 3] = bd.sigmoid(pre[:, 3], Pp[:, 3])
    g[:, 4:6], Pg[:, 4:6] = bd.fl_mul(*bd.softplus(pre[:, 4:6], Pp[:, 4:6]), SCALE_FACTOR)
    g[:, 6:10], Pg[:, 6:10] = bd.normalize4(pre[:, 6:10], Pp[:, 6:10])
    t, Pt = bd.tanh(pre[:, 10:], Pp[:, 10:])
    g[:, 10:], Pg[:, 10:] = bd.fl_add(0.5 * t, 0.5 * Pt, 0.5)            # 0.5f t is exact
    return {"gaussians": (g, Pg), "pre_out": (pre, Pp)}


# ===================================================================================================
_KERNELS = {"rmsnorm_modulate": (_rms_cases, _rms_inputs, _rms_reference), "small_linear": (_sl_cases, _sl_inputs, _sl_reference),
            "shift_bias": (_sb_cases, _sb_inputs, _sb_reference), "layernorm_modulate": (_ln_cases, _ln_inputs, _ln_reference),
            "tiny_mlp_silu": (_mlp_cases, _mlp_inputs, _mlp_reference), "assemble_tokens": (_asm_cases, _asm_inputs, _asm_reference),
            "tiny_attention": (_ta_cases, _ta_inputs, _ta_reference), "surfel_head": (_sh_cases, _sh_inputs, _sh_reference)}
CASES = {k: fns[0]() for k, fns in _KERNELS.items()}
ALL = [c for cs in CASES.values() for c in cs]
assert len({c["name"] for c in ALL}) == len(ALL)


def inputs(case):
    return _KERNELS[case["kernel"]][1](case, _gen(case))


def reference(case, z):
    """{output: (ref, bound)} float64; asserts the caps of the case"""
    return _KERNELS[case["kernel"]][2](case, z)


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound, a zero bound met exactly counting as 0 and anything non-finite as inf"""
    err = (got.to(F64) - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(torch.where(torch.isfinite(r), r, torch.full_like(r, math.inf)).max()) if r.numel() else 0.0
