"""Element-wise error bounds of the bf16-MFMA kernels (and, at the end, of the row kernels around them) against a float64 reference computed from the exact bf16 / fp32 values the
kernel reads.  Every function takes and returns float64 torch tensors (any device).

Model.  u = 2^-24 is the unit roundoff of fp32 round-to-nearest, ub = 2^-8 that of bf16; gamma(n) = n u / (1 - n u) bounds the
relative error of n successive fp32 roundings (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1).

* Accumulation.  A product of two bf16 values (8 significant bits each) is exact in fp32.  Whatever order and grouping the sum of
  the K products takes -- inside an MFMA, across K-tiles, across split-K partials -- it is a tree of K - 1 additions, so its error is
  at most (K - 1) times the largest relative error of one addition times sum_k |a_k w_k|.  Allowing each addition 2u (round toward
  zero as well as to nearest) gives E = gamma(2K) * s with s = |A| |W|^T.
* bf16 store.  Round-to-nearest-even of a value v that carries a propagated pre-rounding error P: |bf16(v) - ref| <= ub |v| + P
  <= ub |ref| + (1 + ub) P.
* Each epilogue below propagates P through its fp32 operations, one rounding (u relative) per operation (a fused multiply-add
  rounds once; the bounds count two roundings and so hold either way).
"""
import math

import torch

U = 2.0 ** -24
UB = 2.0 ** -8
GELU_DMAX = 1.1289                  # max |gelu'(x)| (at x ~ 2.4)
RSQRT_REL = 4 * U                   # rsqrtf: 2 ulp (2^-23 relative each)
# erf by Abramowitz & Stegun 7.1.26 in fp32 (dit_gemm.hip: gelu_erf2): absolute error of erf(|v| / sqrt 2) at most
#   1.5e-7 (the approximation itself) + rounding of the evaluation, counted as
#   x = |v| fl(1/sqrt 2): 2u relative -> < 1u on erf (|d erf / dx| x <= 0.49);
#   t = rcp(1 + p x): fma + 1-ulp rcp, 4u relative -> |d S / dt| t <= sum i |a_i| = 16.2 -> 65u, S(t) = sum a_i t^i;
#   Horner, 4 fma on t <= 1 with sum |a_i| = 4.48 (coefficients rounded to fp32 included): gamma(8) 4.48 + 4.48u -> 41u;
#   exp2(-x^2 log2 e): argument 5u relative -> x^2 e^-x^2 5u <= 1.9u, 1-ulp exp2 -> 2u;  S e (two products) 2u;  1 - S e: 1u
ERF_ABS = 1.5e-7 + 115 * U


def gamma(n):
    return n * U / (1 - n * U)


def accumulation(s, K):
    """E: bound on |fp32 sum - exact sum| of K bf16 products with absolute sum s = |A| |W|^T"""
    return gamma(2 * K) * s


def bf16_store(ref, P):
    """|bf16(v) - ref| where |v - ref| <= P"""
    return UB * ref.abs() + (1 + UB) * P


def add_bias(z, E, b):
    """v = fl(acc + b), |acc - z| <= E: returns (v_ref = z + b, P)"""
    v = z + b
    return v, E + U * (v.abs() + E)


def row_scale(T_sum, t, dim, eps):
    """r = rsqrt(sum_t partials / dim + eps) from t non-negative fp32 partials summing to T_sum (exact): returns (r_ref, rho) with
    |r_hat - r| <= rho r.  fp32 sum of t terms (gamma(t - 1)), 1 / dim rounded, product, + eps: gamma(t + 2) on the argument;
    rsqrt halves a relative argument error x: (1 - x)^(-1/2) - 1 <= x / (2 (1 - x)); then the rsqrtf error."""
    r = torch.rsqrt(T_sum / dim + eps)
    x = gamma(t + 2)
    return r, (1 + x / (2 * (1 - x))) * (1 + RSQRT_REL) - 1


def scale_then_bias(z, E, r, rho, b):
    """v = fl(fl(acc r_hat) + b) (the folded RMSNorm row scale, then the bias): returns (v_ref = z r + b, P)"""
    rhat = r * (1 + rho)
    P = E * rhat + z.abs() * r * rho                # |acc r_hat - z r|
    P = P + U * (z.abs() * r + P)                   # rounding of the product
    v = z * r + b
    return v, P + U * (v.abs() + P)                 # rounding of the sum


def head_norm(v, P, w, eps):
    """The per-head RMSNorm of 64-column groups: y = w v / sqrt(mean v^2 + eps) on rows of [..., G, 64] values v carrying errors P.
    The normaliser n = sqrt(|v|^2 / 64 + eps) is 1/8-Lipschitz in |v|, so the propagated part of its error is |e| / 8 <= |P| / 8
    (the |e| / |z| term, relative to n); the fp32 sum of the 64 squares adds gamma(64) relative, + eps one rounding, rsqrtf its own;
    then y = v fl(r w): two roundings.  Returns (y_ref, P_y)."""
    n = torch.sqrt(v.pow(2).mean(-1, keepdim=True) + eps)
    r = 1 / n
    pn = P.norm(dim=-1, keepdim=True) / 8
    rho_n = pn / (n - pn).clamp_min(1e-300)
    x = gamma(65)
    rho = (1 + rho_n) * (1 + x / (2 * (1 - x))) * (1 + RSQRT_REL) - 1
    y = w * v * r
    Py = w.abs() * r * ((1 + rho) * P + v.abs() * rho + gamma(2) * (1 + rho) * (v.abs() + P))
    return y, Py


def gelu(v):
    return 0.5 * v * (1 + torch.erf(v / math.sqrt(2)))


def gelu_store(v, P):
    """bf16(gelu_erf(v_hat)), |v_hat - v| <= P: |gelu_hat(v_hat) - gelu(v)| <= |gelu_hat(v_hat) - gelu(v_hat)| + max|gelu'| P, the
    first <= 0.5 |v_hat| (ERF_ABS + 3u) (erf error times |v| / 2; the product |v| erf and the sum v + . rounded).  Returns (ref, bound)."""
    ref = gelu(v)
    Pg = GELU_DMAX * P + 0.5 * (v.abs() + P) * (ERF_ABS + 3 * U)
    return ref, bf16_store(ref, Pg)


def residual(x0, g, v, Pv):
    """x = fl(x0 + g v_hat), |v_hat - v| <= Pv: returns (x_ref, R)"""
    x = x0 + g * v
    return x, g.abs() * Pv + gamma(2) * (x0.abs() + g.abs() * (v.abs() + Pv))


def emit_modulated(x, R, m):
    """bf16(x_hat fl(w fl(1 + s))), m = w (1 + s) exact: three roundings.  Returns (ref, bound)."""
    ref = x * m
    P = m.abs() * (R + gamma(3) * (x.abs() + R))
    return ref, bf16_store(ref, P)


def group_sumsq(x, R):
    """fp32 sum of the squares of 64 values x_hat, |x_hat - x| <= R, over [..., G, 64]: returns (ref, bound)"""
    ref = x.pow(2).sum(-1)
    return ref, (2 * x.abs() * R + R * R).sum(-1) + gamma(64) * (x.abs() + R).pow(2).sum(-1)


# ---------------------------------------------------------------------------------------------------------------------------------
# Attention (dit_attention.hip, dit_attention_hd.hip).  Reference: float64 softmax over the exact values the kernel reads; scores
# in LOG2 units S_ij = c sum_d qh_id kh_jd, where qh / kh are the bf16 operands of the kernel's QK^T MFMA and c is what it applies
# after the product (1 where the softmax scale and log2 e are folded into qh; head_dim^-1/2 log2 e in the exponent's FMA otherwise).
#
# 1. Operands.  qh (and kh where K is normalised in the kernel) is bf16(x_hat), x_hat the fp32 evaluation of a deterministic
#    function x of the inputs with |x_hat - x| <= tau |x| (or <= P).  Rounding is monotone, so bf16(x_hat) lies between bf16(x - e)
#    and bf16(x + e): the reference uses bf16(x) itself (the MIRROR) and an element may deviate by dq = max(bf16(x + e) - bf16(x),
#    bf16(x) - bf16(x - e)) -- zero unless x is within e of a rounding boundary, one bf16 ulp there.  (bf16_round rounds float64
#    directly: torch's double -> float -> bfloat16 would round twice.)
# 2. Scores.  Key j of query i carries an uncertainty D_ij (log2 units) of
#      c (dq |kh|^T + |qh| dk^T + dq dk^T)                      operands on the other side of a rounding boundary
#    + (gamma(2 n + 4) + rel_c) (A_ij + smax_i + lazy)           A = c |qh| |kh|^T: fp32 accumulation of n products that starts at
#                                                                 minus the reference maximum, the subtraction (or FMA) that forms the
#                                                                 exponent, the error rel_c of the fp32 value of c; smax_i = max_j |S_ij|
#                                                                 bounds every reference maximum, `lazy` what a score may exceed it by
#    + gamma(T + G + 2) (2 smax_i + lazy)                        roundings of the running reference itself (m += delta once per tile at
#                                                                 most, T tiles; m_g - m_all in the merge of G key groups): a weight is
#                                                                 scaled by exp2 of EXACTLY the delta its reference moved by, so only
#                                                                 these roundings make the references of two keys inconsistent
#    and, in nats, D = ln 2 (the above) + (T + G + 2) EXP2_REL: a weight is a product of at most T + G + 1 v_exp_f32 results.
#    The common factor 2^(m - m_hat) of a lazy or rounded reference cancels between numerator and denominator.
# 3. Output.  The kernel sums weights p_j g_j, g_j in [e^-D_j, e^D_j] (p: exact softmax numerators, out: exact result):
#      |sum p g v / sum p g - out| = |sum p g (v - out)| / sum p g <= sum_j p_j (e^D_j - 1) |v_j - out| / sum_j p_j e^-D_j
#    (sum_j p_j (v_j - out) = 0 removes the g = 1 part); the bf16 rounding of P touches the numerator only: + ub sum p e^D |v| / den;
#    fp32 accumulation of numerator and denominator over Lk terms with a rescale per tile and the merge: gamma(2 (Lk + T + G + 4))
#    times sum p e^D |v| / den for each; 1 / l, the product, then the bf16 store.  v_exp_f32 flushes results below 2^-126 to zero,
#    where g in [e^-D, e^D] does not hold: such a weight is below 2^(lazy - 126) of a row sum >= 1, Lk of them move the output by
#    less than Lk 2^(lazy - 126) max|v| (FLUSH below).
EXP2_REL = 2 * U                    # v_exp_f32: 1 ulp
LOG2E_F32 = 1.44269502162933349609375        # the fp32 value of the kernels' literal 1.4426950408889634f
EPS_F32 = 9.99999974737875163555145263671875e-06    # 1e-5f


def bf16_round(x):
    """float64 -> nearest bf16 value (ties to even), as float64; one rounding"""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.round(m * 256.0) / 256.0, e)


def rounded_operand(x, err):
    """(bf16(x), dq) for a kernel value bf16(x_hat), |x_hat - x| <= err (absolute, elementwise)"""
    ref = bf16_round(x)
    return ref, torch.maximum(bf16_round(x + err) - ref, ref - bf16_round(x - err))


def rms_scale_rel(n):
    """relative error of rsqrtf(fl(fl(sum of n exact fp32 squares) / n) + eps): the sum gamma(n - 1), the division (or product with an
    inexact 1 / n) and the addition of eps gamma(3); rsqrt halves a relative argument error; its own error RSQRT_REL"""
    x = gamma(n + 2)
    return (1 + x / (2 * (1 - x))) * (1 + RSQRT_REL) - 1


def attn_q_fwd(q, wq):
    """dit_attention.hip, q read from memory: qh = bf16(fl(fl(q w) rs)), rs = fl(C rsqrtf(mean q^2 + eps)) with C = 64^-1/2 log2 e as the
    fp32 product 0.125f * 1.4426950408889634f (exact); without the norm qh = bf16(fl(q C)).  q [..., 64] float64 -> (qh, dq)."""
    C = 0.125 * LOG2E_F32
    if wq is None:
        x, tau = q * C, gamma(1)
    else:
        x = q * wq * torch.rsqrt(q.pow(2).mean(-1, keepdim=True) + EPS_F32) * C
        tau = (1 + rms_scale_rel(64)) * (1 + gamma(3)) - 1
    return rounded_operand(x, x.abs() * tau)


def attn_q_proj(A, W, T_sum, tiles, dim, eps, wq):
    """dit_attention.hip, the q projection inside the workgroup: y = (A W^T) r per head, r the folded RMSNorm row scale (T_sum None:
    none), the per-head norm (wq None: none), then qh = bf16(fl(bf16(y_hat) C)) -- two bf16 roundings.  A [rows, K], W [H, 64, K]
    float64 -> (qh, dq) of [rows, H, 64].  Errors of y_hat from accumulation / row_scale / head_norm above (the partial sums of the key
    groups meet in a fixed order: still one summation tree of K products)."""
    K = A.shape[-1]
    z = torch.einsum("rk,hdk->rhd", A, W)
    E = accumulation(torch.einsum("rk,hdk->rhd", A.abs(), W.abs()), K)
    if T_sum is not None:
        r, rho = row_scale(T_sum[:, None, None], tiles, dim, eps)
        z, E = scale_then_bias(z, E, r, rho, torch.zeros_like(z))
    if wq is not None:
        z, E = head_norm(z, E, wq, EPS_F32)
    C = 0.125 * LOG2E_F32
    t_lo, t_ref, t_hi = bf16_round(z - E), bf16_round(z), bf16_round(z + E)
    one = gamma(1)
    ref = bf16_round(t_ref * C)
    lo, hi = bf16_round(t_lo * C - (t_lo * C).abs() * one), bf16_round(t_hi * C + (t_hi * C).abs() * one)
    return ref, torch.maximum(hi - ref, ref - lo)


def attn_rows_normed(x, w, d):
    """bf16(fl(x fl(rs w))), rs = rsqrtf(fl(sum x^2 / d) + eps): K rows normalised while they are staged (both files) and q rows of
    the V^T variant of dit_attention_hd.hip.  x [..., d] float64 -> (xh, dx)."""
    y = x * w * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS_F32)
    tau = (1 + rms_scale_rel(max(d, 64))) * (1 + gamma(2)) - 1
    return rounded_operand(y, y.abs() * tau)


def attn_q_hd(q, d):
    """attention_hd_kernel: qh = bf16(fl(q rs)), rs = fl(rsqrtf(d) log2 e)"""
    x = q * (LOG2E_F32 / math.sqrt(d))
    return rounded_operand(x, x.abs() * (RSQRT_REL + gamma(2)))


def attention(qh, dq, kh, dk, v, c=1.0, n_acc=64, rel_c=0.0, lazy=8.0, tiles=None, groups=1, budget=1 << 27):
    """(out, bound, dominant key) of softmax_j(S_ij ln 2) v_j, S = c qh kh^T (log2 units), by the model above.  qh, dq [P, Lq, d];
    kh, dk [P, Lk, d]; v [P, Lk, dv] float64 (P: batch x heads); chunked over P and Lq so that the [p, q, Lk, dv] tensor of
    |v_j - out_i| stays under `budget` elements."""
    P, Lq, _ = qh.shape
    Lk, dv = v.shape[1], v.shape[2]
    T = tiles if tiles is not None else (Lk + 63) // 64
    G = groups
    LN2 = math.log(2.0)
    out = torch.empty(P, Lq, dv, dtype=torch.float64, device=qh.device)
    bound = torch.empty_like(out)
    dom = torch.empty(P, Lq, dtype=torch.long, device=qh.device)
    qc = max(1, min(Lq, budget // (Lk * dv)))
    pc = max(1, min(P, budget // (qc * Lk * dv)))
    g_acc, g_ref, g_sum = gamma(2 * n_acc + 4) + rel_c, gamma(T + G + 2), gamma(2 * (Lk + T + G + 4))
    flush = Lk * 2.0 ** (lazy - 126)
    for p0 in range(0, P, pc):
        ps = slice(p0, p0 + pc)
        kT, akT, dkT = kh[ps].transpose(1, 2), kh[ps].abs().transpose(1, 2), dk[ps].transpose(1, 2)
        vv, av = v[ps], v[ps].abs()
        vmax = av.amax((1, 2))[:, None, None]
        for q0 in range(0, Lq, qc):
            qs = slice(q0, q0 + qc)
            q_, dq_ = qh[ps, qs], dq[ps, qs]
            S = c * (q_ @ kT)
            A = c * (q_.abs() @ akT)
            smax = S.abs().amax(-1, keepdim=True)
            D = c * (dq_ @ akT + q_.abs() @ dkT + dq_ @ dkT) + g_acc * (A + smax + lazy) + g_ref * (2 * smax + lazy)
            D = LN2 * D + (T + G + 2) * EXP2_REL
            m = S.amax(-1, keepdim=True)
            p = torch.exp((S - m) * LN2)
            o = (p @ vv) / p.sum(-1, keepdim=True)
            den = (p * torch.exp(-D)).sum(-1, keepdim=True)
            up = p * torch.exp(D)
            t1 = torch.einsum("pqk,pqkd->pqd", p * torch.expm1(D), (vv[:, None] - o[:, :, None]).abs()) / den
            num = (up @ av) / den
            Pe = t1 + UB * num + 2 * g_sum * num + flush * vmax
            Pe = Pe + gamma(4) * (o.abs() + Pe)
            out[ps, qs], bound[ps, qs], dom[ps, qs] = o, bf16_store(o, Pe), S.argmax(-1)
    return out, bound, dom


# ---------------------------------------------------------------------------------------------------------------------------------
# Row kernels (dit_ops.hip: rmsnorm_modulate, small_linear, shift_bias; decode_ops.hip: tiny_mlp_silu, layernorm_modulate,
# tiny_attention, surfel_head).  A value is a pair (ref, P): the float64 reference and a bound on |fp32 value - ref|.  fl_add / fl_mul
# propagate such pairs through one fp32 operation (one rounding each; a contracted multiply-add rounds once and is counted as two);
# a division costs DIV_REL.  The references use the fp32 values of the kernels' literals (F32 below).
#
# Math library.  The relative errors of the OCML functions these kernels call are MEASURED, each function alone on a dense grid over
# the argument range of the cases (tools/row_math_probe.hip, output in profiles/row_math_error.txt); the constant is twice the worst
# relative error observed, because a grid can miss the worst argument.  Nothing else here is measured.
TANHF_REL = 2 * 1.6974e-07          # tanhf on [-32, 32]: 2.848 u   (profiles/row_math_error.txt, lines "tanhf")
SINF_REL = 2 * 1.2237e-07           # sinf on [0, 1024]: 2.053 u    (lines "sinf")
COSF_REL = 2 * 1.2371e-07           # cosf on [0, 1024]: 2.076 u    (lines "cosf")
EXPF_REL = 2 * 1.3989e-06           # expf on [-40, 40]: 23.47 u, growing with |x|   (lines "expf", the first two)
EXPF_FREQ_REL = 2 * 4.1033e-07      # expf on [-9.25, 0], the timestep frequencies: 6.884 u   (line "expf", the third)
LOG1PF_REL = 2 * 1.1831e-07         # log1pf on [1e-18, 1e18]: 1.985 u   (lines "log1pf")
SQRTF_REL = 2 * 5.9605e-08          # sqrtf on [1e-30, 1e10]: 1.000 u (correctly rounded)   (lines "sqrtf")
MATH_ARG_MAX = 40.0                 # |argument| of tanhf / expf the grids cover (sinf / cosf: 1024)
# a / b: correctly rounded under hipcc's default; counted as a 1-ulp v_rcp_f32 and a product so that it also holds for a reciprocal
DIV_REL = 2 * U + U
LOG2E_REL = abs(LOG2E_F32 - 1 / math.log(2.0)) * math.log(2.0)     # the fp32 literal 0x1.715476p+0 of __expf against log2 e
SILU_DMAX = 1.0999                  # max |silu'(x)| (at x ~ 2.4)
GELU_TANH_DMAX = 1.13               # max |gelu_tanh'(x)| (at x ~ 2.4; 1.1290)
XSECH2_MAX = 0.4478                 # max |x| sech^2(x) (at x ~ 0.7717): what a relative error of tanh's argument becomes
FLUSH_ABS = 2.0 ** -120             # v_exp_f32 returns 0 below 2^-126 and overflows above 2^128: |v| e^-|v| there is below this


def F32(x):
    """the fp32 value of a literal, as float64"""
    return float(torch.tensor(x, dtype=torch.float32))


def fl_add(a, Pa, b, Pb=0.0):
    """v = fl(a_hat + b_hat): (a + b, Pa + Pb + u (|a + b| + Pa + Pb))"""
    v = a + b
    P = Pa + Pb
    return v, P + U * (v.abs() + P)


def fl_mul(a, Pa, b, Pb=0.0):
    """v = fl(a_hat b_hat): (a b, |a| Pb + |b| Pa + Pa Pb, then one rounding)"""
    v = a * b
    aa = a.abs() if torch.is_tensor(a) else abs(a)
    ab = b.abs() if torch.is_tensor(b) else abs(b)
    P = aa * Pb + ab * Pa + Pa * Pb
    return v, P + U * (v.abs() + P)


def wave_sum(abs_sum, n):
    """|fp32 sum - exact sum| of n fp32 terms with absolute sum abs_sum, in whatever order and grouping (per-lane partial sums, the
    xor butterfly): a tree of n - 1 additions, gamma(n) abs_sum"""
    return gamma(n) * abs_sum


def rms_rows(x, eps):
    """rs = rsqrtf(fl(fl(sum of D fp32 squares) / D) + eps) of rows x [..., D] (exact fp32 values): (r_ref, rho), |rs - r| <= rho r.
    row_scale with D + 1 partials: the squares are rounded too."""
    D = x.shape[-1]
    return row_scale(x.pow(2).sum(-1, keepdim=True), D + 1, D, eps)


def layernorm_stats(x, eps):
    """Two-pass LayerNorm statistics of rows x [..., D] (exact fp32 values), as layernorm_modulate_kernel / surfel_head_kernel (mode 1)
    form them: mean = fl(wave sum / D), centred values e = fl(x - mean), rs = rsqrtf(fl(fl(sum e^2) / D) + eps).
      mean:  |dm| <= Dm = (1 + u) gamma(D) sum|x| / D + u |mean|
      e:     |e_hat - e| <= De = Dm + u (|e| + Dm)
      q = sum e_hat^2:  |q_hat - q| <= sum (2 |e| De + De^2) + gamma(D + 1) sum (|e| + De)^2   (squares rounded, D - 1 additions)
      A = q / D + eps:  |A_hat - A| <= dq / D + gamma(2) (A + dq / D);  rsqrt halves the relative error x of A, then RSQRT_REL
    Returns (e, De, r, rho): y = e r is evaluated by the caller with |rs - r| <= rho r."""
    D = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    Dm = (1 + U) * wave_sum(x.abs().sum(-1, keepdim=True), D) / D + U * mean.abs()
    e = x - mean
    De = Dm + U * (e.abs() + Dm)
    q = e.pow(2).sum(-1, keepdim=True)
    dq = (2 * e.abs() * De + De * De).sum(-1, keepdim=True) + gamma(D + 1) * (e.abs() + De).pow(2).sum(-1, keepdim=True)
    A = q / D + eps
    xa = (dq / D + gamma(2) * (A + dq / D)) / A
    r = torch.rsqrt(A)
    rho = (1 + xa / (2 * (1 - xa))) * (1 + RSQRT_REL) - 1
    return e, De, r, rho


def fast_exp_rel(x):
    """relative error of __expf(x) = v_exp_f32(fl(log2e_f32 x)): the product's rounding and the literal's error move the exponent by
    |x| log2 e (u + LOG2E_REL), a factor exp(|x| (u + LOG2E_REL)); then the 1-ulp exp2"""
    return torch.exp(x.abs() * (U + LOG2E_REL)) * (1 + EXP2_REL) - 1


def _one_plus_exp_rel(v, P, e_rel):
    """relative error of fl(1 + e_hat), e = exp(-v_hat), e_hat = e (1 + e_rel): e_rel e / (1 + e) + u, with e / (1 + e) at its largest
    over |v_hat - v| <= P (it falls as v grows); shared by silu and sigmoid"""
    e = torch.exp(-(v - P))
    return e_rel * e / (1 + e) + U * (1 + e_rel)


def silu(v, P):
    """silu_f(v_hat) = fl(v_hat / fl(1 + __expf(-v_hat))), |v_hat - v| <= P: (silu(v), bound).  Input error: SILU_DMAX P.  Evaluation at
    v_hat: e_hat = e (1 + fast_exp_rel), d = 1 + e has relative error e_rel e / (1 + e) + u, then the division."""
    ref = v * torch.sigmoid(v)
    prop = SILU_DMAX * P
    ed = _one_plus_exp_rel(v, P, fast_exp_rel(v.abs() + P))
    rel = (1 + ed / (1 - ed)) * (1 + DIV_REL) - 1
    return ref, prop + rel * (ref.abs() + prop) + FLUSH_ABS


def sigmoid(v, P):
    """fl(1 / fl(1 + expf(-v_hat))) with OCML's expf (|v| + P <= MATH_ARG_MAX): (sigmoid(v), bound); |sigmoid'| <= 1 / 4"""
    ref = torch.sigmoid(v)
    prop = 0.25 * P
    ed = _one_plus_exp_rel(v, P, EXPF_REL)
    rel = (1 + ed / (1 - ed)) * (1 + DIV_REL) - 1
    return ref, prop + rel * (ref + prop)


SOFTPLUS_THRESHOLD = 20.0


def softplus(v, P):
    """v_hat > 20 ? v_hat : log1pf(expf(v_hat)) (F.softplus, threshold 20): (ref, bound) with the threshold in the reference.
    |softplus'| <= 1: P.  e_hat = e (1 + EXPF_REL) moves log1p by at most e EXPF_REL / (1 + e) <= EXPF_REL min(e, 1); log1pf its own
    relative error.  Where |v - 20| <= P the two sides may take different branches: they differ by log1p(e^-20) < 2.1e-9 there."""
    e = torch.exp(v.clamp(max=SOFTPLUS_THRESHOLD + 1.0))
    lp = torch.log1p(e)
    ref = torch.where(v > SOFTPLUS_THRESHOLD, v, lp)
    b = P + EXPF_REL * e / (1 + e) + LOG1PF_REL * (lp + P)
    return ref, b + torch.where((v - SOFTPLUS_THRESHOLD).abs() <= P, 2.1e-9, 0.0)


def tanh(v, P):
    """tanhf(v_hat), |v| + P <= MATH_ARG_MAX: (tanh(v), bound); |tanh'| <= 1"""
    ref = torch.tanh(v)
    return ref, P + TANHF_REL * (ref.abs() + P)


def gelu_tanh(v, P):
    """gelu_tanh_f(v_hat) = 0.5f v (1 + tanhf(c0 (v + c1 v v v))) with the fp32 literals c0, c1: (ref, bound).  The argument of tanh:
    three products, a sum of two terms of equal sign and a product -- gamma(5) relative, at most XSECH2_MAX gamma(5) on tanh; tanhf its
    own error; 1 + t one rounding; 0.5f v is exact, the last product one rounding.  Input error: GELU_TANH_DMAX P."""
    c0, c1 = F32(0.7978845608028654), F32(0.044715)
    t = torch.tanh(c0 * (v + c1 * v * v * v))
    ref = 0.5 * v * (1 + t)
    dt = XSECH2_MAX * gamma(5) + TANHF_REL * (t.abs() + XSECH2_MAX * gamma(5))
    prop = GELU_TANH_DMAX * P
    ev = 0.5 * (v.abs() + P) * (dt + U * (1 + t + dt + P))          # evaluated at v_hat: |v_hat| <= |v| + P, t_hat <= t + P
    return ref, prop + ev + U * (ref.abs() + prop + ev)


def normalize4(v, P):
    """F.normalize of rows v [..., 4] carrying errors P: g = fl(v_hat fl(1 / max(sqrtf(n2), 1e-12f))), n2 the fp32 sum of four squares.
    The norm n is 1-Lipschitz in v, so the input errors move it by at most |P|_2; n2 (four squares, three additions) carries a
    relative error x = gamma(5), which the square root halves (x / (2 (1 - x))), then SQRTF_REL: dn in all.  max(., 1e-12f) does not
    increase it; the reciprocal DIV_REL, the product one rounding.  A row of exact zeros (P = 0) gives 0 / 1e-12 = 0 with bound 0."""
    n = v.pow(2).sum(-1, keepdim=True).sqrt()
    pn = P.pow(2).sum(-1, keepdim=True).sqrt() if torch.is_tensor(P) else torch.zeros_like(n)
    x = gamma(5)
    dn = pn + (n + pn) * ((1 + x / (2 * (1 - x))) * (1 + SQRTF_REL) - 1)
    m = n.clamp_min(F32(1e-12))
    rho_m = dn / (m - dn).clamp_min(1e-300)
    rho = (1 + rho_m) * (1 + DIV_REL) - 1
    ref = v / m
    b = (P * (1 + rho) + v.abs() * rho) / m
    return ref, b + U * (ref.abs() + b)


def sincos_arg(t, j):
    """arg = fl(t fr_j), fr_j = expf(fl(fl(-c32 j) / 128)) against t exp(-ln(10000) j / 128): (ref, P).  The exponent a = ln(10000) j / 128
    <= 9.21 carries the literal's relative error and one rounding (/ 128 is exact); expf then EXPF_FREQ_REL; the product one rounding.
    t [B, 1], j [128] float64."""
    c = math.log(10000.0)
    dc = abs(F32(9.210340371976184) - c) / c
    a = c * j / 128.0
    f_rel = torch.exp(a * (dc + U)) * (1 + EXPF_FREQ_REL) - 1
    ref = t * torch.exp(-a)
    return ref, ref.abs() * ((1 + f_rel) * (1 + U) - 1)


def sin_cos(arg, P):
    """(cos ref, cos bound, sin ref, sin bound) of cosf / sinf(arg_hat), |arg_hat - arg| <= P, |arg| <= 1024: both 1-Lipschitz"""
    c, s = torch.cos(arg), torch.sin(arg)
    return c, P + COSF_REL * (c.abs() + P), s, P + SINF_REL * (s.abs() + P)


# ---------------------------------------------------------------------------------------------------------------------------------
# The denoiser's head and tail (dit_ops.hip: embed_tokens, final_layer, layernorm_rows, ctx_rmsnorm; tests/_headtail_cases.py).
def fl_add_sparse(a, Pa, b, Pb=0.0):
    """fl_add where an operand may be an exact zero: x + 0 is exact in fp32, so the rounding is counted only where both operands can be
    non-zero.  (The planted weights make most addends of a sum exact zeros; the bound then counts the roundings that can happen.)"""
    v = a + b
    Pa = Pa if torch.is_tensor(Pa) else torch.full_like(v, Pa)
    Pb = Pb if torch.is_tensor(Pb) else torch.full_like(v, Pb)
    P = Pa + Pb
    exact = ((a == 0) & (Pa == 0)) | ((b == 0) & (Pb == 0))
    return v, torch.where(exact.expand_as(v), P, P + U * (v.abs() + P))


def sparse_dot(x, dx, W, bias=None):
    """fl(bias + sum_k x_k W_nk) of mirrored operands x (each may deviate by dx >= 0) against exact weights W [N, K], in any order:
    products with an exact zero weight are exact zeros and adding them is exact, so a row of W with t non-zero entries costs t products
    (exact for bf16 operands, counted as one rounding each for the fp32 ones) and t additions: gamma(2 t) on the absolute sum, as
    `accumulation` counts it, with t in place of K.  Returns (ref, P)."""
    t = (W != 0).sum(-1).to(x.dtype)
    v = x @ W.T
    E = dx @ W.abs().T
    s = x.abs() @ W.abs().T + E
    if bias is not None:
        v, s, t = v + bias, s + bias.abs(), t + (bias != 0).to(x.dtype)
    g = 2 * t * U / (1 - 2 * t * U)
    return v, E + torch.where(t <= 1, torch.zeros_like(s), g * s)       # a single product of bf16 operands is exact


def pivoted_layernorm_stats(x, Px, eps):
    """final_layer_kernel: LayerNorm statistics in ONE reduction about the pivot p = x[0] of rows x_hat [..., D], |x_hat - x| <= Px:
      v = fl(x_hat - p_hat)                     |v_hat - (x - p)| <= Dv = Px + Px[0] + u (|x - p| + Px + Px[0])     (element 0: exactly 0)
      mean = fl(fl(sum v) / D)                  Dm = (1 + u) (sum Dv + gamma(D) sum (|v| + Dv)) / D + u |mean|
      q = fl(sum fl(v^2)),  var = fl(fl(q / D) - fl(mean^2)), clamped at 0 (the true variance is >= 0: the clamp only helps)
                                                dvar = dQ / D + d(mean^2) + gamma(3) (Q / D + mean^2 + their errors)
      A = fl(var + eps), rs = rsqrtf(A)         as layernorm_stats
      e = fl(v - mean)                          De = Dv + Dm + u (|e| + Dv + Dm)
    Q / D and mean^2 are of the size of the spread about the pivot, not of the common offset: that is what the pivot buys, and what
    the gamma(3) term charges an unpivoted kernel for.  Returns (e, De, r, rho)."""
    D = x.shape[-1]
    vv = x - x[..., :1]
    Dv = Px + Px[..., :1] + U * (vv.abs() + Px + Px[..., :1])
    Dv = torch.cat([torch.zeros_like(Dv[..., :1]), Dv[..., 1:]], -1)
    av = vv.abs() + Dv
    mu = vv.mean(-1, keepdim=True)
    Dm = (1 + U) * (Dv.sum(-1, keepdim=True) + gamma(D) * av.sum(-1, keepdim=True)) / D + U * mu.abs()
    e = vv - mu
    De = Dv + Dm + U * (e.abs() + Dv + Dm)
    m2 = vv.pow(2).mean(-1, keepdim=True)
    dm2 = ((2 * vv.abs() * Dv + Dv * Dv).sum(-1, keepdim=True) + gamma(D + 1) * av.pow(2).sum(-1, keepdim=True)) / D
    dmu2 = 2 * mu.abs() * Dm + Dm * Dm
    var = m2 - mu * mu
    dvar = dm2 + dmu2 + gamma(3) * (m2 + dm2 + mu * mu + dmu2)
    A = var + eps
    dA = dvar + U * (A + dvar)
    xa = dA / A
    assert bool((xa < 0.5).all()), "the statistics of a row are not determined to a factor of two: no bound"
    r = torch.rsqrt(A)
    rho = (1 + xa / (2 * (1 - xa))) * (1 + RSQRT_REL) - 1
    return e, De, r, rho
