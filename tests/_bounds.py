"""Element-wise error bounds of the bf16-MFMA kernels against a float64 reference computed from the exact bf16 / fp32 values the
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
