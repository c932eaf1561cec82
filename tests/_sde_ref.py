"""Restatements the SDE sampler tests compare against (include/ga_dit.h: GaSdeStep / ga_sde_step, csrc/ode_sde.hip):

* Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) written twice, independently: with
  Python integers and explicit rounds, and vectorised over numpy uint32 / uint64 arrays;
* the words -> normals transform of the header in float64;
* every phase of ga_sde_step in numpy float32, operation by operation (numpy rounds every float32 operation on its own)."""
import math

import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
(EM, HEUN_PERTURB, HEUN_PREDICT, HEUN_CORRECT, LAST_MEAN, LAST_TWEEDIE, LAST_EULER, LAST_NONE, ADVANCE) = range(9)
(C_T, C_DT, C_SQRT_DT, C_W, C_G, C_R, C_VAR, C_T2, C_W2, C_R2, C_VAR2, C_HALF_DT, C_ALPHA, C_SIG2A) = range(14)
STRIDE = 16


def philox_int(counter, key):
    """one block with Python integers: counter (c0, c1, c2, c3), key (k0, k1) -> four 32-bit words"""
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        hi0, lo0, hi1, lo1 = p0 >> 32, p0 & MASK, p1 >> 32, p1 & MASK
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def _mulhilo(a, b):
    """32 x 32 -> (hi, lo) words from 16-bit limbs in uint32 / uint64 arrays (no 64-bit product of the operands is formed)"""
    a = a.astype(np.uint64)
    al, ah = a & np.uint64(0xFFFF), a >> np.uint64(16)
    bl, bh = np.uint64(b & 0xFFFF), np.uint64(b >> 16)
    ll, lh, hl, hh = al * bl, al * bh, ah * bl, ah * bh
    mid = (ll >> np.uint64(16)) + (lh & np.uint64(0xFFFF)) + (hl & np.uint64(0xFFFF))
    lo = ((mid & np.uint64(0xFFFF)) << np.uint64(16)) | (ll & np.uint64(0xFFFF))
    hi = hh + (lh >> np.uint64(16)) + (hl >> np.uint64(16)) + (mid >> np.uint64(16))
    return hi.astype(np.uint32), lo.astype(np.uint32)


def philox_np(c0, c1, c2, c3, k0, k1):
    """vectorised: uint32 arrays of equal length -> uint32 [len, 4]"""
    c0, c1, c2, c3, k0, k1 = (np.asarray(v, dtype=np.uint32).copy() for v in (c0, c1, c2, c3, k0, k1))
    for r in range(10):
        hi0, lo0 = _mulhilo(c0, M0)
        hi1, lo1 = _mulhilo(c2, M1)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = ((k0.astype(np.uint64) + np.uint64(W0)) & np.uint64(MASK)).astype(np.uint32)
        k1 = ((k1.astype(np.uint64) + np.uint64(W1)) & np.uint64(MASK)).astype(np.uint32)
    return np.stack([c0, c1, c2, c3], 1)


def words(seed, step, stream, n):
    """the uint32 words of the draws 0 .. n - 1: block j / 4 at counter (j / 4, step, stream, 0), key = the 64-bit seed -> [ceil(n / 4), 4]"""
    nb = (n + 3) // 4
    seed &= (1 << 64) - 1
    full = lambda v: np.full(nb, v & MASK, dtype=np.uint32)  # noqa: E731
    return philox_np(np.arange(nb, dtype=np.uint32), full(step), full(stream), full(0), full(seed), full(seed >> 32))


def normals64(w):
    """uint32 [nb, 4] -> float64 [nb * 4]: two Box-Muller pairs per block, 24-bit uniforms, u1 in (0, 1], u2 in [0, 1)"""
    w = w.astype(np.uint64)
    u1 = ((w[:, 0::2] >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    u2 = (w[:, 1::2] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    radius = np.sqrt(-2.0 * np.log(u1))
    theta = 2.0 * math.pi * u2
    return np.stack([radius * np.cos(theta), radius * np.sin(theta)], 2).reshape(-1)


def normals(seed, step, stream, n):
    return normals64(words(seed, step, stream, n))[:n]


def table(rng, ni):
    """a random, well-conditioned coefficient table [ni + 1, STRIDE] float32 (the phases only read it)"""
    c = rng.uniform(0.1, 1.5, size=(ni + 1, STRIDE)).astype(np.float32)
    return c


def _drift(row, v, x, late=False):
    w, r, var = (row[C_W2], row[C_R2], row[C_VAR2]) if late else (row[C_W], row[C_R], row[C_VAR])
    score = (r * v - x) / var
    return v + w * score, score


def spread(xi, n, pairs):
    """the per-element normals from the n_draw drawn ones"""
    return np.concatenate([xi, xi]) if pairs else xi


def phase(p, row, x, v, xhat, k1, xi):
    """float32 arrays in, dict of the buffers the phase writes out (state / xhat / k1 / slot)"""
    f = np.float32
    row = row.astype(f)
    if p == EM:
        drift, _ = _drift(row, v, x)
        mean = x + drift * row[C_DT]
        xn = mean + row[C_G] * (xi * row[C_SQRT_DT])
        return {"state": xn, "slot": xn}
    if p == HEUN_PERTURB:
        return {"xhat": x + row[C_G] * (xi * row[C_SQRT_DT])}
    if p == HEUN_PREDICT:
        kk, _ = _drift(row, v, xhat)
        return {"k1": kk, "state": xhat + row[C_DT] * kk}
    if p == HEUN_CORRECT:
        k2, _ = _drift(row, v, x, late=True)
        xn = xhat + row[C_HALF_DT] * (k1 + k2)
        return {"state": xn, "slot": xn}
    if p == LAST_MEAN:
        drift, _ = _drift(row, v, x)
        return {"slot": x + drift * row[C_DT]}
    if p == LAST_TWEEDIE:
        _, score = _drift(row, v, x)
        return {"slot": x / row[C_ALPHA] + row[C_SIG2A] * score}
    if p == LAST_EULER:
        return {"slot": x + v * row[C_DT]}
    if p == LAST_NONE:
        return {"slot": x.copy()}
    raise ValueError(p)
