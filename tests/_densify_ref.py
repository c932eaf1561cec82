"""Restatement of include/ga_densify.h in numpy float32, operation by operation (every product, quotient, sum and square root a
float32 operation of its own, in the written order).  Shared by tests/test_densify_cpu.py and tests/test_densify_gpu.py; nothing here
touches the device.  The normals of a split are float64 (tests/_sde_ref.py's Philox and Box-Muller with this kernel's counter layout):
the bit-exact comparisons feed ``densify`` the kernel's own ``noise_out``."""
import numpy as np

from tests import _sde_ref as sde

F = np.float32
KEPT, CLONE, SPLIT, PRUNED = 0, 1, 2, 3
PRUNE_ONLY = 1
THREADS, ROWS_PER_LANE = 256, 4                  # GA_DENSIFY_THREADS, GA_DENSIFY_ROWS_PER_LANE
BLOCK_ROWS = THREADS * ROWS_PER_LANE
STREAM = 0x44454E53                              # GA_DENSIFY_STREAM
LOG_1P6 = F(np.log(1.6))                         # GA_DENSIFY_LOG_1P6: rounded once from double


def accumulate(g_means, means, radii, view, tanfov, grad_accum, denom, max_radius):
    """one ga_fit_accumulate: g_means, means [N,3] float32, radii [V,N] int32, view [V,16] float32, the three statistics [N]
    -> the three statistics after it (new arrays)"""
    g, p, vm = np.asarray(g_means, F), np.asarray(means, F), np.asarray(view, F)
    radii = np.asarray(radii, np.int32)
    V, N = radii.shape
    c = np.zeros(N, np.int32)
    zsum = np.zeros(N, F)
    for v in range(V):
        vz = ((vm[v, 2] * p[:, 0] + vm[v, 6] * p[:, 1]) + vm[v, 10] * p[:, 2]) + vm[v, 14]
        vis = radii[v] > 0
        zsum = np.where(vis, zsum + vz, zsum).astype(F)
        c += vis
    with np.errstate(all="ignore"):
        zbar = zsum / np.maximum(c, 1).astype(F)
        norm = np.sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
        acc = np.asarray(grad_accum, F) + (norm * zbar) * F(tanfov)
    seen = c > 0
    rmax = np.maximum(radii.max(axis=0), 0)
    return (np.where(seen, acc, grad_accum).astype(F), np.where(seen, denom + 1, denom).astype(np.int32),
            np.where(seen, np.maximum(max_radius, rmax), max_radius).astype(np.int32))


def classify(opacities, scales, grad_accum, denom, max_radius, *, grad_threshold, min_opacity, percent_dense, extent,
             max_screen_size=0, flags=0):
    """-> codes [N] (KEPT, CLONE, SPLIT, PRUNED)"""
    opa, sc = np.asarray(opacities, F), np.asarray(scales, F)
    thr, mo, pd, ext, mss = F(grad_threshold), F(min_opacity), F(percent_dense), F(extent), F(max_screen_size)
    with np.errstate(all="ignore"):
        avg = np.where(np.asarray(denom) > 0, np.asarray(grad_accum, F) / np.asarray(denom).astype(F), F(0)).astype(F)
        avg = np.where(avg == avg, avg, F(0)).astype(F)
        smax = np.where(sc[:, 0] >= sc[:, 1], sc[:, 0], sc[:, 1])
        prune = opa < mo
        if mss > 0:
            prune = prune | (np.asarray(max_radius).astype(F) > mss) | (smax > F(0.1) * ext)
        selected = ~prune & (avg >= thr) & (not (flags & PRUNE_ONLY))
        small = smax <= pd * ext
    return np.where(prune, PRUNED, np.where(selected & small, CLONE, np.where(selected, SPLIT, KEPT))).astype(np.int32)


def tangents(rotations):
    """the tangent columns tu, tv [N,3] float32 of the rasterizer's preprocess from activated quaternions [N,4] (w, x, y, z)"""
    q = np.asarray(rotations, F)
    q0, q1, q2, q3 = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    qs = F(1) / np.sqrt(((q3 * q3 + q0 * q0) + q1 * q1) + q2 * q2)
    r, x, y, z = q0 * qs, q1 * qs, q2 * qs, q3 * qs
    two, one = F(2), F(1)
    tu = np.stack([one - two * (y * y + z * z), two * (x * y + r * z), two * (x * z - r * y)], 1)
    tv = np.stack([two * (x * y - r * z), one - two * (x * x + z * z), two * (y * z + r * x)], 1)
    return tu.astype(F), tv.astype(F)


def children(raw, scales, rotations, noise):
    """the two children of EVERY row as if it were split: raw [N,13], activated scales [N,2] and rotations [N,4], noise [N,4] float32
    -> [N,2,13] float32"""
    raw, sc, xi = np.asarray(raw, F), np.asarray(scales, F), np.asarray(noise, F)
    tu, tv = tangents(rotations)
    out = np.repeat(raw[:, None, :], 2, axis=1).copy()
    out[:, :, 4:6] = (raw[:, 4:6] - LOG_1P6)[:, None, :]
    for child in range(2):
        du, dv = sc[:, 0] * xi[:, 2 * child], sc[:, 1] * xi[:, 2 * child + 1]
        out[:, child, 0:3] = (raw[:, 0:3] + tu * du[:, None]) + tv * dv[:, None]
    return out


def densify(raw, m, v, act, stats, noise, *, flags=0, **params):
    """one ga_densify.  act: dict with the activated ``opacities`` [N], ``scales`` [N,2], ``rotations`` [N,4]; stats: (grad_accum,
    denom, max_radius); noise [N,4] float32 (the kernel's own noise_out, or ``normals`` rounded) -> dict of raw, m, v [N',13], parent
    [N'] int32, codes [N], kept, cloned, split, pruned, N_after"""
    raw, m, v = (np.asarray(t, F) for t in (raw, m, v))
    codes = classify(act["opacities"], act["scales"], *stats, flags=flags, **params)
    kids = children(raw, act["scales"], act["rotations"], noise)
    emitted = np.asarray([1, 2, 2, 0])[codes]
    parent = np.repeat(np.arange(len(codes)), emitted)
    first = np.cumsum(emitted) - emitted
    which = np.arange(len(parent)) - first[parent]                       # 0 or 1: the row's place among its parent's rows
    split = codes[parent] == SPLIT
    fresh = (split | (which == 1))[:, None]                              # rows that start with zero moments
    out_raw = np.where(split[:, None], kids[parent, which], raw[parent]).astype(F)
    out_m, out_v = np.where(fresh, F(0), m[parent]).astype(F), np.where(fresh, F(0), v[parent]).astype(F)
    return {"raw": out_raw.reshape(-1, 13), "m": out_m.reshape(-1, 13), "v": out_v.reshape(-1, 13), "parent": parent.astype(np.int32), "codes": codes,
            "kept": int((codes == KEPT).sum()), "cloned": int((codes == CLONE).sum()), "split": int((codes == SPLIT).sum()),
            "pruned": int((codes == PRUNED).sum()), "N_after": len(parent)}


def normals(seed, round_, n):
    """float64 [n,4]: the four normals of parent i are the two Box-Muller pairs of the Philox block at counter (i, round, STREAM, 0),
    key = the 64-bit seed"""
    seed &= (1 << 64) - 1
    full = lambda val: np.full(n, val & sde.MASK, dtype=np.uint32)   # noqa: E731
    w = sde.philox_np(np.arange(n, dtype=np.uint32), full(round_), full(STREAM), full(0), full(seed), full(seed >> 32))
    return sde.normals64(w).reshape(n, 4)


def expected_noise(codes, seed, round_):
    """what noise_out holds, in float64: the normals of the split parents, zeros elsewhere"""
    return np.where((np.asarray(codes) == SPLIT)[:, None], normals(seed, round_, len(codes)), 0.0)


def reset_opacity(raw, m, v, cap=0.01):
    raw, m, v = (np.asarray(t, F).copy() for t in (raw, m, v))
    logit = F(np.log(cap / (1.0 - cap)))
    raw[:, 3] = np.where(raw[:, 3] > logit, logit, raw[:, 3])
    m[:, 3] = 0
    v[:, 3] = 0
    return raw, m, v
