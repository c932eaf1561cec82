"""Restatement of ``ga_pc_align_points`` and ``ga_pc_icp`` (include/ga_pointcloud.h, csrc/pc_align.hip), operation by operation.

fp32 for the transformed point and the squared distance (``nearest_f32`` of tests/_pointcloud_ref.py is the match), float64 for the 19
terms, their sums in the stated tree and order, and the solve -- plain Python floats there, which are IEEE doubles with every operation
rounded on its own.  The device outputs must equal these BIT FOR BIT.  ``kabsch_f64`` is the independent reference the restatement
itself is checked against (weighted means, ``np.linalg.svd``, determinant correction, Umeyama scale).  pytorch3d is absent: parity
with it is UNPINNED."""
import math

import numpy as np

from tests._pointcloud_ref import dist2_f32, nearest_f32

F = np.float32
THREADS, TILE, TERMS, SWEEPS = 256, 1024, 19, 6          # kAlignThreads, kAlignTile, GA_PC_ALIGN_TERMS, GA_PC_ALIGN_SWEEPS
RUNNING, CONVERGED, DEGENERATE = 0, 1, 2
IDENTITY = np.array([1, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], F)
_PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def pack(R, T, s):
    return np.concatenate([[s], np.asarray(R).reshape(9), np.asarray(T).reshape(3)]).astype(F)


def apply_transform(x, tf):
    """xt_b = ((x_0 * R_0b + x_1 * R_1b) + x_2 * R_2b) * s + T_b in float32"""
    x, tf = np.asarray(x, F), np.asarray(tf, F)
    cols = []
    for b in range(3):
        a = x[:, 0] * tf[1 + b]
        a = a + x[:, 1] * tf[4 + b]
        a = a + x[:, 2] * tf[7 + b]
        a = a * tf[0]
        cols.append(a + tf[10 + b])
    out = np.stack(cols, 1)
    assert out.dtype == F
    return out


def terms(x, y, w, d2, groups):
    """the [groups * 256, 19] float64 terms of the live pairs (rows past them are exact zeros)"""
    n = x.shape[0]
    v = np.zeros((groups * THREADS, TERMS), np.float64)
    w, x, y = np.asarray(w, F).astype(np.float64), np.asarray(x, F).astype(np.float64), np.asarray(y, F).astype(np.float64)
    v[:n, 0] = w
    for a in range(3):
        wx = w * x[:, a]
        v[:n, 1 + a] = wx
        v[:n, 4 + a] = w * y[:, a]
        for b in range(3):
            v[:n, 7 + 3 * a + b] = wx * y[:, b]
    v[:n, 16] = w * ((x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2])
    v[:n, 17] = w * ((y[:, 0] * y[:, 0] + y[:, 1] * y[:, 1]) + y[:, 2] * y[:, 2])
    v[:n, 18] = w * np.asarray(d2, F).astype(np.float64)
    return v


def tree_sums(v, groups):
    """v[i] += v[i xor 2^l], l = 0 .. 7, inside every group of 256 rows; then the groups in ascending order -> [19] float64"""
    v = v.reshape(groups, THREADS, TERMS)
    lane = np.arange(THREADS)
    for l in range(8):
        v = v + v[:, lane ^ (1 << l), :]
    part = v[:, 0, :]
    total = part[0].copy()
    for g in range(1, groups):
        total = total + part[g]
    return total


def _rotate(A, V, p, q):
    apq = A[p][q]
    if apq == 0.0:
        return
    theta = (A[q][q] - A[p][p]) / (2.0 * apq)
    t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))   # theta * theta may be +inf: t = 0
    t = t if theta >= 0.0 else -t
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    h = t * apq
    A[p][p] = A[p][p] - h
    A[q][q] = A[q][q] + h
    A[p][q] = A[q][p] = 0.0
    for r in range(4):
        if r != p and r != q:
            rp, rq = A[r][p], A[r][q]
            A[r][p] = A[p][r] = c * rp - s * rq
            A[r][q] = A[q][r] = s * rp + c * rq
    for k in range(4):
        vp, vq = V[k][p], V[k][q]
        V[k][p] = c * vp - s * vq
        V[k][q] = s * vp + c * vq


def horn_rotation(M, sweeps=SWEEPS):
    """M [3][3] (floats) -> R [3][3] of the row-vector convention, float64 (not yet rounded)"""
    A = [[0.0] * 4 for _ in range(4)]
    A[0][0] = (M[0][0] + M[1][1]) + M[2][2]
    A[1][1] = (M[0][0] - M[1][1]) - M[2][2]
    A[2][2] = (M[1][1] - M[0][0]) - M[2][2]
    A[3][3] = (M[2][2] - M[0][0]) - M[1][1]
    A[0][1] = A[1][0] = M[1][2] - M[2][1]
    A[0][2] = A[2][0] = M[2][0] - M[0][2]
    A[0][3] = A[3][0] = M[0][1] - M[1][0]
    A[1][2] = A[2][1] = M[0][1] + M[1][0]
    A[1][3] = A[3][1] = M[2][0] + M[0][2]
    A[2][3] = A[3][2] = M[1][2] + M[2][1]
    V = [[1.0 if r == c else 0.0 for c in range(4)] for r in range(4)]
    for _ in range(sweeps):
        for p, q in _PAIRS:
            _rotate(A, V, p, q)
    best = 0
    for c in range(1, 4):
        if A[c][c] > A[best][best]:
            best = c
    q0, q1, q2, q3 = (V[k][best] for k in range(4))
    n = math.sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3)
    w, x, y, z = q0 / n, q1 / n, q2 / n, q3 / n
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    return [[1.0 - 2.0 * (yy + zz), 2.0 * (xy + wz), 2.0 * (xz - wy)],
            [2.0 * (xy - wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz + wx)],
            [2.0 * (xz + wy), 2.0 * (yz - wx), 1.0 - 2.0 * (xx + yy)]]


def solve(S, estimate_scale, sweeps=SWEEPS, rounded=True):
    """the sums [19] -> (transform [13] float32 or None when degenerate, rmse float64 (0 when W is not positive), W > 0)"""
    S = [float(v) for v in S]
    W = S[0]
    if not W > 0.0:
        return None, 0.0, False
    rmse = math.sqrt(S[18] / W)
    xm = [S[1 + a] / W for a in range(3)]
    ym = [S[4 + a] / W for a in range(3)]
    M = [[S[7 + 3 * a + b] / W - xm[a] * ym[b] for b in range(3)] for a in range(3)]
    vx = S[16] / W - ((xm[0] * xm[0] + xm[1] * xm[1]) + xm[2] * xm[2])
    if estimate_scale and not vx > (S[16] / W) * 2.0 ** -40:
        return None, rmse, True
    R = horn_rotation(M, sweeps)
    s = 1.0
    if estimate_scale:
        tr = 0.0
        for a in range(3):
            for b in range(3):
                tr = tr + R[a][b] * M[a][b]
        s = tr / vx
    T = [ym[b] - s * ((xm[0] * R[0][b] + xm[1] * R[1][b]) + xm[2] * R[2][b]) for b in range(3)]
    tf = np.array([s] + [R[a][b] for a in range(3) for b in range(3)] + T, np.float64)
    return (tf.astype(F) if rounded else tf), rmse, True


def groups_of(N):
    return -(-N // THREADS)


def align_points(x, y, weights=None, lengths=None, estimate_scale=False, sweeps=SWEEPS):
    """[B,N,3] pairs -> dict(transform [B,13] f32, rmse [B] f32, status [B] i32)"""
    x, y = np.asarray(x, F), np.asarray(y, F)
    B, N, _ = x.shape
    G = groups_of(N)
    out = dict(transform=np.tile(IDENTITY, (B, 1)), rmse=np.zeros(B, F), status=np.zeros(B, np.int32))
    for b in range(B):
        n = N if lengths is None else min(max(int(lengths[b]), 0), N)
        w = np.ones(n, F) if weights is None else np.asarray(weights[b, :n], F)
        S = tree_sums(terms(x[b, :n], y[b, :n], w, dist2_f32(x[b, :n], y[b, :n]), G), G)
        tf, rmse, _ = solve(S, estimate_scale, sweeps)
        out["rmse"][b] = F(rmse)
        if tf is None:
            out["status"][b] = DEGENERATE
        else:
            out["transform"][b] = tf
    return out


def match_pass(x, y, w, tf, gate2, G):
    """one match pass of one cloud under transform tf -> (sums [19], xt, idx, d2)"""
    xt = apply_transform(x, tf)
    n = x.shape[0]
    if y.shape[0] == 0:
        return np.zeros(TERMS), xt, np.full(n, -1, np.int64), np.full(n, np.inf, F)
    d2, idx = nearest_f32(xt, y)
    wg = w.copy()
    if gate2 is not None:
        wg[d2 > gate2] = 0
    return tree_sums(terms(x, y[idx], wg, d2, G), G), xt, idx, d2


def icp(x, y, x_lengths=None, y_lengths=None, weights=None, init_transform=None, max_iterations=100, relative_rmse_thr=1e-6,
        estimate_scale=False, max_distance=0.0, sweeps=SWEEPS):
    """-> dict(transform [B,13], rmse [B], status [B], iterations [B], history [B,max_iterations+1,14], xt [B,N,3], idx [B,N], dist2 [B,N])"""
    x, y = np.asarray(x, F), np.asarray(y, F)
    B, N, _ = x.shape
    Nt = y.shape[1]
    G = groups_of(N)
    thr = float(F(relative_rmse_thr))
    gate2 = F(max_distance) * F(max_distance) if max_distance > 0 else None
    out = dict(transform=np.tile(IDENTITY, (B, 1)) if init_transform is None else np.array(init_transform, F).reshape(B, 13),
               rmse=np.zeros(B, F), status=np.zeros(B, np.int32), iterations=np.zeros(B, np.int32),
               history=np.zeros((B, max_iterations + 1, 14), F), xt=np.zeros((B, N, 3), F), idx=np.full((B, N), -1, np.int32),
               dist2=np.zeros((B, N), F))
    for b in range(B):
        n = N if x_lengths is None else min(max(int(x_lengths[b]), 0), N)
        m = Nt if y_lengths is None else min(max(int(y_lengths[b]), 0), Nt)
        xb, yb = x[b, :n], y[b, :m]
        w = np.ones(n, F) if weights is None else np.asarray(weights[b, :n], F).copy()
        tf, prev, status, its = out["transform"][b].copy(), 0.0, RUNNING, 0
        for k in range(max_iterations + 1):
            final = k == max_iterations
            if status != RUNNING and not final:
                continue
            S, xt, idx, d2 = match_pass(xb, yb, w, tf, gate2, G)
            if final:
                out["xt"][b, :n], out["idx"][b, :n], out["dist2"][b, :n] = xt, idx, d2
            if status != RUNNING:
                out["history"][b, its + 1:] = out["history"][b, its]
                continue
            new, rmse, has_weight = solve(S, estimate_scale, sweeps)
            out["rmse"][b] = F(rmse)
            out["history"][b, k, :13], out["history"][b, k, 13] = tf, F(rmse)
            if not has_weight:
                status = DEGENERATE
            elif k >= 1 and abs(prev - rmse) <= thr * prev:
                status = CONVERGED
            elif final:
                pass
            elif new is None:
                status = DEGENERATE
            else:
                tf, prev, its = new, rmse, its + 1
        out["transform"][b], out["status"][b], out["iterations"][b] = tf, status, its
    return out


def kabsch_f64(x, y, w=None, estimate_scale=False):
    """the independent float64 reference: -> (R [3,3], T [3], s) of Xt = s * X @ R + T, no reflection"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    w = np.ones(len(x)) if w is None else np.asarray(w, np.float64)
    W = w.sum()
    xm, ym = (w[:, None] * x).sum(0) / W, (w[:, None] * y).sum(0) / W
    xc, yc = x - xm, y - ym
    cov = (w[:, None] * xc).T @ yc / W
    U, sv, Vt = np.linalg.svd(cov)
    E = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        E[2] = -1
    R = (U * E) @ Vt
    s = (sv * E).sum() / ((w * (xc ** 2).sum(1)).sum() / W) if estimate_scale else 1.0
    return R, ym - s * xm @ R, s


def residual_f64(x, y, w, R, T, s):
    """sum of w * |s * x @ R + T - y|^2 in float64"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    w = np.ones(len(x)) if w is None else np.asarray(w, np.float64)
    return float((w * ((s * x @ np.asarray(R, np.float64) + np.asarray(T, np.float64) - y) ** 2).sum(1)).sum())


def bumpy_ellipsoid(m):
    """the ICP target: a Fibonacci sphere of m points scaled by (0.4, 0.25, 0.15) plus 0.02 * sin(7 * p[:, [1, 2, 0]])"""
    i = np.arange(m) + 0.5
    phi = np.arccos(1 - 2 * i / m)
    th = np.pi * (1 + 5 ** 0.5) * i
    p = np.stack([np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)], 1) * np.array([0.4, 0.25, 0.15])
    return (p + 0.02 * np.sin(7 * p[:, [1, 2, 0]])).astype(F)


def rotation(axis, angle):
    """Rodrigues, float64, row-vector convention: x @ R rotates x by `angle` about `axis`"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K).T


def moved(y, R, T, s):
    """x with s * x @ R + T = y, computed in float64 and rounded to float32"""
    return (((np.asarray(y, np.float64) - T) / s) @ np.asarray(R).T).astype(F)


def well_conditioned_problems():
    """the test set of tests/test_align_cpu.py: (x, y, w, estimate_scale) with corresponding rows -- 3 .. 200 Gaussian points (never
    collinear), a random similarity, noise 0 / 1e-3 / 0.3 on y, random weights"""
    rng = np.random.default_rng(20240607)
    out = []
    for noise in (0.0, 1e-3, 0.3):
        for n in (3, 4, 5, 7, 10, 16, 33, 64, 100, 200):
            for scale in (False, True):
                for _ in range(2):
                    x = rng.normal(size=(n, 3)).astype(F)
                    R = rotation(rng.normal(size=3), rng.uniform(0.0, 3.0))
                    s = rng.uniform(0.5, 2.0) if scale else 1.0
                    y = (s * x.astype(np.float64) @ R + rng.normal(size=3) + noise * rng.normal(size=(n, 3))).astype(F)
                    out.append((x, y, rng.uniform(0.1, 1.0, size=n).astype(F), scale))
    return out


def degenerate_problems():
    """planar and collinear sets (the rotation about a line of points is not unique): (x, y, w, estimate_scale)"""
    rng = np.random.default_rng(20240608)
    out = []
    for kind in ("planar", "collinear"):
        for n in (3, 8, 50, 200):
            for noise in (0.0, 1e-3):
                for scale in (False, True):
                    p = rng.normal(size=(n, 3))
                    p[:, 2] = 0.0
                    if kind == "collinear":
                        p[:, 1] = 0.0
                    x = (p @ rotation(rng.normal(size=3), rng.uniform(0.0, 3.0)) + rng.normal(size=3)).astype(F)
                    R = rotation(rng.normal(size=3), rng.uniform(0.0, 3.0))
                    s = rng.uniform(0.5, 2.0) if scale else 1.0
                    y = (s * x.astype(np.float64) @ R + rng.normal(size=3) + noise * rng.normal(size=(n, 3))).astype(F)
                    out.append((x, y, rng.uniform(0.1, 1.0, size=n).astype(F), scale))
    return out
