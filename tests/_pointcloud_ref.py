"""Restatements of farthest point sampling and nearest point for the tests of include/ga_pointcloud.h.

``fps_f32`` / ``nearest_f32`` follow the arithmetic contract of the header operation by operation in numpy float32 (dx*dx, + dy*dy,
+ dz*dz, each rounded on its own; first index at ties) -- the HIP kernels must reproduce them bit for bit.  ``fps_f64`` /
``nearest_f64`` are brute force in float64, written independently (explicit loops over the tie rule rather than ``argmax``): on
dyadic lattice clouds, where every fp32 operation is exact, the two must agree index for index, which pins the tie rule of the
fp32 restatement without trusting it.  pytorch3d itself is absent: parity with it is UNPINNED ('Point clouds')."""
import numpy as np


def dist2_f32(p, q):
    """[N,3] float32 points against one point (or [N,3] against [N,3]) -> [N] float32, contract order"""
    p = np.asarray(p, np.float32)
    q = np.asarray(q, np.float32)
    dx = p[..., 0] - q[..., 0]
    dy = p[..., 1] - q[..., 1]
    dz = p[..., 2] - q[..., 2]
    d = dx * dx
    d = d + dy * dy
    d = d + dz * dz
    assert d.dtype == np.float32
    return d


def fps_f32(points, K, start=0):
    """One cloud [n,3] -> int64 [min(K, n)] indices.  (Coordinate columns and scratch arrays are allocated once: the loop is the
    contract's operations and nothing else, every array float32.)"""
    p = np.ascontiguousarray(points, np.float32)
    n = p.shape[0]
    m = min(int(K), n)
    x, y, z = (np.ascontiguousarray(p[:, a]) for a in range(3))
    closest = np.full(n, np.inf, np.float32)
    d, t = np.empty(n, np.float32), np.empty(n, np.float32)
    out = np.empty(m, np.int64)
    sel = int(start)
    for k in range(m):
        out[k] = sel
        if k + 1 == m:
            break
        np.subtract(x, x[sel], out=d)
        np.multiply(d, d, out=d)            # d = dx*dx
        np.subtract(y, y[sel], out=t)
        np.multiply(t, t, out=t)
        np.add(d, t, out=d)                 # d = d + dy*dy
        np.subtract(z, z[sel], out=t)
        np.multiply(t, t, out=t)
        np.add(d, t, out=d)                 # d = d + dz*dz
        np.minimum(closest, d, out=closest)
        sel = int(np.argmax(closest))       # the first index attaining the maximum
    return out


def fps_f64(points, K, start=0):
    p = np.asarray(points, np.float64)
    n = p.shape[0]
    m = min(int(K), n)
    closest = np.full(n, np.inf)
    out = []
    sel = int(start)
    for k in range(m):
        out.append(sel)
        closest = np.minimum(closest, ((p - p[sel]) ** 2).sum(1))
        best = closest.max()
        sel = int(np.flatnonzero(closest == best)[0])   # the lowest index among the farthest
    return np.asarray(out, np.int64)


def fps_padded(points, lengths, K, starts, fn=fps_f32):
    """A padded batch [B,N,3] -> (idx [B,K] int64 with -1 padding, points [B,K,3] float32 with zero padding)"""
    B = points.shape[0]
    idx = np.full((B, K), -1, np.int64)
    pts = np.zeros((B, K, 3), np.float32)
    for b in range(B):
        got = fn(points[b, :lengths[b]], K, starts[b])
        idx[b, :len(got)] = got
        pts[b, :len(got)] = points[b, got]
    return idx, pts


def nearest_f32(query, target, chunk=256):
    """[Nq,3], [Nt,3] -> (dist2 [Nq] float32, idx [Nq] int64, the first index at ties)"""
    q = np.ascontiguousarray(query, np.float32)
    t = np.ascontiguousarray(target, np.float32)
    d2 = np.empty(q.shape[0], np.float32)
    idx = np.empty(q.shape[0], np.int64)
    for s in range(0, q.shape[0], chunk):
        d = dist2_f32(q[s:s + chunk, None, :], t[None, :, :])
        i = np.argmin(d, axis=1)
        idx[s:s + chunk] = i
        d2[s:s + chunk] = d[np.arange(d.shape[0]), i]
    return d2, idx


def nearest_f64(query, target, chunk=256):
    q = np.asarray(query, np.float64)
    t = np.asarray(target, np.float64)
    d2 = np.empty(q.shape[0])
    idx = np.empty(q.shape[0], np.int64)
    for s in range(0, q.shape[0], chunk):
        d = ((q[s:s + chunk, None, :] - t[None, :, :]) ** 2).sum(-1)
        best = d.min(1)
        for r in range(d.shape[0]):
            idx[s + r] = np.flatnonzero(d[r] == best[r])[0]
        d2[s:s + chunk] = best
    return d2, idx


def chamfer_f64(x, y, point_reduction="mean"):
    """One pair of clouds, squared L2, both directions added (pytorch3d.loss.chamfer_distance without normals)"""
    dx, _ = nearest_f64(x, y)
    dy, _ = nearest_f64(y, x)
    return (dx.mean() + dy.mean()) if point_reduction == "mean" else (dx.sum() + dy.sum())


def lattice_cloud(n, seed, distinct=None):
    """Dyadic lattice cloud: coordinates k/64 with |k| <= 32 -- differences are multiples of 1/64 up to 1, squares multiples of 2^-12
    up to 1, sums of three below 4: every operation of the contract is exact in fp32.  ``distinct``: draw the n points from that many
    lattice points, so that about n - distinct are duplicates."""
    rng = np.random.default_rng(seed)
    if distinct is None:
        k = rng.integers(-32, 33, size=(n, 3))
    else:
        k = rng.integers(-32, 33, size=(distinct, 3))[rng.integers(0, distinct, size=n)]
    return (k / 64.0).astype(np.float32)


def uniform_cloud(shape, seed):
    return np.random.default_rng(seed).uniform(-0.45, 0.45, size=tuple(shape) + (3,)).astype(np.float32)
