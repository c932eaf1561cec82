"""Restatements of ``ga_pc_normals`` and ``ga_pc_surfel_init`` (include/ga_pointcloud.h, csrc/pc_normals.hip) and the clouds their tests
share.

``normals_f32`` and ``surfel_init_f32`` follow the header's operation order in numpy float32, every operation rounded on its own: the
HIP kernels must reproduce them bit for bit.  ``normals_f64`` is the float64 yardstick: the covariance over the same neighbour lists
in float64 and ``np.linalg.eigh``.  ``rasterizer_frame`` is the quaternion -> matrix formula of csrc/surfel_preprocess.hip:51-55.

Neither Open3D nor pytorch3d is on the machine: the definitions (sign rule, invalid rows, frame) are the project's own and nothing
here pins them to another library."""
import functools

import numpy as np

from tests._knn_ref import knn_f32

F = np.float32
SWEEPS = 5           # GA_PC_NORMALS_SWEEPS of include/ga_pointcloud.h
PAIRS = ((0, 1), (0, 2), (1, 2))
INVALID_NORMAL, INVALID_TANGENT = (0.0, 0.0, 1.0), (1.0, 0.0, 0.0)
# The bars of the comparison with float64: 4 x the largest value ``normals_f32`` (5 sweeps) reaches on ``clouds()`` at K = 8 and K = 16
# over the restatement's own lists (tests/test_normals_cpu.py prints the figures); the margin covers another libm or numpy build.
BAR_NORMAL = 4 * 1.761e-7    # sin(angle to the float64 eigenvector) * its eigen-gap / lam2; largest measured 1.761e-7 (sphere, K = 16)
BAR_LAMBDA = 4 * 2.827e-7    # |eigenvalue - float64 eigenvalue| / lam2; largest measured 2.827e-7 (sphere, K = 16)


# ---- the clouds ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clouds(n=2048):
    """-> {'sphere', 'plane', 'cube'}: float32 [n,3] each, read-only; one ``np.random.default_rng(0)`` drawn from in that order"""
    rng = np.random.default_rng(0)
    i = np.arange(n, dtype=np.float64) + 0.5
    phi = np.arccos(1.0 - 2.0 * i / n)
    theta = np.pi * (1.0 + 5.0 ** 0.5) * i
    sphere = 0.5 * np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], 1)
    xy = rng.uniform(-0.5, 0.5, size=(n, 2))
    plane = np.concatenate([xy, (0.3 * xy[:, 0] - 0.2 * xy[:, 1] + 0.1 + rng.normal(0.0, 2e-3, size=n))[:, None]], 1)
    face = rng.integers(0, 6, size=n)
    uv = rng.uniform(0.0, 1.0, size=(n, 2))
    cube = np.empty((n, 3))
    for a in range(3):          # faces 2a (coordinate a = 0) and 2a + 1 (coordinate a = 1) of the unit cube
        on = face // 2 == a
        cube[on, a] = (face[on] % 2).astype(np.float64)
        cube[on, (a + 1) % 3], cube[on, (a + 2) % 3] = uv[on, 0], uv[on, 1]
    out = {"sphere": sphere.astype(F), "plane": plane.astype(F), "cube": cube.astype(F)}
    for v in out.values():
        v.setflags(write=False)
    return out


def cloud_with_copies(n=300, first=100, copies=40, seed=3):
    """``n`` uniform points, rows first .. first + copies - 1 replaced by one point with dyadic coordinates: the partial sums k * x of
    the centroid are exact, so a list of copies has a covariance trace of exactly 0"""
    p = np.random.default_rng(seed).uniform(-0.5, 0.5, size=(n, 3)).astype(F)
    p[first:first + copies] = np.array([0.25, -0.125, 0.375], F)
    return p


def self_knn(points, K):
    """kNN of one cloud [n,3] against itself by the fp32 restatement -> (dist2 [n,min(K,n)] float32, idx int64)"""
    return knn_f32(points, points, K)


# ---- ga_pc_normals -----------------------------------------------------------------------------------------------------------------------
def _norm3(x, y, z):
    return np.sqrt((x * x + y * y) + z * z)


def covariance_f32(points, idx, n, K):
    """centroid and the six covariance terms of rows 0 .. n-1 over m = min(K, n) neighbours in list order -> (trace, A dict)"""
    p = np.ascontiguousarray(points, F)
    m = min(int(K), int(n))
    j = np.clip(np.asarray(idx[:n, :m], np.int64), 0, max(n - 1, 0))
    fm = F(m)
    s = [np.zeros(n, F) for _ in range(3)]
    for k in range(m):
        for a in range(3):
            s[a] = s[a] + p[j[:, k], a]
    c = [s[a] / fm for a in range(3)]
    A = {key: np.zeros(n, F) for key in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))}
    for k in range(m):
        d = [p[j[:, k], a] - c[a] for a in range(3)]
        for (a, b) in A:
            A[(a, b)] = A[(a, b)] + d[a] * d[b]
    for key in A:
        A[key] = A[key] / fm
        assert A[key].dtype == F
    return (A[(0, 0)] + A[(1, 1)]) + A[(2, 2)], A


def jacobi_f32(A, sweeps=SWEEPS, trace_off=None):
    """cyclic Jacobi on the symmetric 3x3 held as six float32 arrays -> (lam [3 arrays], V[k][c] arrays: column c is eigenvector c),
    unsorted.  ``trace_off``: a list that receives max |off-diagonal| / max |diagonal| after every sweep (for choosing ``sweeps``)."""
    A = {k: v.copy() for k, v in A.items()}
    n = A[(0, 0)].shape[0]
    one, zero = np.ones(n, F), np.zeros(n, F)
    V = [[one.copy() if k == c else zero.copy() for c in range(3)] for k in range(3)]
    key = lambda a, b: (min(a, b), max(a, b))
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p, q in PAIRS:
                r = 3 - p - q
                apq = A[(p, q)]
                rot = apq != 0
                theta = (A[(q, q)] - A[(p, p)]) / (F(2) * apq)
                t = F(1) / (np.abs(theta) + np.sqrt(theta * theta + F(1)))
                t = np.where(theta >= 0, t, -t)
                c = F(1) / np.sqrt(t * t + F(1))
                s = t * c
                h = t * apq
                arp, arq = A[key(r, p)], A[key(r, q)]
                new = {(p, p): A[(p, p)] - h, (q, q): A[(q, q)] + h, (p, q): zero,
                       key(r, p): c * arp - s * arq, key(r, q): s * arp + c * arq}
                for kk, val in new.items():
                    A[kk] = np.where(rot, val, A[kk]).astype(F)
                for k in range(3):
                    vp, vq = V[k][p], V[k][q]
                    V[k][p] = np.where(rot, c * vp - s * vq, vp).astype(F)
                    V[k][q] = np.where(rot, s * vp + c * vq, vq).astype(F)
            if trace_off is not None:
                off = np.maximum(np.maximum(np.abs(A[(0, 1)]), np.abs(A[(0, 2)])), np.abs(A[(1, 2)])).astype(np.float64)
                dia = np.maximum(np.maximum(np.abs(A[(0, 0)]), np.abs(A[(1, 1)])), np.abs(A[(2, 2)])).astype(np.float64)
                trace_off.append(float(np.max(off / dia)))
    return [A[(0, 0)], A[(1, 1)], A[(2, 2)]], V


def _sorted_ascending(lam, V):
    """the stable three-element sort of the header: compare-and-swap (0,1), (1,2), (0,1), swapping only on a strict 'greater'"""
    lam = list(lam)
    cols = [[V[k][c] for k in range(3)] for c in range(3)]
    for i, j in ((0, 1), (1, 2), (0, 1)):
        sw = lam[i] > lam[j]
        lam[i], lam[j] = np.where(sw, lam[j], lam[i]), np.where(sw, lam[i], lam[j])
        for k in range(3):
            cols[i][k], cols[j][k] = np.where(sw, cols[j][k], cols[i][k]), np.where(sw, cols[i][k], cols[j][k])
    return lam, cols


def _unit_with_default_sign(v):
    x, y, z = v
    l = _norm3(x, y, z)
    x, y, z = x / l, y / l, z / l
    big, ab = x, np.abs(x)
    sel = np.abs(y) > ab
    big, ab = np.where(sel, y, big), np.where(sel, np.abs(y), ab)
    sel = np.abs(z) > ab
    big = np.where(sel, z, big)
    flip = big < 0
    return [np.where(flip, -c, c).astype(F) for c in (x, y, z)]


def normals_f32(points, idx, n=None, K=None, viewpoint=None, sweeps=SWEEPS):
    """One cloud: points [N,3], idx [N,K] (the self kNN lists), n the cloud's length -> (normal [N,3], tangent [N,3], eigenvalues [N,3])
    float32; rows past n, rows with min(K, n) < 3 and rows of covariance trace 0 hold the invalid values."""
    p = np.ascontiguousarray(points, F)
    N = p.shape[0]
    n = N if n is None else int(n)
    K = idx.shape[1] if K is None else int(K)
    normal = np.tile(np.array(INVALID_NORMAL, F), (N, 1))
    tangent = np.tile(np.array(INVALID_TANGENT, F), (N, 1))
    eig = np.zeros((N, 3), F)
    if min(K, n) < 3:
        return normal, tangent, eig
    trace, A = covariance_f32(p, idx, n, K)
    with np.errstate(all="ignore"):
        lam, cols = _sorted_ascending(*jacobi_f32(A, sweeps))
        nv = _unit_with_default_sign(cols[0])
        tv = _unit_with_default_sign(cols[2])
        if viewpoint is not None:
            vp = np.asarray(viewpoint, F)
            d = [vp[a] - p[:n, a] for a in range(3)]
            flip = ((d[0] * nv[0] + d[1] * nv[1]) + d[2] * nv[2]) < 0
            nv = [np.where(flip, -c, c).astype(F) for c in nv]
    ok = trace != 0
    normal[:n][ok] = np.stack(nv, 1)[ok]
    tangent[:n][ok] = np.stack(tv, 1)[ok]
    eig[:n][ok] = np.stack(lam, 1)[ok]
    assert normal.dtype == F and tangent.dtype == F and eig.dtype == F
    return normal, tangent, eig


def normals_f64(points, idx, n=None, K=None):
    """float64 yardstick over the same lists -> (normal [n,3] (sign free), eigenvalues [n,3] ascending, eigenvectors [n,3,3])"""
    p = np.asarray(points, np.float64)
    n = p.shape[0] if n is None else int(n)
    K = idx.shape[1] if K is None else int(K)
    m = min(K, n)
    nb = p[np.asarray(idx[:n, :m], np.int64)]                     # [n,m,3]
    d = nb - nb.mean(1, keepdims=True)
    cov = np.einsum("nka,nkb->nab", d, d) / m
    w, v = np.linalg.eigh(cov)
    return v[:, :, 0], w, v


def sin_times_gap(normal32, normal64, lam64):
    """per point: sin(angle between the two lines) * (lam1 - lam0) / lam2, float64"""
    a = np.asarray(normal32, np.float64)
    a = a / np.linalg.norm(a, axis=1, keepdims=True)
    sin = np.linalg.norm(np.cross(a, normal64), axis=1)
    return sin * (lam64[:, 1] - lam64[:, 0]) / lam64[:, 2]


# ---- ga_pc_surfel_init -----------------------------------------------------------------------------------------------------------------
def surfel_init_f32(points, normal, tangent, dist2, n=None, eigenvalues=None, colors=None, opacity=0.1, scale_factor=1.0,
                    return_branch=False):
    """One cloud -> gaussians [N,13] float32 (xyz, opacity, scale(2), rotation wxyz, rgb), the header's operation order.  A row is
    invalid past n, with min(K, n) < 4, with eigenvalues given and not eigenvalues[:, 2] > 0, or when n or the projected tangent has
    no length."""
    p = np.ascontiguousarray(points, F)
    N = p.shape[0]
    n = N if n is None else int(n)
    K = dist2.shape[1]
    out = np.zeros((N, 13), F)
    out[:, 0:3] = p
    out[:, 4:6] = F(1e-4)
    out[:, 6] = F(1)
    out[:, 10:13] = F(0.5)
    branch = np.full(N, -1)
    if min(K, n) < 4:
        return (out, branch) if return_branch else out
    nx, ny, nz = (np.ascontiguousarray(normal[:n, a], F) for a in range(3))
    tx, ty, tz = (np.ascontiguousarray(tangent[:n, a], F) for a in range(3))
    d2 = np.ascontiguousarray(dist2[:n], F)
    with np.errstate(all="ignore"):
        s = F(scale_factor) * np.sqrt(np.maximum(((d2[:, 1] + d2[:, 2]) + d2[:, 3]) / F(3), F(1e-7)))
        nl = _norm3(nx, ny, nz)
        nx, ny, nz = nx / nl, ny / nl, nz / nl
        d = (tx * nx + ty * ny) + tz * nz
        ux, uy, uz = tx - d * nx, ty - d * ny, tz - d * nz
        ul = _norm3(ux, uy, uz)
        ux, uy, uz = ux / ul, uy / ul, uz / ul
        bx, by, bz = ny * uz - nz * uy, nz * ux - nx * uz, nx * uy - ny * ux
        # R[row][col], columns (t', b, n)
        R00, R10, R20, R01, R11, R21, R02, R12, R22 = ux, uy, uz, bx, by, bz, nx, ny, nz
        tr = (R00 + R11) + R22
        b0 = tr > 0
        b1 = ~b0 & (R00 > R11) & (R00 > R22)
        b2 = ~b0 & ~b1 & (R11 > R22)
        S0 = np.sqrt(tr + F(1)) * F(2)
        S1 = np.sqrt(((F(1) + R00) - R11) - R22) * F(2)
        S2 = np.sqrt(((F(1) + R11) - R00) - R22) * F(2)
        S3 = np.sqrt(((F(1) + R22) - R00) - R11) * F(2)
        q0 = (F(0.25) * S0, (R21 - R12) / S0, (R02 - R20) / S0, (R10 - R01) / S0)
        q1 = ((R21 - R12) / S1, F(0.25) * S1, (R01 + R10) / S1, (R02 + R20) / S1)
        q2 = ((R02 - R20) / S2, (R01 + R10) / S2, F(0.25) * S2, (R12 + R21) / S2)
        q3 = ((R10 - R01) / S3, (R02 + R20) / S3, (R12 + R21) / S3, F(0.25) * S3)
        q = [np.where(b0, q0[k], np.where(b1, q1[k], np.where(b2, q2[k], q3[k]))).astype(F) for k in range(4)]
        ql = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
        q = [c / ql for c in q]
        neg = q[0] < 0
        q = [np.where(neg, -c, c).astype(F) for c in q]
    ok = (nl > 0) & (ul > 0)
    if eigenvalues is not None:
        ok &= np.asarray(eigenvalues[:n, 2], F) > 0
    row = np.zeros((n, 13), F)
    row[:, 0:3] = p[:n]
    row[:, 3] = F(opacity)
    row[:, 4], row[:, 5] = s, s
    for k in range(4):
        row[:, 6 + k] = q[k]
    row[:, 10:13] = F(0.5) if colors is None else np.asarray(colors[:n], F)
    out[:n][ok] = row[ok]
    branch[:n][ok] = np.where(b0, 0, np.where(b1, 1, np.where(b2, 2, 3)))[ok]
    assert out.dtype == F
    return (out, branch) if return_branch else out


def rasterizer_frame(q):
    """csrc/surfel_preprocess.hip:51-55 in numpy float32: q [N,4] wxyz -> (tu, tv, nn), the three columns of the rotation matrix"""
    q = np.asarray(q, F)
    qs = F(1) / np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    r, x, y, z = q[:, 0] * qs, q[:, 1] * qs, q[:, 2] * qs, q[:, 3] * qs
    one, two = F(1), F(2)
    tu = np.stack([one - two * (y * y + z * z), two * (x * y + r * z), two * (x * z - r * y)], 1)
    tv = np.stack([two * (x * y - r * z), one - two * (x * x + z * z), two * (y * z + r * x)], 1)
    nn = np.stack([two * (x * z + r * y), two * (y * z - r * x), one - two * (x * x + y * y)], 1)
    return tu, tv, nn
