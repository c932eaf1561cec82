"""numpy restatement of ``ga_mesh_sample`` and ``ga_mesh_point_distance`` (include/ga_mesh.h, csrc/mesh_ops.hip), operation by operation
in the header's order: fp32 arrays stay fp32 under numpy's elementwise operators (each rounded on its own, division and square root
correctly rounded), the two float64 sums are ``np.cumsum`` (a sequential accumulation, as the kernels' single lane), the searches are
``np.searchsorted`` on the non-decreasing arrays the kernels search by bisection.  The GPU tests compare for EQUALITY, bit for bit.

Also here: a float64 brute-force distance written independently (Ericson's 5.1.5 with its own dot products at every corner), and the
small mesh zoo the tests share."""
import numpy as np

from tests._sde_ref import philox_np

F32 = np.float32
FACES_PER_GROUP = 256          # GA_MESH_AREA_FACES
PHILOX_STREAM = 0x4853454D     # GA_MESH_PHILOX_STREAM
REGIONS = ("A", "B", "AB", "C", "AC", "BC", "IN")


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def triangles(vertices, faces):
    """the header's "weight of a face": dict of fp32 arrays a, ab, ac, n (each [F,3]), w [F], and idx [F,3] (zeroed when out of range)"""
    v = np.ascontiguousarray(vertices, F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    inside = ((f >= 0) & (f < v.shape[0])).all(1)
    idx = np.where(inside[:, None], f, 0)
    a, b, c = v[idx[:, 0]], v[idx[:, 1]], v[idx[:, 2]]
    with np.errstate(all="ignore"):
        ab, ac = b - a, c - a
        nx = ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1]
        ny = ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2]
        nz = ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]
        w = np.sqrt((nx * nx + ny * ny) + nz * nz)
        w = np.where(inside & (w < F32(np.inf)), w, F32(0))
    return dict(a=a, ab=ab, ac=ac, n=np.stack([nx, ny, nz], 1), w=w.astype(F32), idx=idx)


def cumulative(w):
    """fp32 weights [F] -> (prefix [F] float64: the running sum inside each group of 256 faces, off [G + 1] float64: the running sum of
    the group sums, off[G] the total)"""
    n = w.shape[0]
    G = -(-n // FACES_PER_GROUP)
    padded = np.zeros(G * FACES_PER_GROUP, np.float64)
    padded[:n] = w.astype(np.float64)
    with np.errstate(all="ignore"):
        prefix = np.cumsum(padded.reshape(G, FACES_PER_GROUP), axis=1)
        off = np.concatenate([[0.0], np.cumsum(prefix[:, -1])])
    return prefix.reshape(-1)[:n], off


def sample(vertices, faces, num_samples, seed, colors=None):
    """-> dict(points [S,3], face [S] int32, bary [S,3], normals [S,3], colors [S,3] or None), fp32"""
    tri = triangles(vertices, faces)
    v = np.ascontiguousarray(vertices, F32).reshape(-1, 3)
    S, n = int(num_samples), tri["w"].shape[0]
    prefix, off = cumulative(tri["w"])
    G, total = off.shape[0] - 1, off[-1]
    out = dict(points=np.zeros((S, 3), F32), face=np.full(S, -1, np.int32), bary=np.zeros((S, 3), F32), normals=np.zeros((S, 3), F32),
               colors=None if colors is None else np.zeros((S, 3), F32))
    if not (total > 0.0 and total < np.inf):
        return out
    seed = int(seed) & ((1 << 64) - 1)
    full = lambda x: np.full(S, x, np.uint32)   # noqa: E731
    x = philox_np(np.arange(S, dtype=np.uint32), full(0), full(0), full(PHILOX_STREAM), full(seed & 0xFFFFFFFF), full(seed >> 32))
    x64 = x.astype(np.uint64)
    u = (((x64[:, 0] >> np.uint64(5)) << np.uint64(26)) | (x64[:, 1] >> np.uint64(6))).astype(np.float64) * 2.0 ** -53
    t = u * total
    g = np.searchsorted(off[1:], t, side="right")
    g = np.where(g == G, np.searchsorted(off[1:], total, side="left"), g)
    tl = t - off[g]
    face = np.empty(S, np.int64)
    for blk in np.unique(g):
        rows = np.nonzero(g == blk)[0]
        pg = prefix[blk * FACES_PER_GROUP:min(n, (blk + 1) * FACES_PER_GROUP)]
        j = np.searchsorted(pg, tl[rows], side="right")
        j = np.where(j == pg.shape[0], np.searchsorted(pg, pg[-1], side="left"), j)
        face[rows] = blk * FACES_PER_GROUP + j
    u1 = ((x[:, 2] >> np.uint32(8)) + np.uint32(1)).astype(F32) * F32(2.0 ** -24)
    u2 = (x[:, 3] >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)
    r = np.sqrt(u1)
    w0, w1, w2 = F32(1) - r, r * (F32(1) - u2), r * u2
    idx = tri["idx"][face]
    mix = lambda rows: (w0[:, None] * rows[idx[:, 0]] + w1[:, None] * rows[idx[:, 1]]) + w2[:, None] * rows[idx[:, 2]]   # noqa: E731
    out["face"] = face.astype(np.int32)
    out["bary"] = np.stack([w0, w1, w2], 1)
    out["points"] = mix(v)
    out["normals"] = tri["n"][face] / tri["w"][face][:, None]
    if colors is not None:
        out["colors"] = mix(np.ascontiguousarray(colors, F32).reshape(-1, 3))
    return out


def _closest(rec, p):
    """the header's region test for every (query, triangle) pair: rec = triangles(...), p [N,3] fp32 -> (dist2, v, w, closest, region),
    each [N,F] (closest [N,F,3]); region indexes REGIONS"""
    a, ab, ac = rec["a"][None], rec["ab"][None], rec["ac"][None]
    abab = _dot(ab[..., 0], ab[..., 1], ab[..., 2], ab[..., 0], ab[..., 1], ab[..., 2])
    abac = _dot(ab[..., 0], ab[..., 1], ab[..., 2], ac[..., 0], ac[..., 1], ac[..., 2])
    acac = _dot(ac[..., 0], ac[..., 1], ac[..., 2], ac[..., 0], ac[..., 1], ac[..., 2])
    p = p[:, None, :]
    ap = p - a
    d1 = _dot(ab[..., 0], ab[..., 1], ab[..., 2], ap[..., 0], ap[..., 1], ap[..., 2])
    d2 = _dot(ac[..., 0], ac[..., 1], ac[..., 2], ap[..., 0], ap[..., 1], ap[..., 2])
    d3, d4, d5, d6 = d1 - abab, d2 - abac, d1 - abac, d2 - acac
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e, g = d4 - d3, d5 - d6
    rA = (d1 <= 0) & (d2 <= 0)
    rB = ~rA & (d3 >= 0) & (d4 <= d3)
    rAB = ~rA & ~rB & (vc <= 0) & (d1 >= 0) & (d3 <= 0)
    pre_c = rA | rB | rAB
    rC = ~pre_c & (d6 >= 0) & (d5 <= d6)
    rAC = ~pre_c & ~rC & (vb <= 0) & (d2 >= 0) & (d6 <= 0)
    pre_bc = pre_c | rC | rAC
    rBC = ~pre_bc & (va <= 0) & (e >= 0) & (g >= 0)
    rIN = ~pre_bc & ~rBC
    one, zero = F32(1), F32(0)
    num = np.where(rAB, d1, np.where(rAC, d2, np.where(rBC, e, np.where(rIN, one, zero))))
    den = np.where(rAB, d1 - d3, np.where(rAC, d2 - d6, np.where(rBC, e + g, np.where(rIN, (va + vb) + vc, one))))
    q = num / den
    v = np.where(rB, one, np.where(rAB, q, np.where(rBC, one - q, np.where(rIN, vb * q, zero))))
    w = np.where(rC, one, np.where(rAC | rBC, q, np.where(rIN, vc * q, zero)))
    c = (a + ab * v[..., None]) + ac * w[..., None]
    d = p - c
    dist2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    region = np.select([rA, rB, rAB, rC, rAC, rBC], [0, 1, 2, 3, 4, 5], 6)
    return dist2.astype(F32), v.astype(F32), w.astype(F32), c.astype(F32), region


def pair_dist2(points, vertices, faces):
    """[N,F] fp32 squared distances as the main kernel sees them (+inf where a triangle is skipped or the distance is NaN: neither
    ever wins) and the [N,F] regions"""
    rec = triangles(vertices, faces)
    p = np.ascontiguousarray(points, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        d, _, _, _, region = _closest(rec, p)
    d = np.where((rec["w"] > 0)[None, :] & ~np.isnan(d), d, F32(np.inf))
    return d, region


def point_distance(points, vertices, faces, count=None, face_chunk=2048):
    """-> dict(dist2 [N], face [N] int32, closest [N,3], bary [N,3], region [N] (-1 without a face)), fp32; rows past ``count`` are
    0 / -1 / zeros, a live row without a valid triangle +inf / -1 / zeros"""
    p = np.ascontiguousarray(points, F32).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int32).reshape(-1, 3)
    N = p.shape[0]
    live = N if count is None else max(0, min(N, int(count)))
    best = np.full(N, np.inf, F32)
    face = np.full(N, -1, np.int64)
    for f0 in range(0, f.shape[0], face_chunk):   # the chunking cannot matter: strict <, ascending faces
        d, _ = pair_dist2(p, vertices, f[f0:f0 + face_chunk])
        j = np.argmin(d, axis=1)
        dj = d[np.arange(N), j]
        better = dj < best
        best = np.where(better, dj, best)
        face = np.where(better, f0 + j, face)
    out = dict(dist2=np.zeros(N, F32), face=np.full(N, -1, np.int32), closest=np.zeros((N, 3), F32), bary=np.zeros((N, 3), F32),
               region=np.full(N, -1, np.int64))
    out["dist2"][:live] = best[:live]
    rows = np.nonzero((face >= 0) & (np.arange(N) < live))[0]
    if rows.size:
        rec = triangles(vertices, f[face[rows]])
        with np.errstate(all="ignore"):
            _, v, w, c, region = _closest(rec, p[rows])
        k = np.arange(rows.size)
        v, w = v[k, k], w[k, k]
        out["face"][rows] = face[rows]
        out["closest"][rows] = c[k, k]
        out["bary"][rows] = np.stack([(F32(1) - v) - w, v, w], 1)
        out["region"][rows] = region[k, k]
    return out


# ---- float64 brute force, written independently ------------------------------------------------------------------------------------

def point_distance64(points, vertices, faces):
    """Ericson 5.1.5 in float64 with the dot products taken at every corner; triangles with an index out of range or zero area (in
    float64) are skipped.  -> (dist2 [N] float64, face [N], all [N,F] float64)"""
    p = np.asarray(points, np.float64).reshape(-1, 3)[:, None, :]
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    ok = ((f >= 0) & (f < v.shape[0])).all(1)
    f = np.where(ok[:, None], f, 0)
    a, b, c = v[f[:, 0]][None], v[f[:, 1]][None], v[f[:, 2]][None]
    ok &= np.linalg.norm(np.cross(b[0] - a[0], c[0] - a[0]), axis=1) > 0
    ab, ac = b - a, c - a
    dot = lambda x, y: (x * y).sum(-1)   # noqa: E731
    ap, bp, cp = p - a, p - b, p - c
    d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    with np.errstate(all="ignore"):
        tab, tac, tbc = d1 / (d1 - d3), d2 / (d2 - d6), (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = 1.0 / (va + vb + vc)
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    pts = [a + 0 * p, b + 0 * p, a + tab[..., None] * ab, c + 0 * p, a + tac[..., None] * ac, b + tbc[..., None] * (c - b)]
    with np.errstate(all="ignore"):
        inner = a + ab * (vb * den)[..., None] + ac * (vc * den)[..., None]
    closest = inner
    for cond, pt in zip(reversed(conds), reversed(pts)):
        closest = np.where(cond[..., None], pt, closest)
    d = ((p - closest) ** 2).sum(-1)
    d = np.where(ok[None, :] & ~np.isnan(d), d, np.inf)
    face = np.argmin(d, axis=1)
    best = d[np.arange(d.shape[0]), face]
    return best, np.where(np.isfinite(best), face, -1), d


# ---- the mesh zoo -----------------------------------------------------------------------------------------------------------------

def icosphere(subdivisions):
    """unit icosphere, 20 * 4^s faces, outward winding -> (vertices [V,3] fp32, faces [F,3] int32)"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    v = [tuple(np.asarray(x, np.float64) / np.linalg.norm(x)) for x in v]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def midpoint(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                m = (np.asarray(v[i]) + np.asarray(v[j])) / 2.0
                v.append(tuple(m / np.linalg.norm(m)))
                mid[key] = len(v) - 1
            return mid[key]
        for i, j, k in f:
            a, b, c = midpoint(i, j), midpoint(j, k), midpoint(k, i)
            nf += [(i, a, c), (j, b, a), (k, c, b), (a, b, c)]
        f = nf
    return np.asarray(v, F32), np.asarray(f, np.int32)


def unit_square():
    """two triangles sharing the diagonal (0,0,0)-(1,1,0)"""
    return np.asarray([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], F32), np.asarray([[0, 1, 2], [0, 2, 3]], np.int32)


def pair_1_3():
    """two triangles, areas 1/2 and 3/2: weights exactly 1 and 3"""
    return (np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [5, 0, 0], [2, 1, 0]], F32),
            np.asarray([[0, 1, 2], [3, 4, 5]], np.int32))


def soup(num_faces=96, seed=7, min_angle_deg=15.0, extent=1.0):
    """seeded, unconnected triangles in [-extent, extent]^3 with edge lengths around 0.3 extent and no angle under ``min_angle_deg``"""
    rng = np.random.default_rng(seed)
    tris = []
    while len(tris) < num_faces:
        centre = rng.uniform(-extent, extent, 3)
        t = centre + rng.uniform(-0.3 * extent, 0.3 * extent, (3, 3))
        e = [t[1] - t[0], t[2] - t[1], t[0] - t[2]]
        cos = [-(e[i] @ e[i - 1]) / (np.linalg.norm(e[i]) * np.linalg.norm(e[i - 1])) for i in range(3)]
        if np.degrees(np.arccos(np.clip(max(cos), -1, 1))) >= min_angle_deg:
            tris.append(t)
    v = np.asarray(tris, np.float64).reshape(-1, 3).astype(F32)
    return v, np.arange(3 * num_faces, dtype=np.int32).reshape(-1, 3)


def spliced_soup(num_faces=96, seed=7):
    """the soup with faces that must never count spliced in (every 7th slot, cycling through: a repeated index, three collinear vertices,
    an index of -1, an index of V, an index of 2^31 - 1) and a repeated valid face after every 11th -> (vertices, faces, dead [F] bool)"""
    v, f = soup(num_faces, seed)
    v = np.concatenate([v, np.asarray([[0, 0, 0], [0.25, 0.25, 0.25], [0.5, 0.5, 0.5]], F32)])   # exactly collinear in fp32
    V = v.shape[0]
    bad = [lambda t: (t[0], t[0], t[2]), lambda t: (V - 3, V - 2, V - 1), lambda t: (-1, t[1], t[2]), lambda t: (t[0], V, t[2]),
           lambda t: (t[0], t[1], 2 ** 31 - 1)]
    faces, dead = [], []
    for i, t in enumerate(f.tolist()):
        if i % 7 == 0:
            faces.append(bad[(i // 7) % len(bad)](t))
            dead.append(True)
        faces.append(tuple(t))
        dead.append(False)
        if i % 11 == 0:
            faces.append(tuple(t))
            dead.append(False)
    return v, np.asarray(faces, np.int64).astype(np.int32), np.asarray(dead)


def strip(num_faces):
    """a triangle strip along x with widths that vary from face to face (no two neighbouring weights equal)"""
    n = num_faces + 2
    k = np.arange(n)
    x = (k // 2).astype(np.float64) * 0.01 + (k % 7) * 0.001
    y = np.where(k % 2 == 0, 0.0, 1.0 + (k % 5) * 0.1)
    v = np.stack([x, y, np.zeros(n)], 1).astype(F32)
    f = np.stack([k[:-2], k[1:-1], k[2:]], 1).astype(np.int32)
    return v, f


def region_queries(vertices, faces, offset=0.02, height=0.01):
    """queries built to land in each of the seven regions of every triangle: offsets from the three vertices (along the outward bisector),
    from the three edge midpoints (along the in-plane outward normal of the edge) and from the centroid, all lifted by ``height`` along
    the face normal -> [7 F, 3] fp32, rows in REGIONS order per face (A, B, AB, C, AC, BC, IN)"""
    v = np.asarray(vertices, np.float64)
    out = []
    for ia, ib, ic in np.asarray(faces).tolist():
        a, b, c = v[ia], v[ib], v[ic]
        n = np.cross(b - a, c - a)
        n /= np.linalg.norm(n)
        unit = lambda x: x / np.linalg.norm(x)   # noqa: E731
        corner = lambda p, q, r: p - offset * unit(unit(q - p) + unit(r - p))   # noqa: E731
        edge = lambda p, q, r: (p + q) / 2 + offset * unit(np.cross(q - p, n)) * np.sign(np.cross(q - p, n) @ ((p + q) / 2 - r))   # noqa: E731
        out += [corner(a, b, c), corner(b, a, c), edge(a, b, c), corner(c, a, b), edge(a, c, b), edge(b, c, a), (a + b + c) / 3]
        out[-7:] = [q + height * n for q in out[-7:]]
    return np.asarray(out, np.float64).astype(F32)


def tie_mesh_and_queries():
    """the unit square (two triangles sharing the diagonal) followed by a far triangle given twice -> (vertices, faces, queries, ties):
    query 0 sits above the middle of the shared diagonal (all coordinates dyadic: the two distances are equal bit for bit), query 1
    above the duplicated triangle; ``ties`` lists, per query, the faces that must attain the minimum"""
    v, f = unit_square()
    v = np.concatenate([v, np.asarray([[4, 0, 0], [5, 0, 0], [4, 1, 0]], F32)])
    f = np.concatenate([f, np.asarray([[4, 5, 6], [4, 5, 6]], np.int32)])
    q = np.asarray([[0.5, 0.5, 0.25], [4.25, 0.25, 0.5]], F32)
    return v, f, q, [(0, 1), (2, 3)]
