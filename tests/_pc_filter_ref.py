"""numpy restatement of ``ga_pc_filter_views`` and ``ga_pc_voxel_thin`` (include/ga_pointcloud.h, csrc/pc_filter.hip): the float32 one
the kernels must equal bit for bit -- votes, kept rows, order, padding and counts included -- and the analytic two-sphere scene the
tests of the filter share.

Every array below is float32 and every numpy operation on float32 arrays rounds once, so the expressions are the header's, operation by
operation.  The voxel side keeps its table in a Python dict.  No torch, no GPU."""
import numpy as np

F = np.float32
DEPTH_Z, DEPTH_RAY = 0, 1
VOXEL_FIRST, VOXEL_CENTER = 0, 1
THREADS, BAND_ROWS = 256, 1024        # GA_PC_FILTER_THREADS, GA_PC_FILTER_BAND_ROWS
MAX_INDEX = (1 << 20) - 1             # GA_PC_VOXEL_MAX_INDEX

# what one view says of one point
SKIPPED_OWN, BEHIND, OUTSIDE, SUPPORT, CONFLICT, CARVED, OCCLUDED, UNDECIDED = range(8)


def plan(rows):
    """-> (bands of the flag and scatter launches, trips of the single scan workgroup)"""
    bands = -(-rows // BAND_ROWS)
    return bands, -(-bands // THREADS)


def live_rows(rows, in_count):
    return rows if in_count is None else min(max(int(in_count), 0), rows)


def votes_f32(points, depth, cameras, source=None, mask=None, in_count=None, depth_kind=DEPTH_Z, depth_min=0.0, depth_max=np.inf,
              mask_threshold=0.5, tol_abs=0.0, tol_rel=0.01, window=1, carve=False):
    """-> (support [rows] int64, conflicts [rows] int64, classes [rows,V] int8); rows that are not live have no votes and class
    SKIPPED_OWN everywhere"""
    p = np.asarray(points, F)
    depth, cam = np.asarray(depth, F), np.asarray(cameras, F)
    V, H, W = depth.shape
    rows = p.shape[0]
    live = live_rows(rows, in_count)
    p = p[:live]
    own = np.full(live, -1, np.int64)
    if source is not None:
        s = np.asarray(source, np.int64)[:live]
        own[s >= 0] = s[s >= 0] // (H * W)
    support, conflicts = np.zeros(rows, np.int64), np.zeros(rows, np.int64)
    classes = np.full((rows, V), SKIPPED_OWN, np.int8)
    with np.errstate(all="ignore"):
        surf = (F(depth_min) < depth) & (depth < F(depth_max))
        if mask is not None:
            surf &= np.asarray(mask, F) >= F(mask_threshold)
        for u in range(V):
            c = cam[u]
            ex, ey, ez = p[:, 0] - c[9], p[:, 1] - c[10], p[:, 2] - c[11]
            qx = (c[0] * ex + c[3] * ey) + c[6] * ez
            qy = (c[1] * ex + c[4] * ey) + c[7] * ez
            qz = (c[2] * ex + c[5] * ey) + c[8] * ez
            fx, fy, cx, cy, sk = c[12], c[13], c[14], c[15], c[16]
            xl, yl = qx / qz, qy / qz
            vv = yl * fy + cy
            uu = ((xl * fx + cx) - (cy * sk) / fy) + (sk * vv) / fy
            a, b = uu * F(W), vv * F(H)
            voting = own != u
            front = voting & (qz > 0)
            inside = front & (a >= 0) & (a < F(W)) & (b >= 0) & (b < F(H))
            x = np.where(inside, a, 0).astype(np.int64)
            y = np.where(inside, b, 0).astype(np.int64)
            d = np.sqrt((qx * qx + qy * qy) + qz * qz) if depth_kind == DEPTH_RAY else qz
            n_in, n_surf = np.zeros(live, np.int64), np.zeros(live, np.int64)
            zmin, zmax = np.full(live, np.inf, F), np.full(live, -np.inf, F)
            centre = np.zeros(live, bool)
            for dy in range(-window, window + 1):
                for dx in range(-window, window + 1):
                    xx, yy = x + dx, y + dy
                    ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
                    xc, yc = np.clip(xx, 0, W - 1), np.clip(yy, 0, H - 1)
                    z, sf = depth[u, yc, xc], surf[u, yc, xc] & ok
                    n_in += ok
                    n_surf += sf
                    zmin = np.where(sf & (z < zmin), z, zmin)
                    zmax = np.where(sf & (z > zmax), z, zmax)
                    if dx == 0 and dy == 0:
                        centre = sf
            lo = zmin - (F(tol_abs) + F(tol_rel) * zmin)
            hi = zmax + (F(tol_abs) + F(tol_rel) * zmax)
            any_surf = n_surf > 0
            sup = inside & any_surf & centre & (lo <= d) & (d <= hi)
            con = inside & any_surf & (n_surf == n_in) & (d < lo)
            crv = inside & ~any_surf & bool(carve)
            cls = np.full(live, UNDECIDED, np.int8)
            cls[inside & any_surf & centre & (d > hi)] = OCCLUDED
            cls[sup], cls[con], cls[crv] = SUPPORT, CONFLICT, CARVED
            cls[front & ~inside] = OUTSIDE
            cls[voting & ~front] = BEHIND
            cls[~voting] = SKIPPED_OWN
            classes[:live, u] = cls
            support[:live] += sup
            conflicts[:live] += con | crv
    return support, conflicts, classes


def compact(keep, points, colors=None, normals=None, source=None, capacity=None, num_views=None, view_pixels=None, multiplicity=None):
    """the ordered compaction of both calls -> dict, padded as the kernels pad; ``multiplicity`` is per INPUT row"""
    keep = np.asarray(keep, bool)
    rows = keep.shape[0]
    cap = rows if capacity is None else int(capacity)
    kept = np.flatnonzero(keep)
    count, n = len(kept), min(len(kept), cap)
    out = dict(count=count, kept_rows=np.full(cap, -1, np.int32), points=np.zeros((cap, 3), F), colors=None, normals=None, source=None,
               view_counts=None, multiplicity=None)
    out["kept_rows"][:n] = kept[:n]
    out["points"][:n] = np.asarray(points, F)[kept[:n]]
    for name, t in (("colors", colors), ("normals", normals)):
        if t is not None:
            out[name] = np.zeros((cap, 3), F)
            out[name][:n] = np.asarray(t, F)[kept[:n]]
    if source is not None:
        s = np.asarray(source, np.int32)
        out["source"] = np.full(cap, -1, np.int32)
        out["source"][:n] = s[kept[:n]]
        if num_views is not None:
            v = s[kept].astype(np.int64)
            v = v[v >= 0] // int(view_pixels)
            out["view_counts"] = np.bincount(v[v < num_views], minlength=num_views).astype(np.int32)
    if multiplicity is not None:
        out["multiplicity"] = np.zeros(cap, np.int32)
        out["multiplicity"][:n] = np.asarray(multiplicity)[kept[:n]]
    return out


def filter_views_f32(points, depth, cameras, colors=None, normals=None, source=None, mask=None, in_count=None, capacity=None,
                     min_support=1, max_conflicts=0, want_view_counts=True, **rule):
    """the whole contract of ``ga_pc_filter_views`` -> the dict of ``compact`` plus ``support`` / ``conflicts`` [rows] uint8 and the
    unsaturated ``classes``"""
    support, conflicts, classes = votes_f32(points, depth, cameras, source=source, mask=mask, in_count=in_count, **rule)
    rows = support.shape[0]
    keep = (support >= min_support) & (conflicts <= max_conflicts) & (np.arange(rows) < live_rows(rows, in_count))
    V, H, W = np.asarray(depth).shape
    out = compact(keep, points, colors, normals, source, capacity, V if want_view_counts else None, H * W)
    out.update(support=np.minimum(support, 255).astype(np.uint8), conflicts=np.minimum(conflicts, 255).astype(np.uint8), classes=classes,
               keep=keep)
    return out


def voxel_cells(points, voxel_size, origin=(0.0, 0.0, 0.0), keep=VOXEL_CENTER, in_count=None):
    """-> (ok [rows] bool, key [rows] int64, rank [rows] uint64): live rows that fall into the grid, their cell and their rank"""
    p = np.asarray(points, F)
    rows = p.shape[0]
    live = live_rows(rows, in_count)
    o, vs = np.asarray(origin, F), F(voxel_size)
    with np.errstate(all="ignore"):
        g = (p - o[None, :]) / vs
        fl = np.floor(g)
        ok = (np.isfinite(g) & (np.abs(fl) <= F(MAX_INDEX))).all(1) & (np.arange(rows) < live)
        i = np.where(ok[:, None], fl, 0).astype(np.int64)
        key = ((i[:, 0] + (1 << 20)) << 42) | ((i[:, 1] + (1 << 20)) << 21) | (i[:, 2] + (1 << 20))
        rank = np.arange(rows, dtype=np.uint64)
        if keep == VOXEL_CENTER:
            c = (i.astype(F) + F(0.5)) * vs + o[None, :]
            dl = np.where(ok[:, None], p - c, 0).astype(F)
            dist2 = (dl[:, 0] * dl[:, 0] + dl[:, 1] * dl[:, 1]) + dl[:, 2] * dl[:, 2]
            rank = (dist2.astype(F).view(np.uint32).astype(np.uint64) << np.uint64(32)) | rank
    return ok, key, rank


def voxel_thin_f32(points, voxel_size, origin=(0.0, 0.0, 0.0), keep=VOXEL_CENTER, colors=None, normals=None, source=None, in_count=None,
                   capacity=None, num_views=None, view_pixels=None):
    """the whole contract of ``ga_pc_voxel_thin`` -> the dict of ``compact`` plus ``dropped`` and ``keep``"""
    ok, key, rank = voxel_cells(points, voxel_size, origin, keep, in_count)
    rows = ok.shape[0]
    best, members = {}, {}
    for r in np.flatnonzero(ok).tolist():
        k, rk = int(key[r]), int(rank[r])
        if k not in best or rk < best[k][0]:
            best[k] = (rk, r)
        members[k] = members.get(k, 0) + 1
    flag, mult = np.zeros(rows, bool), np.zeros(rows, np.int64)
    for k, (_, r) in best.items():
        flag[r], mult[r] = True, members[k]
    out = compact(flag, points, colors, normals, source, capacity, num_views, view_pixels, multiplicity=mult)
    out.update(dropped=live_rows(rows, in_count) - int(ok.sum()), keep=flag)
    return out


# ---- the analytic scene: two spheres seen from a ring of cameras ------------------------------------------------------------------------
SPHERES = (((0.0, 0.0, 0.0), 0.30), ((0.22, 0.10, 0.05), 0.12))


def ring_cameras(V=8, radius=1.5, tanfov=0.25):
    """[V,21] float32: on a circle of ``radius`` in the x-z plane at height ``radius * 0.35 * sin(2 a + 0.3)``, looking at the origin;
    fx = fy = 1 / (2 tanfov), cx = cy = 0.5, no skew"""
    cam = np.zeros((V, 21), np.float64)
    for k in range(V):
        a = 2.0 * np.pi * k / V
        pos = np.array([radius * np.cos(a), radius * 0.35 * np.sin(2.0 * a + 0.3), radius * np.sin(a)])
        z = -pos / np.linalg.norm(pos)
        x = np.cross([0.0, 1.0, 0.0], z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        cam[k, :9] = np.stack([x, y, z], 1).reshape(-1)          # camera-to-world, columns x y z
        cam[k, 9:12] = pos
        cam[k, 12:14] = 1.0 / (2.0 * tanfov)
        cam[k, 14:16] = 0.5
    return cam.astype(F)


def raycast_z(cameras, H, W, spheres=SPHERES):
    """camera-z depth [V,H,W] of the nearest sphere along every pixel's ray, ray-cast in float64 and stored as float32; 0 where the ray
    meets nothing"""
    cam = np.asarray(cameras, F).astype(np.float64)
    V = cam.shape[0]
    u = ((np.arange(W) + 0.5) / W)[None, None, :]
    v = ((np.arange(H) + 0.5) / H)[None, :, None]
    k = lambda i: cam[:, i][:, None, None]
    fx, fy, cx, cy, sk = k(12), k(13), k(14), k(15), k(16)
    xl = (u - cx + cy * sk / fy - sk * v / fy) / fx
    yl = np.broadcast_to((v - cy) / fy, xl.shape)
    d = np.stack([k(3 * a) * xl + k(3 * a + 1) * yl + k(3 * a + 2) for a in range(3)], -1)      # camera z of d is 1
    o = cam[:, 9:12][:, None, None, :]
    best = np.full((V, H, W), np.inf)
    for centre, r in spheres:
        oc = o - np.asarray(centre)
        A, B, C = (d * d).sum(-1), 2.0 * (d * oc).sum(-1), (oc * oc).sum(-1) - r * r
        disc = B * B - 4.0 * A * C
        s = (-B - np.sqrt(np.maximum(disc, 0.0))) / (2.0 * A)
        best = np.where((disc > 0) & (s > 0) & (s < best), s, best)
    return np.where(np.isfinite(best), best, 0.0).astype(F)


def add_floaters(depth, fraction=0.03, seed=0, scale=(0.6, 0.85)):
    """-> (depth with ``fraction`` of its surface pixels pulled towards the camera by a factor from ``scale``, [V,H,W] bool: which)"""
    rng = np.random.default_rng(seed)
    surface = np.flatnonzero(depth.reshape(-1) > 0)
    pick = rng.choice(surface, size=max(1, int(round(fraction * len(surface)))), replace=False)
    out = depth.copy().reshape(-1)
    out[pick] = (out[pick].astype(np.float64) * rng.uniform(scale[0], scale[1], size=len(pick))).astype(F)
    which = np.zeros(depth.size, bool)
    which[pick] = True
    return out.reshape(depth.shape), which.reshape(depth.shape)
