"""numpy restatement of ``ga_pc_unproject`` (include/ga_pointcloud.h, csrc/pc_unproject.hip): the float32 one the kernels must equal bit
for bit -- erosion, validity, order, padding and counts included -- and a float64 version of the geometry alone.

Every array below is float32 and every numpy operation on float32 arrays rounds once, so the expressions are the header's, operation by
operation.  No torch, no GPU."""
import numpy as np

F = np.float32
DEPTH_Z, DEPTH_RAY = 0, 1
THREADS, TILE_PIXELS = 256, 1024      # GA_PC_UNPROJECT_THREADS, GA_PC_UNPROJECT_TILE_PIXELS


def plan(V, H, W):
    """-> (rows_per_block, blocks_per_view, num_blocks) of the flag and scatter launches, from the kernel's constants"""
    r = min(H, max(1, TILE_PIXELS // W))
    bpv = -(-H // r)
    return r, bpv, V * bpv


def cameras_from_pose25(c):
    """[V,25] -> [V,21]: rotation row-major, position, fx, fy, cx, cy, sk, four zeros"""
    c = np.asarray(c, F)
    out = np.zeros((c.shape[0], 21), F)
    out[:, :9] = c[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]
    out[:, 9:12] = c[:, [3, 7, 11]]
    out[:, 12:17] = c[:, [16, 20, 18, 21, 17]]
    return out


def cameras_from_view(cam_view, tanfov):
    """the formulas of ``cameras.cameras_from_view`` in float32: R = cam_view[:3,:3], position -(R @ cam_view[3,:3]), fx = fy =
    1 / (2 tanfov), cx = cy = 0.5, sk = 0.  (The position's three-term sums may round in another order than torch's matmul: this
    restates the formulas, the GPU tests hand the kernel the same camera rows they hand the restatement.)"""
    view = np.asarray(cam_view, F)
    out = np.zeros((view.shape[0], 21), F)
    R = view[:, :3, :3]
    out[:, :9] = R.reshape(-1, 9)
    out[:, 9:12] = -np.einsum("vab,vb->va", R, view[:, 3, :3]).astype(F)
    out[:, 12:14] = F(1.0 / (2.0 * float(tanfov)))
    out[:, 14:16] = F(0.5)
    return out


def eroded_foreground(mask, threshold, erode):
    """[V,H,W] bool: mask >= threshold, then ``erode`` iterations of the 3 x 3 cross erosion; a neighbour outside the image never
    erodes anything"""
    fg = np.asarray(mask, F) >= F(threshold)
    for _ in range(int(erode)):
        p = np.pad(fg, ((0, 0), (1, 1), (1, 1)), constant_values=True)
        fg = p[:, 1:-1, 1:-1] & p[:, :-2, 1:-1] & p[:, 2:, 1:-1] & p[:, 1:-1, :-2] & p[:, 1:-1, 2:]
    return fg


def lift_f32(depth, cameras, depth_kind=DEPTH_Z, clip=0.0):
    """the point of EVERY pixel, float32 [V,H,W,3], the header's operation order (invalid depths give whatever they give)"""
    depth, cam = np.asarray(depth, F), np.asarray(cameras, F)
    V, H, W = depth.shape
    with np.errstate(all="ignore"):
        inv_w, half_w = F(1) / F(W), F(0.5) / F(W)
        inv_h, half_h = F(1) / F(H), F(0.5) / F(H)
        u = (np.arange(W, dtype=F) * inv_w + half_w)[None, None, :]
        v = (np.arange(H, dtype=F) * inv_h + half_h)[None, :, None]
        k = lambda i: cam[:, i][:, None, None]
        fx, fy, cx, cy, sk = k(12), k(13), k(14), k(15), k(16)
        xl = (((u - cx) + (cy * sk) / fy) - (sk * v) / fy) / fx
        yl = np.broadcast_to((v - cy) / fy, xl.shape)
        d = [(k(3 * a) * xl + k(3 * a + 1) * yl) + k(3 * a + 2) for a in range(3)]
        if depth_kind == DEPTH_RAY:
            l = np.maximum(np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]), F(1e-12))
            d = [x / l for x in d]
        p = np.stack([k(9 + a) + depth * d[a] for a in range(3)], -1).astype(F)
        if clip > 0:
            p = np.minimum(np.maximum(p, -F(clip)), F(clip))
    return p


def lift_f64(depth, cameras, depth_kind=DEPTH_Z):
    """the geometry alone in float64, from the float32 inputs: [V,H,W,3], no clamp"""
    depth, cam = np.asarray(depth, np.float64), np.asarray(cameras, F).astype(np.float64)
    V, H, W = depth.shape
    u = ((np.arange(W) + 0.5) / W)[None, None, :]
    v = ((np.arange(H) + 0.5) / H)[None, :, None]
    k = lambda i: cam[:, i][:, None, None]
    fx, fy, cx, cy, sk = k(12), k(13), k(14), k(15), k(16)
    xl = (u - cx + cy * sk / fy - sk * v / fy) / fx
    yl = np.broadcast_to((v - cy) / fy, xl.shape)
    d = np.stack([k(3 * a) * xl + k(3 * a + 1) * yl + k(3 * a + 2) for a in range(3)], -1)
    if depth_kind == DEPTH_RAY:
        d = d / np.maximum(np.linalg.norm(d, axis=-1, keepdims=True), 1e-12)
    with np.errstate(all="ignore"):
        return cam[:, 9:12][:, None, None, :] + depth[..., None] * d


def valid_pixels(depth, cameras, mask=None, depth_kind=DEPTH_Z, depth_min=0.0, depth_max=np.inf, mask_threshold=0.5, erode=0,
                 clip=0.0, drop_zero=False, pixel_stride=1):
    """-> (valid [V,H,W] bool, points float32 [V,H,W,3])"""
    depth = np.asarray(depth, F)
    V, H, W = depth.shape
    s = int(pixel_stride)
    ok = np.zeros((V, H, W), bool)
    ok[:, ::s, ::s] = True
    with np.errstate(all="ignore"):
        ok &= (F(depth_min) < depth) & (depth < F(depth_max))
        if mask is not None:
            ok &= eroded_foreground(mask, mask_threshold, erode)
        p = lift_f32(depth, cameras, depth_kind, clip)
        if clip > 0:
            ok &= ~(np.abs(p) == F(clip)).any(-1)
        if drop_zero:
            ok &= ~(p == 0).any(-1)
    return ok, p


def unproject_f32(depth, cameras, mask=None, color=None, normal=None, depth_kind=DEPTH_Z, depth_min=0.0, depth_max=np.inf,
                  mask_threshold=0.5, erode=0, clip=0.0, drop_zero=False, pixel_stride=1, capacity=None):
    """the whole contract -> dict(points [capacity,3], colors, normals (or None), source [capacity] int32, count int, view_counts [V]
    int32), padded as the kernel pads"""
    depth = np.asarray(depth, F)
    V, H, W = depth.shape
    ok, p = valid_pixels(depth, cameras, mask, depth_kind, depth_min, depth_max, mask_threshold, erode, clip, drop_zero, pixel_stride)
    s = int(pixel_stride)
    cap = V * (-(-H // s)) * (-(-W // s)) if capacity is None else int(capacity)
    src = np.flatnonzero(ok.reshape(-1)).astype(np.int64)      # ascending (v * H + y) * W + x
    count, n = len(src), min(len(src), cap)
    src = src[:n]
    out = dict(points=np.zeros((cap, 3), F), colors=None, normals=None, source=np.full(cap, -1, np.int32), count=count,
               view_counts=ok.reshape(V, -1).sum(1).astype(np.int32))
    out["points"][:n] = p.reshape(-1, 3)[src]
    out["source"][:n] = src
    if color is not None:
        c = np.asarray(color)
        c = c.astype(F) / F(255) if c.dtype == np.uint8 else c.astype(F)
        out["colors"] = np.zeros((cap, 3), F)
        out["colors"][:n] = c.transpose(0, 2, 3, 1).reshape(-1, 3)[src]
    if normal is not None:
        nm = np.asarray(normal, F).transpose(0, 2, 3, 1).reshape(-1, 3)[src]
        with np.errstate(all="ignore"):
            l = np.sqrt((nm[:, 0] * nm[:, 0] + nm[:, 1] * nm[:, 1]) + nm[:, 2] * nm[:, 2])
            unit = nm / l[:, None]
        unit[~(l > 0)] = (0, 0, 1)
        out["normals"] = np.zeros((cap, 3), F)
        out["normals"][:n] = unit
    return out
