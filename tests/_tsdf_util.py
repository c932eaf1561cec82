"""Shared parts of the TSDF tests: synthetic RGB-D frames (analytic z-depth), the inverse of ``TSDFVolume.dense()``, the named
marching-cubes volumes, an independent statement of the vertex set, and the comparisons the GPU tests hold the kernels to
(tests/test_tsdf_cpu.py shows, on the oracle's own output with one planted defect at a time, that each of them can fail).

Bars (tests/test_tsdf_gpu.py): opened units, ``allocated``, weights and triangle index lists are integer artefacts -- identical;
tsdf, vertex positions and vertex colours within 1e-6, the colour volume (values up to 255) within 1e-4."""
import functools

import numpy as np

from oracle import tsdf as otsdf

UNIT = 16
TSDF_BAR, COLOR_VOLUME_BAR, VERTEX_BAR = 1e-6, 1e-4, 1e-6


def sphere_frames(n_views=3, size=64, radius=0.3, centre=(0.02, -0.01, 0.03)):
    """analytic z-depth of a sphere seen from the in-tree evaluation cameras"""
    from gaussiananything_amd import synthetic
    from gaussiananything_amd.mesh import to_cam_open3d_compat
    cams = synthetic.eval_cameras(max(n_views, 1))
    frames = []
    for i in range(n_views):
        c = {"cam_view": cams["cam_view"][i], "cam_pos": cams["cam_pos"][i], "tanfov": cams["tanfov"]}
        intr, ext = to_cam_open3d_compat(c, size)
        fx, fy, cx, cy = intr
        pose = np.linalg.inv(ext)
        v, u = np.meshgrid(np.arange(size), np.arange(size), indexing="ij")
        d_cam = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u, dtype=np.float64)], -1)   # per unit of z-depth
        d_w = d_cam @ pose[:3, :3].T
        o = pose[:3, 3] - np.asarray(centre)
        a = (d_w * d_w).sum(-1)
        b = 2.0 * (d_w @ o)
        cc = float(o @ o) - radius * radius
        disc = b * b - 4 * a * cc
        hit = disc > 0
        z = np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0.0))) / (2 * a), 0.0)
        p = pose[:3, 3] + d_w * z[..., None]
        n = (p - np.asarray(centre)) / radius
        rgb = np.where(hit[None], np.moveaxis(0.5 + 0.5 * n, -1, 0), 1.0).astype(np.float32)
        alpha = hit.astype(np.float32)
        frames.append(dict(cam=c, intr=intr, ext=ext, rgb=rgb, depth=z.astype(np.float32), alpha=alpha,
                           depth_trunc=float(np.linalg.norm(pose[:3, 3]) + 0.8)))
    return frames


def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """4x4 world -> camera, the camera looking along +z with x to the right and y down (Open3D's pinhole convention)"""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    z = (target - eye) / np.linalg.norm(target - eye)
    x = np.cross(z, up)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    ext = np.eye(4)
    ext[:3, :3] = np.stack([x, y, z])
    ext[:3, 3] = -ext[:3, :3] @ eye
    return ext


def analytic_frames(eyes, target, H, W, fx, fy, cx, cy, sphere=None, plane=None, depth_trunc=3.0, up=(0.0, 0.0, 1.0)):
    """Float64 ray casting of the union of a sphere ``(centre, radius)`` and a plane ``(point, normal)`` (either may be None), one
    frame per eye, every camera looking at ``target``: z-depth of the nearest hit in front of the camera, the sphere coloured
    0.5 + 0.5 normal, the plane by a smooth pattern of the hit point; no hit: depth 0, alpha 0, white.  Same dicts as
    ``sphere_frames`` (without ``cam``)."""
    frames = []
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d_cam = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)                     # per unit of z-depth
    for eye in eyes:
        ext = look_at(eye, target, up)
        pose = np.linalg.inv(ext)
        o, d_w = pose[:3, 3], d_cam @ pose[:3, :3].T
        z = np.full((H, W), np.inf)
        rgb = np.ones((H, W, 3))
        if sphere is not None:
            centre, radius = np.asarray(sphere[0], np.float64), float(sphere[1])
            oc = o - centre
            a, b, cc = (d_w * d_w).sum(-1), 2.0 * (d_w @ oc), float(oc @ oc) - radius * radius
            disc = b * b - 4 * a * cc
            zs = np.where(disc > 0, (-b - np.sqrt(np.maximum(disc, 0.0))) / (2 * a), np.inf)
            zs = np.where(zs > 0, zs, np.inf)
            n = (o + d_w * np.where(np.isfinite(zs), zs, 0.0)[..., None] - centre) / radius
            rgb = np.where((zs < z)[..., None], 0.5 + 0.5 * n, rgb)
            z = np.minimum(z, zs)
        if plane is not None:
            point, normal = np.asarray(plane[0], np.float64), np.asarray(plane[1], np.float64)
            den = d_w @ normal
            with np.errstate(divide="ignore", invalid="ignore"):
                zp = np.where(np.abs(den) > 1e-12, ((point - o) @ normal) / den, np.inf)
            zp = np.where(zp > 0, zp, np.inf)
            p = o + d_w * np.where(np.isfinite(zp), zp, 0.0)[..., None]
            pattern = 0.5 + 0.5 * np.sin(9.0 * p + np.array([0.0, 1.0, 2.0]))
            rgb = np.where((zp < z)[..., None], pattern, rgb)
            z = np.minimum(z, zp)
        hit = np.isfinite(z)
        frames.append(dict(intr=(float(fx), float(fy), float(cx), float(cy)), ext=ext,
                           rgb=np.ascontiguousarray(np.moveaxis(rgb, -1, 0)).astype(np.float32),
                           depth=np.where(hit, z, 0.0).astype(np.float32), alpha=hit.astype(np.float32), depth_trunc=float(depth_trunc)))
    return frames


# ---- unit-blocked storage ---------------------------------------------------------------------------------------------------
def block(arr, units):
    """[X, Y, Z] -> the flat unit-blocked order of include/ga_tsdf.h (the inverse of ``TSDFVolume.dense()``'s unblock): voxel
    (x, y, z) at ((ux Uy + uy) Uz + uz) 4096 + (z & 15) 256 + (x & 15) 16 + (y & 15)"""
    ux, uy, uz = units
    a = np.asarray(arr).reshape(ux, UNIT, uy, UNIT, uz, UNIT)           # (ux, lx, uy, ly, uz, lz)
    return np.ascontiguousarray(a.transpose(0, 2, 4, 5, 1, 3)).reshape(-1)


def load_dense(hvol, tsdf, weight, color, allocated):
    """write [X,Y,Z] host arrays (colour [3,X,Y,Z], allocated [Ux,Uy,Uz]) into a TSDFVolume's storage"""
    import torch
    units = tuple(hvol.units)
    assert tsdf.shape == tuple(UNIT * u for u in units) and np.asarray(allocated).shape == units
    hvol.tsdf.copy_(torch.from_numpy(block(np.asarray(tsdf, np.float32), units)))
    hvol.weight.copy_(torch.from_numpy(block(np.asarray(weight, np.float32), units)))
    hvol.color.copy_(torch.from_numpy(np.stack([block(np.asarray(color[c], np.float32), units) for c in range(3)])))
    hvol.allocated.copy_(torch.from_numpy(np.ascontiguousarray(allocated).astype(np.uint8).reshape(-1)))


def hip_volume_like(ovol, dev, depth_sampling_stride=4):
    """a TSDFVolume over the same box of units as the oracle volume"""
    from gaussiananything_amd import mesh
    ul = ovol.voxel_length * UNIT
    lo = [(u + 0.5) * ul for u in ovol.unit0]
    hi = [(u0 + n - 0.5) * ul for u0, n in zip(ovol.unit0, ovol.units)]
    hvol = mesh.TSDFVolume(ovol.voxel_length, ovol.sdf_trunc, lo, hi, device=dev, depth_sampling_stride=depth_sampling_stride)
    assert hvol.units == list(ovol.units) and hvol.unit0 == list(ovol.unit0)
    return hvol


def fuse_both(dev, frames, units, unit0, voxel, trunc, alpha_thres=0.08, stride=4):
    """the frames through the oracle and through the HIP path; the opened units are compared frame by frame"""
    import torch
    ovol = otsdf.Volume(units, unit0, voxel, trunc)
    hvol = hip_volume_like(ovol, dev, stride)
    for f in frames:
        with np.errstate(invalid="ignore", over="ignore"):
            touched = otsdf.integrate(ovol, f["rgb"], f["depth"], f["alpha"], alpha_thres, f["depth_trunc"], f["intr"], f["ext"],
                                      stride=stride)
        hvol.integrate(torch.from_numpy(f["rgb"]), torch.from_numpy(f["depth"]), f["intr"], f["ext"], f["depth_trunc"],
                       alpha=None if f["alpha"] is None else torch.from_numpy(f["alpha"]), alpha_thres=alpha_thres)
        check_units(hvol.touched.cpu().numpy().reshape(units).astype(bool), touched)
    return ovol, hvol


# ---- the named marching-cubes volumes ------------------------------------------------------------------------------------------
MC_NAMES = ("M1", "M2", "M3", "M4", "M5a", "M5b", "M5c", "M5d")


def _noise_volume(units, unit0, voxel, seed):
    rng = np.random.default_rng(seed)
    vol = otsdf.Volume(units, unit0, voxel, 6 * voxel)
    vol.tsdf[:] = rng.uniform(-1, 1, vol.tsdf.shape).astype(np.float32)
    vol.color[:] = rng.uniform(0, 255, vol.color.shape).astype(np.float32)
    vol.weight[:] = 1
    vol.allocated[:] = True
    return vol, rng


def _unit_slices(u):
    return tuple(slice(UNIT * k, UNIT * (k + 1)) for k in u)


@functools.lru_cache(maxsize=None)
def mc_volume(name):
    """One of the named volumes (built once, shared, never written to by a test).  The input keeps the contract the kernels rely
    on -- a unit that is not allocated holds weight 0 only -- since the oracle does not look at ``allocated``."""
    if name == "M1":      # white noise: practically all of the 256 cube cases, every ambiguous face next to every other
        vol, _ = _noise_volume((2, 2, 2), (0, 0, 0), 1.0, 7)
    elif name == "M2":    # holes scattered through the volume, a unit never opened, a unit opened and empty
        vol, rng = _noise_volume((2, 3, 2), (-1, -2, 0), 0.0125, 11)
        vol.weight[rng.uniform(size=vol.weight.shape) < 0.03] = 0
        vol.weight[_unit_slices((1, 1, 0))] = 0
        vol.allocated[1, 1, 0] = False
        vol.weight[_unit_slices((0, 2, 1))] = 0
    elif name == "M3":    # more than 1024 units: linear indices 1023 and 1024 are neighbours along z
        vol, rng = _noise_volume((3, 3, 120), (0, 0, -60), 0.01, 13)
        seen = np.zeros(vol.units, bool)
        for u in ((0, 0, 5), (1, 1, 0), (2, 2, 63), (2, 2, 64), (2, 2, 119)):
            seen[u] = True
        assert (2 * 3 + 2) * 120 + 63 == 1023
        vol.allocated[:] = seen
        vol.weight[:] = np.repeat(np.repeat(np.repeat(seen, UNIT, 0), UNIT, 1), UNIT, 2)
    elif name == "M4":    # exact zeros of both signs and saturated values
        vol, rng = _noise_volume((1, 2, 1), (3, -1, 0), 0.5, 17)
        r = rng.uniform(size=vol.tsdf.shape)
        for lo, hi, val in ((0.0, 0.05, 0.0), (0.05, 0.10, -0.0), (0.10, 0.20, 1.0), (0.20, 0.30, -1.0)):
            vol.tsdf[(r >= lo) & (r < hi)] = np.float32(val)
        assert (np.signbit(vol.tsdf) & (vol.tsdf == 0)).any() and (~np.signbit(vol.tsdf) & (vol.tsdf == 0)).any()
    elif name in ("M5a", "M5b", "M5c", "M5d"):    # one sign change in the middle, on the first voxel, on the last voxel, none
        vol, _ = _noise_volume((1, 1, 1), (-1, 0, 2), 0.25, 19)
        vol.tsdf[:] = 0.5
        at = {"M5a": (7, 7, 7), "M5b": (0, 0, 0), "M5c": (15, 15, 15), "M5d": None}[name]
        if at is not None:
            vol.tsdf[at] = -0.5
    else:
        raise KeyError(name)
    assert not vol.weight[np.repeat(np.repeat(np.repeat(~vol.allocated, UNIT, 0), UNIT, 1), UNIT, 2)].any()
    for a in (vol.tsdf, vol.weight, vol.color, vol.allocated):
        a.setflags(write=False)
    return vol


def mc_volumes():
    return {name: mc_volume(name) for name in MC_NAMES}


@functools.lru_cache(maxsize=None)
def mc_oracle_mesh(name):
    """the oracle's mesh of a named volume: computed once, shared, left unchanged"""
    out = otsdf.extract_mesh(mc_volume(name))
    for a in out:
        a.setflags(write=False)
    return out


def cube_cases(vol):
    """[X-1, Y-1, Z-1] case of every cube, -1 where a corner has not been observed"""
    R = vol.tsdf.shape
    ins, seen = vol.tsdf < 0, vol.weight != 0
    case = np.zeros(tuple(r - 1 for r in R), np.int32)
    valid = np.ones(case.shape, bool)
    for i in range(8):
        o = (i & 1, (i >> 1) & 1, (i >> 2) & 1)
        sl = tuple(slice(o[k], R[k] - 1 + o[k]) for k in range(3))
        case |= ins[sl].astype(np.int32) << i
        valid &= seen[sl]
    return np.where(valid, case, -1)


def independent_vertices(vol):
    """Which edges carry a vertex, and where, without the case table and without the ownership formulas: the edge from voxel p
    along an axis carries one iff ``tsdf < 0`` differs at its ends and one of the (up to four) cubes around it has eight observed
    corners.  -> [n, 3] float32, sorted lexicographically."""
    f, R = vol.tsdf, vol.tsdf.shape
    ins = f < 0
    whole = cube_cases(vol) >= 0
    vl, half = vol.voxel_length, vol.voxel_length * 0.5
    out = []
    for axis in range(3):
        others = [k for k in range(3) if k != axis]
        lo = tuple(slice(0, R[k] - 1) if k == axis else slice(None) for k in range(3))
        hi = tuple(slice(1, R[k]) if k == axis else slice(None) for k in range(3))
        around = np.zeros(ins[lo].shape, bool)
        for da in (0, 1):
            for db in (0, 1):      # the cube anchored da below the edge on the one other axis, db on the other
                sl = [slice(None)] * 3
                sl[others[0]] = slice(da, R[others[0]] - 1 + da)
                sl[others[1]] = slice(db, R[others[1]] - 1 + db)
                around[tuple(sl)] |= whole
        p = np.stack(np.nonzero((ins[lo] != ins[hi]) & around), 1)
        q = p.copy()
        q[:, axis] += 1
        f0 = np.abs(f[tuple(p.T)].astype(np.float64))
        f1 = np.abs(f[tuple(q.T)].astype(np.float64))
        pt = half + vl * (p & 15).astype(np.float64)
        pt[:, axis] += f0 * vl / (f0 + f1)
        org = (np.array(vol.unit0) + (p >> 4)).astype(np.float64) * vol.unit_length
        out.append((pt + org).astype(np.float32))
    return sort_rows(np.concatenate(out))


def sort_rows(v):
    v = np.asarray(v)
    return v[np.lexsort((v[:, 2], v[:, 1], v[:, 0]))] if len(v) else v.reshape(0, 3)


# ---- the comparisons -----------------------------------------------------------------------------------------------------------
def _largest(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return float(d.max()) if d.size else 0.0


def check_units(got, want):
    """opened / allocated units: identical"""
    got, want = np.asarray(got).astype(bool), np.asarray(want).astype(bool)
    assert got.shape == want.shape and np.array_equal(got, want), f"units differ at {np.argwhere(got != want)[:4].tolist()}"


def check_volume(got, want):
    """``(tsdf, weight, colour[3], allocated)`` of the HIP path against the oracle's: no voxel exempt.  -> the figures"""
    (t, w, c, a), (ot, ow, oc, oa) = got, want
    check_units(a, oa)
    assert np.array_equal(w, ow), f"observation counts differ at {np.argwhere(np.asarray(w) != np.asarray(ow))[:4].tolist()}"
    figures = dict(tsdf=_largest(t, ot), color=_largest(c, oc), tsdf_not_identical=int((np.asarray(t) != np.asarray(ot)).sum()),
                   color_not_identical=int((np.asarray(c) != np.asarray(oc)).sum()))
    print("volume against the oracle:", figures)
    worst = np.unravel_index(np.argmax(np.abs(np.asarray(t, np.float64) - ot)), np.shape(t))
    assert figures["tsdf"] <= TSDF_BAR, (figures, "voxel", worst)              # (a NaN fails both)
    assert figures["color"] <= COLOR_VOLUME_BAR, figures
    return figures


def check_mesh(got, want):
    """``(vertices, colours, triangles)`` of the HIP path against the oracle's: the same counts, identical index lists, positions and
    colours within the bar, every slot written (no NaN, no -1).  -> the figures"""
    (v, c, t), (ov, oc, ot) = got, want
    assert v.shape == ov.shape and c.shape == oc.shape and t.shape == ot.shape, (v.shape, ov.shape, t.shape, ot.shape)
    assert not np.isnan(v).any() and not np.isnan(c).any() and not (np.asarray(t) < 0).any(), "a slot was not written"
    assert np.array_equal(t, ot), f"triangle index lists differ from triangle {int(np.argwhere((t != ot).any(1))[0, 0])} on"
    figures = dict(vertices=_largest(v, ov), colors=_largest(c, oc), vertices_not_identical=int((v != ov).any(1).sum()) if len(v) else 0,
                   colors_not_identical=int((c != oc).any(1).sum()) if len(c) else 0)
    print("mesh against the oracle:", len(v), "vertices", len(t), "triangles", figures)
    assert figures["vertices"] <= VERTEX_BAR and figures["colors"] <= VERTEX_BAR, figures
    return figures


def check_mesh_invariants(triangles, nv, base=0):
    """what every mesh of this extraction has, whatever the field: indices in [base, base + nv), every vertex referenced, an
    undirected edge used at most twice and a directed edge at most once (int64 keys a nv + b)"""
    t = np.asarray(triangles, np.int64).reshape(-1, 3) - base
    if nv == 0 or len(t) == 0:
        assert nv == 0 and len(t) == 0, (nv, len(t))
        return
    assert t.min() >= 0 and t.max() < nv, (int(t.min()), int(t.max()), nv)
    assert len(np.unique(t)) == nv, f"{nv - len(np.unique(t))} vertices are not referenced"
    a, b = np.concatenate([t[:, 0], t[:, 1], t[:, 2]]), np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    assert (a != b).all(), "degenerate triangle"
    _, directed = np.unique(a * nv + b, return_counts=True)
    _, undirected = np.unique(np.minimum(a, b) * nv + np.maximum(a, b), return_counts=True)
    assert directed.max() <= 1, "a directed edge is used twice"
    assert undirected.max() <= 2, "an edge is shared by more than two triangles"
