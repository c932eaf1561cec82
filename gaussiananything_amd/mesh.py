"""TSDF fusion of the rendered views and mesh export -- the host side of include/ga_tsdf.h.

Mirrors the reference's mesh export of a generated object, function by function:
    FlowMatchingEngine_gs.export_mesh_from_2dgs   /root/reference/nsr/lsgm/flow_matching_trainer.py:1244-1315
    FlowMatchingEngine_gs.extract_mesh_bounded    /root/reference/nsr/lsgm/flow_matching_trainer.py:1318-1395
    to_cam_open3d_compat, post_process_mesh       /root/reference/utils/mesh_util.py:80-110, 22-44
with Open3D's ScalableTSDFVolume (CPU, third party) replaced by ``TSDFVolume`` (HIP kernels, csrc/tsdf.hip; dense over the
bounding cube, which 288 GB of HBM afford).  Fusion, marching cubes and the connected-component filter of ``post_process_mesh`` run on the GPU; the OBJ
writer is a host function of the library.  There is no CPU
fallback: without the HIP library the calls raise.

Meshes IN, at the end of the file (include/ga_mesh.h, csrc/mesh_ops.hip): ``sample_points_from_mesh`` (area-weighted
surface samples), ``point_mesh_distance`` (distance to the surface, brute force) and ``mesh_cloud_distance`` (our own, unpinned
accuracy / completeness / F-score between a mesh and a cloud)."""
import collections
import ctypes
import math
import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from .pointcloud import _stream

UNIT = 16


def to_cam_open3d_compat(c: dict, image_size: int = 512):
    """utils/mesh_util.py:80-110: pinhole intrinsics (fx, fy, cx, cy) and the 4x4 world->camera extrinsic of one camera in the
    reference's 3DGS format (``cam_view`` row-vector convention; ``projection_matrix`` if present, else ``tanfov``)."""
    W = H = image_size
    if "projection_matrix" in c:
        pm = torch.as_tensor(c["projection_matrix"]).float().cpu()
        ndc2pix = torch.tensor([[W / 2, 0, 0, (W - 1) / 2], [0, H / 2, 0, (H - 1) / 2], [0, 0, 0, 1]]).float().T
        intr = (pm @ ndc2pix)[:3, :3].T
        fx, fy, cx, cy = intr[0, 0].item(), intr[1, 1].item(), intr[0, 2].item(), intr[1, 2].item()
    else:
        t = c["tanfov"]
        tx, ty = (t, t) if not isinstance(t, (tuple, list)) else t
        # getProjectionMatrix stores 1 / tan(fov / 2) in a float32 matrix; the product with W / 2 is a float32 product
        fx = float(np.float32(1.0 / float(tx)) * np.float32(W / 2))
        fy = float(np.float32(1.0 / float(ty)) * np.float32(H / 2))
        cx, cy = float(np.float32((W - 1) / 2)), float(np.float32((H - 1) / 2))
    extrinsic = np.asarray(torch.as_tensor(c["cam_view"]).float().cpu().T.numpy(), dtype=np.float64)
    return (fx, fy, cx, cy), extrinsic


class TSDFVolume:
    """Dense stand-in for ``o3d.pipelines.integration.ScalableTSDFVolume(voxel_length, sdf_trunc, RGB8)`` over the box
    [bound_min, bound_max] (rounded outwards to whole 16^3-voxel units of Open3D's unit lattice)."""

    def __init__(self, voxel_length: float, sdf_trunc: float, bound_min: Sequence[float], bound_max: Sequence[float],
                 device="cuda", depth_sampling_stride: int = 4):
        self.voxel_length, self.sdf_trunc = float(voxel_length), float(sdf_trunc)
        self.stride = int(depth_sampling_stride)
        ul = self.voxel_length * UNIT
        self.unit0 = [int(math.floor(float(b) / ul)) for b in bound_min]
        hi = [int(math.floor(float(b) / ul)) for b in bound_max]
        self.units = [h - l + 1 for l, h in zip(self.unit0, hi)]
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("TSDFVolume runs on the GPU only (no CPU fallback)")
        n_units = self.units[0] * self.units[1] * self.units[2]
        self.nvox = n_units * UNIT ** 3
        self.tsdf = torch.zeros(self.nvox, dtype=torch.float32, device=self.device)
        self.weight = torch.zeros(self.nvox, dtype=torch.float32, device=self.device)
        self.color = torch.zeros(3, self.nvox, dtype=torch.float32, device=self.device)
        self.touched = torch.zeros(n_units, dtype=torch.uint8, device=self.device)
        self.allocated = torch.zeros(n_units, dtype=torch.uint8, device=self.device)
        self._c = _lib.GaTsdfVolume((ctypes.c_int32 * 3)(*self.units), (ctypes.c_int32 * 3)(*self.unit0), self.voxel_length,
                                    self.sdf_trunc, self.tsdf.data_ptr(), self.weight.data_ptr(), self.color.data_ptr(),
                                    self.touched.data_ptr(), self.allocated.data_ptr())

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def integrate(self, rgb: torch.Tensor, depth: torch.Tensor, intrinsic, extrinsic, depth_trunc: float,
                  alpha: Optional[torch.Tensor] = None, alpha_thres: float = 0.0):
        """``volume.integrate(RGBDImage.create_from_color_and_depth(uint8(clip(rgb) * 255), depth, depth_trunc, depth_scale=1),
        intrinsic, extrinsic)`` with ``depth[alpha < alpha_thres] = 0`` applied first (flow_matching_trainer.py:1371-1390).
        rgb [3,H,W], depth [H,W] or [1,H,W], alpha likewise; intrinsic = (fx, fy, cx, cy); extrinsic 4x4 world->camera."""
        rgb = rgb.detach().to(self.device, torch.float32).contiguous()
        depth = depth.detach().to(self.device, torch.float32).reshape(depth.shape[-2], depth.shape[-1]).contiguous()
        H, W = depth.shape
        if rgb.shape != (3, H, W):
            raise ValueError(f"rgb {tuple(rgb.shape)} does not match depth {tuple(depth.shape)}")
        if alpha is not None:
            alpha = alpha.detach().to(self.device, torch.float32).reshape(H, W).contiguous()
        ext = np.asarray(extrinsic, dtype=np.float64).reshape(4, 4)
        pose = np.linalg.inv(ext)
        fx, fy, cx, cy = (float(v) for v in intrinsic)
        fr = _lib.GaTsdfFrame(H, W, rgb.data_ptr(), depth.data_ptr(), alpha.data_ptr() if alpha is not None else None,
                              float(alpha_thres), float(depth_trunc), fx, fy, cx, cy,
                              (ctypes.c_double * 16)(*ext.reshape(-1).tolist()), (ctypes.c_double * 16)(*pose.reshape(-1).tolist()),
                              self.stride)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().ga_tsdf_integrate(ctypes.byref(self._c), ctypes.byref(fr), self._stream()), "ga_tsdf_integrate")

    def extract_triangle_mesh(self):
        """-> vertices [nv,3] float32 (world), vertex colours [nv,3] in [0,1], triangles [nt,3] int32, on the device."""
        L = _lib.lib()
        nbytes = int(L.ga_tsdf_mesh_scratch_bytes(ctypes.byref(self._c)))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        counts = torch.zeros(2, dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(L.ga_tsdf_mesh_count(ctypes.byref(self._c), scratch.data_ptr(), nbytes, counts.data_ptr(), self._stream()),
                       "ga_tsdf_mesh_count")
            nv, nt = (int(v) for v in counts.cpu().tolist())   # the one read-back: the size of the mesh
            vertices = torch.empty(nv, 3, dtype=torch.float32, device=self.device)
            colors = torch.empty(nv, 3, dtype=torch.float32, device=self.device)
            triangles = torch.empty(nt, 3, dtype=torch.int32, device=self.device)
            _lib.check(L.ga_tsdf_mesh_emit(ctypes.byref(self._c), scratch.data_ptr(), nbytes, nv, nt, vertices.data_ptr(),
                                           colors.data_ptr(), triangles.data_ptr(), self._stream()), "ga_tsdf_mesh_emit")
        return vertices, colors, triangles

    def dense(self):
        """(tsdf, weight, colour[3]) as [X, Y, Z] arrays on the host (unit-blocked storage undone): for tests and inspection."""
        ux, uy, uz = self.units

        def unblock(t):
            return t.reshape(ux, uy, uz, UNIT, UNIT, UNIT).permute(0, 4, 1, 5, 2, 3).reshape(ux * UNIT, uy * UNIT, uz * UNIT).cpu().numpy()

        return unblock(self.tsdf), unblock(self.weight), np.stack([unblock(self.color[c]) for c in range(3)])


def extract_mesh_bounded(rgbmaps, depthmaps, alpha_maps, cam_pathes, aabb, alpha_thres: float = 0.08, image_size: int = 512,
                         device="cuda"):
    """flow_matching_trainer.py:1318-1395 with the aabb branch it always takes: voxel = radius / 160, sdf_trunc = 12 voxels,
    per-camera depth_trunc = |campos - centre| + radius.  ``cam_pathes``: the reference's 3DGS-format camera dicts
    (``cam_view``, ``cam_pos``, ``tanfov`` or ``projection_matrix``); maps indexed [i][0] as in the reference."""
    aabb = np.asarray(aabb, dtype=np.float64).reshape(2, 3)
    center = aabb.mean(0)
    radius = float(np.linalg.norm(aabb[1] - aabb[0]) * 0.5)
    voxel_size = radius / 160
    sdf_trunc = voxel_size * 12
    # every depth point within a camera's depth_trunc lies in the ball of `radius` about the centre or in front of it; the box
    # of the dense volume is that ball plus the truncation band (Open3D would also open units further out: include/ga_tsdf.h)
    volume = TSDFVolume(voxel_size, sdf_trunc, center - radius - sdf_trunc, center + radius + sdf_trunc, device=device)
    for i, cam in enumerate(cam_pathes):
        intr, ext = to_cam_open3d_compat(cam, image_size)
        campos = torch.as_tensor(cam["cam_pos"]).detach().cpu().numpy().astype(np.float64).reshape(-1)[:3]
        depth_trunc = float(np.linalg.norm(campos - center, axis=-1) + radius)
        volume.integrate(rgbmaps[i][0], depthmaps[i][0], intr, ext, depth_trunc, alpha=alpha_maps[i][0], alpha_thres=alpha_thres)
    return volume.extract_triangle_mesh()


def _propagate_labels(a, b, nt, dev):
    """min-label propagation with root hooking and pointer jumping, device-agnostic torch operations (round 2-4's device path)"""
    label = torch.arange(nt, device=dev, dtype=torch.int32)   # (32-bit labels: native atomic min)
    for _ in range(100000):
        la, lb = label[a], label[b]
        act = la != lb       # a pair whose ends already share a label changes nothing in this round; leaving it out keeps
        aa, bb, la, lb = a[act], b[act], la[act].long(), lb[act].long()   # the atomics off the big clusters' representatives
        m = torch.minimum(la, lb).to(torch.int32)
        # hook the smaller label under both triangles and under their current representatives (links trees, not only
        # neighbours: logarithmically many rounds instead of one per edge of the longest chain), then jump pointers
        new = label.scatter_reduce(0, la, m, "amin").scatter_reduce(0, lb, m, "amin")
        new = new.scatter_reduce(0, aa, m, "amin").scatter_reduce(0, bb, m, "amin")
        new = new[new.long()]
        new = new[new.long()]
        if torch.equal(new, label):
            break
        label = new
    post_process_mesh.rounds = _ + 1
    return label


def post_process_mesh(vertices, colors, triangles):
    """utils/mesh_util.py:22-44: keep the (at most) ten largest connected triangle clusters and none below 50 triangles
    (clusters = triangles joined through shared edges, Open3D's cluster_connected_triangles), then drop unreferenced vertices
    and degenerate triangles.  Tensors in, tensors out, on the tensors' device (the mesh of a generated object has about a
    million triangles: Open3D and a scipy restatement take half a second on the host for this; here the edge sort, the
    min-label propagation with pointer jumping and the compaction are device-wide torch operations, a few milliseconds).
    numpy arrays are accepted too (and returned as numpy)."""
    if isinstance(vertices, np.ndarray):
        dev = torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")
        out = post_process_mesh(torch.from_numpy(vertices).to(dev), torch.from_numpy(colors).to(dev), torch.from_numpy(triangles).to(dev))
        return tuple(o.cpu().numpy() for o in out)
    t = triangles.long()
    nt, nv = t.shape[0], vertices.shape[0]
    if nt == 0:
        return vertices[:0], colors[:0], triangles[:0].to(torch.int32)
    dev = t.device
    ea, eb = torch.cat([t[:, 0], t[:, 1], t[:, 2]]), torch.cat([t[:, 1], t[:, 2], t[:, 0]])
    key, order = torch.sort(torch.minimum(ea, eb) * nv + torch.maximum(ea, eb))
    owner = torch.arange(nt, device=dev).repeat(3)[order]
    same = key[1:] == key[:-1]
    a, b = owner[:-1][same], owner[1:][same]          # triangles that share an edge
    if dev.type == "cuda":
        # round 5: one lock-free union-find pass on the device (ga_mesh_cluster_labels, csrc/tsdf.hip): labels = the smallest triangle of
        # each cluster, as the propagation below converges to
        label = torch.empty(nt, device=dev, dtype=torch.int32)
        a, b = a.contiguous(), b.contiguous()
        _lib.check(_lib.lib().ga_mesh_cluster_labels(a.data_ptr(), b.data_ptr(), a.numel(), label.data_ptr(), nt,
                                                     ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "ga_mesh_cluster_labels")
        post_process_mesh.rounds = 1
    else:
        label = _propagate_labels(a, b, nt, dev)      # host tensors (the CPU tests): the same clusters with torch operations
    label = label.long()
    # cluster sizes at the clusters' smallest triangles.  Not torch.bincount: a generated object is ONE big cluster, i.e. a million
    # atomic increments of one address (12 of the 14 ms of this function on the device); a sort and run lengths instead
    uniq, counts = torch.unique_consecutive(torch.sort(label).values, return_counts=True)
    cluster_n = torch.zeros(nt, dtype=torch.long, device=dev)
    cluster_n[uniq] = counts
    sizes = torch.sort(cluster_n[cluster_n > 0]).values
    cluster_to_keep = min(int(sizes.numel()), 10)
    n_cluster = max(int(sizes[-cluster_to_keep]), 50)
    t = t[cluster_n[label] >= n_cluster]
    flags = torch.zeros(nv, dtype=torch.bool, device=dev)          # referenced vertices, ascending (what torch.unique's sort gave)
    flags[t.reshape(-1)] = True
    used = flags.nonzero().squeeze(1)
    remap = torch.cumsum(flags, 0) - 1
    t = remap[t]
    t = t[(t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])]
    return vertices[used], colors[used], t.to(torch.int32)


def rotation_matrix_x(theta_degrees: float) -> np.ndarray:
    """flow_matching_trainer.py:67-75"""
    th = np.radians(theta_degrees)
    c, s = np.cos(th), np.sin(th)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def rotation_matrix_y(theta: float) -> np.ndarray:
    """flow_matching_trainer.py (rotation about y by theta RADIANS, as the reference's helper takes it)"""
    c, s = np.cos(theta), np.sin(theta)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def write_obj(path: str, vertices, colors, triangles):
    """Wavefront OBJ with per-vertex colours (`v x y z r g b`), the form o3d.io.write_triangle_mesh gives a coloured mesh;
    written by the library's host function ga_mesh_write_obj (1.6 M lines in a fraction of a second)."""
    def host(x, dt):
        if isinstance(x, torch.Tensor):
            x = x.detach().cpu().numpy()
        return np.ascontiguousarray(x, dtype=dt)
    v, c, t = host(vertices, np.float32), host(colors, np.float32), host(triangles, np.int32)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    _lib.check(_lib.lib().ga_mesh_write_obj(os.fsencode(path), v.ctypes.data, c.ctypes.data, t.ctypes.data, v.shape[0], t.shape[0]),
               "ga_mesh_write_obj")


def export_mesh_from_2dgs(all_rgbs, all_depths, all_alphas, cam_pathes, mesh_output_path: str, image_size: int = 512, device="cuda"):
    """flow_matching_trainer.py:1244-1315: fuse, write `<name>-mesh_raw.obj`, post-process, rotate (x by -90 degrees, then y by
    pi) and write `<name>.obj`; returns the post-processed path.  ``mesh_output_path`` is the raw mesh's path
    (must end in `_raw.obj`)."""
    aabb = np.array([-0.45, -0.45, -0.45, 0.45, 0.45, 0.45]).reshape(2, 3) * 1.1
    v, c, t = extract_mesh_bounded(all_rgbs, all_depths, all_alphas, cam_pathes, aabb, image_size=image_size, device=device)
    write_obj(mesh_output_path, v, c, t)
    pv, pc, pt = post_process_mesh(v, c, t)
    rot = torch.from_numpy(rotation_matrix_y(np.pi) @ rotation_matrix_x(-90)).to(pv.device)   # x by -90 degrees, then y by pi
    pv = (pv.double() @ rot.T).float()
    post_path = mesh_output_path.replace("_raw.obj", ".obj")
    write_obj(post_path, pv, pc, pt)
    return post_path


# ---- meshes in: surface sampling and the point-to-surface distance (include/ga_mesh.h, csrc/mesh_ops.hip) --------------------------
# One mesh per call: batches of meshes are not built, a caller loops.

def _mesh(vertices, faces):
    """fp32 [V,3] and int32 [F,3] contiguous device copies of a mesh; GPU only"""
    if not isinstance(vertices, torch.Tensor) or not isinstance(faces, torch.Tensor):
        raise ValueError("vertices and faces are tensors")
    if vertices.dim() != 2 or vertices.shape[1] != 3 or vertices.shape[0] < 1 or faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise ValueError("a mesh is vertices [V, 3] and faces [F, 3] with V, F >= 1 (one mesh per call)")
    if vertices.device.type != "cuda" or faces.device != vertices.device:
        raise RuntimeError("the mesh must be on the GPU (no CPU fallback)")
    return vertices.detach().to(torch.float32).contiguous(), faces.detach().to(torch.int32).contiguous()


def mesh_sample_plan(num_faces: int, num_samples: int = 1) -> dict:
    """What ``ga_mesh_sample`` does for a mesh of ``num_faces``: {'threads', 'faces_per_group', 'sums_per_trip', 'num_groups',
    'workspace_bytes'}."""
    pl = _lib.GaMeshSamplePlan()
    _lib.check(_lib.lib().ga_mesh_sample_plan(int(num_faces), int(num_samples), ctypes.byref(pl)), "ga_mesh_sample_plan")
    return {n: int(getattr(pl, n)) for n, _ in pl._fields_}


def point_mesh_distance_plan(num_points: int, num_faces: int) -> dict:
    """What ``ga_mesh_point_distance`` does: {'threads', 'tile', 'tiles_per_chunk', 'num_chunks', 'workspace_bytes'}."""
    pl = _lib.GaMeshPointDistancePlan()
    _lib.check(_lib.lib().ga_mesh_point_distance_plan(int(num_points), int(num_faces), ctypes.byref(pl)), "ga_mesh_point_distance_plan")
    return {n: int(getattr(pl, n)) for n, _ in pl._fields_}


@torch.no_grad()
def sample_points_from_mesh(vertices, faces, num_samples: int = 10000, *, colors=None, seed=0, return_normals: bool = False,
                            return_faces: bool = False):
    """Area-weighted samples of a triangle mesh's surface, what ``pytorch3d.ops.sample_points_from_meshes`` gives for one mesh (its
    barycentric formula; the random stream and the face search are this project's, parity unpinned): -> points [S,3], or a tuple
    (points[, normals][, colors][, (face [S] int64, bary [S,3])]) in that order for what is asked.  ``colors`` [V,3]: per-vertex
    colours, interpolated barycentrically.  ``seed``: an int, or a device tensor of two 32-bit words (int32 or uint32: low, high) that
    the kernel reads when it runs -- a captured graph draws fresh samples after the tensor is overwritten.  Faces with an index out of
    range or of zero or non-finite area are never drawn; a mesh without any other face yields face -1 and zero rows.  Three launches
    on the current stream, no host read; the tensors stay on the mesh's device."""
    v, f = _mesh(vertices, faces)
    S = int(num_samples)
    if S < 1:
        raise ValueError("num_samples must be at least 1")
    dev = v.device
    vc = None
    if colors is not None:
        if colors.shape != v.shape or colors.device != dev:
            raise ValueError("colors is a [V, 3] tensor on the mesh's device")
        vc = colors.detach().to(torch.float32).contiguous()
    words, host_seed = None, 0
    if isinstance(seed, torch.Tensor):
        if seed.device != dev or seed.numel() != 2 or seed.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or not seed.is_contiguous():
            raise ValueError("a device seed is a contiguous tensor of two 32-bit words on the mesh's device")
        words = seed
    else:
        host_seed = int(seed) & ((1 << 64) - 1)
    L = _lib.lib()
    pl = _lib.GaMeshSamplePlan()
    _lib.check(L.ga_mesh_sample_plan(f.shape[0], S, ctypes.byref(pl)), "ga_mesh_sample_plan")
    ws = torch.empty(pl.workspace_bytes, dtype=torch.uint8, device=dev)
    points = torch.empty(S, 3, dtype=torch.float32, device=dev)
    face = torch.empty(S, dtype=torch.int32, device=dev)
    bary = torch.empty(S, 3, dtype=torch.float32, device=dev)
    normals = torch.empty(S, 3, dtype=torch.float32, device=dev) if return_normals else None
    out_colors = torch.empty(S, 3, dtype=torch.float32, device=dev) if vc is not None else None
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    args = _lib.GaMeshSampleArgs(v.shape[0], f.shape[0], S, 0, host_seed, ptr(words), v.data_ptr(), f.data_ptr(), ptr(vc),
                                 points.data_ptr(), face.data_ptr(), bary.data_ptr(), ptr(normals), ptr(out_colors), ws.data_ptr(),
                                 pl.workspace_bytes)
    with torch.cuda.device(dev):
        _lib.check(L.ga_mesh_sample(ctypes.byref(args), _stream(dev)), "ga_mesh_sample")
    ret = [points] + ([normals] if return_normals else []) + ([out_colors] if vc is not None else []) + \
          ([(face.long(), bary)] if return_faces else [])
    return ret[0] if len(ret) == 1 else tuple(ret)


PointMeshDistance = collections.namedtuple("PointMeshDistance", "dist2 face closest bary")
PointMeshDistance.__doc__ = """``point_mesh_distance``'s result: dist2 [N] squared distance to the surface, face [N] int64 (the lowest
index among equally near faces; -1 on padding rows and without a valid triangle), closest [N,3] the nearest surface point, bary [N,3]
its barycentric weights on that face"""


def point_mesh_distance(points, vertices, faces, *, differentiable: bool = False):
    """Squared distance of every point to the SURFACE of a triangle mesh (not to its vertices), brute force over all faces on the
    device: -> ``PointMeshDistance``.  ``points``: a [N,3] tensor, or an untrimmed ``UnprojectedCloud`` / ``FilteredCloud`` (anything with
    ``points`` [N,3] and a device ``count``): rows past the count get distance 0 and face -1, the padding of ``nearest_points``.
    Degenerate and out-of-range faces are skipped; a row with no valid face gets +inf and -1.

    ``differentiable=True``: ``dist2`` is computed again in torch as ``|p - sum_k bary_k * vertices[faces[face], k]|^2`` with ``bary``
    and ``face`` detached.  The nearest point minimises the distance over the triangle, so by the envelope argument the derivative of
    the minimum is the derivative of this expression at the fixed minimiser: it is the gradient with respect to both ``points`` and
    ``vertices`` wherever the nearest face is unique.  No backward kernel is needed, and none is built."""
    count = None
    if not isinstance(points, torch.Tensor):
        points, count = points.points, points.count
    v, f = _mesh(vertices, faces)
    if points.dim() != 2 or points.shape[1] != 3 or points.shape[0] < 1 or points.device != v.device:
        raise ValueError("points is a [N, 3] tensor with N >= 1 on the mesh's device")
    p = points.detach().to(torch.float32).contiguous()
    dev, N = v.device, p.shape[0]
    if count is not None:
        count = count.detach().to(torch.int32).reshape(-1)[:1].contiguous()
    L = _lib.lib()
    pl = _lib.GaMeshPointDistancePlan()
    _lib.check(L.ga_mesh_point_distance_plan(N, f.shape[0], ctypes.byref(pl)), "ga_mesh_point_distance_plan")
    with torch.no_grad():
        ws = torch.empty(pl.workspace_bytes, dtype=torch.uint8, device=dev)
        dist2 = torch.empty(N, dtype=torch.float32, device=dev)
        face = torch.empty(N, dtype=torch.int32, device=dev)
        closest = torch.empty(N, 3, dtype=torch.float32, device=dev)
        bary = torch.empty(N, 3, dtype=torch.float32, device=dev)
        args = _lib.GaMeshPointDistanceArgs(N, v.shape[0], f.shape[0], 0, p.data_ptr(), count.data_ptr() if count is not None else None,
                                            v.data_ptr(), f.data_ptr(), dist2.data_ptr(), face.data_ptr(), closest.data_ptr(),
                                            bary.data_ptr(), ws.data_ptr(), pl.workspace_bytes)
        with torch.cuda.device(dev):
            _lib.check(L.ga_mesh_point_distance(ctypes.byref(args), _stream(dev)), "ga_mesh_point_distance")
        face = face.long()
    if differentiable:
        hit = face >= 0
        corners = vertices[faces.long()[face.clamp(min=0)]]                      # [N,3,3], differentiable in `vertices`
        nearest = (bary.unsqueeze(-1) * corners.to(torch.float32)).sum(1)
        d = ((points.to(torch.float32) - nearest) ** 2).sum(-1)
        dist2 = torch.where(hit, d, dist2)                                       # padding and faceless rows keep 0 / +inf, no gradient
    return PointMeshDistance(dist2, face, closest, bary)


@torch.no_grad()
def mesh_cloud_distance(vertices, faces, points, *, num_samples: int = 100000, threshold: Optional[float] = None, seed=0,
                        align: Optional[str] = None, max_iterations: int = 100):
    """How far a mesh lies from a cloud -- this project's OWN definition (no reference code for it runs here: UNPINNED):
        accuracy      mean distance from ``num_samples`` surface samples of the mesh to their nearest cloud point (``nearest_points``)
        completeness  mean distance from the cloud's points to the mesh surface (``point_mesh_distance``)
    and, with ``threshold`` (a distance), precision = the share of samples within it, recall = the share of cloud points within it and
    fscore = their harmonic mean (0 when both are 0).  ``points`` [N,3].  Distances, not squared.  -> dict of 0-dim device tensors;
    nothing is read back.

    ``align`` = "rigid" | "similarity" first registers the cloud to the mesh's surface samples (``pointcloud.iterative_closest_point``,
    at most ``max_iterations`` iterations, without / with scale) and measures the registered cloud; the dict then also holds
    ``transform`` (SimilarityTransform of one cloud: R [1,3,3], T [1,3], s [1]), ``converged`` [1] and ``points`` [N,3], the registered
    cloud.  ICP finds the nearest local optimum: a cloud far from the mesh's frame needs a coarse pose first.  ``align=None`` (the
    default) measures the cloud as given."""
    from .pointcloud import iterative_closest_point, nearest_points
    if align not in (None, "rigid", "similarity"):
        raise ValueError('align is None, "rigid" or "similarity"')
    samples = sample_points_from_mesh(vertices, faces, num_samples, seed=seed)
    cloud = points.detach().to(torch.float32).contiguous()
    extra = {}
    if align is not None:
        sol = iterative_closest_point(cloud[None], samples[None], max_iterations=max_iterations, estimate_scale=align == "similarity")
        cloud = sol.Xt[0]
        extra = {"transform": sol.RTs, "converged": sol.converged, "points": cloud}
    to_cloud = nearest_points(samples[None], cloud[None])[0][0].sqrt()
    to_mesh = point_mesh_distance(cloud, vertices, faces).dist2.sqrt()
    out = {"accuracy": to_cloud.mean(), "completeness": to_mesh.mean()}
    if threshold is not None:
        precision, recall = (to_cloud <= threshold).float().mean(), (to_mesh <= threshold).float().mean()
        both = precision + recall
        out.update(precision=precision, recall=recall, fscore=torch.where(both > 0, 2 * precision * recall / both.clamp(min=1e-30), both))
    out.update(extra)
    return out
