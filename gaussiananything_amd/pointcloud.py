"""Point-cloud operations of the generation side -- the host side of include/ga_pointcloud.h (HIP kernels, csrc/pointcloud.hip).

    sample_farthest_points   pytorch3d.ops.sample_farthest_points: what turns an arbitrary cloud into the ``fps-xyz`` of stage 2
                             (/root/reference/nsr/lsgm/flow_matching_trainer.py:1079, :1110-1134) and generated surfels into the
                             ``fps-4096.ply`` the geometry metrics are computed on (/root/reference/scripts/save_pcd_from_gs.py:148-185)
    nearest_points           nearest target (squared distance, index) of every query
    chamfer_distance         pytorch3d.loss.chamfer_distance for squared L2 without normals (/root/reference/nsr/train_nv_util.py:2244);
                             forward only by default, with gradients for ``differentiable=True`` (the reference's use as a loss)
    knn_points, knn_gather   pytorch3d.ops.knn_points / knn_gather (nsr/srt/encoder.py:884-923 of the reference), K <= 32, squared L2,
                             with gradients through ``ga_pc_knn_backward``
    remove_statistical_outliers   mean distance to the k nearest neighbours against the cloud's mean + ratio * deviation: OUR OWN
                             definition, parity with Open3D's filter of the same name is not claimed
    estimate_normals         PCA normals (and tangents, eigenvalues) from the k nearest neighbours, ``ga_pc_normals`` (csrc/pc_normals.hip):
                             OUR OWN definition, sign and invalid-row rules included
    surfels_from_cloud       initial 2D surfels [B,N,13] from a cloud, ``ga_pc_surfel_init``: 2DGS's distance rule for the scale, the
                             PCA frame for the rotation (``fitting.surfels_from_points`` is the single-cloud front end)
    unproject_depth_views    posed depth views (with optional mask, colour and normal maps) -> an ordered, compacted world-space cloud,
                             ``ga_pc_unproject`` (csrc/pc_unproject.hip): the reference's ``save_pcd_from_depth`` geometry
                             (/root/reference/scripts/save_pcd.py:323-403), three launches, the count stays on the device
    cloud_from_render        the same for the dict ``GaussianRenderer2DGS.render`` returns
    filter_view_consistency  keeps the points of such a cloud (or of any cloud) that the depth maps of the other views support and do
                             not contradict, ``ga_pc_filter_views`` (csrc/pc_filter.hip): OUR OWN rule, three launches, no host read
    voxel_thin               one measured point per occupied cell of a grid, ``ga_pc_voxel_thin``: a hash table filled with integer
                             atomics, the result a function of the input alone; five launches, no host read

pytorch3d is absent from this image; its published behaviour is restated, parity UNPINNED ('Point clouds').  The tensors
stay on the device and the work goes on the current stream.  There is no CPU fallback: without the HIP library, or on a CPU tensor,
the calls raise."""
from __future__ import annotations

import collections
import ctypes
import random
from typing import Optional

import torch

from . import _lib


def fps_plan(num_points: int, num_samples: int = 1) -> dict:
    """What ``ga_pc_fps`` does for clouds of ``num_points``: {'variant': 'register' | 'streaming', 'threads', 'points_per_lane'}."""
    pl = _lib.GaFpsPlan()
    _lib.check(_lib.lib().ga_pc_fps_plan(int(num_points), int(num_samples), ctypes.byref(pl)), "ga_pc_fps_plan")
    return {"variant": "streaming" if pl.variant == _lib.GA_FPS_VARIANT_STREAMING else "register", "threads": pl.threads,
            "points_per_lane": pl.points_per_lane}


def _cloud(t, name):
    if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[-1] != 3 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{name} is a [B, N, 3] tensor with B, N >= 1")
    if t.device.type != "cuda":
        raise RuntimeError(f"{name} must be on the GPU (no CPU fallback)")
    return t.detach().to(torch.float32).contiguous()


def _lengths(lengths, B, N, device, name):
    """host validation (1 <= length <= N) and the int32 device copy the kernels read; None stays None (= all N)"""
    if lengths is None:
        return None, [N] * B
    host = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
    if len(host) != B:
        raise ValueError(f"{name} has {len(host)} entries for a batch of {B}")
    if min(host) < 1 or max(host) > N:
        raise ValueError(f"{name} must lie in [1, {N}]")
    return torch.tensor(host, dtype=torch.int32, device=device), host


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


@torch.no_grad()
def sample_farthest_points(points: torch.Tensor, lengths=None, K: int = 50, random_start_point: bool = False, start_idx=None):
    """-> (points [B,K,3], idx [B,K] int64), pytorch3d's signature and return: slots past a cloud's length hold index -1 and zero
    points.  ``random_start_point`` draws each start with ``random.randint(0, n - 1)``, as pytorch3d does; ``start_idx`` ([B] ints)
    fixes the starts instead."""
    p = _cloud(points, "points")
    B, N, _ = p.shape
    K = int(K)
    if K < 1:
        raise ValueError("K must be at least 1")
    dev_lengths, host_lengths = _lengths(lengths, B, N, p.device, "lengths")
    if start_idx is not None:
        starts = [int(v) for v in (start_idx.tolist() if isinstance(start_idx, torch.Tensor) else start_idx)]
        if len(starts) != B or any(s < 0 or s >= n for s, n in zip(starts, host_lengths)):
            raise ValueError("start_idx needs one index in [0, length) per cloud")
    elif random_start_point:
        starts = [random.randint(0, n - 1) for n in host_lengths]
    else:
        starts = None
    dev_starts = torch.tensor(starts, dtype=torch.int32, device=p.device) if starts is not None else None
    L = _lib.lib()
    out_idx = torch.empty(B, K, dtype=torch.int32, device=p.device)
    out_points = torch.empty(B, K, 3, dtype=torch.float32, device=p.device)
    nbytes = int(L.ga_pc_fps_workspace_bytes(B, N, K))
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=p.device) if nbytes else None
    args = _lib.GaFpsArgs(B, N, K, p.data_ptr(), dev_lengths.data_ptr() if dev_lengths is not None else None,
                          dev_starts.data_ptr() if dev_starts is not None else None, out_idx.data_ptr(), out_points.data_ptr(),
                          workspace.data_ptr() if workspace is not None else None, nbytes)
    with torch.cuda.device(p.device):
        _lib.check(L.ga_pc_fps(ctypes.byref(args), _stream(p.device)), "ga_pc_fps")
    return out_points, out_idx.long()


@torch.no_grad()
def nearest_points(x: torch.Tensor, y: torch.Tensor, x_lengths=None, y_lengths=None):
    """For every point of ``x`` [B,Nx,3] its nearest point of ``y`` [B,Ny,3]: -> (dist2 [B,Nx] float32, idx [B,Nx] int64, the lowest
    index among equal distances).  Slots past ``x_lengths`` hold distance 0 and index -1."""
    xs, ys = _cloud(x, "x"), _cloud(y, "y")
    if xs.shape[0] != ys.shape[0] or xs.device != ys.device:
        raise ValueError("x and y need the same batch size and device")
    B, Nx, _ = xs.shape
    Ny = ys.shape[1]
    xl, _ = _lengths(x_lengths, B, Nx, xs.device, "x_lengths")
    yl, _ = _lengths(y_lengths, B, Ny, xs.device, "y_lengths")
    dist2 = torch.empty(B, Nx, dtype=torch.float32, device=xs.device)
    idx = torch.empty(B, Nx, dtype=torch.int32, device=xs.device)
    args = _lib.GaNearestArgs(B, Nx, Ny, xs.data_ptr(), ys.data_ptr(), xl.data_ptr() if xl is not None else None,
                              yl.data_ptr() if yl is not None else None, dist2.data_ptr(), idx.data_ptr())
    with torch.cuda.device(xs.device):
        _lib.check(_lib.lib().ga_pc_nearest(ctypes.byref(args), _stream(xs.device)), "ga_pc_nearest")
    return dist2, idx.long()


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _knn_backward(q, t, ql, tl, idx, grad, want_query, want_target):
    """``ga_pc_knn_backward`` on fp32 contiguous clouds, int32 ``idx`` [B,Nq,K] and fp32 ``grad`` [B,Nq,K] -> (grad_query, grad_target),
    each None when not wanted"""
    B, Nq, _ = q.shape
    Nt = t.shape[1]
    K = idx.shape[2]
    gq = torch.empty_like(q) if want_query else None
    gt = torch.empty_like(t) if want_target else None
    args = _lib.GaKnnBackwardArgs(B, Nq, Nt, K, q.data_ptr(), t.data_ptr(), _ptr(ql), _ptr(tl), idx.data_ptr(), grad.data_ptr(),
                                  _ptr(gq), _ptr(gt))
    with torch.cuda.device(q.device):
        _lib.check(_lib.lib().ga_pc_knn_backward(ctypes.byref(args), _stream(q.device)), "ga_pc_knn_backward")
    return gq, gt


class _NearestDist2(torch.autograd.Function):
    """squared distance of every point of ``x`` to its nearest point of ``y``: forward ``ga_pc_nearest``, backward
    ``ga_pc_knn_backward`` with k = 1 on the saved indices (the -1 of padded slots is never dereferenced: validity is the lengths')"""

    @staticmethod
    def forward(ctx, x, y, xl, yl):
        xs, ys = _cloud(x, "x"), _cloud(y, "y")
        B, Nx, _ = xs.shape
        dist2 = torch.empty(B, Nx, dtype=torch.float32, device=xs.device)
        idx = torch.empty(B, Nx, dtype=torch.int32, device=xs.device)
        args = _lib.GaNearestArgs(B, Nx, ys.shape[1], xs.data_ptr(), ys.data_ptr(), _ptr(xl), _ptr(yl), dist2.data_ptr(), idx.data_ptr())
        with torch.cuda.device(xs.device):
            _lib.check(_lib.lib().ga_pc_nearest(ctypes.byref(args), _stream(xs.device)), "ga_pc_nearest")
        ctx.save_for_backward(xs, ys, idx)
        ctx.lengths = (xl, yl)
        ctx.dtypes = (x.dtype, y.dtype)
        return dist2

    @staticmethod
    def backward(ctx, grad):
        xs, ys, idx = ctx.saved_tensors
        gx, gy = _knn_backward(xs, ys, ctx.lengths[0], ctx.lengths[1], idx.unsqueeze(-1), grad.to(torch.float32).contiguous().unsqueeze(-1),
                               ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return (gx.to(ctx.dtypes[0]) if gx is not None else None, gy.to(ctx.dtypes[1]) if gy is not None else None, None, None)


def chamfer_distance(x: torch.Tensor, y: torch.Tensor, x_lengths=None, y_lengths=None, batch_reduction: Optional[str] = "mean",
                     point_reduction: str = "mean", single_directional: bool = False, differentiable: bool = False):
    """-> (loss, None): ``pytorch3d.loss.chamfer_distance`` for squared L2 without normals -- for each direction the squared distance
    of every point to its nearest neighbour in the other cloud, summed (``point_reduction='sum'``) or averaged over the cloud's
    length ('mean'), the two directions added, then summed / averaged over the batch (``batch_reduction`` 'sum' | 'mean' | None =
    one value per cloud).  Two ``ga_pc_nearest`` launches and torch reductions on the device.  ``single_directional`` (pytorch3d's
    keyword) drops the y -> x term.  Forward only unless ``differentiable``: then the per-point distances come from an autograd
    function whose backward is ``ga_pc_knn_backward`` (k = 1), the same reductions carry the weights, and the loss has the bits of
    the forward-only one."""
    if point_reduction not in ("mean", "sum"):
        raise ValueError('point_reduction must be one of ["mean", "sum"]')
    if batch_reduction not in ("mean", "sum", None):
        raise ValueError('batch_reduction must be one of ["mean", "sum"] or None')
    if differentiable:
        xs, ys = _cloud(x, "x"), _cloud(y, "y")
        if xs.shape[0] != ys.shape[0] or xs.device != ys.device:
            raise ValueError("x and y need the same batch size and device")
        xl, _ = _lengths(x_lengths, xs.shape[0], xs.shape[1], xs.device, "x_lengths")
        yl, _ = _lengths(y_lengths, xs.shape[0], ys.shape[1], xs.device, "y_lengths")
        cham_x = _NearestDist2.apply(x, y, xl, yl)
        cham_y = None if single_directional else _NearestDist2.apply(y, x, yl, xl)
    else:
        if (isinstance(x, torch.Tensor) and x.requires_grad) or (isinstance(y, torch.Tensor) and y.requires_grad):
            raise RuntimeError("chamfer_distance is forward only: an input requires grad")
        cham_x, _ = nearest_points(x, y, x_lengths, y_lengths)   # padded slots hold 0
        cham_y = None if single_directional else nearest_points(y, x, y_lengths, x_lengths)[0]
    B, Nx = cham_x.shape

    def reduce(cham, lengths):
        N = cham.shape[1]
        cham = cham.sum(1)
        if point_reduction == "mean":
            cham = cham / torch.as_tensor(lengths if lengths is not None else [N] * B, device=cham.device).to(torch.float32)
        if batch_reduction is not None:
            cham = cham.sum()
            if batch_reduction == "mean":
                cham = cham / B
        return cham

    cham_x = reduce(cham_x, x_lengths)
    if single_directional:
        return cham_x, None
    return cham_x + reduce(cham_y, y_lengths), None


KNN = collections.namedtuple("KNN", "dists idx knn")


def knn_plan(num_query: int, num_target: int, K: int = 1) -> dict:
    """What ``ga_pc_knn`` launches: {'k_slots', 'threads', 'tile', 'grid_x', 'grid_y'} (the grid is grid_x by grid_y * B)."""
    pl = _lib.GaKnnPlan()
    _lib.check(_lib.lib().ga_pc_knn_plan(int(num_query), int(num_target), int(K), ctypes.byref(pl)), "ga_pc_knn_plan")
    return {"k_slots": pl.k_slots, "threads": pl.threads, "tile": pl.tile, "grid_x": pl.grid_x, "grid_y": pl.grid_y}


def _knn_forward(q, t, ql, tl, K):
    B, Nq, _ = q.shape
    dist2 = torch.empty(B, Nq, K, dtype=torch.float32, device=q.device)
    idx = torch.empty(B, Nq, K, dtype=torch.int32, device=q.device)
    args = _lib.GaKnnArgs(B, Nq, t.shape[1], K, q.data_ptr(), t.data_ptr(), _ptr(ql), _ptr(tl), dist2.data_ptr(), idx.data_ptr())
    with torch.cuda.device(q.device):
        _lib.check(_lib.lib().ga_pc_knn(ctypes.byref(args), _stream(q.device)), "ga_pc_knn")
    return dist2, idx


class _KnnDist2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, p1, p2, l1, l2, K):
        q, t = _cloud(p1, "p1"), _cloud(p2, "p2")
        dist2, idx = _knn_forward(q, t, l1, l2, K)
        ctx.save_for_backward(q, t, idx)
        ctx.lengths = (l1, l2)
        ctx.dtypes = (p1.dtype, p2.dtype)
        idx64 = idx.long()
        ctx.mark_non_differentiable(idx64)
        return dist2, idx64

    @staticmethod
    def backward(ctx, grad, _grad_idx):
        q, t, idx = ctx.saved_tensors
        gq, gt = _knn_backward(q, t, ctx.lengths[0], ctx.lengths[1], idx, grad.to(torch.float32).contiguous(),
                               ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return (gq.to(ctx.dtypes[0]) if gq is not None else None, gt.to(ctx.dtypes[1]) if gt is not None else None, None, None, None)


def knn_points(p1: torch.Tensor, p2: torch.Tensor, lengths1=None, lengths2=None, norm: int = 2, K: int = 1, version: int = -1,
               return_nn: bool = False, return_sorted: bool = True):
    """-> KNN(dists [B,N1,K] float32 SQUARED, idx [B,N1,K] int64, knn [B,N1,K,3] or None): ``pytorch3d.ops.knn_points`` for the
    squared L2 norm.  Lists are ascending, the lower index first among equal distances; slots past ``min(K, lengths2[b])`` and the
    rows past ``lengths1[b]`` hold distance 0 and index 0, pytorch3d's zero padding.  ``version`` is accepted and ignored; the output
    is always sorted, which also satisfies ``return_sorted=False``.  When ``p1`` or ``p2`` requires grad, ``dists`` carries the
    gradient (``ga_pc_knn_backward``)."""
    if norm == 1:
        raise NotImplementedError("knn_points: the L1 norm is not built, only norm=2")
    if norm != 2:
        raise ValueError("knn_points supports norm=2 (squared L2) only")
    K = int(K)
    if K < 1 or K > _lib.GA_PC_KNN_MAX_K:
        raise ValueError(f"K must lie in [1, {_lib.GA_PC_KNN_MAX_K}]: the sorted list lives in registers, {_lib.GA_PC_KNN_MAX_K} is the limit")
    q, t = _cloud(p1, "p1"), _cloud(p2, "p2")
    if q.shape[0] != t.shape[0] or q.device != t.device:
        raise ValueError("p1 and p2 need the same batch size and device")
    B, N1, _ = q.shape
    l1, _ = _lengths(lengths1, B, N1, q.device, "lengths1")
    l2, _ = _lengths(lengths2, B, t.shape[1], q.device, "lengths2")
    if torch.is_grad_enabled() and (p1.requires_grad or p2.requires_grad):
        dists, idx = _KnnDist2.apply(p1, p2, l1, l2, K)
    else:
        dists, idx = _knn_forward(q, t, l1, l2, K)
        idx = idx.long()
    return KNN(dists, idx, knn_gather(p2, idx, lengths2) if return_nn else None)


def knn_gather(x: torch.Tensor, idx: torch.Tensor, lengths=None):
    """``pytorch3d.ops.knn_gather``: x [B,M,C], idx [B,N,K] -> [B,N,K,C] with out[b,n,k] = x[b, idx[b,n,k]], zero where
    ``k >= lengths[b]`` (``lengths`` [B]: the lengths of ``x``'s clouds).  Plain torch ``gather``, differentiable in ``x``."""
    if x.dim() != 3 or idx.dim() != 3 or x.shape[0] != idx.shape[0]:
        raise ValueError("x is [B, M, C] and idx [B, N, K] with the same B")
    B, M, C = x.shape
    _, N, K = idx.shape
    out = x[:, :, None].expand(-1, -1, K, -1).gather(1, idx[:, :, :, None].expand(-1, -1, -1, C))
    if lengths is not None:
        ln = torch.as_tensor(lengths, device=x.device).to(torch.int64)
        if ln.shape != (B,):
            raise ValueError("lengths is a [B] tensor")
        pad = ln[:, None] <= torch.arange(K, device=x.device)[None]          # [B,K]
        out = out.masked_fill(pad[:, None, :, None], 0)
    return out


@torch.no_grad()
def remove_statistical_outliers(points: torch.Tensor, lengths=None, nb_neighbors: int = 20, std_ratio: float = 2.0):
    """-> (points [B,N,3], lengths [B] int64, keep_mask [B,N] bool).  Per valid point, m_i is the mean of sqrt(dist2) to its
    ``nb_neighbors`` nearest OTHER points (``knn_points`` of the cloud against itself with K = nb_neighbors + 1, the first entry --
    the point itself, or a duplicate of it at distance 0 -- dropped); per cloud, mu and sigma are the mean and the population
    standard deviation of m; point i stays iff m_i <= mu + std_ratio * sigma.  Kept points move to the front in their original
    order, zeros follow.  This is our own definition: parity with Open3D's ``remove_statistical_outlier`` is not claimed."""
    p = _cloud(points, "points")
    B, N, _ = p.shape
    nb = int(nb_neighbors)
    if nb < 1 or nb + 1 > _lib.GA_PC_KNN_MAX_K:
        raise ValueError(f"nb_neighbors must lie in [1, {_lib.GA_PC_KNN_MAX_K - 1}]")
    _, host = _lengths(lengths, B, N, p.device, "lengths")
    if min(host) < nb + 1:
        raise ValueError(f"a cloud of {min(host)} points has no {nb} neighbours per point")
    m = knn_points(p, p, host, host, K=nb + 1).dists[:, :, 1:].sqrt().mean(-1)                        # [B,N]
    ln = torch.tensor(host, dtype=torch.int64, device=p.device)
    valid = torch.arange(N, device=p.device)[None] < ln[:, None]
    cnt = ln.to(torch.float32)
    mu = (m * valid).sum(1) / cnt
    sigma = (((m - mu[:, None]).square() * valid).sum(1) / cnt).sqrt()
    keep = valid & (m <= (mu + float(std_ratio) * sigma)[:, None])
    order = torch.argsort((~keep).to(torch.uint8), dim=1, stable=True)                               # kept first, original order
    out = p.gather(1, order[:, :, None].expand(-1, -1, 3)) * keep.gather(1, order)[:, :, None]
    return out, keep.sum(1), keep


# ---- normals and the surfel initialiser (include/ga_pointcloud.h, csrc/pc_normals.hip) ------------------------------------------------
def normals_plan(num_points: int, K: int = 16) -> dict:
    """What ``ga_pc_normals`` launches: {'threads', 'grid_x', 'grid_y', 'sweeps'} (the grid is grid_x by grid_y * B)."""
    pl = _lib.GaNormalsPlan()
    _lib.check(_lib.lib().ga_pc_normals_plan(int(num_points), int(K), ctypes.byref(pl)), "ga_pc_normals_plan")
    return {"threads": pl.threads, "grid_x": pl.grid_x, "grid_y": pl.grid_y, "sweeps": pl.sweeps}


def _per_point(t, like, name):
    """an optional [B,N,3] companion of the cloud ``like`` -> fp32 contiguous on its device"""
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(like.shape):
        raise ValueError(f"{name} is a tensor of the cloud's shape {list(like.shape)}")
    if t.device != like.device:
        raise RuntimeError(f"{name} must be on the cloud's device {like.device} (no CPU fallback)")
    return t.detach().to(torch.float32).contiguous()


def _pca_frames(p, dev_lengths, K, viewpoint=None, want_frame=True):
    """self-kNN and ``ga_pc_normals`` on an fp32 contiguous cloud [B,N,3] -> (normal, tangent, eigenvalues, dist2, idx); tangent and
    eigenvalues None unless ``want_frame``.  Two launches on the current stream, no host read."""
    B, N, _ = p.shape
    dist2, idx = _knn_forward(p, p, dev_lengths, dev_lengths, K)
    normal = torch.empty(B, N, 3, dtype=torch.float32, device=p.device)
    tangent = torch.empty_like(normal) if want_frame else None
    eig = torch.empty_like(normal) if want_frame else None
    args = _lib.GaNormalsArgs(B, N, K, 0, p.data_ptr(), _ptr(dev_lengths), idx.data_ptr(), _ptr(viewpoint), normal.data_ptr(),
                              _ptr(tangent), _ptr(eig))
    with torch.cuda.device(p.device):
        _lib.check(_lib.lib().ga_pc_normals(ctypes.byref(args), _stream(p.device)), "ga_pc_normals")
    return normal, tangent, eig, dist2, idx


def _check_k(K, lo, what):
    K = int(K)
    if K < lo or K > _lib.GA_PC_KNN_MAX_K:
        raise ValueError(f"K must lie in [{lo}, {_lib.GA_PC_KNN_MAX_K}] for {what}")
    return K


@torch.no_grad()
def estimate_normals(points: torch.Tensor, lengths=None, K: int = 16, viewpoint=None, return_frame: bool = False):
    """PCA normals of a padded batch of clouds [B,N,3] -> ``normals`` [B,N,3] float32, or ``(normals, tangents, eigenvalues)`` with
    ``return_frame``: per point the covariance of its ``K`` nearest points (itself included; ``knn_points`` of the cloud against
    itself), the unit eigenvector of the smallest eigenvalue as the normal, that of the largest as the tangent, the eigenvalues
    ascending.  Sign: the component of largest magnitude is positive; with ``viewpoint`` ([3] or [B,3]) the normal is turned towards
    it.  Rows past ``lengths``, clouds of fewer than 3 points and points whose neighbours all coincide get normal (0,0,1), tangent
    (1,0,0), eigenvalues 0.  The definition is the project's own (include/ga_pointcloud.h); normals are not propagated along the
    surface, so without a viewpoint two neighbours may point to opposite sides.  Two launches on the current stream, no host read."""
    K = _check_k(K, _lib.GA_PC_NORMALS_MIN_K, "a normal: a plane needs three points")
    p = _cloud(points, "points")
    B, N, _ = p.shape
    dev_lengths, _ = _lengths(lengths, B, N, p.device, "lengths")
    vp = None
    if viewpoint is not None:
        vp = torch.as_tensor(viewpoint, dtype=torch.float32, device=p.device)
        if tuple(vp.shape) not in ((3,), (B, 3)):
            raise ValueError(f"viewpoint is [3] or [{B}, 3], not {list(vp.shape)}")
        vp = vp.expand(B, 3).contiguous()
    normal, tangent, eig, _, _ = _pca_frames(p, dev_lengths, K, vp, return_frame)
    return (normal, tangent, eig) if return_frame else normal


@torch.no_grad()
def surfels_from_cloud(points: torch.Tensor, lengths=None, colors=None, normals=None, K: int = 16, opacity: float = 0.1,
                       scale_factor: float = 1.0):
    """Activated surfels [B,N,13] (xyz, opacity, scale(2), rotation wxyz, rgb) from a padded batch of clouds: ``ga_pc_surfel_init`` on
    the PCA frames of ``estimate_normals``.  Scale: ``scale_factor`` times the root mean squared distance to the three nearest other
    points (2DGS's rule), in both columns; rotation: the disc lies in the tangent plane, its normal the PCA normal or, with
    ``normals`` [B,N,3], the given one (the PCA tangent is projected onto its plane).  Invalid rows (those of ``estimate_normals``,
    clouds of fewer than 4 points, a given normal of length 0) get opacity 0, scale 1e-4, the identity rotation."""
    K = _check_k(K, _lib.GA_PC_SURFEL_MIN_K, "an initial scale: the three nearest other points")
    if not (0.0 <= float(opacity) <= 1.0) or not (0.0 < float(scale_factor) < float("inf")):
        raise ValueError("opacity must lie in [0, 1] and scale_factor must be positive and finite")
    p = _cloud(points, "points")
    B, N, _ = p.shape
    dev_lengths, _ = _lengths(lengths, B, N, p.device, "lengths")
    col = _per_point(colors, p, "colors") if colors is not None else None
    given = _per_point(normals, p, "normals") if normals is not None else None
    normal, tangent, eig, dist2, _ = _pca_frames(p, dev_lengths, K)
    out = torch.empty(B, N, _lib.GA_PC_SURFEL_FLOATS, dtype=torch.float32, device=p.device)
    args = _lib.GaSurfelInitArgs(B, N, K, float(opacity), float(scale_factor), 0, p.data_ptr(),
                                 (given if given is not None else normal).data_ptr(), tangent.data_ptr(), dist2.data_ptr(),
                                 _ptr(dev_lengths), eig.data_ptr(), _ptr(col), out.data_ptr())
    with torch.cuda.device(p.device):
        _lib.check(_lib.lib().ga_pc_surfel_init(ctypes.byref(args), _stream(p.device)), "ga_pc_surfel_init")
    return out


# ---- point clouds from posed depth views (include/ga_pointcloud.h, csrc/pc_unproject.hip) ----------------------------------------------
class UnprojectedCloud:
    """What ``unproject_depth_views`` returns, everything on the device and padded to ``capacity`` rows: ``points`` [capacity,3],
    ``colors`` and ``normals`` [capacity,3] or None, ``source`` [capacity] int32 (the pixel ``(v * H + y) * W + x`` of each row, -1 on
    padding), ``count`` [1] int32 (the number of valid pixels, even beyond ``capacity``) and ``view_counts`` [V] int32.  Rows are in
    ascending ``source`` order.  ``trimmed()`` does the one host read."""

    __slots__ = ("points", "colors", "normals", "source", "count", "view_counts", "capacity")

    def __init__(self, points, colors, normals, source, count, view_counts):
        self.points, self.colors, self.normals, self.source = points, colors, normals, source
        self.count, self.view_counts, self.capacity = count, view_counts, int(points.shape[0])

    def trimmed(self, count=None):
        """-> an ``UnprojectedCloud`` of exactly ``count`` rows (views of the same storage).  Reads ``count`` back -- the one host
        synchronisation of the feature; a caller that has read it already hands it in -- and raises when the cloud did not fit its
        capacity."""
        n = int(self.count.item()) if count is None else int(count)
        if n > self.capacity:
            raise RuntimeError(f"{n} valid pixels do not fit the capacity of {self.capacity} rows: nothing past it was written")
        cut = lambda t: t[:n] if t is not None else None
        return UnprojectedCloud(cut(self.points), cut(self.colors), cut(self.normals), cut(self.source), self.count, self.view_counts)


_DEPTH_KINDS = {"z": _lib.GA_PC_DEPTH_Z, "ray": _lib.GA_PC_DEPTH_RAY}


def _view_map(t, name, V, C, H, W, like, u8=False):
    """an optional per-view map [V,C,H,W] (C == 1: [V,H,W] as well) -> contiguous fp32 (or uint8) on the depth's device"""
    shapes = ((V, C, H, W),) + (((V, H, W),) if C == 1 else ())
    if not isinstance(t, torch.Tensor) or tuple(t.shape) not in shapes:
        raise ValueError(f"{name} is a tensor of shape {' or '.join(str(list(s)) for s in shapes)}, the depth's views")
    if not (t.is_floating_point() or (u8 and t.dtype == torch.uint8)):
        raise TypeError(f"{name} must be floating point" + (" or uint8" if u8 else ""))
    if t.device != like.device:
        raise RuntimeError(f"{name} must be on the depth's device {like.device} (no CPU fallback)")
    t = t.detach()
    return t.contiguous() if t.dtype == torch.uint8 else t.to(torch.float32).contiguous()


def _check_views(depth, cameras, depth_kind, depth_range, mask_threshold, max_width=None):
    """what ``unproject_depth_views`` and ``filter_view_consistency`` ask of their views, in this order -> (V, H, W, lo, hi, thr)"""
    if not isinstance(depth, torch.Tensor) or depth.dim() not in (3, 4) or (depth.dim() == 4 and depth.shape[1] != 1) or depth.numel() == 0:
        raise ValueError("depth is a [V, H, W] or [V, 1, H, W] tensor")
    if not depth.is_floating_point():
        raise TypeError("depth must be floating point")
    V, H, W = int(depth.shape[0]), int(depth.shape[-2]), int(depth.shape[-1])
    if max_width is None:
        if V * H * W >= 2 ** 31:
            raise ValueError("V * H * W stays below 2^31")
    elif W > max_width or V * H * W >= 2 ** 31:
        raise ValueError(f"views are at most {max_width} wide and V * H * W stays below 2^31")
    if depth_kind not in _DEPTH_KINDS:
        raise ValueError("depth_kind is 'z' (camera z) or 'ray' (distance along the normalised ray)")
    if not isinstance(cameras, torch.Tensor) or cameras.dim() != 2 or cameras.shape[0] != V or cameras.shape[1] not in (25, 21):
        raise ValueError(f"cameras is a pose25 tensor [{V}, 25] or cameras_from_view's [{V}, 21]")
    lo, hi = (float(x) for x in depth_range)
    if lo != lo or hi != hi or not lo < hi:
        raise ValueError("depth_range is (min, max) with min < max")
    thr = float(mask_threshold)
    if thr != thr:
        raise ValueError("mask_threshold must not be NaN")
    return V, H, W, lo, hi, thr


def _views_f32(depth, cameras):
    """checked views, once their devices are known to be right -> the depth and the [V,21] cameras the kernels read: fp32, contiguous"""
    from . import cameras as _cameras
    cam = (_cameras.cameras_from_pose25(cameras) if cameras.shape[1] == 25 else cameras.detach().to(torch.float32)).contiguous()
    return depth.detach().to(torch.float32).contiguous(), cam


def unproject_candidates(V: int, H: int, W: int, pixel_stride: int = 1) -> int:
    """the pixels ``unproject_depth_views`` looks at: those with ``y % pixel_stride == 0 and x % pixel_stride == 0``"""
    s = int(pixel_stride)
    return int(V) * (-(-int(H) // s)) * (-(-int(W) // s))


@torch.no_grad()
def unproject_depth_views(depth: torch.Tensor, cameras: torch.Tensor, *, mask=None, color=None, normal=None, depth_kind: str = "z",
                          depth_range=(0.0, float("inf")), mask_threshold: float = 0.5, erode: int = 0, clip=None,
                          drop_zero: bool = False, pixel_stride: int = 1, capacity=None) -> UnprojectedCloud:
    """Posed depth views -> an ordered, compacted world-space cloud on the device (``ga_pc_unproject``: three launches on the current
    stream, no host read; the count stays in device memory).

    ``depth`` [V,H,W] or [V,1,H,W]; ``cameras`` the reference's pose25 ``c`` [V,25] or ``cameras.cameras_from_view(cam_view, tanfov)``
    [V,21]; ``mask`` (alpha) [V,H,W] or [V,1,H,W], foreground where ``mask >= mask_threshold``, eroded ``erode`` (0..4) times by the
    3 x 3 cross; ``color`` [V,3,H,W] fp32 or uint8 (``/ 255``); ``normal`` [V,3,H,W] world space, re-normalised.  ``depth_kind``: 'z'
    (camera z, what ``render`` returns) or 'ray' (distance along the normalised ray, the reference's g-buffers).  A pixel is valid when
    ``depth_range[0] < depth < depth_range[1]`` (NaN and inf never are), it is foreground, with ``clip`` no coordinate reaches
    ``+-clip`` and with ``drop_zero`` none is exactly 0; ``pixel_stride`` s looks at every s-th row and column only.  ``capacity``
    (None: every candidate pixel) is the number of rows allocated; more valid pixels than that are reported by ``count`` alone.
    The arithmetic is the header's, operation by operation; GPU only, no fallback."""
    V, H, W, lo, hi, thr = _check_views(depth, cameras, depth_kind, depth_range, mask_threshold, _lib.GA_PC_UNPROJECT_MAX_WIDTH)
    erode, stride = int(erode), int(pixel_stride)
    if not 0 <= erode <= _lib.GA_PC_UNPROJECT_MAX_ERODE:
        raise ValueError(f"erode must lie in [0, {_lib.GA_PC_UNPROJECT_MAX_ERODE}]")
    if erode and mask is None:
        raise ValueError("erode needs a mask")
    if stride < 1:
        raise ValueError("pixel_stride must be at least 1")
    clip = 0.0 if clip is None else float(clip)
    if clip != 0.0 and not (0.0 < clip < float("inf")):
        raise ValueError("clip must be positive and finite (None: no clipping)")
    cap = unproject_candidates(V, H, W, stride) if capacity is None else int(capacity)
    if cap < 1 or cap >= 2 ** 31:
        raise ValueError("capacity must lie in [1, 2^31)")
    m = _view_map(mask, "mask", V, 1, H, W, depth) if mask is not None else None
    col = _view_map(color, "color", V, 3, H, W, depth, u8=True) if color is not None else None
    nrm = _view_map(normal, "normal", V, 3, H, W, depth) if normal is not None else None
    if depth.device.type != "cuda":
        raise RuntimeError("depth must be on the GPU (no CPU fallback)")
    dev = depth.device
    if cameras.device != dev:
        raise RuntimeError(f"cameras must be on the depth's device {dev} (no CPU fallback)")
    d, cam = _views_f32(depth, cameras)
    L = _lib.lib()
    with torch.cuda.device(dev):
        points = torch.empty(cap, 3, dtype=torch.float32, device=dev)
        colors = torch.empty(cap, 3, dtype=torch.float32, device=dev) if col is not None else None
        normals = torch.empty(cap, 3, dtype=torch.float32, device=dev) if nrm is not None else None
        source = torch.empty(cap, dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        view_counts = torch.empty(V, dtype=torch.int32, device=dev)
        nbytes = int(L.ga_pc_unproject_workspace_bytes(V, H, W))
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        args = _lib.GaUnprojectArgs(V, H, W, _DEPTH_KINDS[depth_kind],
                                    _lib.GA_PC_COLOR_U8 if col is not None and col.dtype == torch.uint8 else _lib.GA_PC_COLOR_F32,
                                    erode, int(bool(drop_zero)), stride, cap, lo, hi, thr, clip, 0, d.data_ptr(), _ptr(m), _ptr(col),
                                    _ptr(nrm), cam.data_ptr(), points.data_ptr(), _ptr(colors), _ptr(normals), source.data_ptr(),
                                    count.data_ptr(), view_counts.data_ptr(), workspace.data_ptr(), nbytes)
        _lib.check(L.ga_pc_unproject(ctypes.byref(args), _stream(dev)), "ga_pc_unproject")
    return UnprojectedCloud(points, colors, normals, source, count, view_counts)


# ---- cross-view consistency filter and voxel thinning (include/ga_pointcloud.h, csrc/pc_filter.hip) --------------------------------------
class FilteredCloud(UnprojectedCloud):
    """What ``filter_view_consistency`` and ``voxel_thin`` return: an ``UnprojectedCloud`` (``source`` and ``view_counts`` None for a
    cloud that came without ``source``) plus ``kept_rows`` [capacity] int32 (the input row of every row, -1 on padding) and, from the
    filter with ``return_votes``, ``support`` / ``conflicts`` [input rows] uint8, or, from the thinning, ``multiplicity`` [capacity]
    int32 (the live input rows in the row's cell) and ``dropped`` [1] int32 (rows outside the grid).  ``trimmed()`` cuts the
    per-row outputs; the votes are per INPUT row and stay whole."""

    __slots__ = ("kept_rows", "multiplicity", "support", "conflicts", "dropped")

    def __init__(self, points, colors, normals, source, count, view_counts, kept_rows, multiplicity=None, support=None, conflicts=None,
                 dropped=None):
        super().__init__(points, colors, normals, source, count, view_counts)
        self.kept_rows, self.multiplicity, self.support, self.conflicts, self.dropped = kept_rows, multiplicity, support, conflicts, dropped

    def trimmed(self, count=None):
        n = int(self.count.item()) if count is None else int(count)
        if n > self.capacity:
            raise RuntimeError(f"{n} kept rows do not fit the capacity of {self.capacity} rows: nothing past it was written")
        cut = lambda t: t[:n] if t is not None else None
        return FilteredCloud(cut(self.points), cut(self.colors), cut(self.normals), cut(self.source), self.count, self.view_counts,
                             cut(self.kept_rows), cut(self.multiplicity), self.support, self.conflicts, self.dropped)


_VOXEL_KEEP = {"first": _lib.GA_PC_VOXEL_FIRST, "center": _lib.GA_PC_VOXEL_CENTER}
VOXEL_WAVE_MERGE = True      # the measured choice (profiles/pc_filter_bench.txt); the outputs are the same either way


def _filter_input(cloud, colors, normals, what):
    """an ``UnprojectedCloud`` (trimmed or not) or a [N,3] tensor -> (points, colors, normals, source, in_count), fp32 and contiguous"""
    if isinstance(cloud, UnprojectedCloud):
        if colors is not None or normals is not None:
            raise ValueError(f"{what}: colors and normals go with a [N, 3] tensor; an UnprojectedCloud brings its own")
        pts, colors, normals, source, in_count = cloud.points, cloud.colors, cloud.normals, cloud.source, cloud.count
    else:
        pts, source, in_count = cloud, None, None
    if not isinstance(pts, torch.Tensor) or pts.dim() != 2 or pts.shape[1] != 3 or pts.shape[0] < 1:
        raise ValueError(f"{what}: the cloud is an UnprojectedCloud or a [N, 3] tensor with N >= 1")
    if not pts.is_floating_point():
        raise TypeError(f"{what}: the points must be floating point")
    if pts.shape[0] > _lib.GA_PC_FILTER_MAX_ROWS:
        raise ValueError(f"{what}: at most {_lib.GA_PC_FILTER_MAX_ROWS} rows")
    f32 = lambda t: t.detach().to(torch.float32).contiguous()
    for name, t in (("colors", colors), ("normals", normals)):
        if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(pts.shape) or t.device != pts.device or
                              not t.is_floating_point()):
            raise ValueError(f"{what}: {name} is a floating-point [N, 3] tensor on the cloud's device")
    if pts.device.type != "cuda":
        raise RuntimeError(f"{what}: the cloud must be on the GPU (no CPU fallback)")
    return f32(pts), f32(colors) if colors is not None else None, f32(normals) if normals is not None else None, source, in_count


def _filter_outputs(cap, dev, colors, normals, source, num_views):
    e = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device=dev)
    return dict(points=e(cap, 3), colors=e(cap, 3) if colors is not None else None, normals=e(cap, 3) if normals is not None else None,
                source=e(cap, dtype=torch.int32) if source is not None else None, kept_rows=e(cap, dtype=torch.int32),
                count=e(1, dtype=torch.int32),
                view_counts=e(num_views, dtype=torch.int32) if source is not None and num_views else None)


def _capacity(capacity, rows):
    cap = rows if capacity is None else int(capacity)
    if cap < 1 or cap >= 2 ** 31:
        raise ValueError("capacity must lie in [1, 2^31)")
    return cap


@torch.no_grad()
def filter_view_consistency(cloud, depth: torch.Tensor, cameras: torch.Tensor, *, mask=None, depth_kind: str = "z",
                            depth_range=(0.0, float("inf")), mask_threshold: float = 0.5, tolerance=(0.0, 0.01), window: int = 1,
                            min_support: int = 1, max_conflicts: int = 0, carve: bool = False, capacity=None,
                            return_votes: bool = False) -> FilteredCloud:
    """Keep the points of ``cloud`` that the depth maps of the OTHER views agree with (``ga_pc_filter_views``: three launches on the
    current stream, no host read).

    ``cloud`` is an ``UnprojectedCloud`` (trimmed or not: its ``count`` is read on the device, its ``source`` names each point's own
    view, which does not vote) or a [N,3] tensor (a foreign cloud: every view votes).  ``depth`` [V,H,W] or [V,1,H,W], ``mask`` and
    ``cameras`` (pose25 [V,25] or [V,21]) are as in ``unproject_depth_views``; a map pixel is surface when ``depth_range[0] < z <
    depth_range[1]`` and, with a mask, ``mask >= mask_threshold``.  Every point is projected into every other view (nearest pixel) and
    compared with the smallest and largest surface depth of the ``(2 window + 1)^2`` pixels around it, ``tolerance`` = (absolute,
    relative): within them and on a surface pixel it is SUPPORTED; in front of a window that is all surface it is in CONFLICT, and with
    ``carve`` also where the window is all empty; behind the surface (occluded), on a silhouette, outside the image or behind the
    camera the view says nothing.  A point stays when ``support >= min_support and conflicts <= max_conflicts``; the survivors keep
    their order.  ``capacity`` (None: the input's rows) is the number of rows allocated.  ``return_votes`` adds the per-input-row
    ``support`` and ``conflicts`` (uint8, saturated).  The arithmetic is the header's, operation by operation; GPU only, no fallback."""
    what = "filter_view_consistency"
    V, H, W, lo, hi, thr = _check_views(depth, cameras, depth_kind, depth_range, mask_threshold)
    tol_abs, tol_rel = (float(x) for x in tolerance)
    if not (0.0 <= tol_abs < float("inf") and 0.0 <= tol_rel < float("inf")):
        raise ValueError("tolerance is (absolute, relative), both finite and not negative")
    if int(window) not in (0, 1):
        raise ValueError("window is 0 (the nearest pixel) or 1 (the 3 x 3 pixels around it)")
    if int(min_support) < 0 or int(max_conflicts) < 0:
        raise ValueError("min_support and max_conflicts must not be negative")
    pts, colors, normals, source, in_count = _filter_input(cloud, None, None, what)
    rows = int(pts.shape[0])
    cap = _capacity(capacity, rows)
    dev = pts.device
    if depth.device != dev or cameras.device != dev:
        raise RuntimeError(f"depth and cameras must be on the cloud's device {dev} (no CPU fallback)")
    m = _view_map(mask, "mask", V, 1, H, W, depth) if mask is not None else None
    d, cam = _views_f32(depth, cameras)
    L = _lib.lib()
    with torch.cuda.device(dev):
        o = _filter_outputs(cap, dev, colors, normals, source, V)
        sup = torch.empty(rows, dtype=torch.uint8, device=dev) if return_votes else None
        con = torch.empty(rows, dtype=torch.uint8, device=dev) if return_votes else None
        nbytes = int(L.ga_pc_filter_views_workspace_bytes(rows))
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        args = _lib.GaFilterViewsArgs(rows, cap, V, H, W, _DEPTH_KINDS[depth_kind], int(window), int(min_support), int(max_conflicts),
                                      int(bool(carve)), lo, hi, thr, tol_abs, tol_rel, 0, _ptr(in_count), pts.data_ptr(), _ptr(colors),
                                      _ptr(normals), _ptr(source), d.data_ptr(), _ptr(m), cam.data_ptr(), o["points"].data_ptr(),
                                      _ptr(o["colors"]), _ptr(o["normals"]), _ptr(o["source"]), o["kept_rows"].data_ptr(),
                                      o["count"].data_ptr(), _ptr(o["view_counts"]), _ptr(sup), _ptr(con), workspace.data_ptr(), nbytes)
        _lib.check(L.ga_pc_filter_views(ctypes.byref(args), _stream(dev)), "ga_pc_filter_views")
    return FilteredCloud(o["points"], o["colors"], o["normals"], o["source"], o["count"], o["view_counts"], o["kept_rows"],
                         support=sup, conflicts=con)


@torch.no_grad()
def voxel_thin(cloud, voxel_size: float, *, origin=(0.0, 0.0, 0.0), keep: str = "center", colors=None, normals=None, capacity=None,
               view_pixels=None, wave_merge: bool = VOXEL_WAVE_MERGE) -> FilteredCloud:
    """One point per occupied cell of the grid of ``voxel_size`` cells anchored at ``origin`` (``ga_pc_voxel_thin``: five launches on
    the current stream, no host read).

    ``cloud`` is an ``UnprojectedCloud`` (trimmed or not, with its own colours, normals and source) or a [N,3] tensor with optional
    ``colors`` / ``normals`` [N,3].  The point kept of a cell is a MEASURED one with its own colour and normal -- ``keep='center'``:
    the nearest to the cell's centre, ``'first'``: the first in input order; ties go to the lowest row -- never an average, so the
    result is a function of the input alone.  The survivors keep their order.  A row with a non-finite coordinate or more than 2^20 - 1
    cells from the origin is dropped and counted in ``dropped``.  ``multiplicity`` is the number of input rows in each kept row's cell.
    ``view_pixels`` (H * W of the views ``source`` names) asks for ``view_counts``; without it they are None.  ``capacity`` (None: the
    input's rows) is the number of rows allocated.  ``wave_merge`` inserts neighbouring rows of one cell into the table once (the
    same outputs, another speed).  GPU only, no fallback."""
    what = "voxel_thin"
    vs = float(voxel_size)
    if not (0.0 < vs < float("inf")):
        raise ValueError("voxel_size must be positive and finite")
    org = [float(x) for x in origin]
    if len(org) != 3 or not all(abs(x) < float("inf") for x in org):
        raise ValueError("origin is three finite numbers")
    if keep not in _VOXEL_KEEP:
        raise ValueError("keep is 'center' (the point nearest the cell's centre) or 'first' (the first in input order)")
    num_views = 0
    if view_pixels is not None:
        if not isinstance(cloud, UnprojectedCloud) or cloud.view_counts is None or int(view_pixels) < 1:
            raise ValueError("view_pixels (>= 1) goes with an UnprojectedCloud that has view_counts")
        num_views = int(cloud.view_counts.shape[0])
    pts, colors, normals, source, in_count = _filter_input(cloud, colors, normals, what)
    rows = int(pts.shape[0])
    cap = _capacity(capacity, rows)
    dev = pts.device
    L = _lib.lib()
    with torch.cuda.device(dev):
        o = _filter_outputs(cap, dev, colors, normals, source, num_views)
        mult = torch.empty(cap, dtype=torch.int32, device=dev)
        dropped = torch.empty(1, dtype=torch.int32, device=dev)
        nbytes = int(L.ga_pc_voxel_thin_workspace_bytes(rows, 0))
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        args = _lib.GaVoxelThinArgs(rows, cap, _VOXEL_KEEP[keep], num_views, int(view_pixels) if num_views else 0,
                                    _lib.GA_PC_VOXEL_WAVE_MERGE if wave_merge else 0,
                                    (ctypes.c_float * 3)(*org), vs, 0, _ptr(in_count), pts.data_ptr(), _ptr(colors), _ptr(normals),
                                    _ptr(source), o["points"].data_ptr(), _ptr(o["colors"]), _ptr(o["normals"]), _ptr(o["source"]),
                                    o["kept_rows"].data_ptr(), o["count"].data_ptr(), _ptr(o["view_counts"]), mult.data_ptr(),
                                    dropped.data_ptr(), workspace.data_ptr(), nbytes)
        _lib.check(L.ga_pc_voxel_thin(ctypes.byref(args), _stream(dev)), "ga_pc_voxel_thin")
    return FilteredCloud(o["points"], o["colors"], o["normals"], o["source"], o["count"], o["view_counts"], o["kept_rows"],
                         multiplicity=mult, dropped=dropped)


def cloud_from_render(out: dict, cam_view: torch.Tensor, tanfov, *, batch_index: int = 0, **kw) -> UnprojectedCloud:
    """The dict ``GaussianRenderer2DGS.render`` returns -> the cloud of ONE batch item: depth = ``out['depth']`` (camera z), mask =
    ``out['alpha']``, colour = ``out['image']``, normal = ``out['rend_normal']``; ``cam_view`` [V,4,4] or [B,V,4,4] and ``tanfov`` as
    ``render`` took them.  Maps of [V,C,H,W] are taken as they are, maps of [B,V,C,H,W] at ``batch_index``.  ``kw`` goes to
    ``unproject_depth_views`` (``mask=None`` / ``color=None`` / ``normal=None`` there drop a map)."""
    from . import cameras as _cameras
    for k in ("depth", "alpha", "image", "rend_normal"):
        if k not in out or not isinstance(out[k], torch.Tensor) or out[k].dim() not in (4, 5):
            raise ValueError(f"out['{k}'] is missing or is no [V,C,H,W] / [B,V,C,H,W] tensor: out is what render returns")
    pick = lambda t, nd: t[int(batch_index)] if t.dim() == nd + 1 else t
    if not isinstance(cam_view, torch.Tensor) or cam_view.dim() not in (3, 4):
        raise ValueError("cam_view is [V, 4, 4] or [B, V, 4, 4]")
    cam = _cameras.cameras_from_view(pick(cam_view, 3), tanfov)
    maps = dict(mask=pick(out["alpha"], 4), color=pick(out["image"], 4), normal=pick(out["rend_normal"], 4))
    maps.update({k: kw.pop(k) for k in ("mask", "color", "normal") if k in kw})
    if "depth_kind" in kw:
        raise ValueError("render's depth is the camera z: depth_kind is not a choice here")
    return unproject_depth_views(pick(out["depth"], 4), cam.to(out["depth"].device), depth_kind="z", **maps, **kw)


# ---- registration (include/ga_pointcloud.h, csrc/pc_align.hip) ----------------------------------------------------------------------------
SimilarityTransform = collections.namedtuple("SimilarityTransform", "R T s")
ICPSolution = collections.namedtuple("ICPSolution", "converged rmse Xt RTs t_history iterations idx dist2 history")


def align_plan(num_points: int, num_target: int = 1) -> dict:
    """What ``ga_pc_align_points`` and ``ga_pc_icp`` launch: {'threads', 'tile', 'grid_x', 'solve_threads', 'sweeps', 'terms'} (the
    accumulate grid is grid_x by B, the solve grid B)."""
    pl = _lib.GaAlignPlan()
    _lib.check(_lib.lib().ga_pc_align_plan(int(num_points), int(num_target), ctypes.byref(pl)), "ga_pc_align_plan")
    return {k: getattr(pl, k) for k in ("threads", "tile", "grid_x", "solve_threads", "sweeps", "terms")}


def _device_lengths(lengths, B, N, device, name):
    """an int tensor already on the device is taken as it is (no host read; the kernels clamp it), anything else as ``_lengths`` does"""
    if isinstance(lengths, torch.Tensor) and lengths.device.type == "cuda":
        if lengths.shape != (B,) or lengths.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"{name} is an int32 / int64 tensor of {B} entries")
        return lengths.to(device=device, dtype=torch.int32).contiguous()
    return _lengths(lengths, B, N, device, name)[0]


def _pair_weights(weights, B, N, device):
    if weights is None:
        return None
    if not isinstance(weights, torch.Tensor) or weights.shape != (B, N):
        raise ValueError(f"weights is a [{B}, {N}] tensor")
    return weights.detach().to(device=device, dtype=torch.float32).contiguous()


def _no_reflection(allow_reflection, what):
    if allow_reflection:
        raise NotImplementedError(f"{what}: reflections are not built, only allow_reflection=False (Horn's method yields proper rotations)")


def _unpack_transform(rts):
    return SimilarityTransform(rts[:, 1:10].reshape(-1, 3, 3), rts[:, 10:13], rts[:, 0])


def _pack_transform(t, B, device):
    """SimilarityTransform (or any (R [B,3,3], T [B,3], s [B]) triple) or a packed [B,13] tensor -> [B,13] fp32 on the device"""
    if isinstance(t, torch.Tensor):
        if t.shape != (B, _lib.GA_PC_TRANSFORM_FLOATS):
            raise ValueError(f"a packed transform is [{B}, {_lib.GA_PC_TRANSFORM_FLOATS}]: s, R row-major, T")
        return t.detach().to(device=device, dtype=torch.float32).contiguous()
    try:
        R, T, s = t
    except (TypeError, ValueError):
        raise ValueError("a transform is a SimilarityTransform(R, T, s) or a packed [B, 13] tensor") from None
    if not all(isinstance(v, torch.Tensor) for v in (R, T, s)) or R.shape != (B, 3, 3) or T.shape != (B, 3) or s.shape != (B,):
        raise ValueError(f"a SimilarityTransform holds R [{B},3,3], T [{B},3] and s [{B}]")
    f = lambda v: v.detach().to(device=device, dtype=torch.float32)
    return torch.cat([f(s)[:, None], f(R).reshape(B, 9), f(T)], 1).contiguous()


@torch.no_grad()
def apply_similarity_transform(X: torch.Tensor, RTs) -> torch.Tensor:
    """``s * X @ R + T`` for X [B,N,3] and a SimilarityTransform (or a packed [B,13] tensor), with the kernels' own fp32 expression,
    ``((x_0 * R_0b + x_1 * R_1b) + x_2 * R_2b) * s + T_b`` and every operation rounded on its own: the result has the bits of the ``Xt``
    that ``iterative_closest_point`` returns.  Plain torch on X's device; no gradient."""
    if not isinstance(X, torch.Tensor) or X.dim() != 3 or X.shape[-1] != 3:
        raise ValueError("X is a [B, N, 3] tensor")
    x = X.detach().to(torch.float32)
    t = _pack_transform(RTs, x.shape[0], x.device)
    cols = []
    for b in range(3):
        a = x[:, :, 0] * t[:, None, 1 + b]
        a = a + x[:, :, 1] * t[:, None, 4 + b]
        a = a + x[:, :, 2] * t[:, None, 7 + b]
        a = a * t[:, None, 0]
        cols.append(a + t[:, None, 10 + b])
    return torch.stack(cols, 2)


@torch.no_grad()
def corresponding_points_alignment(X: torch.Tensor, Y: torch.Tensor, weights=None, estimate_scale: bool = False,
                                   allow_reflection: bool = False, eps: float = 1e-9, *, lengths=None, return_status: bool = False):
    """-> SimilarityTransform(R [B,3,3], T [B,3], s [B]) with ``s * X @ R + T ~ Y`` in the weighted least-squares sense:
    ``pytorch3d.ops.corresponding_points_alignment`` for [B,N,3] clouds whose rows correspond (``ga_pc_align_points``: fp64 sums in a
    fixed order, Horn's quaternion method, the result rounded to fp32 -- a function of the inputs alone).  ``weights`` [B,N] >= 0;
    ``lengths`` [B] for padded batches; ``allow_reflection=True`` is not built; ``eps`` is accepted and unused (nothing is divided by a
    clamped weight sum: a cloud without positive weight, or without extent when the scale is wanted, is DEGENERATE and gets the
    identity).  ``return_status=True`` -> (transform, rmse [B] of the pairs as given, status [B] int32: 0 solved, 2 degenerate).
    Outputs carry no gradient: an input that requires grad is detached."""
    _no_reflection(allow_reflection, "corresponding_points_alignment")
    float(eps)
    x, y = _cloud(X, "X"), _cloud(Y, "Y")
    if x.shape != y.shape or x.device != y.device:
        raise ValueError("X and Y need the same shape and device: row i of Y is the partner of row i of X")
    B, N, _ = x.shape
    dev = x.device
    w = _pair_weights(weights, B, N, dev)
    ln = _device_lengths(lengths, B, N, dev, "lengths")
    L = _lib.lib()
    with torch.cuda.device(dev):
        rts = torch.empty(B, _lib.GA_PC_TRANSFORM_FLOATS, dtype=torch.float32, device=dev)
        rmse = torch.empty(B, dtype=torch.float32, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        nbytes = int(L.ga_pc_align_workspace_bytes(B, N))
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        args = _lib.GaAlignArgs(B, N, int(bool(estimate_scale)), 0, x.data_ptr(), y.data_ptr(), _ptr(w), _ptr(ln), rts.data_ptr(),
                                rmse.data_ptr(), status.data_ptr(), workspace.data_ptr(), nbytes)
        _lib.check(L.ga_pc_align_points(ctypes.byref(args), _stream(dev)), "ga_pc_align_points")
    out = _unpack_transform(rts)
    return (out, rmse, status) if return_status else out


@torch.no_grad()
def iterative_closest_point(X: torch.Tensor, Y: torch.Tensor, init_transform=None, max_iterations: int = 100,
                            relative_rmse_thr: float = 1e-6, estimate_scale: bool = False, allow_reflection: bool = False,
                            verbose: bool = False, *, x_lengths=None, y_lengths=None, weights=None, max_correspondence_distance=None,
                            return_history: bool = False) -> ICPSolution:
    """``pytorch3d.ops.iterative_closest_point`` for X [B,N,3] against Y [B,M,3]: -> ICPSolution(converged [B] bool, rmse [B], Xt [B,N,3],
    RTs = SimilarityTransform, t_history, iterations [B] int32, idx [B,N] int64, dist2 [B,N], history), all on the device.  ONE enqueue
    (``ga_pc_icp``): ``max_iterations`` x (match + sum, solve) and a final match pass; convergence, freezing and the iteration count are
    decided on the device, nothing is read back, and the call can be captured into a graph (with ``x_lengths`` / ``y_lengths`` None or
    int tensors already on the device).  ``verbose=True`` is the only thing that reads back, after the call.

    ``weights`` [B,N] >= 0 weigh the points of X; ``max_correspondence_distance`` drops the pairs farther apart than it from every
    solve and from the rmse (the only robust device built).  ``return_history`` -> ``t_history``, the list of the ``max_iterations + 1``
    transforms the passes ran under (pytorch3d's field), and ``history`` [B, max_iterations + 1, 14], the packed tensor its entries
    view: s, R row-major, T and the rmse of the pass; the rows behind a frozen cloud's last pass repeat that pass.
    Two deliberate differences from pytorch3d (include/ga_pointcloud.h): the rmse is the match pass's own (Open3D's definition), and
    the transform is always solved from the original X, so stable matches converge for any threshold >= 0.
    ``converged`` is False for a cloud that hit ``max_iterations`` and for a DEGENERATE one (no pair with positive weight, or no
    extent when the scale is wanted), which keeps the transform it had.  ``allow_reflection=True`` is not built.  Outputs carry no
    gradient: an input that requires grad is detached."""
    _no_reflection(allow_reflection, "iterative_closest_point")
    max_iterations = int(max_iterations)
    if max_iterations < 0 or max_iterations > _lib.GA_PC_ICP_MAX_ITERATIONS:
        raise ValueError(f"max_iterations must lie in [0, {_lib.GA_PC_ICP_MAX_ITERATIONS}]")
    thr = float(relative_rmse_thr)
    if not (0.0 <= thr < float("inf")):
        raise ValueError("relative_rmse_thr is a finite number >= 0")
    gate = 0.0 if max_correspondence_distance is None else float(max_correspondence_distance)
    if max_correspondence_distance is not None and not (0.0 < gate < float("inf")):
        raise ValueError("max_correspondence_distance is a positive finite distance (or None)")
    x, y = _cloud(X, "X"), _cloud(Y, "Y")
    if x.shape[0] != y.shape[0] or x.device != y.device:
        raise ValueError("X and Y need the same batch size and device")
    B, N, _ = x.shape
    M = y.shape[1]
    dev = x.device
    w = _pair_weights(weights, B, N, dev)
    xl = _device_lengths(x_lengths, B, N, dev, "x_lengths")
    yl = _device_lengths(y_lengths, B, M, dev, "y_lengths")
    init = _pack_transform(init_transform, B, dev) if init_transform is not None else None
    L = _lib.lib()
    with torch.cuda.device(dev):
        rts = torch.empty(B, _lib.GA_PC_TRANSFORM_FLOATS, dtype=torch.float32, device=dev)
        rmse = torch.empty(B, dtype=torch.float32, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        iterations = torch.empty(B, dtype=torch.int32, device=dev)
        history = torch.empty(B, max_iterations + 1, _lib.GA_PC_ALIGN_HISTORY_FLOATS, dtype=torch.float32, device=dev) \
            if return_history else None
        xt = torch.empty(B, N, 3, dtype=torch.float32, device=dev)
        idx = torch.empty(B, N, dtype=torch.int32, device=dev)
        dist2 = torch.empty(B, N, dtype=torch.float32, device=dev)
        nbytes = int(L.ga_pc_align_workspace_bytes(B, N))
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        args = _lib.GaIcpArgs(B, N, M, max_iterations, int(bool(estimate_scale)), 0, thr, gate, x.data_ptr(), y.data_ptr(), _ptr(w),
                              _ptr(xl), _ptr(yl), _ptr(init), rts.data_ptr(), rmse.data_ptr(), status.data_ptr(), iterations.data_ptr(),
                              _ptr(history), xt.data_ptr(), idx.data_ptr(), dist2.data_ptr(), workspace.data_ptr(), nbytes)
        _lib.check(L.ga_pc_icp(ctypes.byref(args), _stream(dev)), "ga_pc_icp")
    t_history = [_unpack_transform(history[:, k, :_lib.GA_PC_TRANSFORM_FLOATS]) for k in range(max_iterations + 1)] \
        if return_history else None
    sol = ICPSolution(status == _lib.GA_PC_ALIGN_CONVERGED, rmse, xt, _unpack_transform(rts), t_history, iterations, idx.long(), dist2, history)
    if verbose:   # the one host read, after everything has been enqueued
        for b, (c, it, r) in enumerate(zip(sol.converged.tolist(), iterations.tolist(), rmse.tolist())):
            print(f"ICP cloud {b}: {'converged' if c else 'not converged'} after {it} iterations, rmse {r:.6e}")
    return sol
