"""Point-cloud operations of the generation side -- the host side of include/ga_pointcloud.h (HIP kernels, csrc/pointcloud.hip).

    sample_farthest_points   pytorch3d.ops.sample_farthest_points: what turns an arbitrary cloud into the ``fps-xyz`` of stage 2
                             (/root/reference/nsr/lsgm/flow_matching_trainer.py:1079, :1110-1134) and generated surfels into the
                             ``fps-4096.ply`` the geometry metrics are computed on (/root/reference/scripts/save_pcd_from_gs.py:148-185)
    nearest_points           nearest target (squared distance, index) of every query
    chamfer_distance         pytorch3d.loss.chamfer_distance for squared L2 without normals (/root/reference/nsr/train_nv_util.py:2244),
                             forward only

pytorch3d is absent from this image; its published behaviour is restated, parity UNPINNED ('Point clouds').  The tensors
stay on the device and the work goes on the current stream.  There is no CPU fallback: without the HIP library, or on a CPU tensor,
the calls raise."""
from __future__ import annotations

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


def chamfer_distance(x: torch.Tensor, y: torch.Tensor, x_lengths=None, y_lengths=None, batch_reduction: Optional[str] = "mean",
                     point_reduction: str = "mean"):
    """-> (loss, None): ``pytorch3d.loss.chamfer_distance`` for squared L2 without normals -- for each direction the squared distance
    of every point to its nearest neighbour in the other cloud, summed (``point_reduction='sum'``) or averaged over the cloud's
    length ('mean'), the two directions added, then summed / averaged over the batch (``batch_reduction`` 'sum' | 'mean' | None =
    one value per cloud).  Two ``ga_pc_nearest`` launches and torch reductions on the device.  Forward only."""
    if point_reduction not in ("mean", "sum"):
        raise ValueError('point_reduction must be one of ["mean", "sum"]')
    if batch_reduction not in ("mean", "sum", None):
        raise ValueError('batch_reduction must be one of ["mean", "sum"] or None')
    if (isinstance(x, torch.Tensor) and x.requires_grad) or (isinstance(y, torch.Tensor) and y.requires_grad):
        raise RuntimeError("chamfer_distance is forward only: an input requires grad")
    cham_x, _ = nearest_points(x, y, x_lengths, y_lengths)   # padded slots hold 0
    cham_y, _ = nearest_points(y, x, y_lengths, x_lengths)
    B, Nx = cham_x.shape
    Ny = cham_y.shape[1]
    cham_x, cham_y = cham_x.sum(1), cham_y.sum(1)
    if point_reduction == "mean":
        xl = torch.as_tensor(x_lengths if x_lengths is not None else [Nx] * B, device=cham_x.device).to(torch.float32)
        yl = torch.as_tensor(y_lengths if y_lengths is not None else [Ny] * B, device=cham_x.device).to(torch.float32)
        cham_x, cham_y = cham_x / xl, cham_y / yl
    if batch_reduction is not None:
        cham_x, cham_y = cham_x.sum(), cham_y.sum()
        if batch_reduction == "mean":
            cham_x, cham_y = cham_x / B, cham_y / B
    return cham_x + cham_y, None
