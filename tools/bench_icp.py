#!/usr/bin/env python
"""ICP in one enqueue (``pointcloud.iterative_closest_point`` -> ``ga_pc_icp``) against the composition a user writes without it, on the
same device: ``pointcloud.nearest_points``, a torch Kabsch with ``torch.linalg.svd`` and pytorch3d's per-iteration host read of the
convergence test.  Both sides run the same scene; medians of alternating rounds with their ranges.  Also one match-accumulate launch
(``max_iterations=0``: the final pass and its solve) against one ``ga_pc_nearest`` launch: the price of the fused reduction.

    python tools/bench_icp.py [--rounds 9] [--out profiles/icp_bench.txt]
"""
import argparse
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gaussiananything_amd import pointcloud as pc   # noqa: E402


def scene(B, N, M, device, seed=0):
    """a bumpy ellipsoid of M points, X = N of them (with replacement) rotated by 0.1 rad and shifted by 0.02"""
    g = torch.Generator().manual_seed(seed)
    i = torch.arange(M, dtype=torch.float64) + 0.5
    phi, th = torch.acos(1 - 2 * i / M), math.pi * (1 + 5 ** 0.5) * i
    p = torch.stack([th.cos() * phi.sin(), th.sin() * phi.sin(), phi.cos()], 1) * torch.tensor([0.4, 0.25, 0.15], dtype=torch.float64)
    y = p + 0.02 * torch.sin(7 * p[:, [1, 2, 0]])
    xs = []
    for _ in range(B):
        a = torch.randn(3, generator=g, dtype=torch.float64)
        a = a / a.norm()
        K = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
        R = torch.eye(3, dtype=torch.float64) + math.sin(0.1) * K + (1 - math.cos(0.1)) * K @ K
        xs.append((y[torch.randint(M, (N,), generator=g)] - 0.02 * a) @ R)
    return torch.stack(xs).float().to(device), y.float()[None].expand(B, -1, -1).contiguous().to(device)


def composed_icp(X, Y, max_iterations, thr):
    """what a user composes today, after pytorch3d.ops.iterative_closest_point: nearest points, Kabsch by SVD, apply, rmse, and a host
    read of the convergence test in every iteration"""
    Xt = X
    prev = None
    R = torch.eye(3, device=X.device).expand(X.shape[0], 3, 3)
    T = torch.zeros(X.shape[0], 3, device=X.device)
    it = 0
    for it in range(1, max_iterations + 1):
        _, idx = pc.nearest_points(Xt, Y)
        P = torch.gather(Y, 1, idx[:, :, None].expand(-1, -1, 3))
        xm, pm = X.mean(1, keepdim=True), P.mean(1, keepdim=True)
        U, _, Vh = torch.linalg.svd((X - xm).transpose(1, 2) @ (P - pm))
        E = torch.ones(X.shape[0], 3, device=X.device)
        E[:, 2] = torch.sign(torch.linalg.det(U @ Vh))
        R = (U * E[:, None, :]) @ Vh
        T = pm[:, 0] - (xm @ R)[:, 0]
        Xt = X @ R + T[:, None]
        rmse = ((Xt - P) ** 2).sum(2).mean(1).sqrt()
        if prev is not None and bool((((prev - rmse).abs() / prev.clamp(min=1e-30)) <= thr).all()):   # the host read
            break
        prev = rmse
    return R, T, it


def timed(fn, device):
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(device)
    return (time.perf_counter() - t0) * 1e3, out


def fmt(ts):
    return f"{statistics.median(ts):9.3f} [{min(ts):9.3f} .. {max(ts):9.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"# tools/bench_icp.py --rounds {a.rounds}   device: {torch.cuda.get_device_name(dev)}",
             "# wall-clock ms from enqueue to synchronize: median [min .. max] of alternating rounds; speed-up = composed median / ga_pc_icp median",
             "# composed = pointcloud.nearest_points + torch Kabsch (torch.linalg.svd) + a host read of the convergence test per iteration",
             f"{'shape, setting':44s}{'ga_pc_icp (one enqueue)':>36s}{'composed':>36s}{'speed-up':>10s}  notes"]
    for B, N, M in ((1, 100000, 100000), (8, 4096, 4096)):
        X, Y = scene(B, N, M, dev)
        for label, thr, iters in (("thr 0, 20 iterations", 0.0, 20), ("default thr 1e-6, cap 100", 1e-6, 100)):
            # thr = 0: the composed loop never breaks before the cap unless the rmse repeats exactly; ours freezes a cloud whose rmse repeats
            # bit for bit, so `iterations` is reported with it
            ours = lambda: pc.iterative_closest_point(X, Y, max_iterations=iters, relative_rmse_thr=thr)
            theirs = lambda: composed_icp(X, Y, iters, thr)
            timed(ours, dev), timed(theirs, dev)                                   # warm-up
            to, tt = [], []
            for _ in range(a.rounds):
                t, sol = timed(ours, dev)
                to.append(t)
                t, (R, T, it) = timed(theirs, dev)
                tt.append(t)
            dR = float((sol.RTs.R - R).abs().max())
            lines.append(f"{f'{B} x {N} x {M}, {label}':44s}{fmt(to):>36s}{fmt(tt):>36s}{statistics.median(tt) / statistics.median(to):9.2f}x"
                         f"  iterations ours {sol.iterations.tolist()} composed {it}; converged {sol.converged.tolist()}; "
                         f"largest difference in R {dR:.1e}")
        one = lambda: pc.iterative_closest_point(X, Y, max_iterations=0)
        near = lambda: pc.nearest_points(X, Y)
        timed(one, dev), timed(near, dev)
        to, tt = [], []
        for _ in range(a.rounds):
            to.append(timed(one, dev)[0])
            tt.append(timed(near, dev)[0])
        lines.append(f"{f'{B} x {N} x {M}, one match pass':44s}{fmt(to):>36s}{fmt(tt):>36s}{statistics.median(tt) / statistics.median(to):9.2f}x"
                     f"  left: init + match-accumulate (writes Xt, idx, dist2) + solve; right: one ga_pc_nearest")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
