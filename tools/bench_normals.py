"""Times ``pointcloud.estimate_normals`` (ga_pc_knn + ga_pc_normals) against the same computation composed in torch on the same device
in the same run, and writes profiles/normals_bench.txt.

    python tools/bench_normals.py [--rounds 9] [--out profiles/normals_bench.txt]

The torch side is what a user without the kernel would write: ``knn_points`` (the project's own kernel: torch has none) +
``knn_gather`` + the centred covariance + ``torch.linalg.eigh``, the eigenvector of the smallest eigenvalue as the normal.  Both sides
therefore pay the same kNN; it is timed alone as a third column, so the share of the part that differs can be read off.  The sides
are timed alternately with device events after a warm-up of each; the table reports the median and the range."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gaussiananything_amd import pointcloud  # noqa: E402

SHAPES = [(1, 100000, 16), (1, 4096, 16)]


def torch_normals(p, K):
    knn = pointcloud.knn_points(p, p, K=K)
    nb = pointcloud.knn_gather(p, knn.idx)                       # [B,N,K,3]
    d = nb - nb.mean(2, keepdim=True)
    cov = d.transpose(2, 3) @ d / K                              # [B,N,3,3]
    lam, vec = torch.linalg.eigh(cov)
    return vec[..., 0], lam


def time_many(fns, rounds):
    """alternating timings of the callables -> one list of times in ms per callable"""
    out = [[] for _ in fns]
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for fn, acc in zip(fns, out):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            acc.append(start.elapsed_time(stop))
    return out


def cell(times):
    return f"{statistics.median(times):9.3f} [{min(times):8.3f} ..{max(times):8.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "normals_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_normals.py needs the GPU: a timing on anything else says nothing")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    lines = [f"# tools/bench_normals.py --rounds {a.rounds}   device: {torch.cuda.get_device_name(0)}",
             "# times in ms: median [min .. max] of alternating rounds, device events.  HIP = estimate_normals(return_frame=True):",
             "# ga_pc_knn + ga_pc_normals; torch = knn_points + knn_gather + centred covariance + torch.linalg.eigh; kNN = knn_points alone,",
             "# which both sides pay.  'beyond kNN' = median minus the kNN median: the part in which the two sides differ.",
             f"{'shape':<20} {'plan':<22} {'HIP':>9} {'':<21} {'torch':>9} {'':<21} {'kNN alone':>9} {'':<21} {'torch / HIP':>11}  beyond kNN: HIP, torch"]
    for B, N, K in SHAPES:
        # a surface, not a volume: points on a sphere of radius 0.45 with 1 % radial noise
        v = torch.randn(B, N, 3, generator=gen)
        p = (v / v.norm(dim=-1, keepdim=True) * (0.45 * (1 + 0.01 * torch.randn(B, N, 1, generator=gen)))).to(dev)
        pl = pointcloud.normals_plan(N, K)
        plan = f"{pl['grid_x']} x {pl['threads']} lanes, {pl['sweeps']} sweeps"
        n_hip, _, lam_hip = pointcloud.estimate_normals(p, K=K, return_frame=True)
        n_t, lam_t = torch_normals(p, K)
        sin = torch.linalg.cross(n_hip.double(), n_t.double()).norm(dim=-1)
        gap = ((lam_t[..., 1] - lam_t[..., 0]) / lam_t[..., 2]).double()
        agree = float((sin * gap).max())
        t = time_many([lambda: pointcloud.estimate_normals(p, K=K, return_frame=True), lambda: torch_normals(p, K),
                       lambda: pointcloud.knn_points(p, p, K=K)], a.rounds)
        mh, mt, mk = (statistics.median(x) for x in t)
        verdict = "HIP faster" if mh < mt else "HIP LOSES at this shape"
        lines.append(f"{f'{B} x {N} K {K}':<20} {plan:<22} {cell(t[0])}  {cell(t[1])}  {cell(t[2])}  {mt / mh:10.2f}x  "
                     f"{mh - mk:.3f}, {mt - mk:.3f} ms; kNN is {100 * mk / mh:.0f} % of HIP, {100 * mk / mt:.0f} % of torch; {verdict}; "
                     f"largest sin(angle to torch's normal) * gap {agree:.2e}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
