"""Times ga_pc_fps and ga_pc_nearest against the same operations written in torch, on the same device in the same run, and writes
profiles/pointcloud_bench.txt.

    python tools/bench_pointcloud.py [--reps 5] [--out profiles/pointcloud_bench.txt]

The torch restatements are what a user without the kernels would write: FPS as K dependent iterations of broadcast distance, minimum
and argmax over the padded batch (about six launches an iteration); nearest point as chunked broadcast distances and ``min``.  The
two sides are timed alternately with device events, after a warm-up of each; the table reports the median and the spread."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gaussiananything_amd import pointcloud  # noqa: E402

# the last row is a yardstick, not a target: the largest register-resident cloud, for variant (a)'s per-point rate beside (b)'s
FPS_SHAPES = [(1, 73728, 768), (1, 100000, 4096), (8, 73728, 4096), (1, 16384, 4096)]
NEAREST_SHAPES = [(4096, 4096), (73728, 768), (100000, 100000)]


def torch_fps(points, K):
    B, N, _ = points.shape
    closest = torch.full((B, N), float("inf"), device=points.device)
    idx = torch.empty(B, K, dtype=torch.int64, device=points.device)
    sel = torch.zeros(B, dtype=torch.int64, device=points.device)
    rows = torch.arange(B, device=points.device)
    for k in range(K):
        idx[:, k] = sel
        d = (points - points[rows, sel][:, None, :]).square().sum(-1)
        closest = torch.minimum(closest, d)
        sel = closest.argmax(1)
    return idx


def torch_nearest(x, y, chunk_elems=1 << 27):
    chunk = max(1, chunk_elems // y.shape[1])
    d2 = torch.empty(x.shape[:2], device=x.device)
    idx = torch.empty(x.shape[:2], dtype=torch.int64, device=x.device)
    for s in range(0, x.shape[1], chunk):
        d = (x[:, s:s + chunk, None, :] - y[:, None, :, :]).square().sum(-1)
        d2[:, s:s + chunk], idx[:, s:s + chunk] = d.min(-1)
    return d2, idx


def time_pair(fn_a, fn_b, reps):
    """alternating timings of two callables -> (times_a, times_b) in ms"""
    out = ([], [])
    for fn in (fn_a, fn_b):
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for fn, acc in zip((fn_a, fn_b), out):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            acc.append(start.elapsed_time(stop))
    return out


def row(name, plan, hip, ref):
    mh, mr = statistics.median(hip), statistics.median(ref)
    return (f"{name:<34} {plan:<22} {mh:10.3f} [{min(hip):9.3f} ..{max(hip):9.3f}]  {mr:10.3f} [{min(ref):9.3f} ..{max(ref):9.3f}]"
            f"  {mr / mh:8.1f}x")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pointcloud_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    lines = [f"# tools/bench_pointcloud.py --reps {a.reps}   device: {torch.cuda.get_device_name(0)}",
             "# times in ms: median [min .. max] of alternating runs; speed-up = torch median / HIP median",
             f"{'operation (shape)':<34} {'plan':<22} {'HIP':>10} {'':<24} {'torch':>10} {'':<24} {'speed-up':>9}"]
    for B, N, K in FPS_SHAPES:
        p = ((torch.rand(B, N, 3, generator=gen) - 0.5) * 0.9).to(dev)
        pl = pointcloud.fps_plan(N, K)
        got = pointcloud.sample_farthest_points(p, K=K)[1]
        same = bool(torch.equal(got[:, :64], torch_fps(p, 64)))   # informative only: torch may contract or reassociate the sums
        hip, ref = time_pair(lambda: pointcloud.sample_farthest_points(p, K=K), lambda: torch_fps(p, K), a.reps)
        lines.append(row(f"fps {B} x {N} -> {K}", f"{pl['variant']} {pl['threads']}x{pl['points_per_lane']}", hip, ref)
                     + f"   first 64 indices equal torch's: {same}; {statistics.median(hip) * 1e6 / (K * N * B):.3f} ns per point-iteration")
        print(lines[-1], flush=True)
    for Nq, Nt in NEAREST_SHAPES:
        x = ((torch.rand(1, Nq, 3, generator=gen) - 0.5) * 0.9).to(dev)
        y = ((torch.rand(1, Nt, 3, generator=gen) - 0.5) * 0.9).to(dev)
        same = bool(torch.equal(pointcloud.nearest_points(x, y)[1], torch_nearest(x, y)[1]))
        hip, ref = time_pair(lambda: pointcloud.nearest_points(x, y), lambda: torch_nearest(x, y), a.reps)
        lines.append(row(f"nearest {Nq} x {Nt}", "256 lanes, 1024 tile", hip, ref)
                     + f"   indices equal torch's: {same}; {Nq * Nt / statistics.median(hip) * 1e-6:.1f} G pairs/s")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
