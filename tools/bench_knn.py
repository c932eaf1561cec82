"""Times ga_pc_knn and ga_pc_knn_backward against the same operations written in torch, on the same device in the same run, with
ga_pc_nearest beside every K = 1 row, and writes profiles/knn_bench.txt.

    python tools/bench_knn.py [--reps 5] [--out profiles/knn_bench.txt]

The torch restatements are what a user without the kernels would write: kNN as chunked broadcast distances and ``topk``; the
backward as a gather, the products, a sum over K for the query side and ``index_add_`` for the target side (whose atomics make its
summation order, unlike the kernel's, vary from run to run).  The sides are timed alternately with device events, after a warm-up
of each; the table reports the median and the spread."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gaussiananything_amd import pointcloud  # noqa: E402

KNN_SHAPES = [(4096, 4096, 1), (4096, 4096, 8), (4096, 4096, 32), (100000, 100000, 1), (100000, 100000, 16), (73728, 768, 4)]
BACKWARD_SHAPES = [(4096, 4096, 1), (100000, 100000, 1)]


def torch_knn(x, y, K, chunk_elems=1 << 27):
    chunk = max(1, chunk_elems // y.shape[1])
    d2 = torch.empty(x.shape[:2] + (K,), device=x.device)
    idx = torch.empty(x.shape[:2] + (K,), dtype=torch.int64, device=x.device)
    for s in range(0, x.shape[1], chunk):
        d = (x[:, s:s + chunk, None, :] - y[:, None, :, :]).square().sum(-1)
        d2[:, s:s + chunk], idx[:, s:s + chunk] = d.topk(K, dim=-1, largest=False)
    return d2, idx


def torch_knn_backward(x, y, idx, grad):
    """one cloud pair [1,N,3]: -> (grad_x, grad_y)"""
    u = (2.0 * grad)[0, :, :, None] * (x[0, :, None, :] - y[0][idx[0]])          # [Nq,K,3]
    gy = torch.zeros_like(y[0]).index_add_(0, idx[0].reshape(-1), -u.reshape(-1, 3))
    return u.sum(1)[None], gy[None]


def time_many(fns, reps):
    """alternating timings of the callables -> one list of times in ms per callable"""
    out = [[] for _ in fns]
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for fn, acc in zip(fns, out):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            acc.append(start.elapsed_time(stop))
    return out


def cell(times):
    return f"{statistics.median(times):10.3f} [{min(times):9.3f} ..{max(times):9.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    lines = [f"# tools/bench_knn.py --reps {a.reps}   device: {torch.cuda.get_device_name(0)}",
             "# times in ms: median [min .. max] of alternating runs; speed-up = torch median / HIP median; the last column is",
             "# ga_pc_nearest on the same clouds (K = 1 rows only)",
             f"{'operation (shape)':<36} {'plan':<30} {'HIP':>10} {'':<24} {'torch':>10} {'':<24} {'speed-up':>9}  {'ga_pc_nearest':>13}"]
    clouds = {}

    def pair(Nq, Nt):
        if (Nq, Nt) not in clouds:
            clouds[(Nq, Nt)] = (((torch.rand(1, Nq, 3, generator=gen) - 0.5) * 0.9).to(dev),
                                ((torch.rand(1, Nt, 3, generator=gen) - 0.5) * 0.9).to(dev))
        return clouds[(Nq, Nt)]

    for Nq, Nt, K in KNN_SHAPES:
        x, y = pair(Nq, Nt)
        pl = pointcloud.knn_plan(Nq, Nt, K)
        plan = f"{pl['k_slots']} slots, {pl['grid_x']} x {pl['threads']} lanes, tile {pl['tile']}"
        same = bool(torch.equal(pointcloud.knn_points(x, y, K=K).idx, torch_knn(x, y, K)[1]))   # informative: torch may contract the sums
        fns = [lambda: pointcloud.knn_points(x, y, K=K), lambda: torch_knn(x, y, K)]
        if K == 1:
            fns.append(lambda: pointcloud.nearest_points(x, y))
        t = time_many(fns, a.reps)
        mh, mr = statistics.median(t[0]), statistics.median(t[1])
        lines.append(f"{f'knn {Nq} x {Nt} K {K}':<36} {plan:<30} {cell(t[0])}  {cell(t[1])}  {mr / mh:8.1f}x  "
                     f"{statistics.median(t[2]) if K == 1 else float('nan'):13.3f}"
                     f"   indices equal torch's: {same}; {Nq * Nt / mh * 1e-6:.1f} G pairs/s")
        print(lines[-1], flush=True)
    for Nq, Nt, K in BACKWARD_SHAPES:
        x, y = pair(Nq, Nt)
        out = pointcloud.knn_points(x, y, K=K)
        idx32 = out.idx.to(torch.int32).contiguous()
        grad = (torch.rand(1, Nq, K, generator=gen) * 2 - 1).to(dev)
        xs, ys = x.contiguous(), y.contiguous()
        hq, ht = pointcloud._knn_backward(xs, ys, None, None, idx32, grad, True, True)
        rq, rt = torch_knn_backward(x, y, out.idx, grad)
        err = max(float((hq - rq).abs().max()), float((ht - rt).abs().max()))
        t = time_many([lambda: pointcloud._knn_backward(xs, ys, None, None, idx32, grad, True, True),
                       lambda: torch_knn_backward(x, y, out.idx, grad), lambda: pointcloud.nearest_points(x, y)], a.reps)
        mh, mr = statistics.median(t[0]), statistics.median(t[1])
        lines.append(f"{f'knn backward {Nq} x {Nt} K {K}':<36} {'query + target side':<30} {cell(t[0])}  {cell(t[1])}  {mr / mh:8.1f}x  "
                     f"{statistics.median(t[2]):13.3f}   largest difference to torch's: {err:.2e}; "
                     f"{Nq * K * Nt / mh * 1e-6:.1f} G index compares/s")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
