"""Times ``pointcloud.voxel_thin`` (ga_pc_voxel_thin) and ``pointcloud.filter_view_consistency`` (ga_pc_filter_views) against what a
user composes in torch today, on the same device in the same run, and writes profiles/pc_filter_bench.txt.

    python tools/bench_pc_filter.py [--rounds 9] [--out profiles/pc_filter_bench.txt] [--trace-only]

The clouds are those of 8 x 512 x 512 and 8 x 128 x 128 views of a rendered surfel scene (``cloud_from_render``), trimmed.  The torch
side of the thinning: packed int64 keys -> ``torch.unique(return_inverse=True)`` (a sort) -> ``scatter_reduce(amin)`` of the rank ->
boolean-mask index of points, colours and normals; of the filter: project -> gather the 3 x 3 window -> compare, per view, -> boolean-
mask index.  Both indices read a count back to the host, which is part of what they cost.  The sides are timed alternately with device
events around the whole Python call after a warm-up of each; the table reports the median and the range.  The voxel sizes are found by
bisection so that the thinning keeps about 1 / 4 and about 1 / 30 of the points.  ``--trace-only`` runs the HIP calls alone, 12 times
per row, for a kernel trace (profiles/pc_filter_kernel_times.txt)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gaussiananything_amd import cameras, pointcloud, synthetic  # noqa: E402
from gaussiananything_amd.gs_surfel import GaussianRenderer2DGS  # noqa: E402

SHAPES = [(8, 512), (8, 128)]
THIN = (4.0, 30.0)
TOL = 0.01


def rendered_views(V, S, dev):
    cams = synthetic.eval_cameras(V)
    cv, cvp, cp = (cams[k][:V].to(dev) for k in ("cam_view", "cam_view_proj", "cam_pos"))
    g = synthetic.random_surfels(4000, seed=3)
    g[..., 4:6] *= 4.0
    with torch.no_grad():
        out = GaussianRenderer2DGS(S, 3, {}).render(g.to(dev), cv[None], cvp[None], cp[None], cams["tanfov"])
    cam = cameras.cameras_from_view(cv, cams["tanfov"]).to(dev)
    return out, cv, cams["tanfov"], cam


def torch_thin(p, colors, normals, vs):
    cell = torch.floor(p / vs)
    g = cell.long() + (1 << 20)
    key = (g[:, 0] << 42) | (g[:, 1] << 21) | g[:, 2]
    uniq, inv = torch.unique(key, return_inverse=True)
    d = p - (cell + 0.5) * vs
    dist2 = (d * d).sum(-1)
    rank = (dist2.view(torch.int32).long() << 32) | torch.arange(p.shape[0], device=p.device)
    best = torch.full((uniq.numel(),), 2 ** 62, dtype=torch.int64, device=p.device).scatter_reduce(0, inv, rank, "amin")
    keep = best[inv] == rank
    return p[keep], colors[keep], normals[keep], keep.nonzero()[:, 0]


def torch_filter(p, colors, normals, source, depth, mask, cam):
    V, H, W = depth.shape
    own = source.long() // (H * W)
    surf = (depth > 0) & torch.isfinite(depth) & (mask >= 0.5)
    support = torch.zeros(p.shape[0], dtype=torch.int32, device=p.device)
    conflicts = torch.zeros_like(support)
    inf = torch.tensor(float("inf"), device=p.device)
    for u in range(V):
        R, t = cam[u, :9].reshape(3, 3), cam[u, 9:12]
        q = (p - t) @ R
        qz = q[:, 2]
        uu = q[:, 0] / qz * cam[u, 12] + cam[u, 14]
        vv = q[:, 1] / qz * cam[u, 13] + cam[u, 15]
        a, b = uu * W, vv * H
        ok = (own != u) & (qz > 0) & (a >= 0) & (a < W) & (b >= 0) & (b < H)
        x, y = a.clamp(0, W - 1).long(), b.clamp(0, H - 1).long()
        zmin, zmax = torch.full_like(qz, float("inf")), torch.full_like(qz, -float("inf"))
        n_in, n_surf = torch.zeros_like(support), torch.zeros_like(support)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                xx, yy = x + dx, y + dy
                inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
                at = yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)
                z, s = depth[u].reshape(-1)[at], surf[u].reshape(-1)[at] & inside
                n_in += inside
                n_surf += s
                zmin = torch.where(s, torch.minimum(zmin, z), zmin)
                zmax = torch.where(s, torch.maximum(zmax, z), zmax)
                if dx == 0 and dy == 0:
                    centre = s
        lo, hi = zmin - TOL * zmin, zmax + TOL * zmax
        support += ok & centre & (lo <= qz) & (qz <= hi)
        conflicts += ok & (n_surf > 0) & (n_surf == n_in) & (qz < torch.where(n_surf > 0, lo, -inf))
    keep = (support >= 1) & (conflicts <= 0)
    return p[keep], colors[keep], normals[keep], source[keep]


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
    return f"{statistics.median(times):8.3f} [{min(times):7.3f} ..{max(times):7.3f}]"


def voxel_for(cloud, factor):
    """the voxel size at which ``voxel_thin`` keeps about 1 / factor of the rows, by bisection"""
    n = cloud.points.shape[0]
    lo, hi = 1e-4, 1.0
    for _ in range(24):
        mid = (lo * hi) ** 0.5
        kept = int(pointcloud.voxel_thin(cloud, mid).count.item())
        lo, hi = (mid, hi) if kept * factor > n else (lo, mid)
    return (lo * hi) ** 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pc_filter_bench.txt"))
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_pc_filter.py needs the GPU: a timing on anything else says nothing")
    dev = torch.device("cuda:0")
    lines = [f"# tools/bench_pc_filter.py --rounds {a.rounds}   device: {torch.cuda.get_device_name(0)}",
             "# times in ms: median [min .. max] of alternating rounds, device events around the whole Python call.  HIP = voxel_thin",
             "# (ga_pc_voxel_thin, five launches) / filter_view_consistency (ga_pc_filter_views, three launches) with their allocations,",
             "# no host read; torch = the same result composed from tensor operations (unique + scatter_reduce / project + gather +",
             "# compare per view) with a boolean-mask index (one host read-back).  Clouds: cloud_from_render of a rendered surfel scene.",
             "# HIP = the front end's default (pointcloud.VOXEL_WAVE_MERGE: neighbouring lanes of a wave with one key are inserted once);",
             "# 'HIP, plain insert' = the A/B, one atomic chain per row, timed in the same alternating rounds.",
             f"{'shape':<14} {'operation':<18} {'rows':>8} {'kept':>8} {'HIP':>8} {'':<19} {'HIP, plain insert':>17} {'':<10} {'torch':>8} {'':<19} "
             f"{'torch / HIP':>11}"]
    for V, S in SHAPES:
        out, cv, tanfov, cam = rendered_views(V, S, dev)
        cloud = pointcloud.cloud_from_render(out, cv[None], tanfov).trimmed()
        depth, mask = out["depth"][0, :, 0].contiguous(), out["alpha"][0, :, 0].contiguous()
        n = cloud.points.shape[0]
        jobs = []
        for factor in THIN:
            vs = voxel_for(cloud, factor)
            # HIP is the front end's default; the other insert is the A/B: one atomic chain per row against one per run of equal keys
            jobs.append((f"thin, voxel {vs:.4f}", [lambda vs=vs: pointcloud.voxel_thin(cloud, vs),
                                                   lambda vs=vs: pointcloud.voxel_thin(cloud, vs, wave_merge=False)],
                         lambda vs=vs: torch_thin(cloud.points, cloud.colors, cloud.normals, vs)))
        jobs.append(("filter, window 1", [lambda: pointcloud.filter_view_consistency(cloud, depth, cam, mask=mask, tolerance=(0.0, TOL))],
                     lambda: torch_filter(cloud.points, cloud.colors, cloud.normals, cloud.source, depth, mask, cam)))
        for name, hips, ref in jobs:
            if a.trace_only:
                for hip in hips:
                    for _ in range(13):
                        hip()
                torch.cuda.synchronize()
                continue
            got, want = hips[0](), ref()
            kept = int(got.count.item())
            theirs = want[3].numel()
            if name.startswith("thin"):
                agree = "same rows" if kept == theirs and torch.equal(got.kept_rows[:kept].long(), want[3]) else \
                    f"torch keeps {theirs} rows (its cell arithmetic rounds p / voxel and the centre differently)"
                other = hips[1]()
                assert torch.equal(other.kept_rows, got.kept_rows) and torch.equal(other.multiplicity, got.multiplicity)
            else:
                agree = "same rows" if kept == theirs and torch.equal(got.source[:kept], want[3]) else \
                    f"torch keeps {theirs} rows (its projection is a matrix product and rounds differently)"
            t = time_many(hips + [ref], a.rounds)
            mh, mt = statistics.median(t[0]), statistics.median(t[-1])
            verdict = "HIP faster" if mh < mt else "HIP LOSES at this shape"
            plain = cell(t[1]) if len(hips) > 1 else f"{'-':>28}"
            lines.append(f"{f'{V} x {S} x {S}':<14} {name:<18} {n:>8} {kept:>8} {cell(t[0])}  {plain}  {cell(t[-1])}  {mt / mh:10.2f}x  {verdict}; {agree}")
            print(lines[-1], flush=True)
    if a.trace_only:
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
