"""Times ``pointcloud.unproject_depth_views`` (ga_pc_unproject: three launches, the count stays on the device) against the same cloud
composed in torch on the same device in the same run, and writes profiles/unproject_bench.txt.

    python tools/bench_unproject.py [--rounds 9] [--out profiles/unproject_bench.txt]

The torch side is what a user without the kernel writes: the pixel grid, the lift through the intrinsics, the rotation, the
normalisation of the rays, the point, the validity tests, then a boolean-mask index of points, colours, normals and pixel numbers --
the index reads the count back to the host, which is part of what it costs.  Both sides get ray-distance depth, an alpha mask, fp32
colours and normals, the clip and the zero filter of the reference's hand-off.  The sides are timed alternately with device events
after a warm-up of each; the table reports the median and the range.  The HIP side is timed twice: as the front end allocates
(``capacity=None``) and into a capacity of the true count, the second being what a caller who knows its scene pays."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gaussiananything_amd import cameras, pointcloud  # noqa: E402

SHAPES = [(8, 512), (8, 128)]
CLIP, DEPTH_MIN = 0.45, 1.05


def torch_cloud(depth, c, alpha, color, normal):
    V, H, W = depth.shape
    dev = depth.device
    c2w = c[:, :16].reshape(V, 4, 4)
    fx, sk, cx, fy, cy = c[:, 16, None, None], c[:, 17, None, None], c[:, 18, None, None], c[:, 20, None, None], c[:, 21, None, None]
    u = (torch.arange(W, device=dev, dtype=torch.float32) * (1.0 / W) + 0.5 / W)[None, None, :]
    v = (torch.arange(H, device=dev, dtype=torch.float32) * (1.0 / H) + 0.5 / H)[None, :, None]
    xl = (u - cx + cy * sk / fy - sk * v / fy) / fx
    yl = ((v - cy) / fy).expand_as(xl)
    cam_dir = torch.stack([xl, yl, torch.ones_like(xl)], -1)                      # [V,H,W,3]
    d = torch.einsum("vab,vhwb->vhwa", c2w[:, :3, :3], cam_dir)
    d = torch.nn.functional.normalize(d, dim=-1)
    p = c2w[:, None, None, :3, 3] + depth[..., None] * d
    p = p.clamp(-CLIP, CLIP)
    ok = (depth >= DEPTH_MIN) & torch.isfinite(depth) & (alpha >= 0.5) & (p.abs() != CLIP).all(-1) & (p != 0).all(-1)
    n = normal.permute(0, 2, 3, 1)[ok]
    return (p[ok], color.permute(0, 2, 3, 1)[ok], torch.nn.functional.normalize(n, dim=-1), ok.reshape(-1).nonzero()[:, 0])


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unproject_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_unproject.py needs the GPU: a timing on anything else says nothing")
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    lines = [f"# tools/bench_unproject.py --rounds {a.rounds}   device: {torch.cuda.get_device_name(0)}",
             "# times in ms: median [min .. max] of alternating rounds, device events.  HIP = unproject_depth_views (ga_pc_unproject, three",
             "# launches, no host read) with its allocations; 'HIP, fitted' = the same into capacity = the true count; torch = the same cloud",
             "# composed from tensor operations with a boolean-mask index (one host read-back).  Ray-distance depth, alpha mask, fp32 colours,",
             "# normals, clip 0.45 and the zero filter on both sides.",
             f"{'shape':<14} {'valid':>9} {'HIP':>8} {'':<19} {'HIP, fitted':>11} {'':<19} {'torch':>8} {'':<19} {'torch / HIP':>11}"]
    for V, S in SHAPES:
        c = torch.from_numpy(cameras.orbit_poses(V)).to(dev)
        depth = (1.77 - 0.35 + 0.3 * (torch.rand(V, S, S, generator=gen) - 0.5)).to(dev)
        depth[torch.rand(V, S, S, generator=gen).to(dev) < 0.1] = 0.0
        alpha = (torch.rand(V, S, S, generator=gen) < 0.8).float().to(dev)
        color = torch.rand(V, 3, S, S, generator=gen).to(dev)
        normal = torch.randn(V, 3, S, S, generator=gen).to(dev)
        lo = float(torch.nextafter(torch.tensor(DEPTH_MIN, dtype=torch.float32), torch.tensor(0.0)))
        kw = dict(mask=alpha, color=color, normal=normal, depth_kind="ray", depth_range=(lo, float("inf")), clip=CLIP, drop_zero=True)
        hip = pointcloud.unproject_depth_views(depth, c, **kw).trimmed()
        tp, tc, tn, ts = torch_cloud(depth, c, alpha, color, normal)
        n = hip.points.shape[0]
        # the two sides round differently: pixels on the clip boundary may differ, everything else is the same cloud
        both = torch.isin(hip.source.long(), ts)
        gap = float((hip.points[both] - tp[torch.isin(ts, hip.source.long())]).abs().max())
        agree = f"{int((~both).sum())} + {int(ts.numel() - both.sum())} pixels kept by one side only, largest coordinate gap {gap:.2e}"
        t = time_many([lambda: pointcloud.unproject_depth_views(depth, c, **kw),
                       lambda: pointcloud.unproject_depth_views(depth, c, capacity=n, **kw),
                       lambda: torch_cloud(depth, c, alpha, color, normal)], a.rounds)
        mh, mf, mt = (statistics.median(x) for x in t)
        verdict = "HIP faster" if mh < mt else "HIP LOSES at this shape"
        lines.append(f"{f'{V} x {S} x {S}':<14} {n:>9} {cell(t[0])}  {cell(t[1])}  {cell(t[2])}  {mt / mh:10.2f}x  {verdict}; {agree}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
