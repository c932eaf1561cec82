"""Times gaussiananything_amd.losses.geometric_loss against the same terms composed in torch, on the same device in the same run,
forward and forward + backward, and writes profiles/geo_loss_bench.txt.

    python tools/bench_geo_loss.py [--reps 9] [--out profiles/geo_loss_bench.txt]

The torch loss is what a user without the kernels writes from the reference's ``depths_to_points_2`` / ``depth_to_normal_2`` for V views
(a meshgrid, two 3 x 3 inverses, a matmul over every pixel, two shifted differences, a cross, a normalise, a scatter into a zero map),
the 2DGS regulariser ``1 - <rend_normal, surf_normal * alpha.detach()>``, ``dist.mean()`` and the L1 of alpha against a mask, with
autograd for the backward.  Its normalise is ``F.normalize`` as the reference has it, so its depth gradient differs from the fused
one where a cross product vanishes; the inputs here have no such pixel.  The sides are timed alternately with
device events, after a warm-up of each; the table reports the median and the spread."""
import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gaussiananything_amd import losses, synthetic  # noqa: E402

SHAPES = [(8, 512, 512), (8, 128, 128)]
LAMBDAS = dict(lambda_normal=0.05, lambda_dist=100.0, lambda_alpha=1.0)


def torch_depth_to_normal(w2c, tanfov, depth):
    """[V,4,4] column-vector world-to-camera, [V,1,H,W] -> [V,3,H,W], batched over the views"""
    V, _, H, W = depth.shape
    dev = depth.device
    c2w = torch.linalg.inv(w2c)
    fx, fy = W / (2 * tanfov), H / (2 * tanfov)
    intrins = torch.tensor([[fx, 0.0, W / 2.0], [0.0, fy, H / 2.0], [0.0, 0.0, 1.0]], device=dev)
    gx, gy = torch.meshgrid(torch.arange(W, device=dev).float(), torch.arange(H, device=dev).float(), indexing="xy")
    pix = torch.stack([gx, gy, torch.ones_like(gx)], dim=-1).reshape(-1, 3)
    rays_d = (pix @ torch.linalg.inv(intrins).T)[None] @ c2w[:, :3, :3].transpose(1, 2)           # [V,HW,3]
    points = (depth.reshape(V, -1, 1) * rays_d + c2w[:, None, :3, 3]).reshape(V, H, W, 3)
    out = torch.zeros_like(points)
    dx = points[:, 2:, 1:-1] - points[:, :-2, 1:-1]
    dy = points[:, 1:-1, 2:] - points[:, 1:-1, :-2]
    out[:, 1:-1, 1:-1] = F.normalize(torch.linalg.cross(dx, dy, dim=-1), dim=-1)
    return out.permute(0, 3, 1, 2)


def torch_loss(pred, w2c, tanfov, mask, lambda_normal, lambda_dist, lambda_alpha):
    surf = torch_depth_to_normal(w2c, tanfov, pred["depth"]) * pred["alpha"].detach()
    normal = (1 - (pred["rend_normal"] * surf).sum(dim=1)).mean()
    return lambda_normal * normal + lambda_dist * pred["dist"].mean() + lambda_alpha * F.l1_loss(pred["alpha"], mask)


def time_many(fns, reps):
    """alternating timings of the callables -> one list of times in ms per callable"""
    out = [[] for _ in fns]
    for fn in fns:
        for _ in range(3):
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
    return f"{statistics.median(times):9.3f} [{min(times):8.3f} ..{max(times):8.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "geo_loss_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    cams = synthetic.eval_cameras(8)
    tanfov = cams["tanfov"]
    lines = [f"# tools/bench_geo_loss.py --reps {a.reps}   device: {torch.cuda.get_device_name(0)}",
             "# geometric_loss (0.05 normal + 100 dist + alpha L1); times in ms: median [min .. max] of alternating runs, host launch",
             "# overhead included on both sides; speed-up = torch median / HIP median",
             f"{'shape':<14} {'pass':<20} {'HIP':>9} {'':<21} {'torch':>9} {'':<21} {'speed-up':>9}"]
    for V, H, W in SHAPES:
        cam_view = cams["cam_view"][:V].to(dev)
        w2c = cam_view.transpose(1, 2).contiguous()
        y, x = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
        depth = (1.7 + 0.2 * torch.sin(3 * x) * torch.cos(2 * y))[None, None] + 0.01 * torch.rand(V, 1, H, W, generator=gen)
        base = {"depth": depth, "alpha": 0.1 + 0.9 * torch.rand(V, 1, H, W, generator=gen),
                "dist": 0.05 * torch.rand(V, 1, H, W, generator=gen),
                "rend_normal": F.normalize(torch.randn(V, 3, H, W, generator=gen), dim=1)}
        mask = (torch.rand(V, 1, H, W, generator=gen) < 0.6).float().to(dev)
        leaves = {k: v.to(dev).requires_grad_(True) for k, v in base.items()}
        batched = {k: v[None] for k, v in leaves.items()}

        def zero():
            for t in leaves.values():
                t.grad = None

        def hip_forward():
            with torch.no_grad():
                return losses.geometric_loss(batched, cam_view[None], tanfov, mask=mask[None], **LAMBDAS)[0]

        def torch_forward():
            with torch.no_grad():
                return torch_loss(leaves, w2c, tanfov, mask, **LAMBDAS)

        def hip_both():
            zero()
            losses.geometric_loss(batched, cam_view[None], tanfov, mask=mask[None], **LAMBDAS)[0].backward()

        def torch_both():
            zero()
            torch_loss(leaves, w2c, tanfov, mask, **LAMBDAS).backward()

        hip_both()
        gh = {k: t.grad.clone() for k, t in leaves.items()}
        torch_both()
        err = max(float((gh[k] - t.grad).norm() / t.grad.norm()) for k, t in leaves.items())
        dl = abs(float(hip_forward()) - float(torch_forward()))
        for name, fns in (("forward", [hip_forward, torch_forward]), ("forward + backward", [hip_both, torch_both])):
            t = time_many(fns, a.reps)
            mh, mr = statistics.median(t[0]), statistics.median(t[1])
            lines.append(f"{f'{V}x{H}x{W}':<14} {name:<20} {cell(t[0])}  {cell(t[1])}  {mr / mh:8.1f}x"
                         f"   loss differs from torch's by {dl:.1e}, worst gradient by {err:.1e} (relative L2)")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
