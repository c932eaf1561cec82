"""Times gaussiananything_amd.losses.photometric_loss against the same loss written in torch, on the same device in the same run,
forward and forward + backward, and writes profiles/photo_loss_bench.txt.

    python tools/bench_photo_loss.py [--reps 9] [--out profiles/photo_loss_bench.txt]

The torch loss is what a user without the kernels writes from the reference's ``calc_2d_rec_loss``: five grouped 11 x 11 ``conv2d``
calls with the 2-D window, the element-wise SSIM, ``mse_loss`` and ``l1_loss``, and autograd for the backward.  The sides are timed
alternately with device events, after a warm-up of each; the table reports the median and the spread.  The lambdas are 1 / 1 / 0.2, so
every term is live on both sides."""
import argparse
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gaussiananything_amd import losses  # noqa: E402

SHAPES = [(8, 3, 512, 512), (50, 3, 128, 128)]
LAMBDAS = dict(l2_lambda=1.0, l1_lambda=1.0, ssim_lambda=0.2)


def torch_window(channel, device):
    g = torch.tensor([math.exp(-(x - 5) ** 2 / (2 * 1.5 ** 2)) for x in range(11)], dtype=torch.float32)
    g = (g / g.sum()).unsqueeze(1)
    return g.mm(g.t()).expand(channel, 1, 11, 11).contiguous().to(device)


def torch_loss(x, y, window, l2_lambda, l1_lambda, ssim_lambda):
    C = x.shape[1]
    mu1, mu2 = F.conv2d(x, window, padding=5, groups=C), F.conv2d(y, window, padding=5, groups=C)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1 = F.conv2d(x * x, window, padding=5, groups=C) - mu1_sq
    s2 = F.conv2d(y * y, window, padding=5, groups=C) - mu2_sq
    s12 = F.conv2d(x * y, window, padding=5, groups=C) - mu1_mu2
    ssim = (((2 * mu1_mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1_sq + mu2_sq + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))).mean()
    return F.mse_loss(x, y) * l2_lambda + (1 - ssim) * ssim_lambda + l1_lambda * F.l1_loss(x, y)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "photo_loss_bench.txt"))
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(0)
    lines = [f"# tools/bench_photo_loss.py --reps {a.reps}   device: {torch.cuda.get_device_name(0)}",
             "# photometric_loss (MSE + L1 + 0.2 (1 - SSIM)); times in ms: median [min .. max] of alternating runs, host launch overhead",
             "# included on both sides; speed-up = torch median / HIP median",
             f"{'shape':<18} {'pass':<20} {'HIP':>9} {'':<21} {'torch':>9} {'':<21} {'speed-up':>9}"]
    for shape in SHAPES:
        x = (torch.rand(shape, generator=gen) * 2 - 1).to(dev)
        y = (x.cpu() + 0.1 * torch.randn(shape, generator=gen)).clamp(-1, 1).to(dev)
        window = torch_window(shape[1], dev)
        xg = x.clone().requires_grad_(True)

        def hip_forward():
            with torch.no_grad():
                return losses.photometric_loss(x, y, **LAMBDAS)[0]

        def torch_forward():
            with torch.no_grad():
                return torch_loss(x, y, window, **LAMBDAS)

        def hip_both():
            xg.grad = None
            losses.photometric_loss(xg, y, **LAMBDAS)[0].backward()

        def torch_both():
            xg.grad = None
            torch_loss(xg, y, window, **LAMBDAS).backward()

        hip_both()
        gh = xg.grad.clone()
        torch_both()
        err = float((gh - xg.grad).norm() / xg.grad.norm())
        dl = abs(float(hip_forward()) - float(torch_forward()))
        for name, fns in (("forward", [hip_forward, torch_forward]), ("forward + backward", [hip_both, torch_both])):
            t = time_many(fns, a.reps)
            mh, mr = statistics.median(t[0]), statistics.median(t[1])
            lines.append(f"{'x'.join(map(str, shape)):<18} {name:<20} {cell(t[0])}  {cell(t[1])}  {mr / mh:8.1f}x"
                         f"   loss differs from torch's by {dl:.1e}, gradient by {err:.1e} (relative L2)")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
