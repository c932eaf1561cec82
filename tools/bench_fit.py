"""Times one iteration of gaussiananything_amd.fitting.SurfelFitter against the loop a user writes without it, on the same device in the
same process, and writes profiles/fit_bench.txt.

    python tools/bench_fit.py [--rounds 9] [--iters 20] [--out profiles/fit_bench.txt]

The other side is: activation in torch, ``GaussianRenderer2DGS.render`` with grad, ``photometric_loss``, ``geometric_loss``,
``.backward()`` and ``torch.optim.Adam`` over the raw parameters (one leaf per column group, which is how Adam gets per-group learning
rates; the five leaves are concatenated into the one raw tensor).  Same lambdas, same scene, same start on both sides.  A round is
``iters`` iterations between two device synchronisations, timed with the host clock (the host's share is what is being compared);
rounds of the two sides alternate; the table gives the median and the range of the per-iteration time over the rounds.  The fitter's
round is one ``step(iters)``: ``iters`` graph replays, one read of the overflow words, one snapshot."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gaussiananything_amd import fitting, losses, synthetic  # noqa: E402
from gaussiananything_amd.gs_surfel import GaussianRenderer2DGS  # noqa: E402

SHAPES = [(100_000, 8, 512), (20_000, 4, 256)]
LAMBDAS = dict(l2=0.0, l1=0.8, ssim=0.2, lambda_normal=0.05, lambda_dist=0.0, lambda_alpha=0.0)
SLICES = {"xyz": slice(0, 3), "opacity": slice(3, 4), "scale": slice(4, 6), "rotation": slice(6, 10), "rgb": slice(10, 13)}


def activate(raw):
    q = raw[:, 6:10]
    return torch.cat([raw[:, 0:3], torch.sigmoid(raw[:, 3:4]), torch.exp(raw[:, 4:6]), q / q.pow(2).sum(1, keepdim=True).sqrt(),
                      torch.sigmoid(raw[:, 10:13])], dim=1)


class AutogradLoop:
    def __init__(self, raw0, cv, cvp, cp, tanfov, targets, size, max_steps):
        self.leaves = {k: raw0[:, s].clone().requires_grad_(True) for k, s in SLICES.items()}
        self.opt = torch.optim.Adam([{"params": [self.leaves[k]], "lr": 1.0} for k in SLICES], betas=(0.9, 0.999), eps=1e-15)
        self.renderer = GaussianRenderer2DGS(size, 3, {})
        self.cv, self.cvp, self.cp, self.tanfov, self.targets = cv[None], cvp[None], cp[None], tanfov, targets
        self.t, self.max_steps, self.loss = 0, max_steps, None

    def step(self, n):
        for _ in range(n):
            for group, k in zip(self.opt.param_groups, SLICES):
                group["lr"] = fitting._lr_at(fitting.DEFAULT_LR[k], self.t, self.max_steps)
            self.opt.zero_grad(set_to_none=True)
            pred = self.renderer.render(activate(torch.cat([self.leaves[k] for k in SLICES], dim=1))[None], self.cv, self.cvp, self.cp,
                                        self.tanfov)
            lp, _ = losses.photometric_loss(pred["image"][0], self.targets, LAMBDAS["l2"], LAMBDAS["l1"], LAMBDAS["ssim"])
            lg, _ = losses.geometric_loss(pred, self.cv, self.tanfov, LAMBDAS["lambda_normal"], LAMBDAS["lambda_dist"],
                                          LAMBDAS["lambda_alpha"])
            self.loss = lp + lg
            self.loss.backward()
            self.opt.step()
            self.t += 1


def cell(times):
    return f"{statistics.median(times):9.3f} [{min(times):8.3f} ..{max(times):8.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_fit.py needs the GPU: a timing on anything else says nothing")
    dev = torch.device("cuda:0")
    max_steps = (a.rounds + 2) * a.iters
    lines = [f"# tools/bench_fit.py --rounds {a.rounds} --iters {a.iters}   device: {torch.cuda.get_device_name(0)}",
             "# one fitting iteration (0.8 L1 + 0.2 (1 - SSIM) + 0.05 normal), ms per iteration: median [min .. max] over alternating rounds",
             f"# of {a.iters} iterations between two device synchronisations, host clock; speed-up = autograd loop median / fitter median",
             f"{'surfels x views x size':<24} {'SurfelFitter.step':>9} {'':<13} {'autograd loop + torch Adam':>9} {'':<4} {'speed-up':>9}"]
    for n, v, size in SHAPES:
        cams = synthetic.eval_cameras(8)
        cv, cvp, cp = (cams[k][:v].to(dev) for k in ("cam_view", "cam_view_proj", "cam_pos"))
        g = synthetic.surface_surfels(n, seed=1)
        with torch.no_grad():
            targets = GaussianRenderer2DGS(size, 3, {}).render(g.to(dev), cv[None], cvp[None], cp[None], cams["tanfov"])["image"][0].contiguous()
        gen = torch.Generator().manual_seed(2)
        start = g.clone()
        start[..., 0:3] += 0.002 * torch.randn(n, 3, generator=gen)
        start[..., 10:13] = (start[..., 10:13] + 0.1 * torch.randn(n, 3, generator=gen)).clamp(0.02, 0.98)
        fit = fitting.SurfelFitter(start.to(dev), cv, cvp, cams["tanfov"], targets, max_steps=max_steps, check_every=a.iters, **LAMBDAS)
        loop = AutogradLoop(fit.raw.clone(), cv, cvp, cp, cams["tanfov"], targets, size, max_steps)
        sides = [fit.step, loop.step]
        times = [[], []]
        for side in sides:                                   # warm-up of each side: one round
            side(a.iters)
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for side, acc in zip(sides, times):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                side(a.iters)
                torch.cuda.synchronize()
                acc.append((time.perf_counter() - t0) * 1e3 / a.iters)
        h = fit.loss_history()["loss"]
        mf, ml = statistics.median(times[0]), statistics.median(times[1])
        lines.append(f"{f'{n} x {v} x {size}^2':<24} {cell(times[0])}  {cell(times[1])}  {ml / mf:8.2f}x"
                     f"   loss {float(h[0]):.5f} -> fitter {float(h[-1]):.5f}, autograd loop {float(loop.loss.detach()):.5f}"
                     f" after {fit.steps} iterations; workspace capacity {fit.capacity}")
        print(lines[-1], flush=True)
        del fit, loop
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
