"""Times one iteration of gaussiananything_amd.fitting.SurfelFitter with view mini-batches selected on the device against the two ways
there were before, on the same device in the same process, and writes profiles/fit_minibatch_bench.txt.

    python tools/bench_fit_minibatch.py [--rounds 9] [--iters 20] [--out profiles/fit_minibatch_bench.txt]

    mini-batch     SurfelFitter(batch_views=B) over a pool of P views on the device: step(iters), iters graph replays
    set_views      a V = B fitter, ``set_views(pool[S[t]])`` and ``step(1)`` per iteration on the same schedule S: per iteration five
                   device-to-device copies enqueued by the host, one read of the overflow words and one snapshot
    full batch     a V = B fitter on B fixed views, step(iters): the same chain without the select launch
    identity       SurfelFitter(batch_views=B) over a pool of those same B views with the identity schedule: what the full-batch
                   fitter renders, plus the select launch -- the mini-batch side renders other views than the full-batch side, so
                   the cost of the select launch alone is identity - full batch

A round is ``iters`` iterations between two device synchronisations, timed with the host clock; rounds of the four sides alternate; the
table gives the median and the range of the per-iteration time over the rounds.  The pool repeats the eight evaluation cameras (the
bytes moved per iteration do not depend on what the views show)."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gaussiananything_amd import fitting, synthetic  # noqa: E402
from gaussiananything_amd.gs_surfel import GaussianRenderer2DGS  # noqa: E402

SHAPES = [(100_000, 64, 8, 512), (20_000, 16, 4, 256)]           # surfels, pool views, batch views, size
LAMBDAS = dict(l2=0.0, l1=0.8, ssim=0.2, lambda_normal=0.05, lambda_dist=0.0, lambda_alpha=0.0)


def cell(times):
    return f"{statistics.median(times):9.3f} [{min(times):8.3f} ..{max(times):8.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_minibatch_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_fit_minibatch.py needs the GPU: a timing on anything else says nothing")
    dev = torch.device("cuda:0")
    max_steps = (a.rounds + 2) * a.iters
    lines = [f"# tools/bench_fit_minibatch.py --rounds {a.rounds} --iters {a.iters}   device: {torch.cuda.get_device_name(0)}",
             "# one fitting iteration (0.8 L1 + 0.2 (1 - SSIM) + 0.05 normal), ms per iteration: median [min .. max] over alternating rounds",
             f"# of {a.iters} iterations between two device synchronisations, host clock.  select = identity median - full batch median",
             f"{'surfels x pool x B x size':<26} {'mini-batch (device select)':<31} {'set_views + step(1) loop':<31} {'full batch, V = B':<31} {'identity schedule over them':<31}"
             f" {'loop / mini-batch':>17} {'select':>10}"]
    for n, pool, batch, size in SHAPES:
        cams = synthetic.eval_cameras(8)
        cv8, cvp8, cp8 = (cams[k].to(dev) for k in ("cam_view", "cam_view_proj", "cam_pos"))
        g = synthetic.surface_surfels(n, seed=1)
        with torch.no_grad():
            t8 = GaussianRenderer2DGS(size, 3, {}).render(g.to(dev), cv8[None], cvp8[None], cp8[None], cams["tanfov"])["image"][0]
        reps = pool // 8
        cv, cvp, targets = cv8.repeat(reps, 1, 1), cvp8.repeat(reps, 1, 1), t8.repeat(reps, 1, 1, 1).contiguous()
        gen = torch.Generator().manual_seed(2)
        start = g.clone()
        start[..., 0:3] += 0.002 * torch.randn(n, 3, generator=gen)
        start[..., 10:13] = (start[..., 10:13] + 0.1 * torch.randn(n, 3, generator=gen)).clamp(0.02, 0.98)
        start = start.to(dev)
        S = fitting.view_schedule(max_steps, pool, batch, seed=0)
        kw = dict(max_steps=max_steps, check_every=a.iters, **LAMBDAS)
        mini = fitting.SurfelFitter(start, cv, cvp, cams["tanfov"], targets, batch_views=batch, view_schedule=S, **kw)
        first = S[0].long().to(dev)
        loop = fitting.SurfelFitter(start, cv[first], cvp[first], cams["tanfov"], targets[first], **kw)
        full = fitting.SurfelFitter(start, cv[:batch], cvp[:batch], cams["tanfov"], targets[:batch], **kw)
        ident = torch.arange(batch, dtype=torch.int32).repeat(max_steps, 1)
        same = fitting.SurfelFitter(start, cv[:batch], cvp[:batch], cams["tanfov"], targets[:batch], batch_views=batch, view_schedule=ident,
                                    **kw)
        rows = [S[t].long().to(dev) for t in range(max_steps)]       # the indices are on the device before the clock starts

        def loop_step(k):
            for _ in range(k):
                idx = rows[loop.steps]
                loop.set_views(cv[idx], cvp[idx], targets[idx])
                loop.step(1)

        sides = [mini.step, loop_step, full.step, same.step]
        times = [[], [], [], []]
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
        med = [statistics.median(t) for t in times]
        hm, hl = mini.loss_history()["loss"], loop.loss_history()["loss"]
        lines.append(f"{f'{n} x {pool} x {batch} x {size}^2':<26} {cell(times[0])}  {cell(times[1])}  {cell(times[2])}  {cell(times[3])}  {med[1] / med[0]:16.2f}x"
                     f" {med[3] - med[2]:+9.3f}   loss {float(hm[0]):.5f} -> mini-batch {float(hm[-1]):.5f}, loop {float(hl[-1]):.5f} after"
                     f" {mini.steps} iterations; workspace capacity {mini.capacity} / {loop.capacity} / {full.capacity}")
        print(lines[-1], flush=True)
        del mini, loop, full, same
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
