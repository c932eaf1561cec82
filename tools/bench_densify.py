"""Measures what adaptive density control costs (gaussiananything_amd.fitting, include/ga_densify.h) and writes
profiles/densify_bench.txt and profiles/densify_fit.txt.

    python tools/bench_densify.py [--rounds 9] [--iters 20] [--out profiles/densify_bench.txt] [--fit-out profiles/densify_fit.txt]

Same process, alternating rounds, medians with ranges, host clock between two device synchronisations (as tools/bench_fit.py):

  1  ``SurfelFitter.step(iters)`` without and with ``ga_fit_accumulate`` in the captured chain.  The fitter without ``densify=`` enqueues
     exactly what it did before density control existed, so its figure is the baseline re-measured in this run.
  2  one ``densify_and_prune`` (about a tenth cloned, a tenth split, a tenth pruned) against the same round composed in torch on the same
     device -- boolean masks, ``cat``, indexing: what a user of the fitter had to write before.  (The torch round leaves the rows in
     another order and draws other normals; the work is the same.)
  3  the wall time of a whole round inside the fitter: the kernel round, every N-sized buffer anew, a fresh plan and workspace, the
     warm-up iteration and the new capture.
  4  (``--fit-out``) a sparse start: targets rendered from 400 surfels, the fit started from 100 of them, with and without density
     control -- the loss curves.  A result, not a condition."""
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

SHAPES = [(100_000, 8, 512), (20_000, 4, 256)]
LAMBDAS = dict(l2=0.0, l1=0.8, ssim=0.2, lambda_normal=0.05, lambda_dist=0.0, lambda_alpha=0.0)
NEVER = dict(extent=1.0, start=10 ** 9, stop=10 ** 9, opacity_reset_every=0)      # the statistic is gathered, no round ever runs
PARAMS = dict(grad_threshold=2e-4, min_opacity=0.05, percent_dense=0.01, extent=2.0)


def cell(times):
    return f"{statistics.median(times):9.3f} [{min(times):8.3f} ..{max(times):8.3f}]"


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def scene(n, v, size, dev):
    cams = synthetic.eval_cameras(8)
    cv, cvp, cp = (cams[k][:v].to(dev) for k in ("cam_view", "cam_view_proj", "cam_pos"))
    g = synthetic.surface_surfels(n, seed=1)
    with torch.no_grad():
        targets = GaussianRenderer2DGS(size, 3, {}).render(g.to(dev), cv[None], cvp[None], cp[None], cams["tanfov"])["image"][0].contiguous()
    gen = torch.Generator().manual_seed(2)
    start = g.clone()
    start[..., 0:3] += 0.002 * torch.randn(n, 3, generator=gen)
    start[..., 10:13] = (start[..., 10:13] + 0.1 * torch.randn(n, 3, generator=gen)).clamp(0.02, 0.98)
    return start.to(dev), cv, cvp, cp, cams["tanfov"], targets


def bench_step(a, dev, lines):
    lines += ["# 1. one fitting iteration, ms: median [min .. max] over alternating rounds; 'without' is the chain as it was before density",
              "#    control existed (densify=None), re-measured here; overhead = with - without (medians), in % of the iteration",
              f"{'surfels x views x size':<24} {'without accumulate':>9} {'':<13} {'with ga_fit_accumulate':>9} {'':<8} {'overhead':>9}"]
    rounds = []
    for n, v, size in SHAPES:
        start, cv, cvp, cp, tanfov, targets = scene(n, v, size, dev)
        kw = dict(max_steps=(a.rounds + 2) * a.iters, check_every=a.iters, **LAMBDAS)
        fits = [fitting.SurfelFitter(start, cv, cvp, tanfov, targets, **kw),
                fitting.SurfelFitter(start, cv, cvp, tanfov, targets, densify=NEVER, **kw)]
        times = [[], []]
        for f in fits:
            f.step(a.iters)
        for _ in range(a.rounds):
            for f, acc in zip(fits, times):
                acc.append(timed(lambda: f.step(a.iters))[0] / a.iters)
        m0, m1 = statistics.median(times[0]), statistics.median(times[1])
        spread = max(max(t) - min(t) for t in times)
        lines.append(f"{f'{n} x {v} x {size}^2':<24} {cell(times[0])}  {cell(times[1])}  {(m1 - m0) * 1e3:+7.1f} us = {100 * (m1 - m0) / m0:+.2f} %"
                     f"   (run-to-run range {spread * 1e3:.1f} us; the kernel moves N (28 + 4 V) = {n * (28 + 4 * v) / 1e6:.1f} MB)")
        print(lines[-1], flush=True)
        if (n, v, size) == SHAPES[0]:
            rounds = bench_fitter_round(fits[1], (start, cv, cvp, tanfov, targets), kw)
        del fits
        torch.cuda.empty_cache()
    return rounds


def bench_fitter_round(probe, views, kw):
    """3: thresholds read off the statistics the probe fitter gathered (a tenth of each kind), a fitter with that config continued from
    the probe's state, ``densify_now()`` timed; the state is loaded again (which resizes back) between the repeats"""
    s = probe.densify_stats()
    g = probe.gaussians()[0]
    avg = s["grad_accum"] / s["denom"].clamp_min(1).float()
    cfg = dict(NEVER, grad_threshold=float(avg.quantile(0.8)), percent_dense=float(g[:, 4:6].max(dim=1).values.median()),
               min_opacity=float(g[:, 3].quantile(0.1)), max_screen_size=0)
    state = probe.state_dict()
    f = fitting.SurfelFitter(*views, densify=cfg, **kw)
    out = []
    for _ in range(3):
        f.load_state_dict(state)
        ms, entry = timed(f.densify_now)
        step_ms = timed(lambda: f.step(1))[0]
        out.append((ms, entry, step_ms))
    return out


def pattern(n, dev, seed):
    """raw / m / v and statistics under which PARAMS clone, split and prune about a tenth each"""
    gen = torch.Generator().manual_seed(seed)
    code = torch.multinomial(torch.tensor([0.7, 0.1, 0.1, 0.1]), n, replacement=True, generator=gen)      # kept, clone, split, pruned
    raw = torch.randn(n, 13, generator=gen)
    raw[:, 3] = torch.where(code == 3, -4.6, 0.0)
    raw[:, 4:6] = torch.where(code == 2, -2.3, -4.6)[:, None] + 0.1 * torch.rand(n, 2, generator=gen)
    den = torch.randint(1, 5, (n,), generator=gen, dtype=torch.int32)
    acc = torch.where((code == 1) | (code == 2), 1e-3, 1e-5) * den.float()
    return [t.to(dev) for t in (raw, torch.randn(n, 13, generator=gen), torch.rand(n, 13, generator=gen), acc, den,
                                torch.zeros(n, dtype=torch.int32))]


def torch_round(raw, m, v, acc, den, rad, grad_threshold, min_opacity, percent_dense, extent):
    """the round a user composes in torch (after 2DGS's densify_and_clone / densify_and_split / prune): masks, cat, indexing"""
    opa, scales = torch.sigmoid(raw[:, 3]), torch.exp(raw[:, 4:6])
    avg = torch.nan_to_num(torch.where(den > 0, acc / den.float(), torch.zeros_like(acc)), nan=0.0)
    smax = scales.max(dim=1).values
    prune = opa < min_opacity
    selected = ~prune & (avg >= grad_threshold)
    clone = selected & (smax <= percent_dense * extent)
    split = selected & ~clone
    stay = ~prune & ~split
    q = torch.nn.functional.normalize(raw[split, 6:10], dim=1)
    w, x, y, z = q.unbind(1)
    tu = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z - w * y)], 1)
    tv = torch.stack([2 * (x * y - w * z), 1 - 2 * (x * x + z * z), 2 * (y * z + w * x)], 1)
    kids = []
    for _ in range(2):
        xi = torch.randn(q.shape[0], 2, device=raw.device)
        kid = raw[split].clone()
        kid[:, 0:3] += tu * (scales[split, 0:1] * xi[:, 0:1]) + tv * (scales[split, 1:2] * xi[:, 1:2])
        kid[:, 4:6] -= 0.4700036292457356
        kids.append(kid)
    fresh = int(clone.sum()) + 2 * q.shape[0]
    zeros = torch.zeros(fresh, 13, device=raw.device)
    return (torch.cat([raw[stay], raw[clone]] + kids), torch.cat([m[stay], zeros]), torch.cat([v[stay], zeros]))


def bench_round(a, dev, lines):
    lines += ["", "# 2. one clone / split / prune round, ms: median [min .. max]; densify_and_prune (ga_fit_activate + ga_densify, its",
              "#    allocations and the one read of the counts) against the same round composed in torch on the same device",
              f"{'surfels':<12} {'densify_and_prune':>9} {'':<13} {'torch masks + cat':>9} {'':<14} {'torch / kernel':>9}"]
    for n in (100_000, 1_000_000):
        t = pattern(n, dev, 3)
        sides = [lambda: fitting.densify_and_prune(*t, seed=1, round=0, **PARAMS), lambda: torch_round(*t, **PARAMS)]
        times = [[], []]
        for side in sides:
            side()
        for _ in range(a.rounds):
            for side, acc in zip(sides, times):
                acc.append(timed(side)[0])
        counts = sides[0]()[4]
        rows = sides[1]()[0].shape[0]
        m0, m1 = statistics.median(times[0]), statistics.median(times[1])
        lines.append(f"{n:<12} {cell(times[0])}  {cell(times[1])}  {m1 / m0:8.2f}x   N' {counts['N_after']} (torch {rows}): cloned "
                     f"{counts['cloned']}, split {counts['split']}, pruned {counts['pruned']}")
        print(lines[-1], flush=True)
        del t
        torch.cuda.empty_cache()


def sparse_fit(dev, out):
    """4: the loss with and without density control on a sparse start"""
    steps, size, v = 400, 128, 4
    cams = synthetic.eval_cameras(8)
    cv, cvp, cp = (cams[k][:v].to(dev) for k in ("cam_view", "cam_view_proj", "cam_pos"))
    g = synthetic.random_surfels(400, seed=3)
    g[..., 4:6] *= 8.0
    with torch.no_grad():
        targets = GaussianRenderer2DGS(size, 3, {}).render(g.to(dev), cv[None], cvp[None], cp[None], cams["tanfov"])["image"][0].contiguous()
    start = g[:, ::4].contiguous().to(dev)
    extent = float((g[0, :, 0:3] - g[0, :, 0:3].mean(0)).norm(dim=1).max())
    kw = dict(max_steps=steps, **LAMBDAS)
    base = dict(extent=extent, start=50, every=50, stop=300, opacity_reset_every=0, max_points=4000)
    probe = fitting.SurfelFitter(start, cv, cvp, cams["tanfov"], targets, densify=dict(base, start=10 ** 6, stop=10 ** 6), **kw)
    probe.step(50)
    s = probe.densify_stats()
    avg = (s["grad_accum"] / s["denom"].clamp_min(1).float())[s["denom"] > 0]
    median = float(avg.median())
    runs = [("no density control", None), ("grad_threshold 2e-4 (the default)", dict(base)),
            (f"grad_threshold {median:.3e} (the median of the statistic after 50 iterations)", dict(base, grad_threshold=median))]
    lines = [f"# tools/bench_densify.py: targets rendered from 400 surfels ({v} views, {size}^2), the fit started from every fourth of them;",
             f"# {steps} iterations, rounds every 50 from 50 to 300, no opacity reset, extent {extent:.3f}; the statistic after 50 iterations:",
             f"# min {float(avg.min()):.3e}, median {median:.3e}, max {float(avg.max()):.3e}", "# loss at iteration:  " +
             "  ".join(f"{t:>9}" for t in range(0, steps, 50)) + f"  {steps - 1:>9}"]
    for name, cfg in runs:
        f = fitting.SurfelFitter(start, cv, cvp, cams["tanfov"], targets, densify=cfg, **kw)
        f.step(steps)
        h = f.loss_history()["loss"]
        lines.append(f"{name}\n    loss             " + "  ".join(f"{float(h[t]):9.5f}" for t in list(range(0, steps, 50)) + [steps - 1]))
        lines.append(f"    surfels {f.num_points}; rounds (step, N before, N after, cloned, split, pruned): {f.densify_log}")
        print("\n".join(lines[-2:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "densify_bench.txt"))
    ap.add_argument("--fit-out", default=os.path.join(ROOT, "profiles", "densify_fit.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_densify.py needs the GPU: a timing on anything else says nothing")
    dev = torch.device("cuda:0")
    lines = [f"# tools/bench_densify.py --rounds {a.rounds} --iters {a.iters}   device: {torch.cuda.get_device_name(0)}"]
    rounds = bench_step(a, dev, lines)
    bench_round(a, dev, lines)
    n, v, size = SHAPES[0]
    lines += ["", f"# 3. a whole round inside the fitter at {n} x {v} x {size}^2, wall ms (densify_now(): the kernel round, the buffers sized by N anew,",
              "#    a fresh plan and workspace, the warm-up iteration, the new capture), and the first step(1) after it"]
    for ms, entry, step_ms in rounds:
        lines.append(f"densify_now {ms:9.3f} ms   (step, N before, N after, cloned, split, pruned) = {entry}   next step(1) {step_ms:.3f} ms")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)
    sparse_fit(dev, a.fit_out)


if __name__ == "__main__":
    main()
