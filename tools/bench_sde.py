#!/usr/bin/env python3
"""Times 250-step SDE sampling (Sampler.sample_sde, Euler-Maruyama, "sigma" form, last step "Mean") of the DiT-L denoisers against the
fixed-grid Euler ODE of the same process, and against two host loops.  Wall clock around whole samples (the host loops do host work),
device synchronised before and after; one untimed sample per variant first (it captures the step the timed samples replay); the
variants ALTERNATE inside every round, so drift of the box lands on every row alike; median and range (min .. max) of the rounds.

    python tools/bench_sde.py [--out profiles] [--rounds 5] [--steps 250]

  profiles/sde_bench.txt   per model (DiT-PixArt-PCD-CLAY-L at CFG batch 2 through forward_with_cfg; its stage-2 twin on one conditional
                           sequence through forward_cond), ms per step of
      ode   sample_euler_fused       the captured, replayed Euler step of sample_ode -- the yardstick
      sde   sample_sde_device        the captured, replayed Euler-Maruyama step, noise drawn in the kernel
      eager the eager loop           GA_ODE_GRAPH=0: one evaluation per step, noise restated on the host (numpy Philox) and copied up
      ref   a reference-shaped loop  two evaluations per step (drift and score call the model separately, transport.py:282-284),
                                     torch.randn on the host plus a copy per step (integrators.py:30)
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def build(arch, in_channels):
    from gaussiananything_amd.dit import DiT_models
    kw = dict(input_size=16, num_classes=0, learn_sigma=False, in_channels=in_channels, roll_out=True)
    with torch.device("cuda"):
        torch.manual_seed(0)
        m = DiT_models[arch](context_dim=1024, pooling_ctx_dim=768, **kw)
        with torch.no_grad():
            for p in m.parameters():     # the reference zero-initialises the adaLN layers and the final linear
                if float(p.abs().max()) == 0.0:
                    p.normal_(0.0, 0.02)
    return m


def reference_shaped(model, x, coef, model_kwargs):
    """the reference's loop as it stands: host noise + copy, the model evaluated once for the drift and once for the score"""
    from gaussiananything_amd.transport import sampler as S
    B, ni = x.size(0), coef.shape[0] - 1
    with torch.no_grad():
        for k in range(ni + 1):
            row = coef[k]
            tv = torch.ones(B, device=x.device) * row[S.C_T]
            v = model(x, tv, **model_kwargs).float()
            score = (row[S.C_R] * model(x, tv, **model_kwargs).float() - x) / row[S.C_VAR]
            mean = x + (v + row[S.C_W] * score) * row[S.C_DT]
            if k == ni:
                return mean
            w_cur = torch.randn(x.size()).to(x)
            x = mean + row[S.C_G] * (w_cur * row[S.C_SQRT_DT])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=250)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sde needs an MI355X: a timing taken anywhere else says nothing")
    from gaussiananything_amd import dit_ops as ops
    from gaussiananything_amd.transport import Sampler, create_transport
    from gaussiananything_amd.transport.sampler import sde_coefficients
    os.makedirs(args.out, exist_ok=True)
    n = args.steps
    lines = [f"# tools/bench_sde.py --rounds {args.rounds} --steps {n}; {torch.cuda.get_device_name(0)}; {ops.lib().ga_dit_version().decode()}",
             f"# ms per step = wall clock of one whole {n}-point sample / {n - 1} intervals (the SDE rows add their last step's evaluation: {n} evaluations",
             "# in all), device synchronised around it; one untimed sample per variant first; variants alternate inside every round;",
             "# median / min / max of the rounds.  One box, one run: only figures of this file stand beside each other."]
    g = torch.Generator(device="cuda").manual_seed(1)
    cases = [("DiT-PixArt-PCD-CLAY-L, CFG batch 2 x 768 x 3 (forward_with_cfg)", "DiT-PixArt-PCD-CLAY-L", 3, 2, "forward_with_cfg"),
             ("DiT-PixArt-PCD-CLAY-stage2-L, 1 x 768 x 10 (forward_cond)      ", "DiT-PixArt-PCD-CLAY-stage2-L", 10, 1, "forward_cond")]
    for label, arch, cin, B, entry in cases:
        m = build(arch, cin)
        x0 = torch.randn(B, 768, cin, device="cuda", generator=g)
        if entry == "forward_with_cfg":
            x0 = torch.cat([x0[:B // 2], x0[:B // 2]], 0)
        ctx = {"img_crossattn": torch.randn(B, 1369, 1024, device="cuda", generator=g), "img_vector": torch.randn(B, 1024, device="cuda", generator=g)}
        if entry == "forward_with_cfg":
            for v in ctx.values():
                v[B // 2:] = 0
        if cin == 10:
            ctx["fps-xyz"] = (torch.rand(B, 768, 3, device="cuda", generator=g) - 0.5) * 0.9
        fn = getattr(m, entry)
        smp = Sampler(create_transport("GVP", "velocity", None, None, None, snr_type="uniform"))
        kw = dict(context=ctx, cfg_scale=4.0)
        coef = sde_coefficients("GVP", "sigma", 1.0, torch.linspace(0, 1 - 0.04, n), 0.04).cuda()

        def eager():
            os.environ["GA_ODE_GRAPH"] = "0"
            try:
                return smp.sample_sde(num_steps=n, seed=1)(x0, fn, **kw)
            finally:
                del os.environ["GA_ODE_GRAPH"]

        variants = [("ode   sample_euler_fused      ", lambda: smp.sample_ode(sampling_method="euler", num_steps=n)(x0, fn, **kw)),
                    ("sde   sample_sde_device       ", lambda: smp.sample_sde(num_steps=n, seed=1)(x0, fn, **kw)),
                    ("eager one evaluation per step ", eager),
                    ("ref   reference-shaped loop   ", lambda: reference_shaped(fn, x0, coef, kw))]
        res = {name: [] for name, _ in variants}
        for name, run in variants:      # untimed: captures, workspace, caches
            out = run()
            assert bool(torch.isfinite(out).all()), name
        for _ in range(args.rounds):
            for name, run in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run()
                torch.cuda.synchronize()
                res[name].append((time.perf_counter() - t0) * 1000 / (n - 1))
        lines.append(label)
        for name, ms in res.items():
            lines.append(f"    {name}  median {statistics.median(ms):8.4f} ms/step   min {min(ms):8.4f}   max {max(ms):8.4f}   (n = {len(ms)})")
        med = {name[:5].strip(): statistics.median(ms) for name, ms in res.items()}
        ode = res[variants[0][0]]
        lines.append(f"    (a) sde / ode = {med['sde'] / med['ode']:.4f}; per evaluation ({n} against {n - 1}): {med['sde'] * (n - 1) / n / med['ode']:.4f}; "
                     f"ode range {max(ode) - min(ode):.4f} ms/step")
        lines.append(f"    (b) eager / sde = {med['eager'] / med['sde']:.3f}   (c) reference-shaped / sde = {med['ref'] / med['sde']:.3f}")
        del m
        torch.cuda.empty_cache()
    open(os.path.join(args.out, "sde_bench.txt"), "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
