#!/usr/bin/env python3
"""bench.py -- headline benchmark of the render half of the hot path (BASELINE.json metric "Msplats/s rasterize").

One STEP = one full forward of the MI355X surfel rasterizer (preprocess, tile binning, per-tile depth sort, blend)
over BASELINE.json configs[1]: 100 000 surface-like surfels x 8 posed 512x512 views, inputs resident in HBM.
    value = N_splats * V * steps * n_gpus / wall / 1e6          [Msplats/s]
Multi-GPU (N>1, launched by torch.distributed.run): every rank renders its own independent sample (weak scaling, no
data-path collective in the timed steps); the rendered RGB-D-N images are collected on rank 0 with ONE RCCL gather
("final image collection"), executed once after the timed steps and timed on its own, and once
inside the timed cascaded sample of every rank.

The timed region holds the K forwards only.  A plain run does nothing else: it sets up, warms up, times the K forwards, writes
the outputs of the last one (--dump-outputs DIR) and prints the JSON line (metric, value, unit, higher_is_better, dtype,
ms_per_step, the configuration).  Everything below runs afterwards, untimed, with --full only (the --no-* switches leave parts
of it out): stage events and the roofline, the stress scene and two streams, the parity check, the CPU baseline, the denoiser /
conditioner / decode sections, the backward and mesh export, the cascade, and for N > 1 the timed gather.

--dump-outputs DIR: what the timed forward hands its caller after the last timed step -- DIR/color.npy [V,3,H,W],
DIR/radii.npy [V,N] (as float32) and DIR/allmap.npy [V,7,H,W] -- in float32, at most 64 MB in all: an array that does not fit
its share is written as DIR/<name>_sample.npy, the elements at a fixed seeded sample of flat indices (sorted).  The inputs are
seeded, so two builds run with the same arguments can be compared output for output.

Also on the JSON line of a --full run:
  parity       -- the bench workload itself, HIP path vs oracle, every view (bit-identical bins, pixel MSE <= 1e-5).
  sec_per_sample / cascade -- BASELINE configs[3]/[4]: one 250-step cascaded sample per GPU (stage-1 DiT-L, stage-2 DiT-L,
                  surfel decode, renders), all ranks, one gather to rank 0; euler (249 NFE per stage) and, at N=1, dopri5.
  roofline     -- the dominant kernel (surfel_blend_kernel): algorithmic bytes (76*D + 40*P per view) over its
                  mean duration measured with HIP events on the launch stream during the timed steps; HBM peak 8 TB/s.
  cpu_baseline -- the CPU oracle (oracle/surfel_raster.c, kind "port": the reference has no CPU rasterizer) timed on
                  this host's cores on a bounded sample of the same workload.  Rank 0, N=1 only.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

os.environ.setdefault("OMP_WAIT_POLICY", "passive")   # the CPU baselines' idle OpenMP workers sleep instead of spinning beside the launch threads

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0          # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8 TB/s spec
FP32_VALU_PEAK_TFLOPS = 157.3  # same guide: peak FP32 vector


class HipEvents:
    """hipEvent_t handles through ctypes (torch.cuda.Event only sees torch's own record calls)."""

    def __init__(self, n):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.hip.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_void_p, ctypes.c_void_p]
        self.arr = (ctypes.c_void_p * n)()
        for i in range(n):
            ev = ctypes.c_void_p()
            assert self.hip.hipEventCreate(ctypes.byref(ev)) == 0
            self.arr[i] = ev

    def elapsed(self, i, j):
        ms = ctypes.c_float()
        self.hip.hipEventSynchronize(ctypes.c_void_p(self.arr[j]))
        rc = self.hip.hipEventElapsedTime(ctypes.byref(ms), ctypes.c_void_p(self.arr[i]), ctypes.c_void_p(self.arr[j]))
        assert rc == 0, rc
        return ms.value


def committed_pmc(name):
    """profiles/<round>_<name> (tools/pmc_to_json.py), newest round first, if the kernel source it was measured on is still the source in
    the tree, else None: counters cannot be collected inside this run, and a quotation of a stale pass would drift from the code silently."""
    import hashlib
    for rnd in ("r6", "r5"):
        path = os.path.join(ROOT, "profiles", f"{rnd}_{name}")
        if not os.path.exists(path):
            continue
        pj = json.load(open(path))
        ok = True
        for rel, want in pj.get("source_sha256", {}).items():
            src = os.path.join(ROOT, rel)
            if not os.path.exists(src) or hashlib.sha256(open(src, "rb").read()).hexdigest() != want:
                ok = False
        if ok:
            return pj
    return None


def host_threads():
    """ONE convention for every `cores` on the line: min(64, hardware threads this process may run on), and every CPU baseline runs with
    exactly that many worker threads (OpenMP for the rasterizer oracle, intra-op threads for the PyTorch DiT oracle).  More only add
    contention on the driver's 256-thread host: measured with all 256, the DiT oracle took 117 s per evaluation (64: ~6 s) and the
    rasterizer oracle 0.45 Msplats/s (less than with 64) -- and the spinning OpenMP pool slowed the launch-bound GPU sections after it."""
    return min(64, len(os.sched_getaffinity(0)))


def stress_scene_line(cams, n, H, W, dev, steps=20):
    """SURVEY.md 8d's second scene (uniform random surfels: radius median 8 px, D/N = 4.8) beside the headline one: the same forward,
    untimed section -- wall time of `steps` back-to-back forwards and the stage times from HIP events."""
    from gaussiananything_amd import synthetic
    from gaussiananything_amd.diff_surfel_rasterization import SurfelForwardPlan
    g = synthetic.random_surfels(n, seed=0)[0]
    m, o, s, r, c = [t.to(dev) for t in synthetic.split_gaussians(g)]
    plan = SurfelForwardPlan(m, o, c, s, r, cams["cam_view"].to(dev), cams["cam_view_proj"].to(dev), torch.ones(3, device=dev), H, W)
    plan.run()
    plan.ensure_capacity()
    for _ in range(5):
        plan.run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        plan.run()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    ev = [HipEvents(5) for _ in range(10)]
    for e in ev:
        plan.set_stage_events(e.arr)
        plan.run()
    torch.cuda.synchronize()
    plan.set_stage_events(None)
    names = ["preprocess", "tile_scan_fill", "tile_sort", "blend"]
    st = plan.ws.status().cpu()
    V = cams["cam_view"].shape[0]
    return {"scene": "stress (uniform random surfels, SURVEY.md 8d)", "ms_per_step": round(ms, 4), "Msplats_per_s": round(n * V / ms / 1e3, 1),
            "num_rendered_D": int(st[0]), "longest_tile_list": int(st[2]),
            "stage_ms": {nm: round(float(np.mean([e.elapsed(i, i + 1) for e in ev])), 5) for i, nm in enumerate(names)}}


def cpu_baseline(g, cams, H, W, min_seconds=3.0):
    """CPU oracle on the host cores: whole views of the SAME scene until >= min_seconds of wall time."""
    from gaussiananything_amd import synthetic
    from oracle import surfel as osurf
    m, o, s, r, c = [t.numpy() for t in synthetic.split_gaussians(g)]
    cores = osurf.lib().oracle_set_threads(host_threads())
    osurf.rasterize(m[:1000], o[:1000], c[:1000], s[:1000], r[:1000], cams["cam_view"][0].numpy(),
                    cams["cam_view_proj"][0].numpy(), np.ones(3, np.float32), 64, 64)  # warm the library
    t0 = time.perf_counter()
    views = 0
    while True:
        v = views % cams["cam_view"].shape[0]
        osurf.rasterize(m, o, c, s, r, cams["cam_view"][v].numpy(), cams["cam_view_proj"][v].numpy(),
                        np.ones(3, np.float32), H, W)
        views += 1
        dt = time.perf_counter() - t0
        if dt >= min_seconds and views >= 2:
            break
    return {"value": round(m.shape[0] * views / dt / 1e6, 4), "unit": "Msplats/s", "cores": int(cores),
            "kind": "port",
            "sample": f"{views} whole 512x512 views of the same 100k-surfel scene, {dt:.1f} s wall; preprocess+binning "
                      f"single-threaded, blend OpenMP over tiles ({cores} threads = min(64, hardware threads), the convention "
                      f"of all CPU baselines on this line); includes numpy buffer setup"}


def dit_flops_per_nfe(D, depth, L, M, ctx, batch, ca_batch=None):
    """FLOPs of one function evaluation with the image-token K/V cached: per block and sequence
    SA: 2L*D*3D + 4L^2*D + 2L*D^2 ; CA: 2L*D^2 (q) + 4L*M*D + 2L*D^2 (out) ; MLP: 16L*D^2.  Returns (algorithmic: every batch
    item through its cross-attention, EXECUTED: only `ca_batch` items do -- the zero-context unconditional half of a CFG
    batch skips it, include/ga_dit.h -- and the attention-only share of the executed count)."""
    ca_batch = batch if ca_batch is None else ca_batch
    sa = 2 * L * D * 3 * D + 4 * L * L * D + 2 * L * D * D
    ca = 2 * L * D * D + 4 * L * M * D + 2 * L * D * D
    mlp = 16 * L * D * D
    return (batch * depth * (sa + ca + mlp), depth * (batch * (sa + mlp) + ca_batch * ca),
            depth * (batch * 4 * L * L * D + ca_batch * 4 * L * M * D))


def bench_attention(dev, reps=50):
    """north_star: 'MFMA utilisation for DiT attention'.  The two attention shapes of a DiT-L evaluation timed alone with HIP
    events around back-to-back launches: self-attention (CFG batch 2 x 16 heads x 768 x 768) and the image cross-attention
    of the conditional half (1 x 16 x 768 x 1369), d = 64; FLOPs = 4 * Lq * Lk * d per (batch, head) (QK^T + PV)."""
    from gaussiananything_amd import dit_ops as ops
    g = torch.Generator().manual_seed(3)
    out = {}
    for name, B, Lq, Lk in (("self_attention_2x16x768x768", 2, 768, 768), ("cross_attention_1x16x768x1369", 1, 768, 1369)):
        H = 16
        Lp = (Lk + 63) // 64 * 64
        q = torch.randn(B, Lq, H, 64, generator=g).to(dev).bfloat16()
        k = torch.randn(B, Lk, H, 64, generator=g).to(dev).bfloat16()
        vt = torch.zeros(B * H * 64, Lp, dtype=torch.bfloat16, device=dev)
        vt[:, :Lk] = torch.randn(B * H * 64, Lk, generator=g).to(dev).bfloat16()
        for _ in range(5):
            ops.attention(q, k, vt)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            ops.attention(q, k, vt)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / reps * 1e3
        fl = 4.0 * B * H * Lq * Lk * 64
        out[name] = {"us": round(us, 2), "tflops": round(fl / (us * 1e-6) / 1e12, 1),
                     "frac_of_bf16_mfma_peak": round(fl / (us * 1e-6) / 1e12 / 2500.0, 4)}
    pj = committed_pmc("attention_pmc.json")
    out["mfma_busy_from_counters"] = ({"kernels": pj["kernels"], "source": pj["source"] + " (committed rocprofv3 PMC pass of exactly these two "
                                        "launches: SQ_VALU_MFMA_BUSY_CYCLES / 1024 SIMDs over GRBM_GUI_ACTIVE / 8 XCDs; dit_attention.hip unchanged "
                                        "since), not measured in this run"} if pj else None)
    out["note"] = "launches on torch's current stream, timed with events on that stream"
    return out


def bench_dit(dev, arch, nfe, warmup, parity_mode=False, samples=1, cond_only=False):
    """ms per function evaluation of forward_with_cfg at the release shapes: CFG batch 2 x samples, 768 latent tokens,
    1369 x 1024 image tokens, seeded random weights (zero-initialised tensors re-drawn).  samples = 4
    (several independent samples batched on one GPU) is reported as a throughput figure only: ms per evaluation; samples = 2 is the
    release's stage-1 shape (i23d-stage1.sh:17, num_samples=2 -> CFG batch 4).  cond_only: the conditional sequence alone through
    ``forward_cond`` -- batch 1, every GEMM at M = 768 -- which is how ``cascade.sample`` runs the release's stage 2 (uc == c)."""
    from gaussiananything_amd.dit import DiT_models
    from gaussiananything_amd.transport import Sampler, create_transport
    torch.manual_seed(0)
    stage2 = "stage2" in arch
    C = 10 if stage2 else 3
    model = DiT_models[arch](input_size=16, in_channels=C, context_dim=1024, pooling_ctx_dim=768, num_classes=0,
                             learn_sigma=False, roll_out=True)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p_ in model.parameters():
            if float(p_.abs().max()) == 0.0:
                p_.copy_(torch.randn(p_.shape, generator=g) * 0.02)
    model.to(dev)
    B, L, M = (samples if cond_only else 2 * samples), 768, 1369
    x = torch.randn(B, L, C, generator=g).to(dev)
    ctx = {"img_crossattn": torch.randn(B, M, 1024, generator=g), "img_vector": torch.randn(B, 1024, generator=g)}
    ctx["img_crossattn"][samples:] = 0     # [conditional | unconditional] halves, as FlowMatchingEngine.sample builds them
    ctx["img_vector"][samples:] = 0
    evaluate = model.forward_cond if cond_only else model.forward_with_cfg
    if stage2:
        ctx["fps-xyz"] = (torch.rand(B, L, 3, generator=g) - 0.5) * 0.9
    ctx = {k: v.to(dev) for k, v in ctx.items()}
    t = torch.full((B,), 0.5, device=dev)
    with torch.no_grad():
        for _ in range(warmup):
            evaluate(x, t, ctx, 4.0)
        torch.cuda.synchronize()
        tw = time.perf_counter()
        while time.perf_counter() - tw < 0.5:     # the GPU idled through the CPU legs before this: let the clocks come back
            for _ in range(10):
                evaluate(x, t, ctx, 4.0)
            torch.cuda.synchronize()
        reps = []
        for _ in range(3):      # median of three timed runs of `nfe` evaluations (one run is at the mercy of a clock dip)
            t0 = time.perf_counter()
            for _ in range(nfe):
                evaluate(x, t, ctx, 4.0)
            torch.cuda.synchronize()
            reps.append((time.perf_counter() - t0) / nfe * 1e3)
        ms = sorted(reps)[1]
        if samples > 2:
            return {"arch": arch, "samples_per_gpu": samples, "cfg_batch": B, "ms_per_nfe": round(ms, 4),
                    "ms_per_nfe_per_sample": round(ms / samples, 4)}
        if os.environ.get("GA_SKIP_SAMPLER") or samples > 1 or cond_only:
            fl, fl_exec, _ = dit_flops_per_nfe(model.embed_dim, model.depth, L, M, 1024, B, ca_batch=samples)
            tf = fl_exec / (ms * 1e-3) / 1e12
            return {"arch": arch, "batch": B, "cfg": not cond_only, "samples_per_gpu": samples, "tokens": L, "ctx_tokens": M,
                    "ms_per_nfe": round(ms, 4), "executed_tflop_per_nfe": round(fl_exec / 1e12, 4), "achieved_tflops": round(tf, 2),
                    "frac_of_mfma_peak": round(tf / 2500.0, 4), "ms_per_nfe_runs": [round(v, 4) for v in reps],
                    "shape_is": "the conditional sequence alone (forward_cond): how cascade.sample runs the release's stage 2 (uc == c)"
                                if cond_only else "the release's stage-1 shape (i23d-stage1.sh:17: num_samples=2 -> CFG batch 4)"}
        # the "250-step" sampler in its deterministic form: euler, 250 grid points = 249 function evaluations
        sampler = Sampler(create_transport("GVP", "velocity", None, None, None, snr_type="uniform"))
        fn = sampler.sample_ode(sampling_method="euler", num_steps=250)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(x, model.forward_with_cfg, context=ctx, cfg_scale=4.0)
        torch.cuda.synchronize()
        sec250 = time.perf_counter() - t0
        extra = {}
        if parity_mode:
            # SURVEY.md 8d metric 2 (ii): the reference's own sampler settings (dopri5, rtol 1e-3, atol 1e-6, 250 output
            # times) with the number of function evaluations recorded -- adaptive, so it depends on the (random) weights
            calls = [0]

            class _TooManyEvaluations(RuntimeError):
                pass

            def counted(xx, tt, **kw):
                calls[0] += 1
                if calls[0] > 4000:   # keeps the default bench run bounded if the random-weight ODE turns out stiff
                    raise _TooManyEvaluations()
                return model.forward_with_cfg(xx, tt, **kw)
            fn5 = sampler.sample_ode(sampling_method="dopri5", num_steps=250, atol=1e-6, rtol=1e-3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            try:
                fn5(x, counted, context=ctx, cfg_scale=4.0)
                finished = True
            except _TooManyEvaluations:
                finished = False
            torch.cuda.synchronize()
            extra["dopri5_parity_mode"] = {"sec": round(time.perf_counter() - t0, 4), "nfe": calls[0], "finished": finished,
                                           "rtol": 1e-3, "atol": 1e-6, "num_steps": 250}
            # CPU figure next to it: the fp32 oracle (PyTorch CPU over the same state dict), one function evaluation
            from oracle import dit as odit
            sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
            cctx = {k: v.float().cpu() for k, v in ctx.items()}
            ncpu = host_threads()
            torch.set_num_threads(ncpu)
            best, runs = float("inf"), []
            for _ in range(3):                             # the first call pays the oneDNN primitive set-up; the host is shared:
                t0 = time.perf_counter()                   # best of 3, every run on the line (737 ... 1047 ms between boxes in round 5)
                odit.forward_with_cfg(sd, x.float().cpu(), t.cpu(), cctx, 4.0)
                runs.append(time.perf_counter() - t0)
                best = min(best, runs[-1])
                if best > 20.0:
                    break
            extra["cpu_baseline"] = {"value": round(best * 1e3, 2), "unit": "ms per function evaluation", "kind": "port",
                                     "cores": ncpu, "runs_ms": [round(v * 1e3, 1) for v in runs],
                                     "sample": "best of 3 forward_with_cfg calls of the fp32 PyTorch oracle on the host "
                                               "cores (CFG batch 2 x 768 tokens); x249 for a 250-step Euler stage; the host is "
                                               "shared with other tenants: the runs differ by box and by minute"}
    fl, fl_exec, fl_attn = dit_flops_per_nfe(model.embed_dim, model.depth, L, M, 1024, B, ca_batch=samples)
    tf = fl_exec / (ms * 1e-3) / 1e12
    return {"arch": arch, "cfg_batch": B, "tokens": L, "ctx_tokens": M, "ms_per_nfe": round(ms, 4),
            "algorithmic_tflop_per_nfe": round(fl / 1e12, 4), "executed_tflop_per_nfe": round(fl_exec / 1e12, 4),
            "achieved_tflops": round(tf, 2), "achieved_tflops_note": "EXECUTED flops (the zero-context half skips its cross-attention) / time",
            "algorithmic_tflops": round(fl / (ms * 1e-3) / 1e12, 2),
            "bf16_mfma_peak_tflops": 2500.0, "frac_of_mfma_peak": round(tf / 2500.0, 4),
            "sec_per_250_step_euler_stage": round(sec250, 4), "nfe_timed": nfe, "ms_per_nfe_runs": [round(v, 4) for v in reps],
            "ms_per_nfe_is": "median of three runs of nfe_timed evaluations", **extra}


def build_cascade_models(dev):
    """The released cascade at full size with seeded random weights (no checkpoints here): DiT-L stage 1, DiT-L stage 2,
    surfel decoder."""
    from gaussiananything_amd.decode import SurfelDecoder
    from gaussiananything_amd.dit import DiT_models
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(4)
    models = []
    for arch, C in (("DiT-PixArt-PCD-CLAY-L", 3), ("DiT-PixArt-PCD-CLAY-stage2-L", 10)):
        m = DiT_models[arch](input_size=16, in_channels=C, context_dim=1024, pooling_ctx_dim=768, num_classes=0,
                             learn_sigma=False, roll_out=True)
        with torch.no_grad():
            for p_ in m.parameters():
                if float(p_.abs().max()) == 0.0:
                    p_.copy_(torch.randn(p_.shape, generator=g) * 0.02)
        models.append(m.to(dev))
    dec = SurfelDecoder()
    with torch.no_grad():
        for name, p_ in dec.named_parameters():
            if name.endswith("pos_embed") or "latent_embedding" in name:
                p_.copy_(torch.randn(p_.shape, generator=g) * 0.5)
            elif p_.dim() >= 2:
                p_.copy_(torch.randn(p_.shape, generator=g) * (0.5 / p_.shape[-1] ** 0.5))
    dec.to(dev)
    return models[0], models[1], dec


def bench_cascade(dev, cams, rank, world, dist, dopri5=True):
    """BASELINE configs[3] / [4]: one cascaded sample PER RANK (independent seeds and conditioning), as ONE measured
    wall-clock figure from the conditioning tensors on the device to the rendered multi-view RGB-D-N collected on rank 0:
    stage-1 DiT-L and stage-2 DiT-L (250 grid points each, CFG batch 2) -> surfel decode -> renders of all four levels for
    8 views -> one gather of [V,9,512,512] per rank (gaussiananything_amd/distributed.py: cascade_per_rank).  Timed between
    barriers, maximum over the ranks.  (i) fixed mode: euler, 249 function evaluations per stage; (ii) parity mode, rank
    0 at N=1 only: the reference's own sampler settings (dopri5, rtol 1e-3, atol 1e-6), evaluations recorded."""
    from gaussiananything_amd import distributed as gd
    m1, m2, dec = build_cascade_models(dev)
    c = {"cam_view": cams["cam_view"][None].to(dev), "cam_view_proj": cams["cam_view_proj"][None].to(dev),
         "cam_pos": cams["cam_pos"][None].to(dev), "tanfov": cams["tanfov"]}

    # SURVEY.md 8d metric 2: "wall-clock from conditioning tensors ON DEVICE to final multi-view RGB-D-N on device" -- every call's
    # conditioning is drawn (CPU generator, 1.4 M numbers) and moved to the device BEFORE its timer starts; each call gets tensors of its
    # own (new addresses, new values), as a serving loop's next request would.  (Rounds 1-5 drew them inside the timed call: ~12 ms.)
    conds = {}

    def prepare(base):
        from gaussiananything_amd.distributed import shard_samples
        conds.clear()
        for i in shard_samples(world, rank, world):
            g = torch.Generator().manual_seed(base + i)
            cond = {"img_crossattn": torch.randn(1, 1369, 1024, generator=g).to(dev), "img_vector": torch.randn(1, 1024, generator=g).to(dev)}
            conds[i] = (cond, {k: torch.zeros_like(v) for k, v in cond.items()})
        torch.cuda.synchronize()

    def cond_fn(i):
        return conds[i]

    def run(method, steps, stats=None):
        return gd.cascade_per_rank(m1, m2, dec, cond_fn, c, world, base_seed=42, num_steps=steps, sampling_method=method,
                                   render_all_scale=True, **({"stats": stats} if stats is not None else {}))

    prepare(1000)
    run("euler", 250)   # warm-up SAMPLE: lazy initialisation, workspaces, and the capture of the two sampler steps -- the timed sample
                        # below (new conditioning tensors, same shapes) replays them, as every later sample of a serving loop does
    prepare(2000)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    gathered, mine = run("euler", 250)
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    sec = gd.max_over_ranks(time.perf_counter() - t0, dev)
    out = {"sec_per_sample": round(sec, 4), "samples": world, "samples_per_sec": round(world / sec, 4),
           "mode": "euler, 250 grid points = 249 function evaluations per stage; one untimed warm-up sample first (it captures the sampler "
                   "steps the timed sample replays on its own conditioning); timed from the conditioning tensors on the device "
                   "(SURVEY 8d; rounds 1-5 also timed drawing them on the host, ~12 ms)",
           "stages": "DiT-L x 249 NFE, stage-2 DiT-L x 249 NFE (cond_key img-xyz: uc == c), decode -> 73728 surfels, renders 8 views x "
                     "{128,256,384,512}^2, gather of [8,9,512,512] fp32 per rank to rank 0",
           "gathered_shape": list(gathered.shape) if gathered is not None else None}
    if dopri5 and world == 1:
        stats = {}
        prepare(3000)
        try:
            run("dopri5", 250)     # warm-up sample (captures the attempted step of both stages)
        except (FloatingPointError, RuntimeError):
            pass
        prepare(4000)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        try:
            run("dopri5", 250, stats)
            torch.cuda.synchronize()
            out["dopri5"] = {"sec_per_sample": round(time.perf_counter() - t0, 4), "rtol": 1e-3, "atol": 1e-6, "num_steps": 250,
                             "nfe_stage1": stats.get("stage1", {}).get("nfe"), "nfe_stage2": stats.get("stage2", {}).get("nfe"),
                             "rejected": [stats.get("stage1", {}).get("rejected"), stats.get("stage2", {}).get("rejected")],
                             "note": "adaptive: the evaluation count depends on the (random) weights"}
        except (FloatingPointError, RuntimeError) as e:   # a random-weight ODE may be too stiff for the step cap
            out["dopri5"] = {"error": f"{type(e).__name__}: {e}"[:200]}
    return out


def parity_check(g, cams, H, W, dev):
    """Untimed: the bench workload itself through the HIP path against the C oracle, every view -- integer artefacts (radii,
    tile rects, per-tile ranges, depth-ordered point lists) bit-identical, pixel MSE per output channel (bar 1e-5), and beside the
    MSE the absolute differences: the largest one per channel group, the number of pixels beyond 1e-4 (bar: <= 3e-4 of the pixels of
    any channel, never more than 24 in one 16 x 16 tile -- a wrong tile is 256 -- and <= 0.25 outside the median-depth channel, whose
    `T > 0.5` pick jumps from one splat's depth to another's), and the same count for the fp32 oracle against ITS OWN loop in double
    (oracle/surfel_raster.c, -DORACLE_BLEND_F64): the pixels where threshold decisions flip or an edge-on splat's cross product
    cancels are no more frequent for the HIP kernel than for any other fp32 evaluation order."""
    from gaussiananything_amd import synthetic
    from gaussiananything_amd.diff_surfel_rasterization import rasterize_views
    from oracle import surfel as osurf
    m, o, s, r, c = synthetic.split_gaussians(g)
    V = cams["cam_view"].shape[0]
    color, radii, allmap, ws = rasterize_views(*[t.to(dev) for t in (m, o, c, s, r)], cams["cam_view"].to(dev),
                                               cams["cam_view_proj"].to(dev), torch.ones(3, device=dev), H, W, 1.0)
    torch.cuda.synchronize()
    N = m.shape[0]
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    st = ws.status().cpu().numpy()
    D = int(st[0])
    tile_start = ws.section("tile_start", torch.int32, V * tiles + 1).cpu().numpy().astype(np.int64)
    rect = ws.section("rect", torch.int16, V * N * 4).cpu().numpy().view(np.uint16).reshape(V, N, 4)
    plist = ws.section("point_list", torch.int32, max(D, 1)).cpu().numpy()[:D]
    color, radii, allmap = color.cpu().numpy(), radii.cpu().numpy(), allmap.cpu().numpy()
    exact, worst, total = True, 0.0, 0
    max_abs, max_abs_median = 0.0, 0.0
    beyond = np.zeros(10, np.int64)
    beyond64 = np.zeros(10, np.int64)
    tile_worst = 0
    args = [t.numpy() for t in (m, o, c, s, r)]
    for v in range(V):
        cam = (cams["cam_view"][v].numpy(), cams["cam_view_proj"][v].numpy(), np.ones(3, np.float32), H, W)
        ov = osurf.rasterize(*args, *cam)
        o64 = osurf.rasterize(*args, *cam, blend_f64=True)
        ts = tile_start[v * tiles:(v + 1) * tiles + 1]
        cnt = ov["ranges"][:, 1].astype(np.int64) - ov["ranges"][:, 0].astype(np.int64)
        exact &= bool(np.array_equal(radii[v], ov["radii"]) and np.array_equal(rect[v].astype(np.uint32), ov["rect"])
                      and np.array_equal(np.diff(ts), cnt)
                      and np.array_equal(plist[ts[0]:ts[0] + ov["D"]].astype(np.uint32), ov["point_list"]))
        total += ov["D"]
        worst = max(worst, float(np.mean((color[v] - ov["color"]) ** 2)),
                    *[float(np.mean((allmap[v, ch] - ov["allmap"][ch]) ** 2)) for ch in range(7)])
        d = np.concatenate([np.abs(color[v] - ov["color"]), np.abs(allmap[v] - ov["allmap"])], 0)       # [10, H, W]
        d64 = np.concatenate([np.abs(ov["color"] - o64["color"]), np.abs(ov["allmap"] - o64["allmap"])], 0)
        med = 3 + 5                                                                                         # allmap channel 5: median depth
        max_abs = max(max_abs, float(np.delete(d, med, 0).max()))
        max_abs_median = max(max_abs_median, float(d[med].max()))
        beyond += (d > 1e-4).reshape(10, -1).sum(1)
        beyond64 += (d64 > 1e-4).reshape(10, -1).sum(1)
        Hp, Wp = (H + 15) // 16 * 16, (W + 15) // 16 * 16
        pad = np.zeros((10, Hp, Wp), bool)
        pad[:, :H, :W] = d > 1e-4
        tile_worst = max(tile_worst, int(pad.reshape(10, Hp // 16, 16, Wp // 16, 16).sum((2, 4)).max()))
    exact &= total == D
    frac = float(beyond.max()) / (V * H * W)
    ok = bool(exact and worst <= 1e-5 and frac <= 3e-4 and tile_worst <= 24 and max_abs <= 0.25)
    return {"against": "oracle/surfel_raster.c (CPU port; parity unpinned vs upstream, see DESIGN.md)", "views": V,
            "bins_bit_identical": bool(exact), "num_rendered_D": D, "max_channel_mse": float(f"{worst:.3e}"),
            "mse_bar": 1e-5, "max_abs": float(f"{max_abs:.3e}"), "max_abs_median_depth_channel": float(f"{max_abs_median:.3e}"),
            "pixels_beyond_1e-4_worst_channel": int(beyond.max()), "pixels_beyond_1e-4_fraction": float(f"{frac:.3e}"),
            "pixels_beyond_1e-4_fp32_oracle_vs_its_fp64_blend": int(beyond64.max()),
            "most_pixels_beyond_1e-4_in_one_tile": tile_worst,
            "max_abs_bars": "<= 3e-4 of the pixels of any channel beyond 1e-4, <= 24 of them in one 16x16 tile, <= 0.25 anywhere outside the "
                            "median-depth channel (decision flips / edge-on splats: as frequent between the fp32 oracle and its own fp64 blend)",
            "pass": ok}


def traj250_evidence():
    """end / worst state of profiles/r6_traj250.txt (BASELINE configs[2] as written: DiT-B, 250 Euler grid points, HIP vs the all-fp32
    oracle trajectory; ~13 min of host time, so committed instead of run here)"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "r6_traj250.txt")
    try:
        vals = {l.split()[0]: float(l.split()[1]) for l in open(path) if l.startswith(("end_state_rel_l2", "worst_state_rel_l2"))}
        return {"end_state_rel_l2": vals["end_state_rel_l2"], "worst_state_rel_l2": vals["worst_state_rel_l2"], "bar": 3e-2,
                "source": "profiles/r6_traj250.txt (committed GPU-box run of tools/parity_r6.py traj250), not measured in this run; "
                          "tests/test_dit_gpu.py asserts the 25-point quantity on every GPU test run"}
    except (OSError, KeyError, ValueError, IndexError):
        return None


def trajectory_parity(dev, points=25):
    """BASELINE configs[2] at real depth, untimed: DiT-PixArt-PCD-CLAY-B (depth 12, seeded weights) integrated from t = 0 to 1 with the
    guided Euler sampler over `points` grid points through the HIP path (bf16 MFMA operands, fused on-device step) against the all-fp32
    trajectory (oracle/dit.py integrated by oracle/ode.py on the host cores): relative L2 of the end state.  The same quantity for
    dopri5 and DiT-L is asserted by tests/test_dit_gpu.py::test_full_depth_sampling_trajectory_against_the_fp32_oracle."""
    from gaussiananything_amd.transport import Sampler, create_transport
    from oracle import trajectory as otraj
    model, sd = otraj.release_model("DiT-PixArt-PCD-CLAY-B", 3)
    x0, ctx = otraj.release_inputs(3, cfg=True)
    t0 = time.perf_counter()
    ref = otraj.integrate(sd, x0, ctx, 4.0, "euler", points, cfg=True, threads=host_threads())
    cpu_s = time.perf_counter() - t0
    model.to(dev)
    sampler = Sampler(create_transport("GVP", "velocity", None, None, None, snr_type="uniform"))
    fn = sampler.sample_ode(sampling_method="euler", num_steps=points)
    with torch.no_grad():
        out = fn(x0.to(dev), model.forward_with_cfg, context={k: v.to(dev) for k, v in ctx.items()}, cfg_scale=4.0)
    got = out.double().cpu().numpy()
    end = otraj.rel_l2(got[-1], ref[-1])
    return {"model": "DiT-PixArt-PCD-CLAY-B depth 12, CFG batch 2 x 768 tokens, scale 4", "method": f"euler, {points} grid points = {points - 1} evaluations",
            "trajectory_rel_l2": float(f"{end:.3e}"), "worst_saved_state_rel_l2": float(f"{max(otraj.rel_l2(got[i], ref[i]) for i in range(1, points)):.3e}"),
            "state_moved_by": round(otraj.rel_l2(ref[-1], ref[0]), 3), "bar": 3e-2, "pass": bool(end < 3e-2),
            "oracle_cpu_seconds": round(cpu_s, 1), "against": "oracle/dit.py (pinned to the reference's classes) integrated by oracle/ode.py, fp32 / fp64"}


def bench_conditioner(dev, reps=5):
    """Image conditioner at the release size: DINOv2 ViT-L/14 with 4 registers at 518 px (1374 tokens, 24 blocks; seeded
    random weights), one image, preprocess (bicubic resize 512 -> 518 + normalisation) included.  FLOPs: 24 x (24 T D^2 +
    4 T^2 D) + patch embedding."""
    from gaussiananything_amd.conditioner import FrozenDinov2ImageEmbedder
    torch.manual_seed(0)
    e = FrozenDinov2ImageEmbedder(arch="vitl", output_cls=True, inp_size=518)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for name, p_ in e.model.named_parameters():
            if name.endswith("gamma"):
                p_.fill_(0.5)
            elif p_.dim() >= 2:
                p_.copy_(torch.randn(p_.shape, generator=g) * (0.5 / p_[0].numel() ** 0.5))
    e.to(dev)
    img = (torch.rand(1, 3, 512, 512, generator=g) * 2 - 1).to(dev)
    e(img)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        tok, cls = e(img)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / reps * 1e3
    T, D = 1374, 1024
    fl = 24 * (24 * T * D * D + 4 * T * T * D) + 2 * 1369 * 588 * D
    return {"arch": "DINOv2 ViT-L/14 reg4 @518", "tokens": T, "ms_per_image": round(ms, 3), "algorithmic_tflop": round(fl / 1e12, 3),
            "achieved_tflops": round(fl / (ms * 1e-3) / 1e12, 1),
            "note": "parity unpinned (third-party model, no weights here): timing and shapes only; once per sample"}


def bench_decode(dev, cams, reps=5):
    """Surfel decode at the release size (DiT2-B/2 backbone: width 768, depth 12, 768 anchors; upsamplers x8, x4, x3 ->
    73 728 surfels; seeded random weights, anchors = one in-tree FPS cloud) and the raster of its finest level at 8 x 512^2
    (BASELINE configs[3] tail).  FLOPs: backbone 12 x (36 M D^2 + 4 N^2 D), upsamplers 24 D^2 per token and layer."""
    from gaussiananything_amd import synthetic
    from gaussiananything_amd.decode import SurfelDecoder
    from gaussiananything_amd.diff_surfel_rasterization import SurfelForwardPlan
    torch.manual_seed(0)
    D, N = 768, 768
    model = SurfelDecoder(embed_dim=D, depth=12, num_heads=12, tokens=N, ldm_z_channels=10)
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for name, p_ in model.named_parameters():
            if name.endswith("pos_embed") or "latent_embedding" in name:
                p_.copy_(torch.randn(p_.shape, generator=g) * 0.5)
            elif p_.dim() >= 2:
                p_.copy_(torch.randn(p_.shape, generator=g) * (0.5 / p_.shape[-1] ** 0.5))
    model.to(dev)
    latent = torch.randn(1, N, 10, generator=g).to(dev)
    xyz = torch.from_numpy(np.load(synthetic.fixture_path("fps_clouds.npz"))["xyz"][0][:N]).float()[None].to(dev)
    out = model.decode(latent, xyz)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = model.decode(latent, xyz)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / reps * 1e3
    fl = 12 * (36 * N * D * D + 4 * N * N * D) + 24 * D * D * (N * 9 * 2 + N * 8 * 5 + N * 32 * 4)
    gs = out["gaussians_upsampled_3"][0]
    m, o, s, r, c = synthetic.split_gaussians(gs)
    plan = SurfelForwardPlan(m, o, c, s, r, cams["cam_view"].to(dev), cams["cam_view_proj"].to(dev),
                             torch.ones(3, device=dev), 512, 512)
    plan.run()
    D_ = plan.ensure_capacity()
    for _ in range(5):
        plan.run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        plan.run()
    torch.cuda.synchronize()
    rms = (time.perf_counter() - t0) / 20 * 1e3
    # the video path of the sampling scripts: 50 cameras x 4 levels per sample (flow_matching_trainer.py:1545-1616), here
    # one rasterizer call per level with all 50 views, camera matrices built on the device
    from gaussiananything_amd import cameras as cammod
    c50 = cammod.c_to_3dgs_format_device(torch.from_numpy(cammod.orbit_poses(50, seed=0)).to(dev)[None])
    model.triplane_decode(out, c50, render_all_scale=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        model.triplane_decode(out, c50, render_all_scale=True)
    torch.cuda.synchronize()
    vms = (time.perf_counter() - t0) / 3 * 1e3
    return {"surfels": int(gs.shape[0]), "ms_per_decode": round(ms, 3), "algorithmic_tflop": round(fl / 1e12, 3),
            "video_50views_x_4levels_ms": round(vms, 3),
            "achieved_tflops": round(fl / (ms * 1e-3) / 1e12, 1),
            "raster_8x512_ms": round(rms, 4), "raster_num_rendered_D": int(D_),
            "note": "random weights: timing and shapes are those of the release, the surfels are not a meaningful object"}


def bench_backward(m, o, c, s, r, cams, H, W, dev, reps=8):
    """forward + backward of the rasterizer through torch.autograd (ga_surfel_backward) on the bench workload."""
    from gaussiananything_amd.diff_surfel_rasterization import rasterize_views
    torch.manual_seed(0)
    leaves = [t.detach().clone().requires_grad_(True) for t in (m, o, c, s, r)]
    vm, pm = cams["cam_view"].to(dev), cams["cam_view_proj"].to(dev)
    bg = torch.ones(3, device=dev)
    wc = torch.rand(vm.shape[0], 3, H, W, device=dev)
    wo = torch.rand(vm.shape[0], 7, H, W, device=dev) * 0.1
    fwd, bwd = [], []
    for k in range(reps + 2):
        for t in leaves:
            t.grad = None
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        color, _, allmap, _ = rasterize_views(leaves[0], leaves[1], leaves[2], leaves[3], leaves[4], vm, pm, bg, H, W)
        e[1].record()
        ((color * wc).sum() + (allmap * wo).sum()).backward()
        e[2].record()
        torch.cuda.synchronize()
        if k >= 2:
            fwd.append(e[0].elapsed_time(e[1])); bwd.append(e[1].elapsed_time(e[2]))
    return {"forward_autograd_ms": round(float(np.median(fwd)), 4), "loss_plus_backward_ms": round(float(np.median(bwd)), 4),
            "grads_finite": bool(all(torch.isfinite(t.grad).all() for t in leaves)),
            "note": "forward through the autograd Function (own workspace per call); backward = ga_surfel_backward + the loss's "
                    "elementwise kernels (~0.1 ms); per-kernel times: profiles/r3_backward_kernel_stats.txt (the backward is unchanged since round 3)"}


def bench_mesh_export(g, cams, dev):
    """the reference's mesh export (flow_matching_trainer.py:1244-1395) on 8 rendered 512^2 views of the bench scene."""
    from gaussiananything_amd import mesh
    from gaussiananything_amd.gs_surfel import GaussianRenderer2DGS
    nv = int(cams["cam_view"].shape[0])
    rnd = GaussianRenderer2DGS(512, nv, {})
    cv, cvp, cp = (cams[k][None].to(dev) for k in ("cam_view", "cam_view_proj", "cam_pos"))
    out = rnd.render(g[None].to(dev), cv, cvp, cp, cams["tanfov"])
    rgbs, depths, alphas = ([out[k][0, i][None] for i in range(nv)] for k in ("image", "depth", "alpha"))
    cam_pathes = [{"cam_view": cams["cam_view"][i], "cam_pos": cams["cam_pos"][i], "tanfov": cams["tanfov"]} for i in range(nv)]
    aabb = np.array([-0.45, -0.45, -0.45, 0.45, 0.45, 0.45]).reshape(2, 3) * 1.1
    res = {}
    for rep in range(2):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        v, c, t = mesh.extract_mesh_bounded(rgbs, depths, alphas, cam_pathes, aabb, device=dev)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        pv, pc, pt = mesh.post_process_mesh(v, c, t)
        torch.cuda.synchronize(); t2 = time.perf_counter()
        res = {"fuse_and_extract_ms": round((t1 - t0) * 1e3, 3), "post_process_ms": round((t2 - t1) * 1e3, 3),
               "views": nv, "vertices": int(v.shape[0]), "triangles": int(t.shape[0]), "post_triangles": int(pt.shape[0])}
    res["note"] = ("volume allocation (0.87 GB zero-fill) + 8 x ga_tsdf_integrate + marching cubes, then the cluster filter (round 5: "
                   "union-find kernel ga_mesh_cluster_labels, 9.9 -> 1.6 ms); per-phase times: profiles/r5_tsdf_bench.json; Open3D on the CPU in the reference")
    return res


def summary_of(out):
    """The line's figures once more, compact, as its last key: stage times [us], parity verdicts, ms per evaluation and fraction of the
    bf16 MFMA peak per denoiser, the two attention launches, the cascade, the CPU baselines."""
    def g(d, *ks):
        for k in ks:
            d = d.get(k) if isinstance(d, dict) else None
        return d
    sm = {"Msplats_s": out.get("value"), "ms_step": out.get("ms_per_step"), "n_gpus": out.get("n_gpus")}
    if out.get("stage_ms"):
        sm["stage_us"] = {k[:4]: round(v * 1e3, 1) for k, v in out["stage_ms"].items()}
    if out.get("roofline"):
        sm["blend"] = {"hbm_frac": out["roofline"]["frac"], "hbm_frac_all_px": out["roofline"].get("frac_all_pixels"),
                       "valu_issue": out["roofline"].get("valu_issue_frac"),
                       "valu_Minsts": None if not out["roofline"].get("valu_wave_instructions_per_launch") else
                       round(out["roofline"]["valu_wave_instructions_per_launch"] / 1e6, 1),
                       "traffic_MB": None if not out["roofline"].get("traffic") else round(out["roofline"]["traffic"] / 1e6, 1)}
    if out.get("stress_scene"):
        sm["stress_ms"] = out["stress_scene"]["ms_per_step"]
    if out.get("two_streams"):
        sm["two_streams_Msplats_s"] = out["two_streams"]["Msplats_per_s"]
    if out.get("parity"):
        pr = out["parity"]
        sm["parity"] = {"pass": pr.get("pass"), "bins_exact": pr.get("bins_bit_identical"), "mse": pr.get("max_channel_mse"),
                        "max_abs": pr.get("max_abs"), "px>1e-4": pr.get("pixels_beyond_1e-4_worst_channel"),
                        "px>1e-4_o32_vs_o64": pr.get("pixels_beyond_1e-4_fp32_oracle_vs_its_fp64_blend"),
                        "traj_rel_l2": pr.get("trajectory_rel_l2"),
                        "traj250_end": (pr.get("trajectory_250_points") or {}).get("end_state_rel_l2")}
    if out.get("cpu_baseline"):
        sm["cpu_Msplats_s"] = [out["cpu_baseline"]["value"], out["cpu_baseline"]["cores"]]
    if out.get("dit"):
        sm["dit"] = {d["arch"].replace("DiT-PixArt-PCD-CLAY-", ""): [d["ms_per_nfe"], d.get("frac_of_mfma_peak")] for d in out["dit"]}
        sm["dit_is"] = "[ms/NFE, frac bf16 MFMA peak]"
        b = out["dit"][0]
        sm["ditB_dopri5"] = [g(b, "dopri5_parity_mode", "sec"), g(b, "dopri5_parity_mode", "nfe")]
        sm["ditB_cpu_ms_nfe"] = g(b, "cpu_baseline", "value")
    if out.get("dit_batched"):
        sm["dit_x4_ms"] = out["dit_batched"]["ms_per_nfe"]
    if out.get("dit_shapes"):
        sm["ditL_b1_cfg4_ms"] = [d["ms_per_nfe"] for d in out["dit_shapes"]]
    if out.get("dit_xl"):
        sm["ditXL_ms"] = out["dit_xl"]["ms_per_nfe"]
    if out.get("attention"):
        at = out["attention"]
        sm["attn_us"] = [g(at, "self_attention_2x16x768x768", "us"), g(at, "cross_attention_1x16x768x1369", "us")]
        ks = g(at, "mfma_busy_from_counters", "kernels")
        sm["attn_mfma_busy"] = [round(v["mfma_busy"], 3) for v in ks.values()] if ks else None
    if out.get("decode"):
        sm["decode_ms"] = out["decode"]["ms_per_decode"]
    if out.get("conditioner"):
        sm["cond_ms"] = out["conditioner"]["ms_per_image"]
    if out.get("backward"):
        sm["bwd_ms"] = [out["backward"]["forward_autograd_ms"], out["backward"]["loss_plus_backward_ms"]]
    if out.get("cascade"):
        sm["sec_per_sample"] = out.get("sec_per_sample")
        sm["sec_per_sample_dopri5"] = out.get("sec_per_sample_dopri5")
        sm["dopri5_nfe"] = [g(out["cascade"], "dopri5", "nfe_stage1"), g(out["cascade"], "dopri5", "nfe_stage2")]
    return sm


DUMP_BUDGET_BYTES = 64 * 10 ** 6 - 4096   # all .npy files of --dump-outputs together, headers included


def dump_outputs(path, plan):
    """--dump-outputs: the arrays of the last forward as float32 .npy files in `path`, smallest first, each in full while it fits
    an even share of what is left of the budget, else a fixed seeded sample of its elements (<name>_sample.npy)."""
    os.makedirs(path, exist_ok=True)
    torch.cuda.synchronize()
    arrays = [(name, t.cpu().numpy().astype(np.float32, copy=False)) for name, t in
              (("color", plan.color), ("radii", plan.radii), ("allmap", plan.allmap))]
    arrays.sort(key=lambda na: na[1].nbytes)
    left = DUMP_BUDGET_BYTES
    for i, (name, a) in enumerate(arrays):
        share = left // (len(arrays) - i)
        if a.nbytes <= share:
            fname, data = f"{name}.npy", a
        else:
            k = share // a.itemsize
            idx = np.sort(np.random.default_rng(20251016).choice(a.size, size=k, replace=False))
            fname, data = f"{name}_sample.npy", a.reshape(-1)[idx]
            print(f"bench.py: {name} {list(a.shape)} is written as {k} of its {a.size} elements at seeded sample indices", file=sys.stderr)
        np.save(os.path.join(path, fname), data)
        left -= data.nbytes


def self_launch(n, argv):
    """Re-execute this script as `n` ranks of one node: python -m torch.distributed.run --nnodes=1 --nproc-per-node n ...
    (rank 0 prints the JSON line on the inherited stdout).  Returns the launcher's exit code."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + list(argv)
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # the host driver only supports dmabuf IPC (RCCL across processes)
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--scene", default="surface", choices=["surface", "stress"])
    ap.add_argument("--points", type=int, default=100_000)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run every untimed section of the report (stage events, roofline, parity, CPU "
                         "baseline, denoisers, decode, conditioner, backward, mesh export, cascade, gather); the --no-* switches "
                         "leave parts of it out")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed forward to DIR/<name>.npy (float32, at most 64 MB in all)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-stage-events", action="store_true")
    ap.add_argument("--no-parity", action="store_true", help="skip the untimed HIP-vs-oracle check of the bench workload")
    ap.add_argument("--no-dit", action="store_true", help="skip the DiT/SiT denoiser and cascade sections of the report")
    ap.add_argument("--no-cascade", action="store_true", help="skip the cascaded-sample section (BASELINE configs[3]/[4])")
    ap.add_argument("--no-extras", action="store_true", help="skip the rasterizer-backward and mesh-export sections (SURVEY 8(f)-4)")
    ap.add_argument("--dit-nfe", type=int, default=20)
    ap.add_argument("--trajectory-parity", action="store_true",
                    help="also integrate BASELINE configs[2] (DiT-B, guided Euler, 25 grid points) with the fp32 oracle on the host cores "
                         "(~40 s) and compare; off by default: tests/test_dit_gpu.py asserts the same quantity and "
                         "profiles/r6_traj250.txt holds the 250-point run")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")

    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` on its own: start the N ranks here (one process per GPU through torch.distributed.run,
        # the launch line the driver uses) instead of silently running one rank and reporting n_gpus = 1
        sys.exit(self_launch(a.gpus, sys.argv[1:]))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but the launcher started WORLD_SIZE={world} ranks")
    launch_only = os.environ.get("GA_BENCH_LAUNCH_ONLY")   # CPU test of the launcher: rendezvous (gloo), report, leave
    if launch_only:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="gloo")
        assert dist.get_world_size() == a.gpus
        t = torch.ones(1)
        dist.all_reduce(t)
        if rank == 0:
            print(json.dumps({"launch_only": True, "n_gpus": dist.get_world_size(), "ranks_seen": int(t.item())}), flush=True)
        dist.destroy_process_group()
        return
    if not torch.cuda.is_available() or local_rank >= torch.cuda.device_count():
        raise SystemExit(f"bench.py: rank {rank} needs cuda:{local_rank}, this node shows {torch.cuda.device_count()} GPU(s); "
                         "there is no CPU path")
    dev = torch.device(f"cuda:{local_rank}")
    torch.cuda.set_device(dev)
    dist = None
    if world > 1 or os.environ.get("GA_BENCH_FORCE_DIST"):   # (the variable lets a 1-GPU box walk the multi-rank code path)
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group(backend="nccl", device_id=dev)
        if dist.get_world_size() != a.gpus:
            raise SystemExit(f"bench.py: RCCL process group has {dist.get_world_size()} ranks, --gpus {a.gpus} was asked")

    from gaussiananything_amd import synthetic
    from gaussiananything_amd.diff_surfel_rasterization import SurfelForwardPlan

    H = W = a.size
    cams = synthetic.eval_cameras(a.views)
    # every rank renders its own independent sample (different seed), as the 8-sample cascade does
    if a.scene == "surface":
        g = synthetic.surface_surfels(a.points, seed=1 + rank)[0]
    else:
        g = synthetic.random_surfels(a.points, seed=rank)[0]
    m, o, s, r, c = [t.to(dev) for t in synthetic.split_gaussians(g)]
    plan = SurfelForwardPlan(m, o, c, s, r, cams["cam_view"].to(dev), cams["cam_view_proj"].to(dev),
                             torch.ones(3, device=dev), H, W)
    plan.run()
    plan.ensure_capacity()
    gathered = None
    payload = None
    if dist is not None and a.full:
        payload = torch.empty((a.views, 10, H, W), dtype=torch.float32, device=dev)
        gathered = torch.empty((world, a.views, 10, H, W), dtype=torch.float32, device=dev) if rank == 0 else None

    # ---- the timed region: EXACTLY `steps` forwards (+ the one gather when N > 1), nothing else ----------------------------
    for _ in range(a.warmup):
        plan.run()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(a.steps):
        plan.run()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if dist is not None:
        tt = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    if rank == 0 and a.dump_outputs:
        dump_outputs(a.dump_outputs, plan)
    # the one exchange of the multi-GPU layout -- the rendered views of every rank collected on rank 0 -- is not a step of
    # the rasterizer: it is executed once here and timed on its own (the cascade section below times it where it belongs,
    # at the end of a whole sample)
    gather_ms = None
    if dist is not None and a.full:
        torch.cuda.synchronize()
        dist.barrier()
        tg = time.perf_counter()
        payload[:, 0:3].copy_(plan.color)
        payload[:, 3:10].copy_(plan.allmap)
        dist.gather(payload, list(gathered.unbind(0)) if rank == 0 else None, dst=0)
        torch.cuda.synchronize()
        dist.barrier()
        gather_ms = (time.perf_counter() - tg) * 1e3
    st = plan.ws.status().cpu()
    assert int(st[1]) == 0, "binned-list overflow inside the timed region"

    # ---- untimed: per-stage durations from HIP events on the launch stream (a separate pass of the same forwards) -------
    stage = total_dev = None
    if rank == 0 and a.full and not a.no_stage_events:
        nev = min(a.steps, 30)
        ev = [HipEvents(5) for _ in range(nev)]
        for k in range(nev):
            plan.set_stage_events(ev[k].arr)
            plan.run()
        torch.cuda.synchronize()
        plan.set_stage_events(None)
        names = ["preprocess", "tile_scan_fill", "tile_sort", "blend"]
        stage = {nm: float(np.mean([e.elapsed(i, i + 1) for e in ev])) for i, nm in enumerate(names)}
        total_dev = float(np.mean([e.elapsed(0, 4) for e in ev]))

    out = None
    if rank == 0:
        n, v = a.points, a.views
        value = n * v * a.steps * world / dt / 1e6
        out = {
            "metric": "Msplats/s rasterize (full forward: preprocess+binning+sort+blend)",
            "value": round(value, 2), "unit": "Msplats/s", "n_gpus": world, "rccl_ranks": dist.get_world_size() if dist is not None else 1,
            "steps": a.steps, "warmup": a.warmup,
            "ms_per_step": round(dt / a.steps * 1e3, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": f"BASELINE configs[1]: {n} {a.scene}-scene surfel Gaussians x {v} posed {H}x{W} "
                                   f"views, forward raster, 1 sample per GPU",
                       "scene": a.scene, "points": n, "views": v, "image": [H, W], "num_rendered_D": int(st[0]),
                       "longest_tile_list": int(st[2]),
                       "multi_gpu": "independent samples per rank, no collective in the timed steps; with --full the one RCCL gather "
                                    "of [V,10,H,W] fp32 per rank to rank 0 runs once after them (gather_ms) and inside the "
                                    "timed cascade sample" if world > 1 else "single GPU",
                       "gather_ms": None if gather_ms is None else round(gather_ms, 3)},
        }
        if stage is not None:
            P = H * W
            # per launch (all V views), SURVEY.md 8d: 76 B per list entry + 40 B per pixel THE BLEND LAUNCH WRITES.  Since round 6 the pixels of
            # the empty tiles (background only) are written by the sort launch in front of it (GA_SURFEL_FLAG_BG_IN_BLEND restores the old
            # placement): they are not counted for this kernel any more -- `algorithmic_bytes_all_pixels` / `frac_all_pixels` keep the
            # earlier rounds' accounting (all P pixels) beside it
            tiles_v = ((W + 15) // 16) * ((H + 15) // 16)
            tstart = plan.ws.section("tile_start", torch.int32, v * tiles_v + 1).cpu().numpy().astype(np.int64)
            nonempty = int((np.diff(tstart) > 0).sum())
            bg_in_blend = bool(plan.flags & 8)
            px_blend = P * v if bg_in_blend else min(P * v, nonempty * 256)
            blend_bytes_all = 76.0 * int(st[0]) + 40.0 * P * v
            blend_bytes = 76.0 * int(st[0]) + 40.0 * px_blend
            achieved = blend_bytes / (stage["blend"] * 1e-3) / 1e9
            traffic, tsrc, valu_frac, valu_insts = None, None, None, None  # PMC counters cannot be collected live: committed rocprofv3 passes
            pj = committed_pmc("blend_pmc.json") if (a.scene == "surface" and n == 100_000 and v == 8 and H == 512) else None
            if pj:
                traffic, valu_frac, valu_insts = pj["traffic_bytes_per_launch"], pj["valu_issue_frac"], pj["SQ_INSTS_VALU"]
                tsrc = f"committed PMC ({pj['source']}; surfel_blend.hip unchanged since), not measured in this run"
            # `achieved` / `peak` / `frac` are the HBM pair the contract asks for (algorithmic bytes over the launch duration); what BINDS
            # the kernel is VALU issue -- `valu_issue_frac` says how much of that roof is in use
            out["roofline"] = {"bound": "valu", "kernel": "surfel_blend_kernel", "achieved": round(achieved, 2),
                               "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5),
                               "valu_issue_frac": valu_frac, "valu_wave_instructions_per_launch": valu_insts,
                               "valu_issue_frac_is": "SQ_INSTS_VALU x 4 cycles / 1024 SIMDs over GRBM_GUI_ACTIVE / 8 XCDs (committed PMC pass)",
                               "traffic": traffic, "traffic_source": tsrc, "algorithmic_bytes_per_launch": int(blend_bytes),
                               "algorithmic_bytes_all_pixels": int(blend_bytes_all), "frac_all_pixels": round(blend_bytes_all / (stage["blend"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 5),
                               "nonempty_tiles": nonempty, "pixels_written_by_the_blend": int(px_blend),
                               "avg_launch_ms": round(stage["blend"], 5),
                               "launch_duration_source": "HIP events on the launch stream, separate untimed pass of the same forwards",
                               "note": "achieved / peak: algorithmic HBM bytes of the blend against the HBM roof (SURVEY.md 8d); the binding roof is "
                                       "VALU issue (bound), see valu_issue_frac and blend_valu"}
            # What the blend actually executes (one untimed forward with the statistics flag): (pixel, splat) pairs that
            # survive the cull boxes, the wave-level evaluation slots they were packed into, and the ~60 flop / pair of
            # SURVEY.md 8d -- the bound that matters for this kernel is VALU issue, not HBM.
            splan = SurfelForwardPlan(m, o, c, s, r, cams["cam_view"].to(dev), cams["cam_view_proj"].to(dev),
                                      torch.ones(3, device=dev), H, W, capacity=plan.ws.capacity, flags=1)
            splan.run()
            torch.cuda.synchronize()
            sst = splan.ws.status().cpu().tolist()
            pairs_ub = 256.0 * int(st[0])
            pairs, slots = float(sst[8]), 64.0 * float(sst[4])
            out["blend_valu"] = {"pairs_upper_bound": int(pairs_ub), "pairs_evaluated": int(pairs),
                                 "culled_fraction": round(1.0 - pairs / max(pairs_ub, 1.0), 4),
                                 "lane_slot_utilisation": round(pairs / max(slots, 1.0), 4),
                                 "tflops_at_60flop_per_evaluated_pair": round(pairs * 60 / (stage["blend"] * 1e-3) / 1e12, 3),
                                 "peak_fp32_valu_tflops": FP32_VALU_PEAK_TFLOPS,
                                 "note": "lanes = pixels of an 8x8 quadrant cannot exceed 0.53 lane use on this scene (tools/blend_sim.py); the "
                                         "split walk (lanes = pairs, then lanes = pixels) was built and measured in round 4: 175 us against "
                                         "140 us (DESIGN_HISTORY.md section 3, GA_SURFEL_FLAG_SPLIT_WALK)"}
            del splan
            out["stage_ms"] = {k: round(x, 5) for k, x in stage.items()}
            out["stage_ms"]["device_total"] = round(total_dev, 5)
            if a.scene == "surface" and not a.no_extras:
                out["stress_scene"] = stress_scene_line(cams, a.points, H, W, dev)
                # untimed, beside the headline (which stays ONE forward at a time on one stream): two INDEPENDENT surfel sets rendered
                # concurrently on two streams -- the latency-bound front-end of one hides under the issue-bound blend of the other
                # (tools/overlap_probe.py, DESIGN_HISTORY.md section 3)
                g2 = synthetic.surface_surfels(a.points, seed=101 + rank)[0]
                m2, o2, s2_, r2, c2 = [t.to(dev) for t in synthetic.split_gaussians(g2)]
                plan2 = SurfelForwardPlan(m2, o2, c2, s2_, r2, cams["cam_view"].to(dev), cams["cam_view_proj"].to(dev), torch.ones(3, device=dev), H, W)
                plan2.run(); plan2.ensure_capacity()
                sA, sB = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
                def pair():
                    with torch.cuda.stream(sA):
                        plan.run()
                    with torch.cuda.stream(sB):
                        plan2.run()
                for _ in range(5):
                    pair()
                torch.cuda.synchronize()
                tp0 = time.perf_counter()
                for _ in range(30):
                    pair()
                torch.cuda.synchronize()
                pms = (time.perf_counter() - tp0) / 30 * 1e3
                out["two_streams"] = {"ms_per_pair_of_forwards": round(pms, 4), "Msplats_per_s": round(2 * n * v / pms / 1e3, 1),
                                      "note": "two independent 100k-surfel sets x 8 views on two streams, NOT the headline (one forward at a time)"}
                del plan2
        if a.full and not a.no_parity:
            out["parity"] = parity_check(g, cams, H, W, dev)
        if a.full and world == 1 and not a.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(g, cams, H, W)
        if a.full and world == 1 and not a.no_dit and not a.no_parity and not a.trajectory_parity:
            ev = traj250_evidence()     # the committed full-length run (tools/parity_r6.py traj250 on a GPU box), quoted -- not measured in this run
            if ev is not None:
                out.setdefault("parity", {})["trajectory_250_points"] = ev
        if a.full and world == 1 and not a.no_dit and not a.no_parity and a.trajectory_parity:
            tp = trajectory_parity(dev)     # BASELINE configs[2] at real depth against the fp32 oracle trajectory (CPU: ~40 s)
            out.setdefault("parity", {})["trajectory"] = tp
            out["parity"]["trajectory_rel_l2"] = tp["trajectory_rel_l2"]
            out["parity"]["pass"] = bool(out["parity"].get("pass", True) and tp["pass"])
        if a.full and world == 1 and not a.no_dit:
            # second half of the headline metric ("sec/sample 250-step cascaded"): the two release-size denoisers
            out["dit"] = [bench_dit(dev, arch, a.dit_nfe, 3, parity_mode=(arch == "DiT-PixArt-PCD-CLAY-B")) for arch in
                          ("DiT-PixArt-PCD-CLAY-B", "DiT-PixArt-PCD-CLAY-L", "DiT-PixArt-PCD-CLAY-stage2-L")]
            # throughput mode: four independent samples batched on the GPU (M = 6144 rows fill the chip; one sample does not)
            out["dit_batched"] = bench_dit(dev, "DiT-PixArt-PCD-CLAY-L", a.dit_nfe, 3, samples=4)
            # the two other shapes a released cascade runs: stage 2 on the conditional sequence alone (batch 1, M = 768) and stage 1 at
            # the release script's num_samples=2 (CFG batch 4, M = 3072)
            out["dit_shapes"] = [bench_dit(dev, "DiT-PixArt-PCD-CLAY-stage2-L", a.dit_nfe, 3, cond_only=True),
                                 bench_dit(dev, "DiT-PixArt-PCD-CLAY-L", a.dit_nfe, 3, samples=2)]
            xl = bench_dit(dev, "DiT-PixArt-PCD-CLAY-XL", max(a.dit_nfe // 2, 5), 2, samples=1, cond_only=False) if not os.environ.get("GA_SKIP_XL") else None
            out["dit_xl"] = xl and {k: xl[k] for k in ("arch", "ms_per_nfe", "achieved_tflops", "frac_of_mfma_peak")}
            out["attention"] = bench_attention(dev)
            from tools.gemm_yardstick import yardstick   # same-run, same-node: torch.matmul beside ga_gemm_bf16 (tools only)
            out["gemm_yardstick"] = yardstick(dev)
            gj = committed_pmc("gemm_pmc.json")   # MFMA busy of the GEMM kernels (committed counter pass, hash-keyed like the blend's)
            out["gemm_yardstick"]["mfma_busy_from_counters"] = ({"kernels": {k: v["mfma_busy"] for k, v in gj["kernels"].items()},
                                                                 "source": gj["source"] + " (committed rocprofv3 PMC pass; dit_gemm.hip unchanged since)"}
                                                                if gj else None)
            out["decode"] = bench_decode(dev, cams)
            out["conditioner"] = bench_conditioner(dev)
        if a.full and world == 1 and not a.no_extras and not a.no_dit:   # (--no-dit is the quick rasterizer-only mode of the tools)
            out["backward"] = bench_backward(m, o, c, s, r, cams, H, W, dev)
            out["mesh_export"] = bench_mesh_export(g, cams, dev)
    # ---- BASELINE configs[3] / [4]: one cascaded sample per GPU, every rank takes part -------------------------------
    if a.full and not a.no_dit and not a.no_cascade:
        del plan
        torch.cuda.empty_cache()
        casc = bench_cascade(dev, cams, rank, world, dist)
        if rank == 0:
            out["cascade"] = casc
            out["sec_per_sample"] = casc["sec_per_sample"]            # 250-step cascaded, euler; N samples on N GPUs
            out["sec_per_sample_dopri5"] = casc.get("dopri5", {}).get("sec_per_sample")
    if dist is not None:
        dist.destroy_process_group()
    if rank == 0:
        out["summary"] = summary_of(out)     # LAST key: the figures of the line in <= 1500 characters (a 2000-character tail keeps them)
        try:   # RCCL's version banner sits in the C stdio buffer: let it out BEFORE the one JSON line, not after it
            ctypes.CDLL(None).fflush(None)
        except OSError:
            pass
        sys.stdout.flush()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
