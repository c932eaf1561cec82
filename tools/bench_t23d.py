#!/usr/bin/env python3
"""Times one function evaluation of the text-to-3D denoisers beside the image denoiser, and the short-context cross-attention kernel
against the long-list one (the A/B behind GA_DIT_SHORT_CA).  HIP events around batches of evaluations, warm-up first, the median and
the spread (min .. max) of the repeats.

    python tools/bench_t23d.py [--out profiles] [--repeats 15] [--batch 20]

  profiles/t23d_bench.txt        DiT-PCD-L at CFG batch 2 and 4, DiT-PCD-L-stage2-xyz2feat at batch 2 (768 tokens, caption 77 x 768) and,
                                 as the yardstick measured beside them, DiT-PixArt-PCD-CLAY-L at batch 2 (1369 x 1024 image tokens);
                                 one process
  profiles/t23d_short_ca_ab.txt  ga_attention_short_bf16 vs ga_attention_bf16 at (1, 16, 768, 77) with q projected inside and at
                                 (2, 16, 768, 77), interleaved in one process; the whole DiT-PCD-L evaluation at CFG batch 2 and 4 with GA_DIT_SHORT_CA = 0 / 1 / 2
                                 and without the weight prefetch (GA_DIT_T_PREFETCH=0) in child processes (the switches are read once per process), interleaved rounds
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def timed(fn, repeats, batch, warmup=10):
    """ms per call: [repeats] figures, each over `batch` back-to-back calls between two events"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / batch)
    return out


def summary(ms):
    return f"median {statistics.median(ms):8.4f} ms   min {min(ms):8.4f}   max {max(ms):8.4f}   (n = {len(ms)})"


def build(arch, in_channels):
    from gaussiananything_amd.dit import DiT_models, DiT_models_t23d
    text = arch in DiT_models_t23d
    kw = dict(input_size=16, num_classes=0, learn_sigma=False, in_channels=in_channels, roll_out=True)
    with torch.device("cuda"):
        torch.manual_seed(0)
        m = DiT_models_t23d[arch](context_dim=768, **kw) if text else DiT_models[arch](context_dim=1024, pooling_ctx_dim=768, **kw)
        with torch.no_grad():
            for p in m.parameters():     # the reference zero-initialises the adaLN layers and the final linear
                if float(p.abs().max()) == 0.0:
                    p.normal_(0.0, 0.02)
    return m, text


def evaluation(arch, in_channels, B, L=768):
    """a callable running one function evaluation at CFG batch B (the second half's conditioning all zeros)"""
    m, text = build(arch, in_channels)
    g = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(B, L, in_channels, device="cuda", generator=g)
    t = torch.full((B,), 0.4, device="cuda")
    if text:
        ctx = {"caption_crossattn": torch.randn(B, 77, 768, device="cuda", generator=g), "caption_vector": torch.randn(B, 768, device="cuda", generator=g)}
    else:
        ctx = {"img_crossattn": torch.randn(B, 1369, 1024, device="cuda", generator=g), "img_vector": torch.randn(B, 1024, device="cuda", generator=g)}
    for v in ctx.values():
        v[B // 2:] = 0
    if in_channels == 10:
        ctx["fps-xyz"] = (torch.rand(B, L, 3, device="cuda", generator=g) - 0.5) * 0.9

    def fn():
        with torch.no_grad():
            m(x, t, ctx)
    return fn, m


def child(args):
    fn, m = evaluation("DiT-PCD-L", 3, args.cfg_batch)
    print("RESULT " + json.dumps(timed(fn, args.repeats, args.batch)))


def kernel_ab(repeats, batch, lines):
    from gaussiananything_amd import dit_ops as ops
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(2)
    H, Lq, Lk, D = 16, 768, 77, 1024
    for B, proj in ((1, True), (2, False)):
        k = torch.randn(B * Lk, D, device=dev, generator=g).bfloat16()
        vt = torch.zeros(B * D, 128, device=dev, dtype=torch.bfloat16)
        vt[:, :Lk] = torch.randn(B * D, Lk, device=dev, generator=g).bfloat16()
        out = torch.empty(B * Lq, D, device=dev, dtype=torch.bfloat16)
        wq = (1 + 0.1 * torch.randn(64, device=dev, generator=g)).float()
        a = ops.GaAttentionArgs(B, H, Lq, Lk, None, k.data_ptr(), vt.data_ptr(), D, D, 128, wq.data_ptr(), None, out.data_ptr(), D)
        keep = [k, vt, out, wq]
        if proj:
            A = torch.randn(B * Lq, D, device=dev, generator=g).bfloat16()
            W = ops.tile_weight((torch.randn(D, D, device=dev, generator=g) / 32).bfloat16())
            rss = torch.rand(B * Lq, 16, device=dev, generator=g) * 128
            a.qp_a, a.qp_w, a.qp_lda, a.qp_k, a.qp_w_tiled = A.data_ptr(), W.data_ptr(), D, D, 1
            a.qp_row_ss, a.qp_row_ss_tiles, a.qp_row_ss_dim, a.qp_row_ss_eps = rss.data_ptr(), 16, D, 1e-5
            keep += [A, W, rss]
        else:
            q = torch.randn(B * Lq, D, device=dev, generator=g).bfloat16()
            a.q = q.data_ptr()
            keep.append(q)
        L = ops.lib()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        fns = {"ga_attention_bf16      ": lambda: ops.check(L.ga_attention_bf16(ctypes.byref(a), stream), "ga_attention_bf16"),
               "ga_attention_short_bf16": lambda: ops.check(L.ga_attention_short_bf16(ctypes.byref(a), stream), "ga_attention_short_bf16")}
        res = {n: [] for n in fns}
        for _ in range(3):                       # interleaved rounds
            for n, f in fns.items():
                res[n] += timed(f, repeats, 10 * batch)
        p = ops.attention_plan(a)
        lines.append(f"kernel, ({B}, {H}, {Lq}, {Lk}), q {'projected inside (K = 1024, tiled, row_ss, q_norm)' if proj else 'given (q_norm)'}; "
                     f"the dispatcher's pick: attention_fwd_kernel<{p.nw},{p.ks}>")
        for n, ms in res.items():
            lines.append(f"    {n}  {summary([1000 * v for v in ms]).replace(' ms', ' us')}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--cfg-batch", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_t23d needs an MI355X: a timing taken anywhere else says nothing")
    if args.child:
        return child(args)
    os.makedirs(args.out, exist_ok=True)
    from gaussiananything_amd import dit_ops as ops
    head = [f"# tools/bench_t23d.py --repeats {args.repeats} --batch {args.batch}; {torch.cuda.get_device_name(0)}; {ops.lib().ga_dit_version().decode()}",
            "# ms per function evaluation (HIP events around `batch` evaluations, 10 warm-up evaluations), median / min / max of the repeats;",
            "# one box, one session: figures from different boxes differ by a few per cent"]
    # ---- 1. the evaluations, one process
    lines = list(head)
    rows = [("DiT-PCD-L                  text, CFG batch 2 x 768 x (77 x 768)    ", "DiT-PCD-L", 3, 2),
            ("DiT-PCD-L                  text, CFG batch 4                       ", "DiT-PCD-L", 3, 4),
            ("DiT-PCD-L-stage2-xyz2feat  text, CFG batch 2                       ", "DiT-PCD-L-stage2-xyz2feat", 10, 2),
            ("DiT-PixArt-PCD-CLAY-L      image, CFG batch 2 x 768 x (1369 x 1024)", "DiT-PixArt-PCD-CLAY-L", 3, 2)]
    fns = [(label, evaluation(arch, cin, B)) for label, arch, cin, B in rows]
    res = {label: [] for label, _ in fns}
    for _ in range(args.rounds):                 # interleaved rounds: drift of the box lands on every row alike
        for label, (fn, _) in fns:
            res[label] += timed(fn, args.repeats, args.batch)
    for label, ms in res.items():
        lines.append(f"{label}  {summary(ms)}")
    t2, im = statistics.median(res[rows[0][0]]), statistics.median(res[rows[3][0]])
    spread = max(res[rows[3][0]]) - min(res[rows[3][0]])
    lines.append(f"# text / image at batch 2: {t2 / im:.3f}  (image spread {spread:.4f} ms; the text evaluation must not be slower than the image one beyond it: "
                 f"{'holds' if t2 <= im + spread else 'DOES NOT HOLD'})")
    open(os.path.join(args.out, "t23d_bench.txt"), "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    del fns
    torch.cuda.empty_cache()
    # ---- 2. the short-context kernel
    lines = list(head)
    kernel_ab(args.repeats, args.batch, lines)
    print("\n".join(lines[len(head):]))
    for B in (2, 4):
        variants = [("GA_DIT_SHORT_CA=0 (long-list kernel)                    ", {"GA_DIT_SHORT_CA": "0"}),
                    ("GA_DIT_SHORT_CA=1 (default: short kernel by shape)      ", {"GA_DIT_SHORT_CA": "1"}),
                    ("GA_DIT_SHORT_CA=2 (short kernel always)                 ", {"GA_DIT_SHORT_CA": "2"})]
        if B == 2:
            variants += [("default, GA_DIT_T_PREFETCH=0 (no weight prefetch)       ", {"GA_DIT_T_PREFETCH": "0"})]
        res = {label: [] for label, _ in variants}
        for _ in range(2):
            for label, env in variants:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--cfg-batch", str(B), "--repeats", str(args.repeats),
                                    "--batch", str(args.batch)], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
                if r.returncode != 0:
                    raise SystemExit(f"child failed ({label}): {r.stderr[-1500:]}")
                res[label] += json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
        lines.append(f"whole evaluation, DiT-PCD-L, CFG batch {B} (child processes, two interleaved rounds)")
        for label, ms in res.items():
            lines.append(f"    {label}  {summary(ms)}")
            print(lines[-1])
    open(os.path.join(args.out, "t23d_short_ca_ab.txt"), "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
