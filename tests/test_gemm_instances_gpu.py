"""Every case of tests/_gemm_cases.py -- together they reach every kernel instance the GEMM dispatcher can launch -- on the GPU, checked
ELEMENT-WISE against a float64 reference computed from the exact bf16 / fp32 values the kernel reads, with the error model of
tests/_bounds.py (no fudge factor: an element over its bound is a kernel bug or a rounding the model is missing).

Around every call: the output is a view into a larger buffer (ldo > N, rows before and after) whose every element outside [M, N] holds
a sentinel that must come back bit-identical, and so must the pad of the V^T image, emit_x and emit_ss; A has lda > K with NaN in the
pad columns and in the rows behind M (and behind k_rows); W, the bias rows, gates and emit multipliers are followed by NaN.  A correct
kernel never lets one of these values into a stored element.  The tiled weight image gives the row-major weight's bits, and a second
launch of the same call gives the same bits."""
import ctypes
import math
import zlib

import numpy as np
import pytest
import torch

from tests import _bounds as bd
from tests import _gemm_cases as gc

pytestmark = pytest.mark.gpu

BF16_SENTINEL, F32_SENTINEL = 0x7FA5, 0x7FC0BEEF       # NaN payloads no kernel produces
BF16_NAN = 0x7FC0


def _bf16_fill(shape, bits, dev):
    return torch.full(shape, bits, dtype=torch.int16, device=dev).view(torch.bfloat16)


def _f32_fill(shape, bits, dev):
    return torch.full(shape, np.int32(np.uint32(bits)).item(), dtype=torch.int32, device=dev).view(torch.float32)


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class _Report:
    def __init__(self, case, plan):
        self.case, self.plan, self.ratios = case, plan, {}

    def check(self, what, got, ref, bound, col0=0):
        err = (got.double() - ref).abs()
        ratio = torch.where(torch.isfinite(err), err / bound.clamp_min(1e-300), torch.full_like(err, math.inf))
        worst = float(ratio.max())
        self.ratios[what] = worst
        if not worst <= 1.0:
            r, c = divmod(int(ratio.argmax()), ratio.shape[1])
            p = self.plan
            raise AssertionError(
                f"{self.case['name']} {what}: element (row {r}, column {c + col0}) = {float(got[r, c])!r}, reference {float(ref[r, c])!r}, "
                f"|err| {float(err[r, c]):.4g} > bound {float(bound[r, c]):.4g} (x{worst:.3g}); output tile (row {r // p.tile_m}, "
                f"column {(c + col0) // p.tile_n}) of {gc.describe(p)}; {int((ratio > 1).sum())} elements over their bound")

    def line(self):
        return f"GEMMCASE {self.case['name']:28s} {gc.describe(self.plan)} | " + " ".join(f"{k} {v:.3f}" for k, v in self.ratios.items())


@pytest.mark.parametrize("case", gc.CASES, ids=[c["name"] for c in gc.CASES])
def test_gemm_instance_elementwise_against_float64(gpu_device, case):
    from gaussiananything_amd import dit_ops as ops
    dev, c = gpu_device, case
    M, N, K, epi, rpb = c["M"], c["N"], c["K"], c["epi"], c["rpb"]
    seed = zlib.crc32(c["name"].encode())
    g = torch.Generator().manual_seed(seed)
    items = (M + rpb - 1) // rpb
    f32 = lambda *s: torch.randn(*s, generator=g).to(dev)          # noqa: E731
    # ---- operands, each followed (or padded) by values no stored element may depend on
    lda = K + 8 * (1 + seed % 3)
    A_buf = _bf16_fill((M + 2, lda), BF16_NAN, dev)
    kr = c["k_rows"] or M
    A_buf[:kr, :K] = torch.randn(kr, K, generator=g).to(dev).bfloat16()
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(dev).bfloat16()
    W_buf = _bf16_fill((N + 8, K), BF16_NAN, dev)
    W_buf[:N] = W
    Wt_buf = None
    if N % 8 == 0:
        Wt_buf = _bf16_fill(((N + 8) * K,), BF16_NAN, dev)
        Wt_buf[:N * K] = ops.tile_weight(W)
    bias = None
    if c["bias"] == "row":
        bias = torch.full((N + 4,), math.nan, device=dev)
        bias[:N] = f32(N)
    elif c["bias"] == "batch":
        bias = torch.full((items, N + 4), math.nan, device=dev)
        bias[:, :N] = f32(items, N)
    gate = None
    if c["gate"]:
        gate = torch.full((items, N + 8), math.nan, device=dev)
        gate[:, :N] = f32(items, N)
    qk_w = [(1 + 0.3 * torch.randn(64, generator=g)).to(dev) for _ in range(2)]
    tiles = c["row_ss"]
    row_ss = None
    if tiles:
        row_ss = torch.zeros(M + 1, gc.ss_ld(tiles), device=dev)       # (the pad entries are zeros: the producer writes them so)
        row_ss[:M, :tiles] = (torch.rand(M, tiles, generator=g) * 128).to(dev)
        row_ss[M] = math.nan
    emit_w = emit_scale = None
    if c["emit"] == "mod":
        emit_w = torch.full((N + 8,), math.nan, device=dev)
        emit_w[:N] = (torch.rand(N, generator=g) + 0.5).to(dev)
        emit_scale = torch.full((items, N + 8), math.nan, device=dev)
        emit_scale[:, :N] = 0.2 * f32(items, N)
    x0 = f32(M, N) if epi == gc.EPI_RES else None
    # ---- outputs: views into sentinel-filled buffers, one row before, one after, pad columns
    Nout = c["vt"] or N
    bf16_out = epi in (gc.EPI_BF16, gc.EPI_GELU)
    ldo = Nout + (4 if (bf16_out and seed % 2) else 8)
    out_init = _bf16_fill((M + 2, ldo), BF16_SENTINEL, dev) if bf16_out else _f32_fill((M + 2, ldo), F32_SENTINEL, dev)
    if x0 is not None:
        out_init[1:M + 1, :N] = x0
    heads_v = (N - c["vt"]) // 64 if c["vt"] else 0
    vt_ld = (rpb + 63) // 64 * 64 + 64
    ss_w = gc.ss_ld(N // 64) if c["emit"] else 0
    ws = ops.splitk_workspace(M, N, dev) if c["splitk"] else None

    def launch(tiled):
        out = out_init.clone()
        vt = _bf16_fill((items * heads_v * 64 + 1, vt_ld), BF16_SENTINEL, dev) if heads_v else None
        ex = _bf16_fill((M + 2, N + 8), BF16_SENTINEL, dev) if c["emit"] else None
        ss = _f32_fill((M + 2, ss_w), F32_SENTINEL, dev) if c["emit"] else None
        ptrs = dict(A=A_buf.data_ptr(), W=(Wt_buf if tiled else W_buf).data_ptr(), out=out[1:].data_ptr(),
                    bias=bias.data_ptr() if bias is not None else None, gate=gate.data_ptr() if gate is not None else None,
                    vt=vt.data_ptr() if vt is not None else None, qk_w0=qk_w[0].data_ptr(), qk_w1=qk_w[1].data_ptr(),
                    row_ss=row_ss.data_ptr() if row_ss is not None else None, emit_x=ex[1:].data_ptr() if ex is not None else None,
                    emit_ss=ss[1:].data_ptr() if ss is not None else None, emit_w=emit_w.data_ptr() if emit_w is not None else None,
                    emit_scale=emit_scale.data_ptr() if emit_scale is not None else None, splitk_ws=ws.data_ptr() if ws is not None else None)
        strides = dict(lda=lda, ldo=ldo, gate_stride=N + 8, bias_stride=N + 4, emit_ld=N + 8, emit_scale_stride=N + 8, vt_ld=vt_ld)
        args = gc.make_args(c, ptrs.get, strides)
        args.w_tiled = 1 if tiled else 0
        prev = ops.splitk_mode(c["splitk"] or -1)
        try:
            plan = ops.gemm_plan(args)
            ops.check(ops.lib().ga_gemm_bf16(ctypes.byref(args), ops._stream(A_buf)), "ga_gemm_bf16")
        finally:
            ops.splitk_mode(prev)
        torch.cuda.synchronize()
        return plan, out, vt, ex, ss

    plan, out, vt, ex, ss = launch(False)
    assert gc.cell(plan) == gc.plan_of(c)[1]          # the plan the CPU coverage test saw
    rep = _Report(c, plan)
    # ---- bit checks: a second launch, and the tiled weight image
    for again in ([launch(False)] + ([launch(True)] if Wt_buf is not None else [])):
        for a, b in zip((out, vt, ex, ss), again[1:]):
            if a is not None:
                assert torch.equal(_bits(a), _bits(b)), f"{c['name']}: not bit-identical to the first launch"
    # ---- sentinels outside the written regions
    inside = torch.zeros(out.shape, dtype=torch.bool, device=dev)
    inside[1:M + 1, :Nout] = True
    sent = BF16_SENTINEL if bf16_out else np.int32(np.uint32(F32_SENTINEL)).item()
    assert bool((_bits(out)[~inside] == sent).all()), f"{c['name']}: a store outside [M, N] of the output"
    # ---- float64 reference
    A64 = torch.zeros(M, K, dtype=torch.float64, device=dev)
    A64[:kr] = A_buf[:kr, :K].double()
    W64 = W.double()
    z = A64 @ W64.T
    E = bd.accumulation(A64.abs() @ W64.abs().T, K)
    item = torch.arange(M, device=dev) // rpb
    if bias is None:
        b = torch.zeros(1, N, dtype=torch.float64, device=dev)
    elif c["bias"] == "row":
        b = bias[:N].double()[None]
    else:
        b = bias[:, :N].double()[item]
    if tiles:
        T = row_ss[:M, :tiles].double().sum(-1, keepdim=True)
        r, rho = bd.row_scale(T, tiles, 64 * tiles, float(np.float32(1e-5)))
        v, P = bd.scale_then_bias(z, E, r, rho, b)
    else:
        v, P = bd.add_bias(z, E, b)
    if epi == gc.EPI_BF16:
        q0, q1 = c["qk"]
        v, P = v.clone(), P.clone()
        for lo, hi, w in ((0, q0, qk_w[0]), (q0, q1, qk_w[1])):
            if hi > lo:
                y, Py = bd.head_norm(v[:, lo:hi].reshape(M, -1, 64), P[:, lo:hi].reshape(M, -1, 64), w.double(),
                                     float(np.float32(1e-5)))
                v[:, lo:hi], P[:, lo:hi] = y.reshape(M, -1), Py.reshape(M, -1)
        bound = bd.bf16_store(v, P)
        rep.check("out", out[1:M + 1, :Nout], v[:, :Nout], bound[:, :Nout])
        if heads_v:
            D = N - c["vt"]
            tok = torch.arange(M, device=dev) - item * rpb
            rows = (item[:, None] * D + torch.arange(D, device=dev)[None])          # [M, D] row of the V^T image
            got = vt[rows, tok[:, None]]
            rep.check("vt", got, v[:, c["vt"]:], bound[:, c["vt"]:], col0=c["vt"])
            written = torch.zeros(vt.shape, dtype=torch.bool, device=dev)
            written[rows, tok[:, None]] = True
            assert bool((_bits(vt)[~written] == BF16_SENTINEL).all()), f"{c['name']}: a V^T store outside the image's rows / tokens"
    elif epi == gc.EPI_GELU:
        ref, bound = bd.gelu_store(v, P)
        rep.check("out", out[1:M + 1, :N], ref, bound)
    elif epi == gc.EPI_F32:
        rep.check("out", out[1:M + 1, :N], v, P)
    else:
        gt = gate[:, :N].double()[item] if gate is not None else torch.ones_like(v)
        x, R = bd.residual(x0.double(), gt, v, P)
        rep.check("out", out[1:M + 1, :N], x, R)
        if c["emit"]:
            if c["emit"] == "mod":
                ref_e, bound_e = bd.emit_modulated(x, R, emit_w[:N].double()[None] * (1 + emit_scale[:, :N].double()[item]))
            else:
                ref_e, bound_e = x, bd.bf16_store(x, R)
            rep.check("emit_x", ex[1:M + 1, :N], ref_e, bound_e)
            ref_s, bound_s = bd.group_sumsq(x.reshape(M, N // 64, 64), R.reshape(M, N // 64, 64))
            rep.check("emit_ss", ss[1:M + 1, :N // 64], ref_s, bound_s)
            assert bool((ss[1:M + 1, N // 64:] == 0).all()), f"{c['name']}: emit_ss pad entries not zero"
            for buf, s_, w_ in ((ex, BF16_SENTINEL, N), (ss, np.int32(np.uint32(F32_SENTINEL)).item(), ss_w)):
                ins = torch.zeros(buf.shape, dtype=torch.bool, device=dev)
                ins[1:M + 1, :w_] = True
                assert bool((_bits(buf)[~ins] == s_).all()), f"{c['name']}: an emit store outside [M, N]"
    if ws is not None:
        assert int(ws[:16384].view(torch.int32).abs().max()) == 0          # split-K counters left clean
    print(rep.line())
