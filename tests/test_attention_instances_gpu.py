"""Every case of tests/_attention_cases.py -- together they reach every kernel instance the attention dispatchers can launch, at every
key / query geometry the instances distinguish, with input families designed so that a wrong key, mask, fragment column, rescale or
merge weight is an O(1) error on named elements -- on the GPU, checked ELEMENT-WISE against a float64 reference computed from the exact
bf16 / fp32 values the kernel reads, with the error model of tests/_bounds.py (no fudge factor: an element over its bound is a kernel
bug or a rounding the model is missing; tests/test_attention_bounds_cpu.py shows that seeded kernel bugs do land over it).

Around every call, through the C ABI so that strides are free: the output is a view into a sentinel-filled buffer (a row in front, a row
behind, out_stride > H d) whose every element outside [B Lq, H d] must come back bit-identical; q, k (and v, A) rows are slices of wider
rows whose other columns hold NaN, followed by NaN rows; V^T rows have vt_ld at its minimum or 64 beyond it, pad columns zero for
ga_attention_bf16 and a large finite value for ga_attention_hd_bf16 (their contracts, include/ga_dit.h), followed by a NaN row; norm
weights, the projection weight and the row sums of squares are followed by NaN.  No stored element may depend on any of them.  A second
launch gives the same bits, and so does the other layout of the projection weight."""
import ctypes
import math
import zlib

import pytest
import torch

from tests import _attention_cases as ac

pytestmark = pytest.mark.gpu

BF16_SENTINEL, BF16_NAN = 0x7FA5, 0x7FC0       # (the sentinel: a NaN payload no kernel produces)


def _fill(shape, bits, dev):
    return torch.full(shape, bits, dtype=torch.int16, device=dev).view(torch.bfloat16)


def _padded(x, rows_behind, width, dev, pad_bits=BF16_NAN):
    """bf16 buffer [rows + rows_behind, width] of pad_bits with x [rows, cols] in its top left corner"""
    buf = _fill((x.shape[0] + rows_behind, width), pad_bits, dev)
    buf[:x.shape[0], :x.shape[1]] = x.to(torch.bfloat16)
    return buf


def _f32_tail(x, n, dev):
    buf = torch.full((x.numel() + n,), math.nan, device=dev)
    buf[:x.numel()] = x.float()
    return buf


@pytest.mark.parametrize("case", ac.CASES, ids=[c["name"] for c in ac.CASES])
def test_attention_instance_elementwise_against_float64(gpu_device, case):
    from gaussiananything_amd import dit_ops as ops
    dev, c = gpu_device, case
    B, H, Lq, Lk, d, kind, qp = c["B"], c["H"], c["Lq"], c["Lk"], c["d"], c["kind"], c["qp"]
    seed = zlib.crc32(c["name"].encode())
    z = {n: t.to(dev) for n, t in ac.inputs(c).items()}
    D, Lp = H * d, (Lk + 63) // 64 * 64
    # ---- operands, each padded with / followed by values no stored element may depend on
    strides = dict(q_stride=D + 8 * (1 + seed % 3), k_stride=D + 16, v_stride=D + 8, vt_ld=Lp + (64 if seed % 2 else 0),
                   out_stride=D + (4 if seed % 2 else 8), qp_lda=(qp["K"] + 8) if qp else 0)
    bufs = {"k": _padded(z["k"].reshape(B * Lk, D), 2, strides["k_stride"], dev),
            "wq": _f32_tail(z["wq"], 4, dev), "wk": _f32_tail(z["wk"], 4, dev)}
    if "q" in z:
        bufs["q"] = _padded(z["q"].reshape(B * Lq, D), 2, strides["q_stride"], dev)
    if kind == "hd":
        bufs["v"] = _padded(z["v"].reshape(B * Lk, D), 2, strides["v_stride"], dev)
    else:
        # V^T rows (b, h, dim) x keys; pad columns: zero (ga_attention_bf16) / a large finite value (ga_attention_hd_bf16); a NaN row behind
        pad = torch.zeros((), dtype=torch.bfloat16) if kind == "fwd" else torch.tensor(1e30, dtype=torch.bfloat16)
        bufs["vt"] = _padded(z["v"].permute(0, 2, 3, 1).reshape(B * D, Lk), 1, strides["vt_ld"], dev, int(pad.view(torch.int16)))
        bufs["vt"][B * D:] = math.nan
    if qp:
        K = qp["K"]
        bufs["A"] = _padded(z["A"], 2, strides["qp_lda"], dev)
        bufs["W_rows"] = _padded(z["W"], 8, K, dev)
        bufs["W_tiled"] = _fill(((D + 8) * K,), BF16_NAN, dev)
        bufs["W_tiled"][:D * K] = ops.tile_weight(z["W"].to(torch.bfloat16))
        if qp["row_ss"]:
            bufs["row_ss"] = torch.cat([z["row_ss"].float(), torch.full((1, z["row_ss"].shape[1]), math.nan, device=dev)])
    out_init = _fill((B * Lq + 2, strides["out_stride"]), BF16_SENTINEL, dev)

    def launch(tiled):
        out = out_init.clone()
        ptrs = {n: t.data_ptr() for n, t in bufs.items()}
        ptrs["out"] = out[1:].data_ptr()
        ptrs["W"] = ptrs.get("W_tiled" if tiled else "W_rows")
        if qp:
            cc = dict(c, qp=dict(qp, tiled=tiled))
        else:
            cc = c
        args = ac.make_args(cc, ptrs.get, strides)
        if kind == "fwd":
            plan = ops.attention_plan(args)
            ops.check(ops.lib().ga_attention_bf16(ctypes.byref(args), ops._stream(out)), "ga_attention_bf16")
        else:
            plan = ops.attention_hd_plan(args)
            ops.check(ops.lib().ga_attention_hd_bf16(ctypes.byref(args), ops._stream(out)), "ga_attention_hd_bf16")
        torch.cuda.synchronize()
        return plan, out

    plan, out = launch(bool(qp and qp["tiled"]))
    fields = lambda p: tuple(getattr(p, n) for n, _ in p._fields_)          # noqa: E731
    assert fields(plan) == fields(ac.plan_of(c)[0]), "the launch's plan is not the plan the CPU coverage test saw"
    # ---- bit checks: a second launch, and the other layout of the projection weight
    for again in [launch(bool(qp and qp["tiled"]))] + ([launch(not qp["tiled"])] if qp else []):
        assert torch.equal(out.view(torch.int16), again[1].view(torch.int16)), f"{c['name']}: not bit-identical to the first launch"
    # ---- sentinels outside the written region
    inside = torch.zeros(out.shape, dtype=torch.bool, device=dev)
    inside[1:B * Lq + 1, :D] = True
    assert bool((out.view(torch.int16)[~inside] == BF16_SENTINEL).all()), f"{c['name']}: a store outside [B Lq, H d] of the output"
    got = out[1:B * Lq + 1, :D].reshape(B, Lq, D)
    assert bool(torch.isfinite(got.float()).all()), f"{c['name']}: {int((~torch.isfinite(got.float())).sum())} non-finite outputs (a pad value leaked in)"
    # ---- float64 reference and bound, element-wise
    ref, bound, dom = ac.reference(c, z, groups=plan.ks, dev=dev)
    worst = ac.assert_within_bound(c["name"], got, ref, bound, dom, plan, H, d)
    print(f"ATTNCASE {c['name']:44s} {ac.describe(plan)} | out {worst:.3f}")
