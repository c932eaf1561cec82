"""ga_attention_short_bf16 on the GPU, every case of tests/_short_attention_cases.py, checked ELEMENT-WISE against a float64 reference
computed from the exact bf16 / fp32 values the kernel reads, with the error model of tests/_bounds.py for one key group (method and
helpers of tests/test_attention_instances_gpu.py; tests/test_t23d_cpu.py confirms on the CPU that a one-pass softmax with the true row
maximum lies inside that bound on every one of these cases, and that seeded bugs land over it).  No case is skipped or sampled.

Around every call, as there: the output is a view into a sentinel-filled buffer whose every element outside [B Lq, H 64] must come back
bit-identical; q, k, A rows are slices of wider rows whose other columns hold NaN, followed by NaN rows; V^T rows have vt_ld at its
minimum or 64 beyond it with zero pad columns, followed by a NaN row; norm weights, the projection weight and the row sums of squares are
followed by NaN.  A second launch gives the same bits, and so does the other layout of the projection weight."""
import ctypes
import zlib

import pytest
import torch

from tests import _attention_cases as ac
from tests import _short_attention_cases as sc
from tests.test_attention_instances_gpu import BF16_NAN, BF16_SENTINEL, _f32_tail, _fill, _padded

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", sc.CASES, ids=[c["name"] for c in sc.CASES])
def test_short_attention_elementwise_against_float64(gpu_device, case):
    from gaussiananything_amd import dit_ops as ops
    dev, c = gpu_device, case
    B, H, Lq, Lk, d, qp = c["B"], c["H"], c["Lq"], c["Lk"], c["d"], c["qp"]
    seed = zlib.crc32(c["name"].encode())
    z = {n: t.to(dev) for n, t in ac.inputs(c).items()}
    D, Lp = H * d, (Lk + 63) // 64 * 64
    strides = dict(q_stride=D + 8 * (1 + seed % 3), k_stride=D + 16, v_stride=D + 8, vt_ld=Lp + (64 if seed % 2 else 0),
                   out_stride=D + (4 if seed % 2 else 8), qp_lda=(qp["K"] + 8) if qp else 0)
    bufs = {"k": _padded(z["k"].reshape(B * Lk, D), 2, strides["k_stride"], dev),
            "wq": _f32_tail(z["wq"], 4, dev), "wk": _f32_tail(z["wk"], 4, dev)}
    if "q" in z:
        bufs["q"] = _padded(z["q"].reshape(B * Lq, D), 2, strides["q_stride"], dev)
    bufs["vt"] = _padded(z["v"].permute(0, 2, 3, 1).reshape(B * D, Lk), 1, strides["vt_ld"], dev, 0)     # zero pad columns, a NaN row behind
    bufs["vt"][B * D:] = float("nan")
    if qp:
        K = qp["K"]
        bufs["A"] = _padded(z["A"], 2, strides["qp_lda"], dev)
        bufs["W_rows"] = _padded(z["W"], 8, K, dev)
        bufs["W_tiled"] = _fill(((D + 8) * K,), BF16_NAN, dev)
        bufs["W_tiled"][:D * K] = ops.tile_weight(z["W"].to(torch.bfloat16))
        if qp["row_ss"]:
            bufs["row_ss"] = torch.cat([z["row_ss"].float(), torch.full((1, z["row_ss"].shape[1]), float("nan"), device=dev)])
    out_init = _fill((B * Lq + 2, strides["out_stride"]), BF16_SENTINEL, dev)

    def launch(tiled):
        out = out_init.clone()
        ptrs = {n: t.data_ptr() for n, t in bufs.items()}
        ptrs["out"] = out[1:].data_ptr()
        ptrs["W"] = ptrs.get("W_tiled" if tiled else "W_rows")
        args = ac.make_args(dict(c, qp=dict(qp, tiled=tiled)) if qp else c, ptrs.get, strides)
        plan = ops.attention_short_plan(args)
        ops.check(ops.lib().ga_attention_short_bf16(ctypes.byref(args), ops._stream(out)), "ga_attention_short_bf16")
        torch.cuda.synchronize()
        return plan, out

    plan, out = launch(bool(qp and qp["tiled"]))
    assert (plan.queries_per_wg, plan.key_tiles, plan.fuses_q) == (64, (Lk + 63) // 64, 1 if qp else 0)
    assert (plan.grid_x, plan.grid_y, plan.grid_z) == (H * B, (Lq + 63) // 64, 1)
    for again in [launch(bool(qp and qp["tiled"]))] + ([launch(not qp["tiled"])] if qp else []):
        assert torch.equal(out.view(torch.int16), again[1].view(torch.int16)), f"{c['name']}: not bit-identical to the first launch"
    inside = torch.zeros(out.shape, dtype=torch.bool, device=dev)
    inside[1:B * Lq + 1, :D] = True
    assert bool((out.view(torch.int16)[~inside] == BF16_SENTINEL).all()), f"{c['name']}: a store outside [B Lq, H d] of the output"
    got = out[1:B * Lq + 1, :D].reshape(B, Lq, D)
    assert bool(torch.isfinite(got.float()).all()), f"{c['name']}: {int((~torch.isfinite(got.float())).sum())} non-finite outputs (a pad value leaked in)"
    # float64 reference and bound, element-wise; for the failure message: the walk as a plan of the long-list kernel would describe it
    # (four query waves, one key group, both tiles in one stage)
    ref, bound, dom = ac.reference(c, z, groups=1, dev=dev)
    as_fwd = ops.GaAttentionPlan(4, 1, 0, 2, plan.queries_per_wg, plan.fuses_q, plan.grid_x, plan.grid_y, plan.grid_z, plan.lds_bytes)
    worst = ac.assert_within_bound(c["name"], got, ref, bound, dom, as_fwd, H, d)
    print(f"SHORTCASE {c['name']:44s} tiles={plan.key_tiles} qproj={plan.fuses_q} grid={plan.grid_x}x{plan.grid_y} | out {worst:.3f}")
