"""Every case of tests/_row_cases.py -- the row kernels with a C-ABI entry of their own (rmsnorm_modulate, small_linear, shift_bias,
layernorm_modulate, tiny_mlp_silu, assemble_tokens, tiny_attention, surfel_head) at the shapes, branches and input families where they
can go wrong -- on the GPU, checked ELEMENT-WISE against a float64 reference computed from the exact bf16 / fp32 values the kernel
reads, with the error model of tests/_bounds.py (no fudge factor and no outlier allowance: an element over its bound is a kernel bug or
a rounding the model is missing; tests/test_row_bounds_cpu.py shows that seeded kernel bugs do land over it).

Around every call, through the C ABI so that strides and optional pointers are free: every output is a view into a sentinel-filled
buffer with a row in front and a row behind, which must come back bit-identical (x of rmsnorm_modulate too: unchanged without row_bias,
exactly fp32 x + row_bias on the rows >= row_bias_first with it); every input array is followed by NaN, the strided ones (the
modulation rows of a [B, 6, D] table, the shift rows of shift_bias) lie between NaN rows / columns; no stored element may be
non-finite.  A second launch gives the same bits, and so does the other layout of the shift_bias weight."""
import ctypes
import math

import pytest
import torch

from tests import _row_cases as rc

pytestmark = pytest.mark.gpu

BF16_SENTINEL, F32_SENTINEL = 0x7FA5, 0x7FA5A5A5       # NaN payloads no kernel produces
OK, ERR_NULL_ARG, ERR_BAD_SHAPE = 0, -1, -2
BF16, F32 = torch.bfloat16, torch.float32


def _sentinel(rows, cols, dtype, dev):
    """[rows + 2, cols] of sentinel bits: the kernel gets the address of row 1"""
    if dtype == BF16:
        return torch.full((rows + 2, cols), BF16_SENTINEL, dtype=torch.int16, device=dev).view(BF16)
    return torch.full((rows + 2, cols), F32_SENTINEL, dtype=torch.int32, device=dev).view(F32)


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _tail(x, dtype, dev, n=16):
    """x flattened, followed by n NaN elements"""
    buf = torch.full((x.numel() + n,), math.nan, dtype=dtype, device=dev)
    buf[:x.numel()] = x.reshape(-1).to(dtype)
    return buf


def _table(t, dev):
    """a [B, 6, D] modulation table whose rows other than 0 (shift) and 1 (scale) hold NaN, followed by a NaN item"""
    B, _, D = t.shape
    buf = torch.full((B + 1, 6, D), math.nan, dtype=F32, device=dev)
    buf[:B, :2] = t[:, :2].to(F32)
    return buf


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


# Each runner: (case, z, dev, variant) -> (rc, {output name: sentinel buffer}); inputs are rebuilt for every launch (x of rmsnorm_modulate
# is written in place).  `keep` holds the device tensors until the launch has finished.
def _run_rmsnorm_modulate(c, z, dev, variant=0):
    from gaussiananything_amd import dit_ops as ops
    M, D = c["M"], c["D"]
    x = _sentinel(M, D, F32, dev)
    x[1:M + 1] = z["x"].to(F32)
    out = _sentinel(M, D, BF16, dev)
    keep = [_tail(z["weight"], F32, dev), _tail(z["row_bias"], F32, dev)]
    scale = shift = None
    stride = 0
    if c["mod"] == "table":
        keep.append(_table(z["table"], dev))
        scale, shift, stride = keep[-1][:, 1], keep[-1][:, 0], 6 * D
    elif c["mod"] == "contig":
        keep += [_tail(z["table"][:, 1], F32, dev), _tail(z["table"][:, 0], F32, dev)]
        scale, shift, stride = keep[-2], keep[-1], D
    a = ops.GaRmsNormArgs(M, D, c["rpb"], x[1:].data_ptr(), keep[0].data_ptr(), _ptr(scale), _ptr(shift), stride, out[1:].data_ptr(),
                          keep[1].data_ptr() if c["first"] is not None else None, c["first"] or 0)
    r = ops.lib().ga_rmsnorm_modulate(ctypes.byref(a), _stream(dev))
    torch.cuda.synchronize()
    return r, {"out": out, "x": x}


def _run_small_linear(c, z, dev, variant=0):
    from gaussiananything_amd import dit_ops as ops
    B, N, K = c["B"], c["N"], c["K"]
    y = _sentinel(B, N, F32, dev)
    keep = [_tail(z["x"], F32, dev), _tail(z["W"], BF16, dev), _tail(z["bias"], F32, dev), _tail(z["add"], F32, dev)]
    a = ops.GaSmallLinearArgs(B, N, K, c["act_in"], c["act_out"], keep[0].data_ptr(), keep[1].data_ptr(),
                              keep[2].data_ptr() if c["bias"] else None, keep[3].data_ptr() if c["add"] else None, y[1:].data_ptr())
    r = ops.lib().ga_small_linear(ctypes.byref(a), _stream(dev))
    torch.cuda.synchronize()
    return r, {"y": y}


def _run_shift_bias(c, z, dev, variant=0):
    """variant 0: the layout the case index picks, 1: the other one"""
    from gaussiananything_amd import dit_ops as ops
    B, N, K = c["batch"], c["N"], c["K"]
    tiled = (c["bias"] + variant) % 2
    W = z["W"].to(BF16)
    Wb = _tail(ops.tile_weight(W) if tiled else W, BF16, dev)
    out = _sentinel(B, N, F32, dev)
    stride = K + 8                                                       # the shift rows as a strided view: NaN columns behind each row
    sh = torch.full((B + 1, stride), math.nan, dtype=F32, device=dev)
    sh[:B, :K] = z["shift"].to(F32)
    bias = _tail(z["bias"], F32, dev)
    r = ops.lib().ga_dit_shift_bias(Wb.data_ptr(), tiled, bias.data_ptr() if c["bias"] else None, N, K, sh.data_ptr(), stride, B,
                                    out[1:].data_ptr(), _stream(dev))
    torch.cuda.synchronize()
    return r, {"out": out}


def _run_layernorm_modulate(c, z, dev, variant=0):
    from gaussiananything_amd import decode_ops as dec
    M, D = c["M"], c["D"]
    out = _sentinel(M, D, BF16, dev)
    keep = [_tail(z["x"], F32, dev), _tail(z["weight"], F32, dev), _tail(z["bias"], F32, dev), _table(z["table"], dev)]
    aff, mod = c["affine"], c["mod"]
    a = dec.GaLayerNormArgs(M, D, c["eps"], keep[0].data_ptr(), keep[1].data_ptr() if aff else None, keep[2].data_ptr() if aff else None,
                            keep[3][:, 1].data_ptr() if mod else None, keep[3][:, 0].data_ptr() if mod else None, 6 * D if mod else 0,
                            out[1:].data_ptr())
    r = dec.lib().ga_layernorm_modulate(ctypes.byref(a), _stream(dev))
    torch.cuda.synchronize()
    return r, {"out": out}


def _run_tiny_mlp_silu(c, z, dev, variant=0):
    from gaussiananything_amd import decode_ops as dec
    M, D = c["M"], c["D"]
    out = _sentinel(M, D, BF16, dev)
    keep = [_tail(z[n], F32, dev) for n in ("x", "w1", "b1", "w2", "b2")]
    a = dec.GaTinyMlpArgs(M, c["Cin"], c["Ch"], D, *[t.data_ptr() for t in keep], out[1:].data_ptr())
    r = dec.lib().ga_tiny_mlp_silu(ctypes.byref(a), _stream(dev))
    torch.cuda.synchronize()
    return r, {"out": out}


def _run_assemble_tokens(c, z, dev, variant=0):
    from gaussiananything_amd import decode_ops as dec
    P, D, f = c["P"], c["D"], c["f"]
    out = _sentinel(P * (1 + f), D, F32, dev)
    keep = [_tail(z["src"], F32, dev), _tail(z["latent_embedding"], F32, dev)]
    a = dec.GaAssembleArgs(P, f, D, c["src_f"], keep[0].data_ptr(), keep[1].data_ptr(), out[1:].data_ptr())
    r = dec.lib().ga_assemble_tokens(ctypes.byref(a), _stream(dev))
    torch.cuda.synchronize()
    return r, {"out": out}


def _run_tiny_attention(c, z, dev, variant=0):
    from gaussiananything_amd import decode_ops as dec
    S, groups, H = c["S"], c["groups"], c["heads"]
    out = _sentinel(groups * S, H * 64, BF16, dev)
    qkv = _tail(z["qkv"], BF16, dev, n=3 * H * 64)                       # a NaN row behind the last group
    a = dec.GaTinyAttentionArgs(groups, S, H, qkv.data_ptr(), out[1:].data_ptr())
    r = dec.lib().ga_tiny_attention(ctypes.byref(a), _stream(dev))
    torch.cuda.synchronize()
    return r, {"out": out}


def _run_surfel_head(c, z, dev, variant=0):
    from gaussiananything_amd import decode_ops as dec
    rows, D, mode = c["rows"], c["D"], c["mode"]
    g, pre = _sentinel(rows, 13, F32, dev), _sentinel(rows, 13, F32, dev)
    k = {n: _tail(z[n], F32, dev) for n in ("x", "ln_weight", "ln_bias", "w", "b", "anchor", "base_pre")}
    a = dec.GaSurfelHeadArgs(rows, D, mode, c["f"], k["x"].data_ptr(), k["ln_weight"].data_ptr() if mode else None,
                             k["ln_bias"].data_ptr() if mode else None, k["w"].data_ptr(), k["b"].data_ptr(), k["anchor"].data_ptr(),
                             k["base_pre"].data_ptr() if mode else None, rc.SKIP_WEIGHT, g[1:].data_ptr(), pre[1:].data_ptr())
    r = dec.lib().ga_surfel_head(ctypes.byref(a), _stream(dev))
    torch.cuda.synchronize()
    return r, {"gaussians": g, "pre_out": pre}


RUN = {"rmsnorm_modulate": _run_rmsnorm_modulate, "small_linear": _run_small_linear, "shift_bias": _run_shift_bias,
       "layernorm_modulate": _run_layernorm_modulate, "tiny_mlp_silu": _run_tiny_mlp_silu, "assemble_tokens": _run_assemble_tokens,
       "tiny_attention": _run_tiny_attention, "surfel_head": _run_surfel_head}


@pytest.mark.parametrize("case", rc.ALL, ids=[c["name"] for c in rc.ALL])
def test_row_kernel_elementwise_against_float64(gpu_device, case):
    dev, c = gpu_device, case
    z = rc.inputs(c)
    refs = rc.reference(c, z)                                            # (asserts the caps of the case before anything is launched)
    run = RUN[c["kernel"]]
    r, outs = run(c, z, dev)
    assert r == OK, f"{c['name']}: the entry point returned {r}"
    # ---- bit checks: a second launch, and the other layout of the shift_bias weight
    for variant in (0, 1) if c["kernel"] == "shift_bias" else (0,):
        r2, again = run(c, z, dev, variant)
        assert r2 == OK
        for n in outs:
            assert torch.equal(_bits(outs[n]), _bits(again[n])), f"{c['name']}: {n} not bit-identical to the first launch (variant {variant})"
    worst = {}
    for n, (ref, bound) in refs.items():
        buf, rows = outs[n], ref.shape[0]
        sent = BF16_SENTINEL if buf.dtype == BF16 else F32_SENTINEL
        # ---- sentinels in front of and behind the written rows
        assert bool((_bits(buf[0]) == sent).all()) and bool((_bits(buf[rows + 1]) == sent).all()), f"{c['name']}: a store outside {n}"
        got = buf[1:rows + 1].to(torch.float64).cpu()
        assert bool(torch.isfinite(got).all()), f"{c['name']}: {int((~torch.isfinite(got)).sum())} non-finite elements of {n} (a pad value leaked in)"
        # ---- float64 reference and bound, element-wise
        worst[n] = rc.worst_ratio(got, ref, bound)
        if worst[n] > 1.0:
            ratio = torch.where(got == ref, torch.zeros_like(ref), (got - ref).abs() / bound)
            i = int(ratio.argmax())
            idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
            pytest.fail(f"{c['name']}: {int((ratio > 1).sum())} of {ratio.numel()} elements of {n} over their bound; worst at {idx}: got "
                        f"{float(got[idx]):.9g}, ref {float(ref[idx]):.9g}, bound {float(bound[idx]):.3g} ({worst[n]:.3g} x)")
    print(f"ROWCASE {c['name']:72s} | " + ", ".join(f"{n} {v:.3f}" for n, v in worst.items()))


def test_entry_points_refuse_what_the_kernels_cannot_run(gpu_device):
    """each refused shape returns its error code and leaves the sentinel output untouched (the buffers are large enough for the shape
    had it been launched)"""
    from gaussiananything_amd import decode_ops as dec
    from gaussiananything_amd import dit_ops as ops
    dev = gpu_device
    n = 1 << 18
    f = torch.zeros(n, dtype=F32, device=dev)
    h = torch.zeros(n, dtype=BF16, device=dev)
    out32, out16 = _sentinel(0, n, F32, dev), _sentinel(0, n, BF16, dev)
    fp, hp, o32, o16 = f.data_ptr(), h.data_ptr(), out32.data_ptr(), out16.data_ptr()
    L, st = dec.lib(), _stream(dev)
    refused = []

    def rms(D, scale=None, shift=None):
        return L.ga_rmsnorm_modulate(ctypes.byref(ops.GaRmsNormArgs(4, D, 1, fp, fp, scale, shift, D, o16, None, 0)), st)

    def ln(D, weight=None, bias=None, scale=None, shift=None):
        return L.ga_layernorm_modulate(ctypes.byref(dec.GaLayerNormArgs(4, D, 1e-5, fp, weight, bias, scale, shift, D, o16)), st)

    def sl(B, K, act_in=0):
        return L.ga_small_linear(ctypes.byref(ops.GaSmallLinearArgs(B, 8, K, act_in, 0, fp, hp, None, None, o32)), st)

    def sb(N, K):
        return L.ga_dit_shift_bias(hp, 0, None, N, K, fp, K, 2, o32, st)

    def head(D):
        return L.ga_surfel_head(ctypes.byref(dec.GaSurfelHeadArgs(4, D, 0, 1, fp, None, None, fp, fp, fp, None, 0.5, o32, o32)), st)

    refused += [("rmsnorm D % 4", rms(6), ERR_BAD_SHAPE), ("rmsnorm D > 2048", rms(2052), ERR_BAD_SHAPE),
                ("rmsnorm scale without shift", rms(64, scale=fp), ERR_BAD_SHAPE), ("rmsnorm shift without scale", rms(64, shift=fp), ERR_BAD_SHAPE),
                ("layernorm D % 4", ln(6), ERR_BAD_SHAPE), ("layernorm D > 2048", ln(2052), ERR_BAD_SHAPE),
                ("layernorm weight without bias", ln(64, weight=fp), ERR_NULL_ARG), ("layernorm bias without weight", ln(64, bias=fp), ERR_NULL_ARG),
                ("layernorm scale without shift", ln(64, scale=fp), ERR_NULL_ARG), ("layernorm shift without scale", ln(64, shift=fp), ERR_NULL_ARG),
                ("small_linear B > 16", sl(17, 64), ERR_BAD_SHAPE), ("small_linear K % 8", sl(4, 12), ERR_BAD_SHAPE),
                ("small_linear act_in 2 with K != 256", sl(4, 264, act_in=2), ERR_BAD_SHAPE),
                ("shift_bias N % 8", sb(12, 64), ERR_BAD_SHAPE), ("shift_bias K % 64", sb(8, 96), ERR_BAD_SHAPE),
                ("tiny_attention S > 16", L.ga_tiny_attention(ctypes.byref(dec.GaTinyAttentionArgs(1, 17, 1, hp, o16)), st), ERR_BAD_SHAPE),
                ("surfel_head D % 4", head(6), ERR_BAD_SHAPE), ("surfel_head D > 2048", head(2052), ERR_BAD_SHAPE),
                ("assemble_tokens D % 4", L.ga_assemble_tokens(ctypes.byref(dec.GaAssembleArgs(4, 1, 6, 0, fp, fp, o32)), st), ERR_BAD_SHAPE)]
    torch.cuda.synchronize()
    for what, got, want in refused:
        assert got == want, f"{what}: returned {got}, expected {want}"
    assert bool((_bits(out32) == F32_SENTINEL).all()) and bool((_bits(out16) == BF16_SENTINEL).all()), "a refused call wrote to its output"
