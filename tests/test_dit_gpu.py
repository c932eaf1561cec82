"""GPU parity of the HIP DiT path (through the C-ABI) against (i) plain PyTorch fp32 references of each op and
(ii) the golden vectors produced by the REFERENCE'S OWN model code (tests/golden/dit_ref_stage*.pt).

Tolerances (bf16 MFMA inputs, fp32 accumulation, fp32 residual stream; the reference itself runs under bf16 autocast):
  per-op      : relative L2 error <= 1e-2 against an fp32 reference fed the same bf16-rounded inputs
  whole model : relative L2 error <= 1.5e-2 against the reference's fp32 output (3e-2 behind classifier-free guidance, which
                amplifies the difference by its scale; measured 5e-3 .. 6e-3), max abs error <= 5e-2 * max|y|
"""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (200, 384, 128), (1536, 1024, 1024), (77, 260, 192),
                                   # K a multiple of 192 but not of 256 (DiT-PixArt-PCD-CLAY-XL: width 1152): the three-slot ring, all four tiles
                                   (1536, 3456, 1152), (1536, 1152, 4608), (768, 1152, 1152), (768, 4608, 1152), (200, 136, 384),
                                   # CFG batch 4 (the release's stage-1 script): 3072 rows
                                   (3072, 1024, 1024), (3072, 1024, 4096)])
def test_gemm_epilogues(gpu_device, M, N, K):
    from gaussiananything_amd import dit_ops as ops
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g).to(gpu_device).bfloat16()
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(gpu_device).bfloat16()
    bias = torch.randn(N, generator=g).to(gpu_device)
    ref = A.float() @ W.float().T + bias
    out = ops.gemm(A, W, bias, ops.EPI_STORE_BF16)
    assert rel_l2(out.float(), ref) < 1e-2
    out = ops.gemm(A, W, bias, ops.EPI_GELU_BF16)
    assert rel_l2(out.float(), torch.nn.functional.gelu(ref)) < 1e-2
    out = ops.gemm(A, W, None, ops.EPI_STORE_F32)
    assert rel_l2(out, A.float() @ W.float().T) < 1e-3           # fp32 store: only accumulation order differs
    rows = 8 if M % 8 == 0 else 7 if M % 7 == 0 else 1
    x0 = torch.randn(M, N, generator=g).to(gpu_device)
    gate = torch.randn(M // rows, 6 * N, generator=g).to(gpu_device)[:, 2 * N:3 * N]
    x = x0.clone()
    ops.gemm(A, W, bias, ops.EPI_RESIDUAL, out=x, gate=gate, rows_per_batch=rows)
    ref_x = x0 + gate.repeat_interleave(rows, 0) * ref
    assert rel_l2(x, ref_x) < 1e-3
    x = x0.clone()
    ops.gemm(A, W, bias, ops.EPI_RESIDUAL, out=x)
    assert rel_l2(x, x0 + ref) < 1e-3


def test_gemm_transposed_v_store(gpu_device):
    """The QKV projection writes q|k row-major and V transposed per (batch, head): [B*H*64, Lpad]."""
    from gaussiananything_amd import dit_ops as ops
    B, L, H, K = 2, 96, 2, 128
    D = H * 64
    g = torch.Generator(device="cpu").manual_seed(9)
    A = torch.randn(B * L, K, generator=g).to(gpu_device).bfloat16()
    W = (torch.randn(3 * D, K, generator=g) / 11).to(gpu_device).bfloat16()
    bias = torch.randn(3 * D, generator=g).to(gpu_device)
    Lp = 128
    vt = torch.zeros(B * D, Lp, device=gpu_device, dtype=torch.bfloat16)
    out = ops.gemm(A, W, bias, ops.EPI_STORE_BF16, rows_per_batch=L, vt=vt, vt_col0=2 * D)
    ref = (A.float() @ W.float().T + bias)
    assert out.shape == (B * L, 2 * D) and rel_l2(out.float(), ref[:, :2 * D]) < 1e-2
    vref = ref[:, 2 * D:].reshape(B, L, H, 64).permute(0, 2, 3, 1).reshape(B * D, L)
    assert rel_l2(vt[:, :L].float(), vref) < 1e-2
    assert float(vt[:, L:].abs().max()) == 0.0


def test_gemm_fused_qk_rmsnorm(gpu_device):
    """Per-head RMSNorm of the q and k column groups in the projection epilogue (dit/norm.py:29-43 semantics)."""
    from gaussiananything_amd import dit_ops as ops
    M, K, H = 200, 128, 3
    D = H * 64
    g = torch.Generator(device="cpu").manual_seed(21)
    A = torch.randn(M, K, generator=g).to(gpu_device).bfloat16()
    W = (torch.randn(3 * D, K, generator=g) / 11).to(gpu_device).bfloat16()
    bias = torch.randn(3 * D, generator=g).to(gpu_device)
    wq = (1 + 0.3 * torch.randn(64, generator=g)).to(gpu_device)
    wk = (1 + 0.3 * torch.randn(64, generator=g)).to(gpu_device)
    out = ops.gemm(A, W, bias, ops.EPI_STORE_BF16, qk_w0=wq, qk_cols0=D, qk_w1=wk, qk_cols1=2 * D)
    ref = (A.float() @ W.float().T + bias).reshape(M, 3, H, 64)
    nrm = lambda t, w: t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + 1e-5) * w  # noqa: E731
    ref = torch.stack([nrm(ref[:, 0], wq), nrm(ref[:, 1], wk), ref[:, 2]], 1).reshape(M, 3 * D)
    assert rel_l2(out.float(), ref) < 1e-2


@pytest.mark.parametrize("M,H,K,L", [(768, 16, 1024, 768), (1536, 16, 1024, 768), (1536, 12, 768, 768), (400, 4, 512, 200)])
def test_qkv_projection_with_head_norm_and_transposed_v_on_every_tile(gpu_device, M, H, K, L):
    """The QKV projection as the DiT calls it -- per-head RMSNorm of q and k, V stored transposed -- at the shapes that pick the
    96 x 64 tile (32-column waves: the head's sum of squares is exchanged between two waves through LDS; M = 768 of DiT-L,
    M = 1536 of DiT-B), the 192 x 128 tile (M = 1536 of DiT-L) and the 64 x 64 one."""
    from gaussiananything_amd import dit_ops as ops
    D = H * 64
    g = torch.Generator(device="cpu").manual_seed(M + H)
    A = torch.randn(M, K, generator=g).to(gpu_device).bfloat16()
    W = (torch.randn(3 * D, K, generator=g) / math.sqrt(K)).to(gpu_device).bfloat16()
    bias = torch.randn(3 * D, generator=g).to(gpu_device)
    wq = (1 + 0.3 * torch.randn(64, generator=g)).to(gpu_device)
    wk = (1 + 0.3 * torch.randn(64, generator=g)).to(gpu_device)
    B = M // L
    Lp = (L + 63) // 64 * 64
    vt = torch.zeros(B * D, Lp, device=gpu_device, dtype=torch.bfloat16)
    out = ops.gemm(A, W, bias, ops.EPI_STORE_BF16, rows_per_batch=L, vt=vt, vt_col0=2 * D, qk_w0=wq, qk_cols0=D, qk_w1=wk, qk_cols1=2 * D)
    ref = (A.float() @ W.float().T + bias).reshape(M, 3, H, 64)
    nrm = lambda t, w: t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + 1e-5) * w  # noqa: E731
    qk = torch.stack([nrm(ref[:, 0], wq), nrm(ref[:, 1], wk)], 1).reshape(M, 2 * D)
    assert out.shape == (M, 2 * D) and rel_l2(out.float(), qk) < 1e-2
    for h in (0, H - 1):     # no head's columns ended up under another head's norm
        assert rel_l2(out[:, h * 64:(h + 1) * 64].float(), qk[:, h * 64:(h + 1) * 64]) < 1e-2
    vref = ref[:, 2].reshape(B, L, H, 64).permute(0, 2, 3, 1).reshape(B * D, L)
    assert rel_l2(vt[:, :L].float(), vref) < 1e-2
    assert L == Lp or float(vt[:, L:].abs().max()) == 0.0


def test_gemm_transposed_v_store_is_width_generic(gpu_device):
    """Round 6: the same V^T store for heads of 72 (width 1152 = 18 column groups of 64, heads straddle them): row b*D + c of the image is
    column c of item b's V, whatever the head dim -- what ga_attention_hd_bf16's tuned variant reads."""
    from gaussiananything_amd import dit_ops as ops
    B, L, D, K = 2, 768, 1152, 1152
    g = torch.Generator(device="cpu").manual_seed(19)
    A = torch.randn(B * L, K, generator=g).to(gpu_device).bfloat16()
    W = (torch.randn(3 * D, K, generator=g) / 34).to(gpu_device).bfloat16()
    bias = torch.randn(3 * D, generator=g).to(gpu_device)
    vt = torch.zeros(B * D, L, device=gpu_device, dtype=torch.bfloat16)
    out = ops.gemm(A, W, bias, ops.EPI_STORE_BF16, rows_per_batch=L, vt=vt, vt_col0=2 * D)
    ref = (A.float() @ W.float().T + bias)
    assert out.shape == (B * L, 2 * D) and rel_l2(out.float(), ref[:, :2 * D]) < 1e-2
    assert rel_l2(vt.float(), ref[:, 2 * D:].reshape(B, L, D).permute(0, 2, 1).reshape(B * D, L)) < 1e-2


def test_gemm_is_transpose_sensitive(gpu_device):
    """A = I with an asymmetric W: a swapped row/column mapping in the epilogue cannot pass."""
    from gaussiananything_amd import dit_ops as ops
    K = 128
    A = torch.eye(K, device=gpu_device).bfloat16()
    W = (torch.arange(256 * K, device=gpu_device).reshape(256, K) % 251).float().bfloat16()
    out = ops.gemm(A, W, None, ops.EPI_STORE_F32)
    assert torch.equal(out, W.float().T)


@pytest.mark.parametrize("M,N,K,epi", [(1536, 4096, 1024, "gelu"), (1536, 1024, 4096, "res"), (768, 1024, 1024, "bf16"),
                                       (1536, 3072, 1024, "bf16"), (200, 264, 192, "f32"), (6144, 1024, 1024, "res"),
                                       (1536, 4608, 1152, "gelu"), (1536, 1152, 4608, "res"), (768, 1152, 1152, "bf16"), (768, 3456, 1152, "bf16")])
def test_gemm_tiled_weight_image_gives_the_same_bits(gpu_device, M, N, K, epi):
    """GaGemmArgs.w_tiled (the [N/8][K/64][8][64] image the DiT stores its weights in): only the addresses the LDS-DMA reads
    from change, so every kernel variant (the three ring tiles and the 2-slot kernel of the small shape) must give the
    row-major call's bits."""
    from gaussiananything_amd import dit_ops as ops
    g = torch.Generator(device="cpu").manual_seed(N + K)
    A = torch.randn(M, K, generator=g).to(gpu_device).bfloat16()
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(gpu_device).bfloat16()
    Wt = ops.tile_weight(W)
    assert Wt.numel() == W.numel() and torch.equal(Wt.reshape(N // 8, K // 64, 8, 64)[3, 1, 5], W[3 * 8 + 5, 64:128])
    bias = torch.randn(N, generator=g).to(gpu_device)
    if epi == "res":
        x0 = torch.randn(M, N, generator=g).to(gpu_device)
        a, b = x0.clone(), x0.clone()
        ops.gemm(A, W, bias, ops.EPI_RESIDUAL, out=a)
        ops.gemm(A, Wt, bias, ops.EPI_RESIDUAL, out=b, w_tiled=True, N=N)
    else:
        e = {"gelu": ops.EPI_GELU_BF16, "bf16": ops.EPI_STORE_BF16, "f32": ops.EPI_STORE_F32}[epi]
        a = ops.gemm(A, W, bias if epi != "f32" else None, e)
        b = ops.gemm(A, Wt, bias if epi != "f32" else None, e, w_tiled=True, N=N)
    assert torch.equal(a, b)
    assert rel_l2(a.float(), (x0 if epi == "res" else 0) + (torch.nn.functional.gelu(A.float() @ W.float().T + bias) if epi == "gelu"
                                                              else A.float() @ W.float().T + (0 if epi == "f32" else bias))) < 1e-2


@pytest.mark.parametrize("mode,M,N,K", [(1, 1536, 1024, 4096), (2, 1536, 1024, 4096), (3, 768, 1024, 4096), (3, 1536, 768, 3072),
                                        (1, 1488, 1024, 4096), (2, 100, 264, 1024), (6, 1536, 1024, 4096), (6, 768, 1024, 4096), (-1, 1536, 1024, 4096)])
def test_gemm_deterministic_split_k(gpu_device, mode, M, N, K):
    """GaGemmArgs.splitk_ws (round 6): 2 / 4 workgroups share the reduction of an output tile, the partial tiles are added in split
    order by whichever arrives last.  Against the fp32 product at the per-op bar and against the unsplit kernel (another summation
    order: close, not equal); BIT-identical from launch to launch whatever the arrival order (20 launches, a cold and a warm scratch);
    the tile counters are left zero; with the gated residual, a per-batch emit (folded modulated pre-norm) and ragged edges."""
    from gaussiananything_amd import dit_ops as ops
    g = torch.Generator(device="cpu").manual_seed(M + N + K + mode)
    A = torch.randn(M, K, generator=g).to(gpu_device).bfloat16()
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(gpu_device).bfloat16()
    bias = torch.randn(N, generator=g).to(gpu_device)
    rpb = M // 2 if M % 96 == 0 else M
    gate = torch.randn(M // rpb, N, generator=g).to(gpu_device)
    x0 = torch.randn(M, N, generator=g).to(gpu_device)
    emit = N % 64 == 0
    ew = torch.rand(N, generator=g).to(gpu_device) + 0.5 if emit else None
    es = (torch.randn(M // rpb, N, generator=g) * 0.1).to(gpu_device) if emit else None

    def run(ws):
        x = x0.clone()
        ex = torch.empty(M, N, device=gpu_device, dtype=torch.bfloat16) if emit else None
        ss = torch.empty(M, N // 64, device=gpu_device) if emit else None
        ops.gemm(A, W, bias, ops.EPI_RESIDUAL, out=x, gate=gate, rows_per_batch=rpb, emit_x=ex, emit_ss=ss, emit_w=ew, emit_scale=es, splitk_ws=ws)
        return x, ex, ss
    ref = x0.double() + gate.double().repeat_interleave(rpb, 0) * (A.double() @ W.double().T + bias.double())
    base = run(None)
    prev = ops.splitk_mode(mode)
    try:
        ws = ops.splitk_workspace(M, N, gpu_device)
        first = run(ws)
        for _ in range(20):
            again = run(ws)
            assert all(torch.equal(a, b) for a, b in zip(first, again) if a is not None)
        assert int(ws[:16384].view(torch.int32).abs().max()) == 0          # counters left clean
        if mode > 0:   # the forced configuration really is another kernel: another summation order somewhere
            assert not torch.equal(first[0], base[0])
        else:          # default: split-K is off (measured slower, profiles/r6_splitk.txt) -- a scratch changes nothing
            assert torch.equal(first[0], base[0])
    finally:
        ops.splitk_mode(prev)
    assert rel_l2(first[0], ref) < 1e-2 and rel_l2(first[0], base[0].double()) < 1e-5
    if emit:
        assert rel_l2(first[1].float(), base[1].float()) < 5e-3 and rel_l2(first[2], base[2]) < 1e-5
        want = (ref * (ew.double() * (1 + es.double().repeat_interleave(rpb, 0)))).float()
        assert rel_l2(first[1].float(), want) < 1e-2


@pytest.mark.parametrize("epi,M,N,K,mode", [("qkv", 768, 3072, 1024, 6), ("gelu", 768, 4096, 1024, 6), ("qkv", 1536, 3072, 1024, 4), ("gelu", 384, 520, 1024, 4),
                                            ("res", 3072, 1024, 4096, 6), ("res", 1536, 1024, 4096, 4)])
def test_gemm_split_k_of_two_on_the_wide_tiles(gpu_device, epi, M, N, K, mode):
    """192 x 128 tiles x 2 splits (configuration 4): the only split the bf16-store epilogues have -- qkv with the per-head q/k RMSNorm,
    the V^T store and a folded row scale + per-batch bias, fc1 with GELU -- chosen by shape at 768 rows (and for fc2 at 3072).  Close to
    the unsplit kernels (another summation order), launch-to-launch bit-identical, counters left zero."""
    from gaussiananything_amd import dit_ops as ops
    g = torch.Generator(device="cpu").manual_seed(M + N + K)
    A = torch.randn(M, K, generator=g).to(gpu_device).bfloat16()
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(gpu_device).bfloat16()
    L = 768 if M % 768 == 0 else M
    bias = torch.randn(M // L, N, generator=g).to(gpu_device)                # one bias row per batch item (folded shift)
    rss = (torch.rand(M, K // 64, generator=g) * 64).to(gpu_device)          # row sums of squares per 64-column group

    def run(ws):
        if epi == "qkv":
            H = N // 192
            vt = torch.zeros((M // L) * H * 64, (L + 63) // 64 * 64, device=gpu_device, dtype=torch.bfloat16)
            qw, kw = torch.rand(64, generator=torch.Generator().manual_seed(1)).to(gpu_device) + 0.5, torch.rand(64, generator=torch.Generator().manual_seed(2)).to(gpu_device) + 0.5
            out = ops.gemm(A, W, bias, ops.EPI_STORE_BF16, rows_per_batch=L, vt=vt, vt_col0=2 * H * 64, qk_w0=qw, qk_cols0=H * 64, qk_w1=kw,
                           qk_cols1=2 * H * 64, row_ss=rss, row_ss_dim=K, splitk_ws=ws)
            return out, vt
        if epi == "gelu":
            return (ops.gemm(A, W, bias, ops.EPI_GELU_BF16, rows_per_batch=L, row_ss=rss, row_ss_dim=K, splitk_ws=ws),)
        x = torch.ones(M, N, device=gpu_device)
        ops.gemm(A, W, bias[0].contiguous(), ops.EPI_RESIDUAL, out=x, rows_per_batch=L, splitk_ws=ws)
        return (x,)
    base = run(None)
    prev = ops.splitk_mode(mode)
    try:
        ws = ops.splitk_workspace(M, N, gpu_device)
        first = run(ws)
        for _ in range(10):
            assert all(torch.equal(a, b) for a, b in zip(first, run(ws)))
        assert int(ws[:16384].view(torch.int32).abs().max()) == 0
    finally:
        ops.splitk_mode(prev)
    assert any(not torch.equal(a, b) for a, b in zip(first, base))             # the split kernel did run
    for a, b in zip(first, base):
        assert rel_l2(a.float(), b.float()) < 4e-3, rel_l2(a.float(), b.float())


# norm: "qk" = q and k RMS-normalised in the kernel (register-staged variant), "q" = only q (k arrives normalised from the
# projection GEMM, as in the DiT forward), "" = neither: the last two run the LDS-DMA variants -- 128-query workgroups when
# they fill half the chip, else 64-query workgroups with two key groups (ragged last tiles, 1-tile and 1-key inputs included)
@pytest.mark.parametrize("B,H,Lq,Lk,norm", [(2, 2, 64, 64, "qk"), (1, 3, 100, 137, "qk"), (2, 16, 768, 768, "qk"),
                                             (2, 4, 96, 1369, "qk"), (1, 2, 48, 80, ""), (2, 16, 768, 768, ""),
                                             (2, 16, 768, 768, "q"), (2, 16, 700, 1369, ""), (1, 16, 768, 1369, "q"),
                                             (3, 16, 768, 100, ""), (3, 16, 520, 1, ""), (1, 1, 5, 63, ""),
                                             (1, 2, 130, 129, "q")])
def test_attention(gpu_device, B, H, Lq, Lk, norm):
    from gaussiananything_amd import dit_ops as ops
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + Lq + Lk)
    D = H * 64
    qkv_q = torch.randn(B, Lq, 3 * D, generator=g).to(gpu_device).bfloat16()
    kvbuf = torch.randn(B, Lk, 2 * D, generator=g).to(gpu_device).bfloat16()
    qn = (1 + 0.2 * torch.randn(64, generator=g)).to(gpu_device)
    kn = (1 + 0.2 * torch.randn(64, generator=g)).to(gpu_device)
    q = qkv_q[..., :D].unflatten(-1, (H, 64))
    k = kvbuf[..., :D].unflatten(-1, (H, 64))
    v = kvbuf[..., D:].unflatten(-1, (H, 64))
    out = ops.attention(q, k, ops.transpose_v(v), qn if "q" in norm else None, kn if "k" in norm else None)
    qf, kf, vf = q.float().permute(0, 2, 1, 3), k.float().permute(0, 2, 1, 3), v.float().permute(0, 2, 1, 3)
    if "q" in norm:
        qf = qf * torch.rsqrt(qf.pow(2).mean(-1, keepdim=True) + 1e-5) * qn
    if "k" in norm:
        kf = kf * torch.rsqrt(kf.pow(2).mean(-1, keepdim=True) + 1e-5) * kn
    ref = torch.softmax(qf @ kf.transpose(-1, -2) * 0.125, -1) @ vf
    ref = ref.permute(0, 2, 1, 3).reshape(B, Lq, D)
    assert rel_l2(out.float(), ref) < 1e-2


@pytest.mark.parametrize("B,H,Lq,Lk,K,fold,tiled", [(1, 16, 768, 1369, 1024, True, True), (1, 12, 768, 1369, 768, False, True),
                                                     (1, 3, 200, 137, 192, True, False), (2, 4, 100, 64, 256, False, False)])
def test_attention_with_the_q_projection_inside_the_workgroup(gpu_device, B, H, Lq, Lk, K, fold, tiled):
    """GaAttentionArgs.qp_* (round 5): q = A W^T per head computed by the attention workgroups themselves -- the denoiser's
    cross-attention (/root/reference/ldm/modules/attention.py:497-522: to_q without bias, per-head q RMSNorm) without a projection
    launch in front -- against the two-launch sequence it replaces (ga_gemm_bf16 with the head norm and, `fold`, the RMSNorm row scale
    in its epilogue, then ga_attention_bf16 on its output) and against fp32; both weight layouts, ragged query / key counts, K = 192
    (one K-slice per key group)."""
    from gaussiananything_amd import dit_ops as ops
    g = torch.Generator().manual_seed(77)
    D = H * 64
    A = torch.randn(B * Lq, K, generator=g).to(gpu_device).bfloat16()
    W = (torch.randn(D, K, generator=g) / K ** 0.5).to(gpu_device).bfloat16()
    wq = (1 + 0.3 * torch.randn(64, generator=g)).to(gpu_device)
    k = torch.randn(B, Lk, H, 64, generator=g).to(gpu_device).bfloat16()
    v = torch.randn(B, Lk, H, 64, generator=g).to(gpu_device).bfloat16()
    vt = ops.transpose_v(v)
    row_ss = None
    if fold:   # partial sums of squares of a (fictitious) un-normalised row, 64 columns each, K / 64 rounded up to a multiple of 4 tiles
        tiles = (K // 64 + 3) // 4 * 4
        row_ss = (torch.rand(B * Lq, tiles, generator=g) * 64 * 3).to(gpu_device)
        row_ss[:, K // 64:] = 0
    q2 = ops.gemm(A, ops.tile_weight(W) if tiled else W, None, ops.EPI_STORE_BF16, qk_w0=wq, qk_cols0=D, qk_cols1=D, row_ss=row_ss,
                  row_ss_dim=K, w_tiled=tiled, N=D)
    want = ops.attention(q2.view(B, Lq, H, 64), k, vt)
    got = ops.attention(None, k, vt, q_norm_weight=wq,
                        qp=dict(a=A, w=ops.tile_weight(W) if tiled else W, tiled=tiled, row_ss=row_ss, row_ss_dim=K, B=B, Lq=Lq, H=H))
    assert rel_l2(got.float(), want.float()) < 4e-3, rel_l2(got.float(), want.float())      # (other summation order of the projection)
    qf = A.float() @ W.float().T
    if fold:
        qf = qf * torch.rsqrt(row_ss.sum(1, keepdim=True) / K + 1e-5)
    qf = qf.view(B, Lq, H, 64)
    qf = qf * torch.rsqrt(qf.pow(2).mean(-1, keepdim=True) + 1e-5) * wq
    sc = torch.einsum("bqhd,bkhd->bhqk", qf, k.float()) / 8.0
    ref = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(sc, -1), v.float()).reshape(B, Lq, D)
    assert rel_l2(got.float(), ref) < 1.2e-2, rel_l2(got.float(), ref)


@pytest.mark.parametrize("B,H,Lq,Lk,d", [(2, 16, 768, 768, 72), (1, 16, 768, 1369, 72), (2, 3, 100, 137, 40), (1, 2, 50, 64, 128), (1, 4, 33, 200, 8),
                                         (1, 2, 3, 5, 24), (3, 5, 130, 65, 104)])
def test_attention_for_head_dims_other_than_64(gpu_device, B, H, Lq, Lk, d):
    """ga_attention_hd_bf16 / ga_head_rmsnorm_bf16 (dit_attention_hd.hip): what DiT-PixArt-PCD-CLAY-XL's 16 heads of 72
    (/root/reference/dit/dit_i23d.py:1526-1535) need -- per-head RMSNorm of q and k, softmax(q k^T / sqrt(d)) v -- against fp32, at the XL
    shapes (self- and cross-attention), ragged sizes, and the smallest / largest head dims the kernel takes."""
    from gaussiananything_amd import dit_ops as ops
    g = torch.Generator().manual_seed(d)
    qkv = torch.randn(B * Lq, 3 * H * d, generator=g).to(gpu_device).bfloat16()
    kv = torch.randn(B * Lk, 2 * H * d, generator=g).to(gpu_device).bfloat16()
    wq = (1 + 0.3 * torch.randn(d, generator=g)).to(gpu_device)
    wk = (1 + 0.3 * torch.randn(d, generator=g)).to(gpu_device)
    nrm = lambda t, w: t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + 1e-5) * w  # noqa: E731
    q_ref = nrm(qkv[:, :H * d].float().view(B, Lq, H, d), wq)
    k_ref = nrm(kv[:, :H * d].float().view(B, Lk, H, d), wk)
    v_ref = kv[:, H * d:].float().view(B, Lk, H, d)
    q_raw, kv_raw = qkv.clone(), kv.clone()
    ops.head_rmsnorm_(qkv, H, d, wq)
    ops.head_rmsnorm_(kv, H, d, wk)
    assert rel_l2(qkv[:, :H * d].float().view(B, Lq, H, d), q_ref) < 6e-3 and rel_l2(kv[:, :H * d].float().view(B, Lk, H, d), k_ref) < 6e-3
    assert torch.equal(kv[:, H * d:].float().view(B, Lk, H, d), v_ref)                      # (only the named columns are touched)
    out = ops.attention_hd(qkv.view(B, Lq, 3 * H * d)[..., :H * d].unflatten(-1, (H, d)), kv.view(B, Lk, 2 * H * d)[..., :H * d].unflatten(-1, (H, d)),
                           kv.view(B, Lk, 2 * H * d)[..., H * d:].unflatten(-1, (H, d)))
    sc = torch.einsum("bqhd,bkhd->bhqk", q_ref, k_ref) / d ** 0.5
    ref = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(sc, -1), v_ref).reshape(B, Lq, H * d)
    assert rel_l2(out.float(), ref) < 1.2e-2, rel_l2(out.float(), ref)
    # round 6, the tuned variant (what ga_dit_forward runs): V^T as the projection GEMM stores it, q's norm inside the kernel
    vt = ops.v_transposed_hd(kv.view(B, Lk, 2 * H * d)[..., H * d:].unflatten(-1, (H, d)))
    k_n = kv.view(B, Lk, 2 * H * d)[..., :H * d].unflatten(-1, (H, d))
    k_raw = kv_raw.view(B, Lk, 2 * H * d)[..., :H * d].unflatten(-1, (H, d))
    # beside the norms: every configuration element-wise against float64 with the error model of tests/_bounds.py (two key groups: the
    # bound of the configuration with the most roundings), from the exact values each launch reads
    from tests import _attention_cases as ac
    q_in = q_raw.view(B, Lq, 3 * H * d)[..., :H * d].unflatten(-1, (H, d))
    z64 = dict(q=q_in.double(), v=v_ref.double(), wq=wq.double(), wk=wk.double())
    exact = {"q": ac.reference(ac.A("hd_dims_qnorm_inside", "hdv", B, H, Lq, Lk, "flat", d=d, norm="q"), dict(z64, k=k_n.double()), groups=2),
             "qk": ac.reference(ac.A("hd_dims_qknorm_inside", "hdv", B, H, Lq, Lk, "flat", d=d, norm="qk"), dict(z64, k=k_raw.double()), groups=2)}
    default_cfg = ops.attention_hd_plan(ac.make_args(ac.A("x", "hdv", B, H, Lq, Lk, "flat", d=d))).config
    instance = {(p.hd16, p.config): p for p in ops.attention_hd_instances() if p.family == ops.ATTN_HD_FAMILY_HDV}
    for force in ("1", "2", "3", "4", None):      # 4 waves x 16 / x 32 queries, 8 waves x 16, two key groups of 4 x 16, then the launcher's own choice
        inst = instance[((d + 15) // 16, int(force) if force else default_cfg)]
        got = _run_hdv(gpu_device, q_in, k_n, vt, wq, None, force)
        assert rel_l2(got.float(), ref) < 1.2e-2, (force, rel_l2(got.float(), ref))
        assert rel_l2(got.float(), out.float()) < 8e-3, (force, rel_l2(got.float(), out.float()))
        worst = ac.assert_within_bound(f"head dim {d}, configuration {force or 'by shape'}, q norm inside", got, *exact["q"], inst, H, d)
        # ... and k's norm inside as well (every workgroup normalises the key rows it stages)
        gotk = _run_hdv(gpu_device, q_in, k_raw, vt, wq, wk, force)
        assert rel_l2(gotk.float(), ref) < 1.2e-2, (force, rel_l2(gotk.float(), ref))
        assert rel_l2(gotk.float(), got.float()) < 4e-3, (force, rel_l2(gotk.float(), got.float()))
        worstk = ac.assert_within_bound(f"head dim {d}, configuration {force or 'by shape'}, q and k norm inside", gotk, *exact["qk"], inst, H, d)
        print(f"ATTNCASE hd_dims_d{d}_{Lq}x{Lk}_forced{force or '-'} {ac.describe(inst)} | out {worst:.3f} out(k norm inside) {worstk:.3f}")
    got2 = ops.attention_hd(qkv.view(B, Lq, 3 * H * d)[..., :H * d].unflatten(-1, (H, d)), k_n, vt=vt)     # q and k normalised by the caller
    assert rel_l2(got2.float(), ref) < 1.2e-2


def _run_hdv(dev, q, k, vt, wq, wk, force_qf):
    """GA_ATTN_HD_QF is read once per process: the forced variants run in a child process on the same tensors (saved / loaded)."""
    from gaussiananything_amd import dit_ops as ops
    if force_qf is None:
        return ops.attention_hd(q, k, vt=vt, q_norm_weight=wq, k_norm_weight=wk)
    import os, subprocess, sys, tempfile
    with tempfile.TemporaryDirectory() as td:
        f = os.path.join(td, "io.pt")
        torch.save({"q": q.cpu(), "k": k.cpu(), "vt": vt.cpu(), "wq": wq.cpu(), "wk": None if wk is None else wk.cpu()}, f)
        code = ("import torch\nfrom gaussiananything_amd import dit_ops as ops\n"
                f"z = torch.load({f!r})\nq, k, vt, wq = (z[n].to('cuda:0') for n in ('q', 'k', 'vt', 'wq'))\n"
                "wk = None if z['wk'] is None else z['wk'].to('cuda:0')\nq = q.contiguous(); k = k.contiguous()\n"
                f"torch.save(ops.attention_hd(q, k, vt=vt, q_norm_weight=wq, k_norm_weight=wk).cpu(), {f + '.out'!r})\n")
        env = dict(os.environ, GA_ATTN_HD_QF=force_qf, PYTHONPATH=os.pathsep.join([os.path.dirname(os.path.dirname(os.path.abspath(__file__)))] + sys.path))
        subprocess.run([sys.executable, "-c", code], check=True, env=env, timeout=600)
        return torch.load(f + ".out").to(dev)


def test_model_with_heads_of_72_matches_the_reference_golden(gpu_device):
    """DiT-PixArt-PCD-CLAY-XL's head geometry (8 heads of 72 at width 576, depth 2) against outputs of the REFERENCE'S OWN classes
    (tests/golden/dit_ref_hd72.pt, make_dit_golden.py: the weights are synthetic.recipe_state_dict, regenerated here): forward and
    forward_with_cfg, the zero-context skip, and the fused Euler sampler on top of it."""
    from gaussiananything_amd import synthetic
    from gaussiananything_amd.dit import DiT_I23D_PCD_PixelArt_noclip
    from gaussiananything_amd.transport import Sampler, create_transport
    z = torch.load(synthetic.fixture_path("dit_ref_hd72.pt"))
    model = DiT_I23D_PCD_PixelArt_noclip(**z["kwargs"])
    model.load_state_dict(synthetic.recipe_state_dict(z["keys"], z["recipe_seed"]), strict=True)
    model.to(gpu_device)
    assert model.embed_dim // model.num_heads == 72
    ctx = {k: v.to(gpu_device) for k, v in z["context"].items()}
    x, t = z["x"].to(gpu_device), z["t"].to(gpu_device)
    with torch.no_grad():
        y = model(x, t, ctx)
        ycfg = model.forward_with_cfg(x, t, ctx, z["cfg_scale"])
    assert rel_l2(y, z["y"].to(gpu_device)) < 1.5e-2, rel_l2(y, z["y"].to(gpu_device))
    assert rel_l2(ycfg, z["y_cfg"].to(gpu_device)) < 3e-2
    assert model._ctx_cache[1][2] == 2                      # the zero-context half skipped its cross-attention
    fn = Sampler(create_transport("GVP", "velocity", None, None, None, snr_type="uniform")).sample_ode(sampling_method="euler", num_steps=6)
    with torch.no_grad():
        traj = fn(x, model.forward_with_cfg, context=ctx, cfg_scale=z["cfg_scale"])
    assert traj.shape == (6,) + tuple(x.shape) and bool(torch.isfinite(traj).all())


def test_attention_online_softmax_rescale_is_exercised(gpu_device):
    """One key in the LAST tile dominates one query: the running-max rescale path must fire and stay exact."""
    from gaussiananything_amd import dit_ops as ops
    B, H, Lq, Lk = 1, 1, 64, 256
    g = torch.Generator(device="cpu").manual_seed(5)
    q = torch.randn(B, Lq, H, 64, generator=g)
    k = torch.randn(B, Lk, H, 64, generator=g)
    v = torch.randn(B, Lk, H, 64, generator=g)
    k[0, 250, 0] = q[0, 7, 0] * 6.0          # score ~ 6*|q|^2/8 >> the rest
    q, k, v = (t.to(gpu_device).bfloat16() for t in (q, k, v))
    out = ops.attention(q, k, ops.transpose_v(v))
    qf, kf, vf = (t.float().permute(0, 2, 1, 3) for t in (q, k, v))
    ref = (torch.softmax(qf @ kf.transpose(-1, -2) * 0.125, -1) @ vf).permute(0, 2, 1, 3).reshape(B, Lq, 64)
    assert rel_l2(out.float(), ref) < 1e-2
    assert (out.float()[0, 7] - v.float()[0, 250, 0]).abs().max() < 0.1


@pytest.mark.parametrize("M,D", [(96, 128), (1536, 1024), (50, 768), (33, 1152)])
def test_rmsnorm_modulate(gpu_device, M, D):
    from gaussiananything_amd import dit_ops as ops
    g = torch.Generator(device="cpu").manual_seed(D)
    rows = 3 if M % 3 == 0 else 1
    x = torch.randn(M, D, generator=g).to(gpu_device) * 3
    w = (1 + 0.1 * torch.randn(D, generator=g)).to(gpu_device)
    mod = torch.randn(M // rows, 6, D, generator=g).to(gpu_device)
    ref = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-5) * w
    out = ops.rmsnorm_modulate(x, w)
    assert rel_l2(out.float(), ref) < 5e-3
    out = ops.rmsnorm_modulate(x, w, mod[:, 1], mod[:, 0], rows_per_batch=rows)
    ref2 = ref * (1 + mod[:, 1].repeat_interleave(rows, 0)) + mod[:, 0].repeat_interleave(rows, 0)
    assert rel_l2(out.float(), ref2) < 5e-3


def test_folded_prenorm_pair_matches_the_unfused_sequence(gpu_device):
    """ga_dit.h 'folded un-modulated RMSNorm': residual GEMM with the emit_* side product + projection (norm weight folded
    into its columns) with row_ss must equal residual GEMM -> rmsnorm -> projection (bf16 rounding moved across the row
    scale: the tolerance of any bf16 op), with and without the per-head q-norm, in the 32- / 64- / 128-row tile
    configurations; the sums of squares are exact and deterministic."""
    from gaussiananything_amd import dit_ops as ops
    g = torch.Generator(device="cpu").manual_seed(21)
    for (M, D, K) in ((200, 256, 128), (1536, 1024, 256), (4500, 768, 64)):
        A = torch.randn(M, K, generator=g).to(gpu_device).bfloat16()
        W1 = (torch.randn(D, K, generator=g) / K ** 0.5).to(gpu_device).bfloat16()
        b1 = torch.randn(D, generator=g).to(gpu_device)
        gate = torch.randn(3, D, generator=g).to(gpu_device)
        rpb = (M + 2) // 3
        x0 = torch.randn(M, D, generator=g).to(gpu_device)
        nw = (1 + 0.2 * torch.randn(D, generator=g)).to(gpu_device)
        W2f = torch.randn(D, D, generator=g) / D ** 0.5
        W2 = W2f.to(gpu_device).bfloat16()
        W2n = (W2.float() * nw[None, :]).bfloat16()
        qw = (1 + 0.2 * torch.randn(64, generator=g)).to(gpu_device)
        x_ref = x0.clone()
        ops.gemm(A, W1, b1, ops.EPI_RESIDUAL, out=x_ref, gate=gate, rows_per_batch=rpb)
        h = ops.rmsnorm_modulate(x_ref, nw)
        x = x0.clone()
        xb = torch.empty(M, D, device=gpu_device, dtype=torch.bfloat16)
        ss = torch.full((M, D // 64), float("nan"), device=gpu_device)
        ops.gemm(A, W1, b1, ops.EPI_RESIDUAL, out=x, gate=gate, rows_per_batch=rpb, emit_x=xb, emit_ss=ss)
        assert torch.equal(x, x_ref) and torch.equal(xb, x.bfloat16())
        assert torch.allclose(ss.sum(1), x.pow(2).sum(1), rtol=1e-5)
        ss2 = torch.empty_like(ss)
        ops.gemm(A, W1, b1, ops.EPI_RESIDUAL, out=x0.clone(), gate=gate, rows_per_batch=rpb, emit_x=xb, emit_ss=ss2)
        assert torch.equal(ss, ss2)
        for qk in (False, True):
            kw = dict(qk_w0=qw, qk_cols0=D, qk_cols1=D) if qk else {}
            y_ref = ops.gemm(h, W2, None, ops.EPI_STORE_BF16, **kw)
            y = ops.gemm(xb, W2n, None, ops.EPI_STORE_BF16, row_ss=ss, row_ss_dim=D, **kw)
            assert rel_l2(y.float(), y_ref.float()) < 8e-3, (M, qk)


def test_folded_modulated_prenorm_pair_matches_the_unfused_sequence(gpu_device):
    """ga_dit.h 'folding a MODULATED RMSNorm': residual GEMM emitting bf16(x w (1 + scale_b)) and the raw sums of squares, then the
    projection with row_ss and the per-batch bias rows bias + shift_b W^T (ga_dit_shift_bias), must equal residual GEMM ->
    rmsnorm_modulate -> projection, for the plain and the GELU epilogue, with the q/k head norm + V^T store of the qkv projection,
    and with rows behind k_rows taking only the bias (the skipped cross-attention).  Tiles whose rows straddle two batch items
    (rows_per_batch not a multiple of the tile) take the per-row bias path."""
    from gaussiananything_amd import dit_ops as ops
    g = torch.Generator(device="cpu").manual_seed(33)
    for (M, D, K, N2, nb) in ((200, 256, 128, 512, 3), (1536, 1024, 1024, 4096, 2), (1000, 768, 256, 768, 1), (1536, 1024, 1024, 3072, 2)):
        rpb = (M + nb - 1) // nb
        A = torch.randn(M, K, generator=g).to(gpu_device).bfloat16()
        W1 = (torch.randn(D, K, generator=g) / K ** 0.5).to(gpu_device).bfloat16()
        b1 = torch.randn(D, generator=g).to(gpu_device)
        gate = torch.randn(nb, D, generator=g).to(gpu_device)
        x0 = torch.randn(M, D, generator=g).to(gpu_device)
        nw = (1 + 0.2 * torch.randn(D, generator=g)).to(gpu_device)
        mod = (0.3 * torch.randn(nb, 6, D, generator=g)).to(gpu_device)
        scale, shift = mod[:, 1], mod[:, 0]
        W2 = (torch.randn(N2, D, generator=g) / D ** 0.5).to(gpu_device).bfloat16()
        b2 = torch.randn(N2, generator=g).to(gpu_device)
        for k_rows in (0, rpb if nb > 1 else 0):
            if k_rows == 0 and M == 1536 and N2 == 3072:
                continue
            # --- unfused
            x_ref = x0.clone()
            if k_rows:
                ops.gemm(A[:k_rows], W1, b1, ops.EPI_RESIDUAL, out=x_ref[:k_rows], rows_per_batch=rpb)
                x_ref[k_rows:] += b1
            else:
                ops.gemm(A, W1, b1, ops.EPI_RESIDUAL, out=x_ref, gate=gate, rows_per_batch=rpb)
            h = ops.rmsnorm_modulate(x_ref, nw, scale, shift, rows_per_batch=rpb)
            # --- folded
            x = x0.clone()
            xb = torch.empty(M, D, device=gpu_device, dtype=torch.bfloat16)
            ss = torch.full((M, D // 64), float("nan"), device=gpu_device)
            ops.gemm(A[:k_rows] if k_rows else A, W1, b1, ops.EPI_RESIDUAL, out=x, gate=None if k_rows else gate, rows_per_batch=rpb,
                     emit_x=xb, emit_ss=ss, emit_w=nw, emit_scale=scale, k_rows=k_rows)
            assert torch.equal(x, x_ref), (M, k_rows)
            mult = (nw[None] * (1 + scale)).repeat_interleave(rpb, 0)[:M]
            assert torch.equal(xb, (x * mult).bfloat16())
            assert torch.allclose(ss.sum(1), x.pow(2).sum(1), rtol=1e-5)
            bias2 = ops.shift_bias(W2, shift, b2)
            ref_b2 = b2[None] + shift @ W2.float().T
            assert torch.allclose(bias2, ref_b2, rtol=1e-4, atol=1e-4)
            bias2_t = ops.shift_bias(ops.tile_weight(W2), shift, b2, w_tiled=True, N=N2)
            assert torch.equal(bias2, bias2_t)
            if D % 256 or D > 1024:
                continue            # (the consumer takes at most 16 partial sums per row, in groups of 4)
            for epi in (ops.EPI_STORE_BF16, ops.EPI_GELU_BF16):
                y_ref = ops.gemm(h, W2, b2, epi)
                y = ops.gemm(xb, W2, bias2, epi, row_ss=ss, row_ss_dim=D, rows_per_batch=rpb)
                assert rel_l2(y.float(), y_ref.float()) < 8e-3, (M, epi, k_rows)
            if N2 == 3 * D:    # the qkv projection: per-head q / k norm and the transposed V store on top
                qw = (1 + 0.2 * torch.randn(64, generator=g)).to(gpu_device)
                kw_ = (1 + 0.2 * torch.randn(64, generator=g)).to(gpu_device)
                Lp = (rpb + 63) // 64 * 64
                outs = []
                for (a_, bias_, extra) in ((h, b2, {}), (xb, bias2, dict(row_ss=ss, row_ss_dim=D))):
                    vt = torch.zeros(nb * D, Lp, device=gpu_device, dtype=torch.bfloat16)
                    qk = ops.gemm(a_, W2, bias_, ops.EPI_STORE_BF16, rows_per_batch=rpb, vt=vt, vt_col0=2 * D, qk_w0=qw, qk_cols0=D,
                                  qk_w1=kw_, qk_cols1=2 * D, **extra)
                    outs.append((qk.float(), vt.float()))
                assert rel_l2(outs[1][0], outs[0][0]) < 8e-3 and rel_l2(outs[1][1], outs[0][1]) < 8e-3


@pytest.mark.parametrize("B,N,K", [(1, 64, 64), (9, 3072, 1024), (4, 520, 2048), (16, 4096, 1024)])
def test_shift_bias_rows(gpu_device, B, N, K):
    """ga_dit_shift_bias: bias + shift_b . W rows in fp32 from the bf16 weight, every batch size (one pass over the weights serves 8
    batch items), a ragged last row-group block, both weight layouts bit-identical."""
    from gaussiananything_amd import dit_ops as ops
    g = torch.Generator(device="cpu").manual_seed(B * 1000 + N)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(gpu_device).bfloat16()
    bias = torch.randn(N, generator=g).to(gpu_device)
    mod = torch.randn(B, 6, K, generator=g).to(gpu_device)
    shift = mod[:, 3]                                      # a strided view, as the model's modulation table is
    out = ops.shift_bias(W, shift, bias)
    ref = bias[None].double() + shift.double() @ W.double().T
    assert torch.allclose(out.double(), ref, rtol=1e-4, atol=1e-4)
    assert torch.equal(out, ops.shift_bias(ops.tile_weight(W), shift, bias, w_tiled=True, N=N))
    assert torch.allclose(ops.shift_bias(W, shift, None).double(), ref - bias[None].double(), rtol=1e-4, atol=1e-4)


def test_small_linear(gpu_device):
    from gaussiananything_amd import dit_ops as ops
    g = torch.Generator(device="cpu").manual_seed(3)
    x = torch.randn(4, 256, generator=g).to(gpu_device)
    W = (torch.randn(384, 256, generator=g) / 16).to(gpu_device).bfloat16()
    b = torch.randn(384, generator=g).to(gpu_device)
    add = torch.randn(4, 384, generator=g).to(gpu_device)
    y = ops.small_linear(x, W, b, add, act_in=1, act_out=1)
    ref = torch.nn.functional.silu(torch.nn.functional.silu(x).bfloat16().float() @ W.float().T + b) + add
    assert rel_l2(y, ref) < 2e-3


def _load_golden(stage, device):
    from gaussiananything_amd.dit import DiT_I23D_PCD_PixelArt_noclip, DiT_I23D_PCD_PixelArt_noclip_clay_stage2
    from gaussiananything_amd import synthetic
    z = torch.load(synthetic.fixture_path(f"dit_ref_stage{stage}.pt"))
    kw = dict(z["kwargs"])
    if stage == 2:
        kw["use_pe_cond"] = True
    cls = DiT_I23D_PCD_PixelArt_noclip if stage == 1 else DiT_I23D_PCD_PixelArt_noclip_clay_stage2
    model = cls(**kw)
    model.load_state_dict(z["state_dict"], strict=True)
    model.to(device)
    ctx = {k: v.to(device) for k, v in z["context"].items()}
    return z, model, ctx


@pytest.mark.parametrize("stage", [1, 2])
def test_model_matches_reference_golden(gpu_device, stage):
    """forward and forward_with_cfg against outputs of the reference's own classes (fp32 on CPU)."""
    z, model, ctx = _load_golden(stage, gpu_device)
    x, t = z["x"].to(gpu_device), z["t"].to(gpu_device)
    with torch.no_grad():
        y = model(x, t, ctx)
        y2 = model(x, t, ctx)                                   # second call: cached K/V path
        ycfg = model.forward_with_cfg(x, t, ctx, z["cfg_scale"])
    assert y.dtype == torch.float32 and y.shape == z["y"].shape
    assert torch.equal(y, y2)
    # the pooled-vector branch is computed once per conditioning vector (GaDitForwardArgs.pooled_vec): same bits as inside the evaluation,
    # and a vector changed in place is noticed
    assert model._pooled_cache is not None
    model.pooled_once = False
    with torch.no_grad():
        assert torch.equal(model(x, t, ctx), y)
    model.pooled_once = True
    saved = ctx["img_vector"].clone()
    ctx["img_vector"].add_(torch.linspace(-1.0, 1.0, saved.shape[-1], device=gpu_device))   # (not a scaling: the branch starts with a LayerNorm)
    with torch.no_grad():
        y_other = model(x, t, ctx)
    ctx["img_vector"].copy_(saved)
    assert not torch.equal(y_other, y)
    with torch.no_grad():
        assert torch.equal(model(x, t, ctx), y)
    ref = z["y"].to(gpu_device)
    assert rel_l2(y, ref) < 1.5e-2, rel_l2(y, ref)
    assert float((y - ref).abs().max()) < 5e-2 * float(ref.abs().max())
    assert rel_l2(ycfg, z["y_cfg"].to(gpu_device)) < 3e-2        # CFG amplifies the difference by the guidance scale


def test_zero_context_items_skip_cross_attention_exactly(gpu_device):
    """The unconditional half of a CFG batch has all-zero image tokens: K = V = 0, uniform softmax over zeros, so its
    cross-attention is `x += to_out.bias`; the forward skips the work for those items.  Must be BIT-identical to running
    it, and must not trigger when a zero item precedes a non-zero one."""
    z, model, ctx = _load_golden(1, gpu_device)
    x, t = z["x"].to(gpu_device), z["t"].to(gpu_device)
    assert float(ctx["img_crossattn"][2:].abs().max()) == 0.0 and float(ctx["img_crossattn"][:2].abs().max()) > 0.0
    with torch.no_grad():
        y_skip = model(x, t, ctx)
        assert model._ctx_cache[1][2] == 2
        model.ca_skip = False
        model._ctx_cache = None
        y_full = model(x, t, ctx)
        assert model._ctx_cache[1][2] == 4
        assert torch.equal(y_skip, y_full)
        model.ca_skip = True
        ctx2 = dict(ctx, img_crossattn=ctx["img_crossattn"].flip(0).contiguous())       # zero items first: no skipping
        y_flip = model(x.flip(0).contiguous(), t, dict(ctx2, img_vector=ctx["img_vector"].flip(0).contiguous()))
        assert model._ctx_cache[1][2] == 4
        assert torch.equal(y_flip.flip(0), y_full)


def test_model_release_shape_against_oracle(gpu_device):
    """DiT-B sized block stack (hidden 768, 12 heads, 768 tokens, 1369 x 1024 context, CFG batch 2) against the fp32
    oracle on the same weights -- the configuration of BASELINE.json configs[2], shortened to depth 2."""
    from gaussiananything_amd.dit import DiT_I23D_PCD_PixelArt_noclip
    from oracle import dit as od
    torch.manual_seed(0)
    model = DiT_I23D_PCD_PixelArt_noclip(input_size=16, patch_size=1, in_channels=3, hidden_size=768, depth=2,
                                         num_heads=12, num_classes=0, learn_sigma=False, context_dim=1024,
                                         pooling_ctx_dim=768, roll_out=True, use_clay_ca=True)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in model.parameters():
            if float(p.abs().max()) == 0.0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    x = torch.randn(2, 768, 3, generator=g)
    t = torch.tensor([0.6, 0.6])
    ctx = {"img_crossattn": torch.randn(2, 1369, 1024, generator=g), "img_vector": torch.randn(2, 1024, generator=g)}
    ctx["img_crossattn"][1] = 0
    ctx["img_vector"][1] = 0
    ref = od.dit_forward(sd, x, t, ctx)
    model.to(gpu_device)
    with torch.no_grad():
        y = model(x.to(gpu_device), t.to(gpu_device), {k: v.to(gpu_device) for k, v in ctx.items()})
    assert rel_l2(y.cpu(), ref) < 1.5e-2, rel_l2(y.cpu(), ref)
    # at this width the pre-norms live in the GEMM epilogues (ga_dit.h): the rows of the skipped cross-attention take the output bias
    # and the folded norm1 through `k_rows` of the output projection -- for those rows bit-identical to running the cross-attention on the zero context
    with torch.no_grad():
        assert model._ctx_cache[1][2] == 1
        model.ca_skip = False
        model._ctx_cache = None
        y_full = model(x.to(gpu_device), t.to(gpu_device), {k: v.to(gpu_device) for k, v in ctx.items()})
        assert model._ctx_cache[1][2] == 2
    # (the item WITH a context goes through other launch configurations when the batch doubles -- other summation orders)
    assert torch.equal(y[1], y_full[1]) and rel_l2(y[0], y_full[0]) < 1e-2


def test_final_layer_statistics_on_rows_with_a_large_common_offset(gpu_device):
    """T2IFinalLayer's LayerNorm (dit_models_xformers.py:62-85) is two-pass upstream; the kernel reduces sum and sum of squares in one
    round.  Rows whose common offset is ~2000 x their spread: E[x^2] - mean^2 in fp32 loses the variance there (a quarter of it at
    this ratio), the pivoted form does not.  The blocks are switched off exactly (zero gates, zero cross-attention output), so the
    final layer sees the token embedding + offset and the fp32 oracle is the yardstick for that kernel alone."""
    from gaussiananything_amd.dit import DiT_I23D_PCD_PixelArt_noclip
    from oracle import dit as od
    torch.manual_seed(0)
    model = DiT_I23D_PCD_PixelArt_noclip(input_size=16, patch_size=1, in_channels=3, hidden_size=768, depth=1,
                                         num_heads=12, num_classes=0, learn_sigma=False, context_dim=1024,
                                         pooling_ctx_dim=768, roll_out=True, use_clay_ca=True)
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if float(p.abs().max()) == 0.0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
        for k, p in model.named_parameters():
            if k.startswith("adaLN_modulation") or k.endswith("scale_shift_table") and k.startswith("blocks") \
                    or "cross_attn_dino.to_out" in k:
                p.zero_()
        model.x_embedder.fc2.bias.add_(100.0)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    x = torch.randn(2, 768, 3, generator=g)
    t = torch.tensor([0.3, 0.3])
    ctx = {"img_crossattn": torch.randn(2, 1369, 1024, generator=g), "img_vector": torch.randn(2, 1024, generator=g)}
    ref = od.dit_forward(sd, x, t, ctx)
    model.to(gpu_device)
    with torch.no_grad():
        y = model(x.to(gpu_device), t.to(gpu_device), {k: v.to(gpu_device) for k, v in ctx.items()})
    assert rel_l2(y.cpu(), ref) < 1e-2, rel_l2(y.cpu(), ref)


@pytest.mark.parametrize("width,heads", [(512, 4), (384, 12), (960, 8), (704, 8)])
def test_models_with_other_head_dims_against_oracle(gpu_device, width, heads):
    """Head dims other than 64 and 72 through ga_dit_forward's head-dim-generic branch against the fp32 oracle, depth 2: heads of 128 at a width
    the four-slot GEMM ring serves (pre-norms folded, 8 partial sums per row), heads of 32 at width 384 (6 K-tiles: the three-slot ring, 6 -> 8
    floats per row of partial sums), heads of 120 at width 960 (15 K-tiles: three slots again, 15 -> 16 floats) and heads of 88 at width 704
    (11 K-tiles: neither ring -- the general 2-slot kernel -- and no fold: the pre-norms as launches of their own)."""
    from gaussiananything_amd.dit import DiT_I23D_PCD_PixelArt_noclip
    from oracle import dit as od
    torch.manual_seed(0)
    model = DiT_I23D_PCD_PixelArt_noclip(input_size=16, patch_size=1, in_channels=3, hidden_size=width, depth=2, num_heads=heads, num_classes=0,
                                         learn_sigma=False, context_dim=1024, pooling_ctx_dim=768, roll_out=True, use_clay_ca=True)
    g = torch.Generator().manual_seed(width)
    with torch.no_grad():
        for p in model.parameters():
            if float(p.abs().max()) == 0.0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    x = torch.randn(2, 768, 3, generator=g)
    t = torch.tensor([0.4, 0.4])
    ctx = {"img_crossattn": torch.randn(2, 257, 1024, generator=g), "img_vector": torch.randn(2, 1024, generator=g)}
    ctx["img_crossattn"][1] = 0
    ctx["img_vector"][1] = 0
    ref = od.dit_forward(sd, x, t, ctx)
    model.to(gpu_device)
    with torch.no_grad():
        y = model(x.to(gpu_device), t.to(gpu_device), {k: v.to(gpu_device) for k, v in ctx.items()})
    assert rel_l2(y.cpu(), ref) < 1.5e-2, rel_l2(y.cpu(), ref)


def test_xl_geometry_against_oracle_folded_and_unfolded(gpu_device):
    """DiT-PixArt-PCD-CLAY-XL's geometry (/root/reference/dit/dit_i23d.py:1526-1535: width 1152, 16 heads of 72) at the release shapes, depth 3,
    against the fp32 oracle: the round-6 path -- three-slot GEMM rings (K = 1152 is no multiple of 256), 18 -> 20 partial sums per row behind
    the folded pre-norms, V^T for heads of 72, q's norm inside the attention kernel -- and, in a child process (GA_DIT_FOLD_MOD is read once),
    the same model with the pre-norms as launches of their own."""
    import subprocess, sys, tempfile
    from gaussiananything_amd.dit import DiT_I23D_PCD_PixelArt_noclip
    from oracle import dit as od
    kw = dict(input_size=16, patch_size=1, in_channels=3, hidden_size=1152, depth=3, num_heads=16, num_classes=0, learn_sigma=False,
              context_dim=1024, pooling_ctx_dim=768, roll_out=True, use_clay_ca=True)
    torch.manual_seed(0)
    model = DiT_I23D_PCD_PixelArt_noclip(**kw)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in model.parameters():
            if float(p.abs().max()) == 0.0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    x = torch.randn(2, 768, 3, generator=g)
    t = torch.tensor([0.6, 0.6])
    ctx = {"img_crossattn": torch.randn(2, 1369, 1024, generator=g), "img_vector": torch.randn(2, 1024, generator=g)}
    ctx["img_crossattn"][1] = 0
    ctx["img_vector"][1] = 0
    torch.set_num_threads(min(64, len(os.sched_getaffinity(0))))
    ref = od.dit_forward(sd, x, t, ctx)
    model.to(gpu_device)
    with torch.no_grad():
        y = model(x.to(gpu_device), t.to(gpu_device), {k: v.to(gpu_device) for k, v in ctx.items()})
    assert rel_l2(y.cpu(), ref) < 1.5e-2, rel_l2(y.cpu(), ref)
    with tempfile.TemporaryDirectory() as td:
        f = os.path.join(td, "io.pt")
        torch.save({"kw": kw, "sd": sd, "x": x, "t": t, "ctx": ctx}, f)
        code = ("import torch\nfrom gaussiananything_amd.dit import DiT_I23D_PCD_PixelArt_noclip\n"
                f"z = torch.load({f!r})\nm = DiT_I23D_PCD_PixelArt_noclip(**z['kw'])\nm.load_state_dict(z['sd'])\nm.to('cuda:0')\n"
                "with torch.no_grad():\n    y = m(z['x'].to('cuda:0'), z['t'].to('cuda:0'), {k: v.to('cuda:0') for k, v in z['ctx'].items()})\n"
                f"torch.save(y.cpu(), {f + '.out'!r})\n")
        env = dict(os.environ, GA_DIT_FOLD_MOD="0", PYTHONPATH=os.pathsep.join([os.path.dirname(os.path.dirname(os.path.abspath(__file__)))] + sys.path))
        subprocess.run([sys.executable, "-c", code], check=True, env=env, timeout=600)
        y_unf = torch.load(f + ".out")
    assert rel_l2(y_unf, ref) < 1.5e-2, rel_l2(y_unf, ref)
    assert rel_l2(y.cpu(), y_unf) < 1e-2 and not torch.equal(y.cpu(), y_unf)       # (two different launch sequences, both at the oracle's bar)


@pytest.mark.parametrize("arch,C", [("DiT-PixArt-PCD-CLAY-L", 3), ("DiT-PixArt-PCD-CLAY-stage2-L", 10), ("DiT-PixArt-PCD-CLAY-XL", 3)])
def test_release_models_full_depth_against_oracle(gpu_device, arch, C):
    """The two released denoisers at FULL size (DiT-L: depth 24, width 1024, 16 heads; stage 2 with the xyz positional
    embedding) at the release shapes -- CFG batch 2 x 768 tokens, 1369 x 1024 image tokens -- against the fp32 oracle
    (oracle/dit.py, itself pinned to the reference's classes) on the same seeded weights: BASELINE.json configs[3].
    Tolerance: bf16 MFMA operands / fp32 accumulate over 24 blocks against an all-fp32 forward; north_star states no
    figure for the denoiser, the reference itself runs under bf16 autocast (SURVEY.md A.2 expects ~1e-2)."""
    from gaussiananything_amd.dit import DiT_models
    from oracle import dit as od
    torch.manual_seed(0)
    model = DiT_models[arch](input_size=16, in_channels=C, context_dim=1024, pooling_ctx_dim=768, num_classes=0,
                             learn_sigma=False, roll_out=True)
    # (round 6: the registry's XL entry as well -- depth 28, width 1152, 16 heads of 72 -- on its own attention / GEMM instances)
    assert (model.depth, model.embed_dim) == ((28, 1152) if arch.endswith("XL") else (24, 1024))
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for p in model.parameters():
            if float(p.abs().max()) == 0.0:
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    x = torch.randn(2, 768, C, generator=g)
    t = torch.tensor([0.35, 0.35])
    ctx = {"img_crossattn": torch.randn(2, 1369, 1024, generator=g), "img_vector": torch.randn(2, 1024, generator=g)}
    ctx["img_crossattn"][1] = 0
    ctx["img_vector"][1] = 0
    if "stage2" in arch:
        ctx["fps-xyz"] = ((torch.rand(2, 768, 3, generator=g) - 0.5) * 0.9) / 0.45
        ctx["fps-xyz"][1] = ctx["fps-xyz"][0]
    torch.set_num_threads(min(64, len(os.sched_getaffinity(0))))
    ref = od.dit_forward(sd, x, t, ctx)
    ref_cfg = od.forward_with_cfg(sd, x, t, ctx, 4.0)
    model.to(gpu_device)
    dctx = {k: v.to(gpu_device) for k, v in ctx.items()}
    with torch.no_grad():
        y = model(x.to(gpu_device), t.to(gpu_device), dctx)
        ycfg = model.forward_with_cfg(x.to(gpu_device), t.to(gpu_device), dctx, 4.0)
    assert rel_l2(y.cpu(), ref) < 1.5e-2, rel_l2(y.cpu(), ref)
    assert rel_l2(ycfg.cpu(), ref_cfg) < 3e-2, rel_l2(ycfg.cpu(), ref_cfg)


def test_dopri5_on_the_golden_model_against_the_ode_oracle(gpu_device):
    """The reference's default sampler -- sample_ode(num_steps=N) = dopri5, rtol 1e-3, atol 1e-6
    (/root/reference/transport/transport.py:384-431, integrators.py:111-118) -- on the HIP denoiser, against oracle/ode.py
    (float64 state, torchdiffeq semantics of SURVEY.md A.3):
      (i)  integrator parity: the oracle integrating the SAME function (the HIP forward_with_cfg) must take the same
           decisions -- function evaluations, accepted and rejected steps -- and give the same saved states;
      (ii) end-to-end: the saved states against the oracle integrating the fp32 DiT oracle on the same golden weights.
           The step sequences differ there by construction: the bf16 rounding noise of the HIP model enters the embedded
           error estimate (the reference under bf16 autocast has the same property), so only the states are compared."""
    from gaussiananything_amd.transport import Sampler, create_transport
    from oracle import dit as od, ode as oo
    z, model, ctx = _load_golden(1, gpu_device)
    x = z["x"]
    n_out = 9
    tgrid = np.linspace(0.0, 1.0, n_out)
    sampler = Sampler(create_transport("GVP", "velocity", None, None, None, snr_type="uniform"))
    fn = sampler.sample_ode(sampling_method="dopri5", num_steps=n_out, atol=1e-6, rtol=1e-3)
    with torch.no_grad():
        out = fn(x.to(gpu_device), model.forward_with_cfg, context=ctx, cfg_scale=z["cfg_scale"])
    s_hip = dict(sampler.last_ode.last_stats)
    assert out.shape == (n_out,) + tuple(x.shape)

    def f_hip(ts, yy):
        with torch.no_grad():
            tt = torch.ones(x.shape[0], device=gpu_device) * torch.tensor(ts, dtype=torch.float32, device=gpu_device)
            return model.forward_with_cfg(torch.from_numpy(yy).float().to(gpu_device), tt, context=ctx,
                                          cfg_scale=z["cfg_scale"]).double().cpu().numpy()

    # the fixed-grid reading of "250 steps" (euler; here through the fused on-device step) against the oracle integrator on
    # the same function: same grid, same number of evaluations, same states
    fn_e = sampler.sample_ode(sampling_method="euler", num_steps=n_out)
    with torch.no_grad():
        out_e = fn_e(x.to(gpu_device), model.forward_with_cfg, context=ctx, cfg_scale=z["cfg_scale"])
    s_e = {}
    same_e = oo.odeint(f_hip, x.double().numpy(), tgrid, method="euler", stats=s_e)
    assert sampler.last_ode.last_stats["nfe"] == s_e["nfe"] == n_out - 1
    assert rel_l2(out_e.cpu().double(), torch.from_numpy(same_e)) < 3e-3

    fn = sampler.sample_ode(sampling_method="dopri5", num_steps=n_out, atol=1e-6, rtol=1e-3)
    s_same = {}
    same = oo.odeint(f_hip, x.double().numpy(), tgrid, method="dopri5", atol=1e-6, rtol=1e-3, stats=s_same)
    assert (s_hip["nfe"], s_hip["steps"], s_hip["rejected"]) == (s_same["nfe"], s_same["steps"], s_same["rejected"]), (s_hip, s_same)
    # same decisions; the states differ by more than fp32-vs-fp64 rounding because the function itself is bf16: an ulp of
    # the fp32 state can round a bf16 operand the other way (measured 7e-4)
    assert rel_l2(out.cpu().double(), torch.from_numpy(same)) < 3e-3

    sd = {k: v.float() for k, v in z["state_dict"].items()}
    cctx = {k: v.float() for k, v in z["context"].items()}

    def f_ref(ts, yy):
        tt = torch.full((x.shape[0],), float(ts))
        return od.forward_with_cfg(sd, torch.from_numpy(yy).float(), tt, cctx, z["cfg_scale"]).double().numpy()

    s_ref = {}
    ref = oo.odeint(f_ref, x.double().numpy(), tgrid, method="dopri5", atol=1e-6, rtol=1e-3, stats=s_ref)
    assert s_ref["rejected"] <= s_ref["steps"] and s_hip["nfe"] >= s_ref["nfe"]
    assert rel_l2(out.cpu().double(), torch.from_numpy(ref)) < 3e-2


def test_device_resident_dopri5_takes_the_decisions_of_the_host_loop(gpu_device, monkeypatch):
    """csrc/ode_dopri5.hip (one attempted step = one replayed HIP graph; controller, accept / reject and dense output on the device)
    against the host loop of transport/odeint.py on the same denoiser: same evaluations, accepted and rejected steps, same states
    -- with and without guidance, and on a grid whose first output times fall inside one accepted step."""
    from gaussiananything_amd.transport import Sampler, create_transport
    z, model, ctx = _load_golden(1, gpu_device)
    x = z["x"].to(gpu_device)
    sampler = Sampler(create_transport("GVP", "velocity", None, None, None, snr_type="uniform"))
    for fwd, n_out in ((model.forward_with_cfg, 9), (model.forward_cond, 9), (model.forward_with_cfg, 250)):
        got = {}
        for flag in ("0", "1"):
            monkeypatch.setenv("GA_ODE_GRAPH", flag)
            fn = sampler.sample_ode(sampling_method="dopri5", num_steps=n_out, atol=1e-6, rtol=1e-3)
            with torch.no_grad():
                out = fn(x, fwd, context=ctx, cfg_scale=z["cfg_scale"])
            got[flag] = (out, dict(sampler.last_ode.last_stats))
        (a, sa), (b, sb) = got["0"], got["1"]
        assert sb.get("device_loop") and not sa.get("device_loop")
        assert (sa["nfe"], sa["steps"], sa["rejected"]) == (sb["nfe"], sb["steps"], sb["rejected"]), (sa, sb)
        assert a.shape == b.shape == (n_out,) + tuple(x.shape)
        assert rel_l2(b, a) < 2e-3, rel_l2(b, a)      # (bf16 function: an ulp of the fp32 state can round an operand the other way)
        assert torch.equal(b[0], x.float())
        # a second call on the same conditioning tensors replays the step captured by the first (no new capture), on another start
        # state; the first result is not overwritten
        held = model._samplers.held("dopri5").graph
        keep = b.clone()
        fn = sampler.sample_ode(sampling_method="dopri5", num_steps=n_out, atol=1e-6, rtol=1e-3)
        with torch.no_grad():
            again = fn(x, fwd, context=ctx, cfg_scale=z["cfg_scale"])
            other = fn(0.5 * x, fwd, context=ctx, cfg_scale=z["cfg_scale"])
        assert model._samplers.held("dopri5").graph is held and torch.equal(again, keep) and torch.equal(b, keep)
        assert not torch.equal(other[-1], keep[-1]) and torch.equal(other[0], 0.5 * x.float())


def test_device_dopri5_is_bit_reproducible_and_refuses_sigma_models(gpu_device):
    """(i) csrc/ode_dopri5.hip adds the error norm in a FIXED order (per-workgroup partials, summed by the controller): two
    integrations of the same problem give bit-identical controller blocks -- error ratio, sum of squares, step sizes, counters -- and
    states, whatever order the workgroups arrive in (round 4 accumulated with atomicAdd(double): a ratio near 1 could flip a decision).
    (ii) a sigma-predicting model (out_channels = 2 x in_channels) has no fused sampler step: ga_dit_forward refuses the step before
    anything is enqueued (round 4 would have written B*L*2C floats into B*L*C buffers), the Python entry raises."""
    from gaussiananything_amd import dit_ops as ops
    from gaussiananything_amd.dit import DiT_I23D_PCD_PixelArt_noclip
    from gaussiananything_amd.transport import Sampler, create_transport
    z, model, ctx = _load_golden(1, gpu_device)
    x = z["x"].to(gpu_device)
    sampler = Sampler(create_transport("GVP", "velocity", None, None, None, snr_type="uniform"))
    runs = []
    for _ in range(3):
        fn = sampler.sample_ode(sampling_method="dopri5", num_steps=17, atol=1e-6, rtol=1e-3)
        with torch.no_grad():
            out = fn(x, model.forward_with_cfg, context=ctx, cfg_scale=z["cfg_scale"])
        st = dict(sampler.last_ode.last_stats)
        assert st.get("device_loop") and len(st["ctl"]) == ops.GA_ODE_CTL_WORDS
        runs.append((out.clone(), st))
    for out, st in runs[1:]:
        assert st["ctl"] == runs[0][1]["ctl"], (st["ctl"], runs[0][1]["ctl"])
        assert torch.equal(out, runs[0][0])
    assert runs[0][1]["ctl"][ops.GA_ODE_RATIO] > 0.0 and runs[0][1]["ctl"][ops.GA_ODE_SUMSQ] > 0.0
    kw = dict(z["kwargs"], learn_sigma=True)
    sig = DiT_I23D_PCD_PixelArt_noclip(**kw).to(gpu_device)
    assert sig.out_channels == 2 * sig.in_channels
    with torch.no_grad():
        y = sig(x, z["t"].to(gpu_device), ctx)
        assert y.shape[-1] == 2 * x.shape[-1]                 # the plain forward of such a model is fine
        with pytest.raises(ValueError):
            sig.sample_dopri5_device(x, [0.0, 0.5, 1.0], ctx)
        with pytest.raises(ValueError):
            sig.sample_euler_fused(x, [0.0, 0.5, 1.0], ctx)
        vel = torch.empty_like(x)
        step = ops.GaDitSamplerStep(1.0, 0, None, None, None, 0, None, vel.data_ptr())
        with pytest.raises(RuntimeError):                     # the C-ABI itself: GA_DIT_ERR_BAD_SHAPE
            sig.forward(x, z["t"].to(gpu_device), ctx, _step=step)


@pytest.mark.parametrize("arch,C,cfg,method,points", [("DiT-PixArt-PCD-CLAY-B", 3, True, "euler", 25),
                                                      ("DiT-PixArt-PCD-CLAY-B", 3, False, "dopri5", 9),
                                                      ("DiT-PixArt-PCD-CLAY-L", 3, False, "euler", 25)])
def test_full_depth_sampling_trajectory_against_the_fp32_oracle(gpu_device, arch, C, cfg, method, points):
    """BASELINE.json configs[2] at REAL depth: the release denoisers (DiT-B depth 12 / DiT-L depth 24, seeded weights of SURVEY 8d
    config #3) integrated from t = 0 to t = 1 through the HIP path -- bf16 MFMA operands, the fused Euler step / the device-resident
    dopri5 -- against the all-fp32 trajectory: oracle/dit.py integrated by oracle/ode.py on the CPU
    (/root/reference/transport/integrators.py:100-119 over /root/reference/dit/dit_i23d.py:1537-1546).  Euler over 25 grid points
    (24 evaluations, guided for B) and the reference's default dopri5 (rtol 1e-3, atol 1e-6) to t = 1; the quantity asserted and
    printed is the relative L2 distance of the END state (and of every saved state).  Bar 3e-2: one evaluation sits at ~6e-3 of the
    fp32 output (test_release_models_full_depth_against_oracle), the drift over a trajectory is measured here (printed)."""
    from gaussiananything_amd.transport import Sampler, create_transport
    from oracle import trajectory as otraj
    model, sd = otraj.release_model(arch, C)
    x0, ctx = otraj.release_inputs(C, cfg=cfg)
    stats_o = {}
    ref = otraj.integrate(sd, x0, ctx, 4.0, method, points, cfg=cfg, threads=min(64, len(os.sched_getaffinity(0))), stats=stats_o)
    model.to(gpu_device)
    sampler = Sampler(create_transport("GVP", "velocity", None, None, None, snr_type="uniform"))
    fn = sampler.sample_ode(sampling_method=method, num_steps=points, atol=1e-6, rtol=1e-3)
    with torch.no_grad():
        out = fn(x0.to(gpu_device), model.forward_with_cfg if cfg else model.forward_cond,
                 context={k: v.to(gpu_device) for k, v in ctx.items()}, cfg_scale=4.0)
    st = dict(sampler.last_ode.last_stats)
    assert out.shape == ref.shape
    got = out.double().cpu().numpy()
    end = otraj.rel_l2(got[-1], ref[-1])
    worst = max(otraj.rel_l2(got[i], ref[i]) for i in range(1, points))
    moved = otraj.rel_l2(ref[-1], ref[0])
    print(f"\n{arch} {method} x {points} points (cfg {cfg}): end-state rel. L2 {end:.3e}, worst saved state {worst:.3e}; "
          f"the state moved by {moved:.2f} of its norm; evaluations HIP {st.get('nfe')} / oracle {stats_o.get('nfe')}, "
          f"rejected {st.get('rejected')} / {stats_o.get('rejected')}")
    assert moved > 0.05                                # (a trajectory that does not move would prove nothing)
    assert end < 3e-2 and worst < 3e-2, (end, worst)
    if method == "euler":
        assert st["nfe"] == stats_o["nfe"] == points - 1 and st.get("fused")
    else:
        assert st.get("device_loop") and st["nfe"] >= 7 and stats_o["nfe"] >= 7


def test_sampling_calls_from_two_streams_and_two_threads_on_one_module(gpu_device):
    """The workspace, the cached K / V, the resident conditioning and the captured sampler steps belong to the module
    (/root/reference/nsr/lsgm/flow_matching_trainer.py:700-744 samples one request at a time; a serving loop with overlap would not).
    (i) Two sampling calls issued back to back from two different streams, with nothing synchronised in between, give the results of
    the same calls run one after the other: the second call's stream waits for the event behind the first call's work.
    (ii) A second host thread entering the module while a call is in progress gets a RuntimeError instead of shared buffers."""
    import threading
    from gaussiananything_amd.transport import Sampler, create_transport
    z, model, ctx = _load_golden(1, gpu_device)
    x = z["x"].to(gpu_device)
    ctx2 = {k: (v * 0.5).contiguous() for k, v in ctx.items()}
    sampler = Sampler(create_transport("GVP", "velocity", None, None, None, snr_type="uniform"))

    def run(xx, cc, method):
        fn = sampler.sample_ode(sampling_method=method, num_steps=12, atol=1e-6, rtol=1e-3)
        with torch.no_grad():
            return fn(xx, model.forward_with_cfg, context=cc, cfg_scale=z["cfg_scale"])

    for method in ("euler", "dopri5"):
        want_a = run(x, ctx, method).clone()
        torch.cuda.synchronize()
        want_b = run(0.7 * x, ctx2, method).clone()
        torch.cuda.synchronize()
        sa, sb = torch.cuda.Stream(gpu_device), torch.cuda.Stream(gpu_device)
        for rep in range(3):
            with torch.cuda.stream(sa):
                got_a = run(x, ctx, method)
            with torch.cuda.stream(sb):              # (no synchronisation: stream sb would race stream sa's replays without the event)
                got_b = run(0.7 * x, ctx2, method)
            torch.cuda.synchronize()
            assert torch.equal(got_a, want_a) and torch.equal(got_b, want_b), (method, rep)
    # (ii) another thread while a call is in progress
    seen = {}
    inside, leave = threading.Event(), threading.Event()
    real = model._forward

    def slow_forward(*a, **k):
        inside.set()
        leave.wait(20)
        return real(*a, **k)

    def first():
        try:
            model._forward = slow_forward
            with torch.no_grad():
                seen["first"] = model(x, z["t"].to(gpu_device), ctx)
        finally:
            model._forward = real

    th = threading.Thread(target=first)
    th.start()
    assert inside.wait(20)
    with pytest.raises(RuntimeError, match="one module per concurrent sampling loop"):
        with torch.no_grad():
            model(x, z["t"].to(gpu_device), ctx)
    leave.set()
    th.join(30)
    with torch.no_grad():
        again = model(x, z["t"].to(gpu_device), ctx)
    assert torch.equal(again, seen["first"])


def test_cpu_tensors_raise(gpu_device):
    z, model, ctx = _load_golden(1, gpu_device)
    with pytest.raises(RuntimeError):
        model(z["x"], z["t"], {k: v.cpu() for k, v in ctx.items()})


@pytest.mark.parametrize("method", ["euler", "heun2"])
def test_sampler_graph_replay_equals_eager_loop(gpu_device, method, monkeypatch):
    """The fixed-grid sampler captures one step into a HIP graph and replays it; the eager Python loop (GA_ODE_GRAPH=0)
    is the reference for it.  Euler is the same arithmetic (bit-identical); heun2 forms t1 in fp32 on the device."""
    from gaussiananything_amd.transport import Sampler, create_transport
    z, model, ctx = _load_golden(1, gpu_device)
    x = z["x"].to(gpu_device)
    sampler = Sampler(create_transport("GVP", "velocity", None, None, None, snr_type="uniform"))
    outs = {}
    for flag in ("0", "1"):   # "1": a refused capture raises instead of silently falling back
        monkeypatch.setenv("GA_ODE_GRAPH", flag)
        fn = sampler.sample_ode(sampling_method=method, num_steps=7)
        with torch.no_grad():
            outs[flag] = fn(x, model.forward_with_cfg, context=ctx, cfg_scale=z["cfg_scale"])
    assert outs["1"].shape == (7,) + tuple(x.shape)
    if method == "euler":
        assert torch.equal(outs["0"], outs["1"])
        assert sampler.last_ode.last_stats.get("fused")      # the on-device step (GaDitSamplerStep) was the one replayed
        held = model._samplers.held("euler").graph                  # a second call on the same conditioning replays the captured step
        with torch.no_grad():
            again = fn(x, model.forward_with_cfg, context=ctx, cfg_scale=z["cfg_scale"])
            other = fn(2.0 * x, model.forward_with_cfg, context=ctx, cfg_scale=z["cfg_scale"])
        assert model._samplers.held("euler").graph is held and torch.equal(again, outs["1"]) and not torch.equal(other[-1], again[-1])
    else:
        assert rel_l2(outs["1"], outs["0"]) < 1e-5


def _three_sampler_kinds(model, z, ctx, device):
    """the three device-resident samplers on the stage-1 golden (CFG state [4, 48, 3]): kind -> call returning (states, dopri5's ctl block)"""
    from gaussiananything_amd.transport import Sampler, create_transport
    sampler = Sampler(create_transport("GVP", "velocity", None, None, None, snr_type="uniform"))
    x = z["x"].to(device)
    assert tuple(x.shape) == (4, 48, 3)
    pairs = torch.cat([x[:2], x[:2]], 0)
    kw = dict(context=ctx, cfg_scale=z["cfg_scale"])

    def euler():
        return sampler.sample_ode(sampling_method="euler", num_steps=7)(x, model.forward_with_cfg, **kw), None

    def dopri5():
        out = sampler.sample_ode(sampling_method="dopri5", num_steps=9, atol=1e-6, rtol=1e-3)(x, model.forward_with_cfg, **kw)
        assert sampler.last_ode.last_stats.get("device_loop")
        return out, list(sampler.last_ode.last_stats["ctl"])

    def sde():
        out = sampler.sample_sde(num_steps=7, seed=5)(pairs, model.forward_with_cfg, **kw)
        assert sampler.last_sde.last_stats.get("fused") is True
        return out, None

    return {"euler": euler, "dopri5": dopri5, "sde": sde}


def test_interleaved_sampler_kinds_keep_their_held_steps(gpu_device):
    """Euler, dopri5 and the SDE sampler called in turn on one module, then again in another order: a call of one kind does not evict the
    captured step of another (the same graph object serves both rounds), and every second result is the first one's, bit for bit."""
    z, model, ctx = _load_golden(1, gpu_device)
    calls = _three_sampler_kinds(model, z, ctx, gpu_device)
    first, graphs = {}, {}
    with torch.no_grad():
        for kind in ("euler", "dopri5", "sde"):
            first[kind] = calls[kind]()
            graphs[kind] = model._samplers.held(kind).graph
        assert all(g is not None for g in graphs.values())
        for kind in ("sde", "euler", "dopri5"):
            out, ctl = calls[kind]()
            assert model._samplers.held(kind).graph is graphs[kind], kind
            assert torch.equal(out, first[kind][0]), kind
            assert ctl == first[kind][1], kind
    assert len(first["dopri5"][1]) > 0
    assert all(model._samplers.held(kind).graph is graphs[kind] for kind in graphs)


def test_a_weight_change_drops_the_held_sampler_steps(gpu_device):
    """A step captured for one weight pack has that pack's weight copies baked in by address: after an in-place weight change every
    kind captures anew, and computes what a freshly constructed module with the changed weights computes -- not what it did before."""
    from gaussiananything_amd.dit import DiT_I23D_PCD_PixelArt_noclip
    z, model, ctx = _load_golden(1, gpu_device)
    calls = _three_sampler_kinds(model, z, ctx, gpu_device)
    kinds = ("euler", "dopri5", "sde")
    with torch.no_grad():
        before = {kind: calls[kind]() for kind in kinds}
        graphs = {kind: model._samplers.held(kind).graph for kind in kinds}
        assert all(g is not None for g in graphs.values())
        w = model.blocks[0].mlp.mlp[2].weight          # fc2 of the first block: non-zero in the golden
        assert float(w.abs().max()) > 0.0
        w.mul_(1.5)
        after = {}
        for kind in kinds:
            after[kind] = calls[kind]()
            assert model._samplers.held(kind).graph is not None and model._samplers.held(kind).graph is not graphs[kind], kind
        fresh = DiT_I23D_PCD_PixelArt_noclip(**z["kwargs"])
        fresh.load_state_dict(model.state_dict(), strict=True)
        fresh.to(gpu_device)
        want = {kind: call() for kind, call in _three_sampler_kinds(fresh, z, ctx, gpu_device).items()}
    for kind in kinds:
        assert torch.equal(after[kind][0], want[kind][0]), kind
        assert after[kind][1] == want[kind][1], kind
        assert not torch.equal(after[kind][0], before[kind][0]), kind
    assert len(after["dopri5"][1]) > 0


@pytest.mark.parametrize("stage", [1, 2])
def test_fused_euler_step_without_guidance_equals_eager_loop(gpu_device, stage, monkeypatch):
    """forward_cond (guidance is a no-op: the release's stage 2) through the fused on-device Euler step, against the eager
    loop over the same callable: bit-identical states at every grid point."""
    from gaussiananything_amd.transport import Sampler, create_transport
    z, model, ctx = _load_golden(stage, gpu_device)
    half = z["x"].shape[0] // 2
    x = z["x"][:half].to(gpu_device)
    c = {k: v[:half].contiguous() for k, v in ctx.items()}
    sampler = Sampler(create_transport("GVP", "velocity", None, None, None, snr_type="uniform"))
    outs = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("GA_ODE_GRAPH", flag)
        fn = sampler.sample_ode(sampling_method="euler", num_steps=9)
        with torch.no_grad():
            outs[flag] = fn(x, model.forward_cond, context=c, cfg_scale=z["cfg_scale"])
    assert torch.equal(outs["0"], outs["1"]) and sampler.last_ode.last_stats.get("fused")


@pytest.mark.parametrize("width,heads", [(768, 12), (1152, 16)])
def test_weight_prefetch_and_tail_placement_are_bit_neutral(gpu_device, width, heads):
    """Round 6: the weight prefetch by the idle workgroups of the cross-attention launch (GA_DIT_PREFETCH), the placement of the shift
    rows behind each block's own cross-attention grid (GA_DIT_SB_ON_CA), the tile -> XCD blocking (GA_GEMM_XMAP) and the write-through
    output stores (GA_GEMM_WT) change where and when bytes move, never a result: a DiT-B-shaped model (12 tile columns: the blocking
    applies) evaluated in fresh processes with everything off and everything on gives the same bits.  (The switches are read once per
    process, hence the subprocesses.)  Width 1152 / heads of 72: the same for the prefetch tail of the head-dim-generic cross-attention launch."""
    import subprocess
    import sys
    code = """
import hashlib, sys, torch
sys.path.insert(0, %r)
from gaussiananything_amd.dit import DiT_I23D_PCD_PixelArt_noclip
torch.manual_seed(0)
m = DiT_I23D_PCD_PixelArt_noclip(input_size=16, patch_size=1, in_channels=3, hidden_size=%d, depth=3, num_heads=%d, num_classes=0, learn_sigma=False,
                                 context_dim=1024, pooling_ctx_dim=768, roll_out=True, use_clay_ca=True)
g = torch.Generator().manual_seed(1)
with torch.no_grad():
    for p in m.parameters():
        if float(p.abs().max()) == 0.0:
            p.copy_(torch.randn(p.shape, generator=g) * 0.02)
x = torch.randn(2, 768, 3, generator=g); t = torch.tensor([0.4, 0.4])
ctx = {"img_crossattn": torch.randn(2, 1369, 1024, generator=g), "img_vector": torch.randn(2, 1024, generator=g)}
ctx["img_crossattn"][1] = 0; ctx["img_vector"][1] = 0
m.cuda()
with torch.no_grad():
    y = m.forward_with_cfg(x.cuda(), t.cuda(), {k: v.cuda() for k, v in ctx.items()}, 4.0)
    y1 = m.forward(x[:1].cuda(), t[:1].cuda(), {k: v[:1].cuda() for k, v in ctx.items()})
print(hashlib.sha256(y.cpu().numpy().tobytes() + y1.cpu().numpy().tobytes()).hexdigest())
""" % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), width, heads)
    hashes = []
    # (where the shift rows are computed does change their summation order when a workgroup has fewer waves than the weights have K-tiles -- 18 at
    #  width 1152, 8 waves behind the self-attention grid, 16 in the launch of their own: GA_DIT_SBTAIL is not toggled here)
    for env in ({"GA_DIT_PREFETCH": "0", "GA_DIT_SB_ON_CA": "0", "GA_GEMM_XMAP": "0", "GA_GEMM_WT": "0"},
                {"GA_DIT_PREFETCH": "4", "GA_DIT_SB_ON_CA": "1", "GA_GEMM_XMAP": "1", "GA_GEMM_WT": "1"}, {}):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        hashes.append(out.stdout.strip().splitlines()[-1])
    assert hashes[0] == hashes[1] == hashes[2], hashes

