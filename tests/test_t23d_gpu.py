"""GPU tests of the caption-conditioned (text-to-3D) denoisers: ``DiT_PCD_PixelArt`` / ``DiT_PCD_PixelArt_tofeat`` against outputs of the
reference's own classes (tests/golden/make_t23d_golden.py), the folded and the unfolded launch sequence of block order 1, the exact
zero-caption skip, the fused samplers, and the cascade on caption conditioning.

The bars of the golden comparison are the ones tests/test_dit_gpu.py::test_model_matches_reference_golden holds the image twins to for the
same kind of comparison (bf16 MFMA forward against the reference's fp32 forward at depth <= 3)."""
import os
import subprocess
import sys
import tempfile

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = ["stage1", "stage2", "L1", "L2"]


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / (b.double().norm() + 1e-30))


def _load(name, device=None):
    from gaussiananything_amd import synthetic
    from gaussiananything_amd.dit import DiT_PCD_PixelArt, DiT_PCD_PixelArt_tofeat
    z = torch.load(synthetic.fixture_path(f"dit_t23d_ref_{name}.pt"))
    cls = DiT_PCD_PixelArt_tofeat if name.endswith("2") else DiT_PCD_PixelArt
    model = cls(**z["kwargs"])
    model.load_state_dict(synthetic.recipe_state_dict(z["keys"], z["recipe_seed"]), strict=True)
    if device is None:
        return z, model, None
    model.to(device)
    return z, model, {k: v.to(device) for k, v in z["context"].items()}


def _within_golden_bar(y, ycfg, z, what):
    ref, ref_cfg = z["y"].to(y.device), z["y_cfg"].to(y.device)
    e, emax, ecfg = rel_l2(y, ref), float((y - ref).abs().max()), rel_l2(ycfg, ref_cfg) if ycfg is not None else 0.0
    print(f"{what}: rel_l2 {e:.3e} (bar 1.5e-2), max|d| {emax:.3e} (bar {5e-2 * float(ref.abs().max()):.3e}), cfg rel_l2 {ecfg:.3e} (bar 3e-2)")
    assert e < 1.5e-2, e
    assert emax < 5e-2 * float(ref.abs().max())
    assert ecfg < 3e-2, ecfg


@pytest.mark.parametrize("name", FIXTURES)
def test_text_model_matches_reference_golden(gpu_device, name):
    """forward, a second forward (the cached K / V path: bit-equal) and forward_with_cfg against the reference's own classes (fp32, CPU).
    stage1 / stage2: width 128, the unfolded sequence; L1 / L2: release width, the folded one."""
    z, model, ctx = _load(name, gpu_device)
    x, t = z["x"].to(gpu_device), z["t"].to(gpu_device)
    with torch.no_grad():
        y = model(x, t, ctx)
        y2 = model(x, t, ctx)
        ycfg = model.forward_with_cfg(x, t, ctx, z["cfg_scale"])
    assert y.dtype == torch.float32 and y.shape == z["y"].shape
    assert torch.equal(y, y2)
    assert model._pooled_cache is not None          # cap_embedder(caption_vector): once per conditioning vector
    model.pooled_once = False
    with torch.no_grad():
        assert torch.equal(model(x, t, ctx), y)
    model.pooled_once = True
    _within_golden_bar(y, ycfg, z, name)


_CHILD = """
import sys, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
from test_t23d_gpu import _load
z, m, ctx = _load({name!r}, 'cuda:0')
with torch.no_grad():
    y = m(z['x'].to('cuda:0'), z['t'].to('cuda:0'), ctx)
    ycfg = m.forward_with_cfg(z['x'].to('cuda:0'), z['t'].to('cuda:0'), ctx, z['cfg_scale'])
torch.save((y.cpu(), ycfg.cpu()), {out!r})
"""


def _forward_in_child(name, env):
    """the same forward in a fresh process (the launch-sequence switches are read once per process)"""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "y.pt")
        code = _CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), name=name, out=out)
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return torch.load(out)


@pytest.mark.parametrize("name", ["L1", "L2"])
def test_folded_and_unfolded_sequences_of_block_order_1(gpu_device, name):
    """Release width: the three pre-norm folds re-wired for self-attention -> cross-attention -> MLP, and in a child process
    (GA_DIT_FOLD_MOD=0) the same blocks with the norms as launches of their own.  Both at the golden bar, close, and not the same bits."""
    z, model, ctx = _load(name, gpu_device)
    x, t = z["x"].to(gpu_device), z["t"].to(gpu_device)
    with torch.no_grad():
        y = model(x, t, ctx)
        ycfg = model.forward_with_cfg(x, t, ctx, z["cfg_scale"])
    _within_golden_bar(y, ycfg, z, name + " folded")
    y_unf, ycfg_unf = _forward_in_child(name, {"GA_DIT_FOLD_MOD": "0"})
    _within_golden_bar(y_unf, ycfg_unf, z, name + " unfolded")
    d = rel_l2(y.cpu(), y_unf)
    print(f"{name}: folded vs unfolded rel_l2 {d:.3e}")
    assert d < 1e-2 and not torch.equal(y.cpu(), y_unf)


@pytest.mark.parametrize("name", ["L1"])
def test_tail_placement_of_block_order_1_is_bit_neutral(gpu_device, name):
    """The weight prefetch behind the cross-attention grid (GA_DIT_T_PREFETCH on / off) moves bytes, never a result -- with the
    short-context kernel on the cross-attention and with the long-list one."""
    for short in ("2", "0"):
        outs = [_forward_in_child(name, {"GA_DIT_T_PREFETCH": v, "GA_DIT_SHORT_CA": short})[0] for v in ("0", "1")]
        assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("name", ["L1", "L2"])
def test_short_context_switch_stays_within_the_golden_bar(gpu_device, name):
    """The release-width model with the cross-attention on the long-list kernel (GA_DIT_SHORT_CA=0), on the short-context kernel where
    its grid leaves the prefetch tail its CUs (1, the default: one sample's conditional half takes it) and always (2), in child
    processes: every one within the golden bar; 0 and 1 are different kernels (not the same bits)."""
    z = _load(name)[0]
    outs = {}
    for v in ("0", "1", "2"):
        y, ycfg = _forward_in_child(name, {"GA_DIT_SHORT_CA": v})
        _within_golden_bar(y, ycfg, z, f"{name} GA_DIT_SHORT_CA={v}")
        outs[v] = y
    assert not torch.equal(outs["0"], outs["1"])
    assert torch.equal(outs["1"], outs["2"])
    assert rel_l2(outs["1"], outs["0"]) < 1e-2


@pytest.mark.parametrize("name", ["stage1", "L1"])
def test_zero_caption_items_skip_cross_attention_exactly(gpu_device, name):
    """RMSNorm(0) = 0 and to_k / to_v have no bias: a zero caption's cross-attention is ``x += to_out.bias``; those items skip the work,
    bit-identically, and not when a zero item precedes a non-zero one."""
    z, model, ctx = _load(name, gpu_device)
    x, t = z["x"].to(gpu_device), z["t"].to(gpu_device)
    B = x.shape[0]
    tok = ctx["caption_crossattn"]
    assert float(tok[B // 2:].abs().max()) == 0.0 and float(tok[:B // 2].abs().max()) > 0.0
    with torch.no_grad():
        y_skip = model(x, t, ctx)
        assert model._ctx_cache[1][2] == B // 2
        model.ca_skip = False
        model._ctx_cache = None
        y_full = model(x, t, ctx)
        assert model._ctx_cache[1][2] == B
        # the items that skipped are bit-identical at every width.  The items that take part are too while the smaller cross-attention batch
        # launches the same kernel configuration (the small model, as in the image twin of this test); at release width one item of two
        # moves the launch from <8,2> with a GEMM q projection to <4,3> with the projection inside: the same values to bf16 rounding
        assert torch.equal(y_skip[B // 2:], y_full[B // 2:])
        if name == "stage1":
            assert torch.equal(y_skip, y_full)
        else:
            assert rel_l2(y_skip[:B // 2], y_full[:B // 2]) < 1e-2
        model.ca_skip = True
        flipped = {k: v.flip(0).contiguous() for k, v in ctx.items()}           # zero items first: no skipping
        y_flip = model(x.flip(0).contiguous(), t, flipped)
        assert model._ctx_cache[1][2] == B
        if name == "stage1":
            assert torch.equal(y_flip.flip(0), y_full)
        else:
            # the folded sequence carries the shift of a modulated pre-norm through the projection weights as one bias row per batch item
            # (ga_dit_shift_bias), and that kernel -- shared with the image models, untouched here -- serves the batch in PAIRS: the even
            # and the odd member of a pair get differently contracted sums, an ulp apart.  An item that moves from batch position 0 to 1
            # therefore gets bias rows that differ in the last bit, and 2 blocks of bf16 rounding carry that to 1e-3 of the output;
            # every GEMM of the chain is position-independent (test_where_the_batch_position_enters_the_folded_sequence pins both facts)
            assert rel_l2(y_flip.flip(0), y_full) < 1e-2


def test_where_the_batch_position_enters_the_folded_sequence(gpu_device):
    """Evidence for the comment above, at release width, op by op through the C ABI: the shift rows of ga_dit_shift_bias are bit-identical
    for batch positions of the same parity (0 and 2, 1 and 3) and differ by rounding only -- at most a few ulps of the row's scale --
    between an even and an odd position; the producer GEMM (gated residual + modulated emit + row sums) and the consumer GEMMs (row
    scale, per-batch bias rows, per-head norms, V^T store; GELU) give every batch item the same bits wherever it sits."""
    from gaussiananything_amd import dit_ops as ops
    dev = gpu_device
    g = torch.Generator().manual_seed(0)
    D, L, B = 1024, 768, 2
    W = (torch.randn(3 * D, D, generator=g) / 32).bfloat16().to(dev)
    Wt = ops.tile_weight(W)
    bias = torch.randn(3 * D, generator=g).to(dev)
    sh = torch.randn(B, D, generator=g).to(dev)
    rows4 = ops.shift_bias(Wt, torch.cat([sh, sh]), bias, w_tiled=True, N=3 * D)          # items 0, 1 again at positions 2, 3
    assert torch.equal(rows4[0], rows4[2]) and torch.equal(rows4[1], rows4[3])
    flipped = ops.shift_bias(Wt, sh.flip(0).contiguous(), bias, w_tiled=True, N=3 * D).flip(0)
    gap = float((flipped - rows4[:2]).abs().max())
    print(f"shift rows, even vs odd pair member: max |d| {gap:.3e} on rows of scale {float(rows4.abs().max()):.2f}")
    assert gap <= 8 * 2.0 ** -23 * float(rows4.abs().max())          # rounding, not a wrong row
    fl = lambda t: t.reshape(B, -1, t.shape[-1]).flip(0).reshape(t.shape).contiguous()          # noqa: E731
    A = torch.randn(B * L, D, generator=g).bfloat16().to(dev)
    Wp = ops.tile_weight((torch.randn(D, D, generator=g) / 32).bfloat16().to(dev))
    x0, gate = torch.randn(B * L, D, generator=g).to(dev), torch.randn(B, D, generator=g).to(dev)
    ew, es, pb = (1 + 0.1 * torch.randn(D, generator=g)).to(dev), (0.1 * torch.randn(B, D, generator=g)).to(dev), torch.randn(D, generator=g).to(dev)

    def producer(A, x0, gate, es):
        x, ex, ss = x0.clone(), torch.empty(B * L, D, dtype=torch.bfloat16, device=dev), torch.empty(B * L, 16, device=dev)
        ops.gemm(A, Wp, pb, ops.EPI_RESIDUAL, out=x, gate=gate, rows_per_batch=L, emit_x=ex, emit_ss=ss, w_tiled=True, N=D, emit_w=ew, emit_scale=es)
        return x, ex, ss

    p = producer(A, x0, gate, es)
    q = producer(fl(A), fl(x0), gate.flip(0).contiguous(), es.flip(0).contiguous())
    assert all(torch.equal(u, fl(v)) for u, v in zip(p, q))
    brow, wn = torch.randn(B, 3 * D, generator=g).to(dev), (1 + 0.1 * torch.randn(64, generator=g)).to(dev)

    def qkv(ex, ss, brow):
        vt = torch.zeros(B * D, L, dtype=torch.bfloat16, device=dev)
        o = ops.gemm(ex, Wt, brow, ops.EPI_STORE_BF16, rows_per_batch=L, vt=vt, vt_col0=2 * D, qk_w0=wn, qk_cols0=D, qk_w1=wn, qk_cols1=2 * D,
                     row_ss=ss, row_ss_dim=D, w_tiled=True, N=3 * D)
        return o, vt

    c1, c2 = qkv(p[1], p[2], brow), qkv(fl(p[1]), fl(p[2]), brow.flip(0).contiguous())
    assert torch.equal(c1[0], fl(c2[0])) and torch.equal(c1[1], c2[1].reshape(B, D, L).flip(0).reshape(B * D, L))
    W1, b1 = ops.tile_weight((torch.randn(4 * D, D, generator=g) / 32).bfloat16().to(dev)), torch.randn(B, 4 * D, generator=g).to(dev)
    g1 = ops.gemm(p[1], W1, b1, ops.EPI_GELU_BF16, rows_per_batch=L, row_ss=p[2], row_ss_dim=D, w_tiled=True, N=4 * D)
    g2 = ops.gemm(fl(p[1]), W1, b1.flip(0).contiguous(), ops.EPI_GELU_BF16, rows_per_batch=L, row_ss=fl(p[2]), row_ss_dim=D, w_tiled=True, N=4 * D)
    assert torch.equal(g1, fl(g2))


def test_fused_euler_on_the_text_model_equals_the_eager_loop(gpu_device):
    """sample_euler_fused over a 10-point grid -- the FinalLayer variant of the fused sampler step: CFG combine and Euler update in the
    final-layer kernel -- is bit-identical to the eager loop of forward_with_cfg plus y += dt * v (rounding contract: include/ga_dit.h)."""
    z, model, ctx = _load("stage1", gpu_device)
    x = z["x"].to(gpu_device)
    x = torch.cat([x[:2], x[:2]], 0)                          # both CFG halves start from the same state
    grid = [float(v) for v in torch.linspace(0.0, 1.0, 10)]
    s = z["cfg_scale"]
    with torch.no_grad():
        fused = model.sample_euler_fused(x, grid, ctx, cfg_scale=s, cfg=True)
        y = x.clone().float()
        eager = [y.clone()]
        for t0, t1 in zip(grid[:-1], grid[1:]):
            tv = torch.full((x.shape[0],), t0, dtype=torch.float32, device=gpu_device)
            v = model.forward_with_cfg(y, tv, ctx, s)
            y = y + (t1 - t0) * v           # (the step size is formed on the host in fp64 and rounded once, as the fused grid is)
            eager.append(y.clone())
        again = model.sample_euler_fused(x, grid, ctx, cfg_scale=s, cfg=True)      # the replayed capture
    eager = torch.stack(eager)
    assert fused.shape == eager.shape
    assert torch.equal(fused, eager)
    assert torch.equal(again, fused)


def test_device_dopri5_on_the_text_model(gpu_device):
    """sample_dopri5_device on the text model against the host dopri5 loop (transport.odeint) on the same function, at the bar
    tests/test_dit_gpu.py::test_device_resident_dopri5_takes_the_decisions_of_the_host_loop holds the image twin to: no error word, the
    SAME decisions -- function evaluations, attempted and rejected steps -- and every requested state within rel_l2 < 2e-3 (a bf16
    function: an ulp of the fp32 state can round an operand the other way), i.e. inside the solve's own rtol of 1e-3 to a factor of two."""
    from gaussiananything_amd import dit_ops as ops
    from gaussiananything_amd.transport.odeint import odeint
    z, model, ctx = _load("stage1", gpu_device)
    x = z["x"].to(gpu_device)
    x = torch.cat([x[:2], x[:2]], 0)
    s, atol, rtol = z["cfg_scale"], 1e-6, 1e-3
    grid = [0.0, 0.25, 0.5, 0.75, 1.0]
    stats, hstats = {}, {}
    with torch.no_grad():
        dev = model.sample_dopri5_device(x, grid, ctx, cfg_scale=s, cfg=True, atol=atol, rtol=rtol, stats=stats)

        def f(tt, yy):
            tv = torch.ones(x.shape[0], device=gpu_device) * tt
            return model.forward_with_cfg(yy, tv, ctx, s)
        host = odeint(f, x.float(), torch.tensor(grid, device=gpu_device), method="dopri5", atol=atol, rtol=rtol, stats=hstats)
    d = rel_l2(dev, host)
    print(f"dopri5 device vs host: rel_l2 {d:.3e} (bar 2e-3); nfe {stats['nfe']} / {hstats['nfe']}, steps {stats['steps']} / {hstats['steps']}, "
          f"rejected {stats['rejected']} / {hstats['rejected']}")
    assert stats["ctl"][ops.GA_ODE_ERROR] == 0 and stats["steps"] > 0 and stats.get("device_loop")
    assert bool(torch.isfinite(dev).all()) and dev.shape == host.shape and torch.equal(dev[0], x.float())
    assert (stats["nfe"], stats["steps"], stats["rejected"]) == (hstats["nfe"], hstats["steps"], hstats["rejected"]), (stats, hstats)
    assert d < 2e-3, d


def test_cascade_on_caption_conditioning(gpu_device):
    """cascade() with caption conditioning, small synthetic text models and SurfelDecoder at its test size (as tests/test_decode_gpu.py
    builds it): finite latents, stage 2 REALLY guided (no noop_cfg_dedup), renders of the expected shapes, and the driver gives what
    its parts give when called one after the other."""
    from gaussiananything_amd import cascade, synthetic
    from gaussiananything_amd.decode import SurfelDecoder
    from gaussiananything_amd.dit import DiT_PCD_PixelArt, DiT_PCD_PixelArt_tofeat
    zd = torch.load(synthetic.fixture_path("decode_ref.pt"))
    cfg = zd["config"]
    dec = SurfelDecoder(embed_dim=cfg["D"], depth=cfg["depth"], num_heads=cfg["heads"], tokens=cfg["tokens"], ldm_z_channels=cfg["z_channels"])
    dec.load_state_dict(zd["state_dict"])
    dec.to(gpu_device)
    L = cfg["tokens"]
    kw = dict(input_size=8, patch_size=1, hidden_size=128, depth=2, num_heads=2, num_classes=0, learn_sigma=False, context_dim=64, roll_out=True)
    models = []
    for cls, cin, seed in ((DiT_PCD_PixelArt, 3, 11), (DiT_PCD_PixelArt_tofeat, cfg["z_channels"], 12)):
        m = cls(in_channels=cin, **kw)
        keys = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
        m.load_state_dict(synthetic.recipe_state_dict(keys, seed), strict=True)
        models.append(m.to(gpu_device))
    g = torch.Generator().manual_seed(3)
    cond, uc = cascade.condition_on_caption(torch.randn(1, 77, 64, generator=g).to(gpu_device), torch.randn(1, 64, generator=g).to(gpu_device))
    cams = synthetic.eval_cameras(2)
    c = {"cam_view": cams["cam_view"][None].to(gpu_device), "cam_view_proj": cams["cam_view_proj"][None].to(gpu_device),
         "cam_pos": cams["cam_pos"][None].to(gpu_device), "tanfov": cams["tanfov"]}
    s = cascade.T23D_CFG_SCALE
    stats = {}
    out = cascade.cascade(models[0], models[1], dec, cond, uc, cameras=c, cfg_scale=s, num_steps=6, sampling_method="euler", seed=3, stats=stats)
    assert "noop_cfg_dedup" not in stats["stage1"] and "noop_cfg_dedup" not in stats["stage2"]
    xyz = cascade.sample(models[0], cond, uc, (L, 3), 1, s, 3, 6, "euler")
    fps = (xyz * 0.164).clip(-0.45, 0.45)
    c2, uc2 = cascade.stage2_caption_conditioning(cond, uc, fps)
    lat = cascade.sample(models[1], c2, uc2, (L, cfg["z_channels"]), 1, s, 3, 6, "euler")
    assert bool(torch.isfinite(xyz).all()) and bool(torch.isfinite(lat).all()) and float(lat.abs().max()) > 0
    ref = dec.decode(lat, fps)
    assert torch.equal(out["query_pcd_xyz"], fps) and torch.equal(out["gaussians_upsampled_3"], ref["gaussians_upsampled_3"])
    assert set(out["renders"]) == set(dec.output_size)
    for key, size in dec.output_size.items():
        img = out["renders"][key]["image"]
        assert img.shape == (1, 2, 3, size, size) and bool(torch.isfinite(img).all())
