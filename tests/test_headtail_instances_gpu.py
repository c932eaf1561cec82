"""Every case of tests/_headtail_cases.py -- the kernels of csrc/dit_ops.hip that run only inside ga_dit_forward, ga_dit_cache_context_ws,
ga_dit_pooled_vector and ga_dit_sampler_advance -- on the GPU, checked ELEMENT-WISE against a float64 reference with the error model of
tests/_bounds.py (no fudge factor and no outlier allowance; tests/test_headtail_bounds_cpu.py shows that seeded kernel bugs land over it).

Everything goes through the existing C ABI with ctypes.  A small Python model gives the GaDitModel pack; the test works on a COPY of the
struct in which every pointer the case plants (the embedding, the conditioning path, the final layer, the blocks' tables / output
projections) leads to a tensor of its own, and makes its own GaDitForwardArgs, so it owns out, workspace, pooled_vec, fps_xyz and step.

Around every call, as tests/test_row_instances_gpu.py: every output is a view into a sentinel-filled buffer with a guard row in front and
behind; the inputs are followed by NaN (img_vector, which a forward with pooled_vec must not read, is all NaN); the workspace starts as
NaN and has guard words behind it; no stored element is non-finite; a second launch gives the same bits.  Once per model the premise of
the pass-through construction is asserted: every weight the case did not plant is re-randomised and the output must not change a bit."""
import ctypes
import math

import pytest
import torch

from tests import _headtail_cases as hc

pytestmark = pytest.mark.gpu

BF16_SENTINEL, F32_SENTINEL, I32_SENTINEL = 0x7FA5, 0x7FA5A5A5, 0x5A5A5A5A
OK, ERR_NULL_ARG, ERR_BAD_SHAPE = 0, -1, -2
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32


def _sentinel(rows, cols, dtype, dev):
    """[rows + 2, cols] of sentinel bits: the kernel gets the address of row 1"""
    if dtype == BF16:
        return torch.full((rows + 2, cols), BF16_SENTINEL, dtype=torch.int16, device=dev).view(BF16)
    if dtype == I32:
        return torch.full((rows + 2, cols), I32_SENTINEL, dtype=I32, device=dev)
    return torch.full((rows + 2, cols), F32_SENTINEL, dtype=torch.int32, device=dev).view(F32)


_SENT = {BF16: BF16_SENTINEL, F32: F32_SENTINEL, I32: I32_SENTINEL}


def _bits(t):
    return t if t.dtype == I32 else t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _tail(x, dtype, dev, n=16):
    """x flattened, followed by n NaN elements"""
    buf = torch.full((x.numel() + n,), math.nan, dtype=dtype, device=dev)
    buf[:x.numel()] = x.reshape(-1).to(dtype)
    return buf


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _copy(struct):
    out = type(struct)()
    ctypes.memmove(ctypes.byref(out), ctypes.byref(struct), ctypes.sizeof(out))
    return out


# --------------------------------------------------------------------------------------------------------------- the small models
_bases = {}


def _base(dev, text, D, depth):
    """(module, pack) of a small denoiser: heads of 64, ctx_tokens 8, context_dim 64; its zero-initialised parameters randomised"""
    key = (str(dev), text, D, depth)
    if key not in _bases:
        from gaussiananything_amd.dit import DiT_I23D_PCD_PixelArt_noclip
        from gaussiananything_amd.dit.dit_trilatent import DiT_PCD_PixelArt
        kw = dict(input_size=16, patch_size=1, in_channels=3, hidden_size=D, depth=depth, num_heads=D // 64, num_classes=0,
                  learn_sigma=False, context_dim=hc.CONTEXT_DIM, roll_out=True)
        with torch.random.fork_rng(devices=[]):                          # (the constructors draw from the global generator: left as it was)
            torch.manual_seed(D + depth)
            model = DiT_PCD_PixelArt(**kw) if text else DiT_I23D_PCD_PixelArt_noclip(pooling_ctx_dim=768, use_clay_ca=True, **kw)
        g = torch.Generator().manual_seed(5)
        with torch.no_grad():
            for p in model.parameters():
                if float(p.abs().max()) == 0.0:
                    p.copy_(torch.randn(p.shape, generator=g) * 0.02)
        _bases[key] = (model, model._prepare(dev))
    return _bases[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_the_models_afterwards():
    """the small models (the 2048-wide ones are 350 MB each) live for this file only"""
    yield
    _bases.clear()
    _premise_done.clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def _rerandomise(pack):
    """every tensor of the pack (the copies of the module's weights; the planted ones are not among them) scaled element by element"""
    g = torch.Generator().manual_seed(11)
    for t in pack["keep"]:
        t.copy_((t.float().cpu() * (0.5 + torch.rand(t.shape, generator=g))).to(t.dtype))
    torch.cuda.synchronize()


class _Planted:
    """a copy of the pack's GaDitModel in which the case's weights are planted; holds the tensors the struct points into"""

    def __init__(self, c, z, dev, pack, final_w, final_b):
        from gaussiananything_amd import dit_ops as ops
        stage2, depth, C, text = hc.forward_shape(c)
        D = c["D"]
        self.keep = keep = []

        def fp(t):
            keep.append(_tail(t, F32, dev))
            return keep[-1].data_ptr()

        def bf(t):
            keep.append(_tail(t, BF16, dev))
            return keep[-1].data_ptr()

        tiled = bool(pack["model"].gemm_weights_tiled)

        def gw(t):                                                       # a weight ga_gemm_bf16 reads, in the pack's layout
            t = t.to(device=dev, dtype=BF16)
            keep.append(ops.tile_weight(t) if tiled else t.contiguous())
            return keep[-1].data_ptr()

        m = self.model = _copy(pack["model"])
        assert m.hidden == D and m.depth == depth and m.context_dim == hc.CONTEXT_DIM
        m.in_channels, m.out_channels, m.stage2 = C, final_w.shape[0], 1 if stage2 else 0
        m.t_mlp2_w, m.t_mlp2_b = bf(torch.zeros(D, D)), fp(z["tb2"])
        if "adaln_w" in z:
            m.adaln_w, m.adaln_b = bf(z["adaln_w"]), fp(z["adaln_b"])
        else:
            m.adaln_w, m.adaln_b = bf(torch.zeros(6 * D, D)), fp(torch.zeros(6 * D))
        m.xe_fc1_w, m.xe_fc1_b = fp(z["w1"]), fp(z["b1"])
        m.xe_fc2_w, m.xe_fc2_b = gw(torch.eye(D)), fp(z["b2"])
        m.xyz_w, m.xyz_b = (fp(z["wx"]), fp(z["bx"])) if stage2 else (None, None)
        m.final_w, m.final_b = fp(final_w), fp(final_b)
        if text:
            m.final_table, m.final_adaln_w, m.final_adaln_b = None, bf(z["fmod_w"]), fp(z["fmod_b"])
        else:
            m.final_table = fp(z["table"])
        self.blocks = blocks = (ops.GaDitBlockWeights * depth)()
        zero_dd, zero_d = gw(torch.zeros(D, D)), fp(torch.zeros(D))
        zero_fc2 = gw(torch.zeros(D, 4 * D)) if "tables" in z else None
        for i in range(depth):
            blocks[i] = _copy(pack["blocks"][i])
            blocks[i].ca_out_w, blocks[i].ca_out_b = zero_dd, zero_d
            if "tables" in z:
                blocks[i].scale_shift_table = fp(z["tables"][i])
                blocks[i].proj_w, blocks[i].proj_b = zero_dd, fp(z["proj_b"][i])
                blocks[i].fc2_w, blocks[i].fc2_b = zero_fc2, fp(z["fc2_b"][i])
            else:
                blocks[i].scale_shift_table = fp(torch.zeros(6, D))
        m.blocks = ctypes.cast(blocks, ctypes.POINTER(ops.GaDitBlockWeights))


def _forward(c, z, dev, planted, step=None, x_buf=None):
    """one ga_dit_forward of the planted model: (rc, out sentinel buffer or None); the caller's step / state buffers are its own"""
    from gaussiananything_amd import dit_ops as ops
    stage2, depth, C, text = hc.forward_shape(c)
    D, B, L = c["D"], c["B"], c["L"]
    M, T, m = B * L, hc.CTX_TOKENS, planted.model
    Lib = ops.lib()
    nbytes = Lib.ga_dit_workspace_bytes(ctypes.byref(m), B, L, T)
    assert nbytes > 0
    guard = 64
    ws = torch.full((nbytes // 4 + 64 + guard,), math.nan, dtype=F32, device=dev)      # NaN where nothing has been written yet
    base = ws.data_ptr() + ((-ws.data_ptr()) % 256)
    first_guard = (base - ws.data_ptr()) // 4 + nbytes // 4
    _bits(ws)[first_guard:first_guard + guard] = F32_SENTINEL
    x = x_buf if x_buf is not None else _tail(z["x"], F32, dev)
    keep = [_tail(z["timesteps"], F32, dev), torch.full((B * hc.CONTEXT_DIM + 16,), math.nan, dtype=F32, device=dev),
            _tail(z["xyz"], F32, dev) if stage2 else None, torch.zeros(depth * B * T * D, dtype=BF16, device=dev),
            torch.zeros(depth * B * D * 64, dtype=BF16, device=dev), _tail(z["pooled"], F32, dev)]
    out = _sentinel(M, m.out_channels, F32, dev) if step is None else None
    a = ops.GaDitForwardArgs(B, L, T, x.data_ptr(), keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr() if stage2 else None,
                             keep[3].data_ptr(), keep[4].data_ptr(), out[1:].data_ptr() if out is not None else None, base, nbytes, 0,
                             ctypes.pointer(step) if step is not None else None, keep[5].data_ptr())
    r = Lib.ga_dit_forward(ctypes.byref(m), ctypes.byref(a), _stream(dev))
    torch.cuda.synchronize()
    assert bool((_bits(ws)[first_guard:first_guard + guard] == F32_SENTINEL).all()), f"{c['name']}: a store behind the workspace"
    return r, out


_premise_done = set()


def _premise(c, z, dev, text, run):
    """once per model: the blocks of the pass-through model are the exact identity -- nothing the case did not plant reaches the output"""
    key = (text, c["D"], hc.forward_shape(c)[1])
    if key in _premise_done:
        return
    _premise_done.add(key)
    before = run()
    _rerandomise(_base(dev, text, c["D"], hc.forward_shape(c)[1])[1])
    after = run()
    for n in before:
        assert torch.equal(_bits(before[n]), _bits(after[n])), f"{c['name']}: {n} depends on a weight the pass-through model does not plant"


# --------------------------------------------------------------------------------------------------------------- runners
def _run_sweep(c, z, dev):
    """embed / gates: D / 16 forwards, final_w one-hot on 16 columns each; the [M, D] matrix of what they show"""
    stage2, depth, C, text = hc.forward_shape(c)
    D, M = c["D"], c["B"] * c["L"]
    pack = _base(dev, text, D, depth)[1]
    y = _sentinel(M, D, F32, dev)
    for s in range(D // 16):
        r, out = _forward(c, z, dev, _Planted(c, z, dev, pack, hc.sweep_weight(D, s), z["final_b"]))
        assert r == OK, f"{c['name']}: ga_dit_forward returned {r}"
        assert bool((_bits(out[0]) == F32_SENTINEL).all()) and bool((_bits(out[M + 1]) == F32_SENTINEL).all()), f"{c['name']}: a store outside out"
        y[1:M + 1, 16 * s:16 * s + 16] = out[1:M + 1]
    return {"y": y}


def _run_final(c, z, dev):
    stage2, depth, C, text = hc.forward_shape(c)
    pack = _base(dev, text, c["D"], depth)[1]
    r, out = _forward(c, z, dev, _Planted(c, z, dev, pack, z["final_w"], z["final_b"]))
    assert r == OK, f"{c['name']}: ga_dit_forward returned {r}"
    return {"out": out}


def _step_buffers(c, z, dev):
    """(GaDitSamplerStep, outputs, x buffer, keep): the state is the x of the evaluation, a view into a sentinel buffer"""
    from gaussiananything_amd import dit_ops as ops
    M, C = c["B"] * c["L"], c["Cout"]
    outs, keep = {}, []
    if c["mode"] == "velocity":
        vel = _sentinel(M, C, F32, dev)
        outs["velocity"] = vel
        return ops.GaDitSamplerStep(c["s"], c["cfg"], None, None, None, 0, None, vel[1:].data_ptr()), outs, None, keep
    state = _sentinel(M, C, F32, dev)
    state[1:M + 1] = z["x"].to(F32)
    outs["state"] = state
    keep += [_tail(z["dt"], F32, dev), torch.tensor([z["counter"], I32_SENTINEL], dtype=I32, device=dev)]
    traj = None
    if c["mode"] == "euler":
        traj = _sentinel(z["slices"], M * C, F32, dev)
        traj[1:z["slices"] + 1] = hc.TRAJ_FILL
        outs["traj"] = traj
    st = ops.GaDitSamplerStep(c["s"], c["cfg"], keep[0].data_ptr(), state[1:].data_ptr(), traj[1:].data_ptr() if traj is not None else None,
                              M * C, keep[1].data_ptr(), None)
    return st, outs, state[1:], keep


def _run_step(c, z, dev):
    pack = _base(dev, 0, c["D"], 1)[1]
    st, outs, xbuf, keep = _step_buffers(c, z, dev)
    r, out = _forward(c, z, dev, _Planted(c, z, dev, pack, z["final_w"], z["final_b"]), step=st, x_buf=xbuf)
    assert r == OK and out is None, f"{c['name']}: ga_dit_forward returned {r}"
    if len(keep) > 1:
        assert keep[1].tolist() == [z["counter"], I32_SENTINEL], f"{c['name']}: the step moved its counter"
    if c["cfg"]:
        half = c["B"] * c["L"] // 2
        for n in ("velocity", "state"):
            if n in outs:
                assert torch.equal(_bits(outs[n][1:half + 1]), _bits(outs[n][half + 1:2 * half + 1])), f"{c['name']}: the CFG halves of {n} differ"
    return outs


def _run_pooled(c, z, dev):
    from gaussiananything_amd import dit_ops as ops
    B, K, D = c["batch"], c["ctx"], c["D"]
    m = _copy(_base(dev, 0, 64, 1)[1]["model"])
    keep = [_tail(z[n], BF16 if n == "W" else F32, dev) for n in ("ln_w", "ln_b", "W", "b", "x")]
    m.hidden, m.heads, m.context_dim = D, D // 64, K
    m.pool_ln_w, m.pool_ln_b, m.pool_w, m.pool_b = (t.data_ptr() for t in keep[:4])
    scratch, out = _sentinel(B, K, F32, dev), _sentinel(B, D, F32, dev)
    r = ops.lib().ga_dit_pooled_vector(ctypes.byref(m), B, keep[4].data_ptr(), scratch[1:].data_ptr(), out[1:].data_ptr(), _stream(dev))
    torch.cuda.synchronize()
    assert r == OK, f"{c['name']}: ga_dit_pooled_vector returned {r}"
    return {"scratch": scratch, "out": out}


def _ctx_model(c, z, dev):
    from gaussiananything_amd import dit_ops as ops
    pack = _base(dev, 1, 64, c["depth"])[1]
    m = _copy(pack["model"])
    K, D = c["ctx"], 64
    m.context_dim = K
    g = torch.Generator().manual_seed(K)
    kv = (torch.randn(2 * D, K, generator=g) / math.sqrt(K)).to(device=dev, dtype=BF16)
    keep = [ops.tile_weight(kv) if m.gemm_weights_tiled else kv]
    blocks = (ops.GaDitBlockWeights * c["depth"])()
    for i in range(c["depth"]):
        blocks[i] = _copy(pack["blocks"][i])
        keep.append(_tail(z["w"][i], F32, dev))
        blocks[i].ctx_norm_w, blocks[i].ca_kv_w = keep[-1].data_ptr(), keep[0].data_ptr()
    m.blocks = ctypes.cast(blocks, ctypes.POINTER(ops.GaDitBlockWeights))
    return m, keep + [blocks]


def _run_ctxnorm(c, z, dev):
    from gaussiananything_amd import dit_ops as ops
    B, T, K, D, depth = c["B"], c["T"], c["ctx"], 64, c["depth"]
    rows, Mp = B * T, (T + 63) // 64 * 64
    m, keep = _ctx_model(c, z, dev)
    need = ops.lib().ga_dit_context_scratch_bytes(ctypes.byref(m), B, T)
    assert need >= rows * K * 2 and need % 256 == 0
    # the scratch as the rows of a [rows + 2, K] sentinel buffer whose row 1 sits on a 256-byte boundary: the guard row in front is the 128
    # elements before it, everything behind the written rows (the alignment pad included) must stay sentinel
    flat = torch.full((128 + need // 2 + 128,), BF16_SENTINEL, dtype=torch.int16, device=dev).view(BF16)
    assert flat.data_ptr() % 256 == 0
    ctx = _tail(z["x"], BF16, dev, n=K)
    ck = torch.zeros(depth * rows * D, dtype=BF16, device=dev)
    cvt = torch.zeros(depth * B * D * Mp, dtype=BF16, device=dev)
    r = ops.lib().ga_dit_cache_context_ws(ctypes.byref(m), B, T, ctx.data_ptr(), ck.data_ptr(), cvt.data_ptr(), flat[128:].data_ptr(), need,
                                          _stream(dev))
    torch.cuda.synchronize()
    assert r == OK, f"{c['name']}: ga_dit_cache_context_ws returned {r}"
    assert bool(torch.isfinite(ck.float()).all()) and bool(torch.isfinite(cvt.float()).all()), f"{c['name']}: non-finite K / V^T"
    assert bool((_bits(flat[:128]) == BF16_SENTINEL).all()) and bool((_bits(flat[128 + rows * K:]) == BF16_SENTINEL).all()), \
        f"{c['name']}: a store outside the scratch rows"
    buf = _sentinel(rows, K, BF16, dev)
    buf[1:rows + 1] = flat[128:128 + rows * K].view(rows, K)
    return {"scratch": buf}


def _run_advance(c, z, dev):
    from gaussiananything_amd import dit_ops as ops
    batch, n = c["batch"], c["grid_len"]
    keep = [_tail(z["t_grid"], F32, dev), _tail(z["dt_grid"], F32, dev)]
    ts, dt, counter = _sentinel(1, batch, F32, dev), _sentinel(1, 1, F32, dev), _sentinel(1, 1, I32, dev)
    counter[1, 0] = c["counter"]
    r = ops.lib().ga_dit_sampler_advance(counter[1:].data_ptr(), keep[0].data_ptr(), keep[1].data_ptr(), n, ts[1:].data_ptr(), batch,
                                         dt[1:].data_ptr(), _stream(dev))
    torch.cuda.synchronize()
    assert r == OK, f"{c['name']}: ga_dit_sampler_advance returned {r}"
    return {"timesteps": ts, "dt": dt, "counter": counter}


RUN = {"embed": _run_sweep, "gates": _run_sweep, "final": _run_final, "step": _run_step, "pooled": _run_pooled, "ctxnorm": _run_ctxnorm,
       "advance": _run_advance}


@pytest.mark.parametrize("case", hc.ALL, ids=[c["name"] for c in hc.ALL])
def test_head_and_tail_kernels_elementwise_against_float64(gpu_device, case):
    dev, c = gpu_device, case
    z = hc.inputs(c)
    refs = hc.reference(c, z)                                            # (asserts what the case reaches before anything is launched)
    run = RUN[c["kernel"]]
    outs = run(c, z, dev)
    again = run(c, z, dev)
    for n in outs:
        assert torch.equal(_bits(outs[n]), _bits(again[n])), f"{c['name']}: {n} not bit-identical to the first launch"
    if c["kernel"] in ("embed", "gates", "final", "step"):
        _premise(c, z, dev, hc.forward_shape(c)[3], lambda: run(c, z, dev))
    worst = {}
    for n, (ref, bound) in refs.items():
        buf, rows = outs[n], ref.shape[0]
        sent = _SENT[buf.dtype]
        assert bool((_bits(buf[0]) == sent).all()) and bool((_bits(buf[rows + 1]) == sent).all()), f"{c['name']}: a store outside {n}"
        got = buf[1:rows + 1].to(torch.float64).cpu()
        assert bool(torch.isfinite(got).all()), f"{c['name']}: {int((~torch.isfinite(got)).sum())} non-finite elements of {n}"
        worst[n] = hc.worst_ratio(got, ref, bound)
        if worst[n] > 1.0:
            ratio = torch.where(got == ref, torch.zeros_like(ref), (got - ref).abs() / bound)
            i = int(ratio.argmax())
            idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape))
            pytest.fail(f"{c['name']}: {int((ratio > 1).sum())} of {ratio.numel()} elements of {n} over their bound; worst at {idx}: got "
                        f"{float(got[idx]):.9g}, ref {float(ref[idx]):.9g}, bound {float(bound[idx]):.3g} ({worst[n]:.3g} x)")
    note = ""
    if "y" in refs:       # seen through one mirrored bf16 rounding: how many elements sit on the other side of a rounding boundary
        got, ref = outs["y"][1:-1].to(torch.float64).cpu(), refs["y"][0]
        note = f" ({int(((got - ref).abs() > 2.0 ** -21 * ref.abs()).sum())} of {ref.numel()} one bf16 ulp off the mirror)"
    print(f"HEADTAIL {c['name']:72s} | " + ", ".join(f"{n} {v:.3f}" for n, v in worst.items()) + note)


def test_entry_points_refuse_what_the_head_and_tail_cannot_run(gpu_device):
    """each refused call returns its error code and leaves the sentinel buffers untouched (they are large enough for the call had it
    been launched): the sampler step (CFG with an odd batch; a state that is not the evaluation's x; a missing dt, state or counter; a
    model whose out_channels differ from its in_channels), ga_dit_pooled_vector (batch 0 and 17), ga_dit_cache_context_ws (no scratch, too
    small a scratch, a misaligned one) and ga_dit_sampler_advance (batch 65, grid_len 0)"""
    from gaussiananything_amd import dit_ops as ops
    dev = gpu_device
    Lib, st = ops.lib(), _stream(dev)
    refused = []
    # ---- the sampler step, on the smallest step case of each kind
    vel = next(c for c in hc.CASES["step"] if c["mode"] == "velocity" and c["D"] == 64)
    eul = next(c for c in hc.CASES["step"] if c["mode"] == "euler" and c["D"] == 64 and c["cfg"] == 0)
    pack = _base(dev, 0, 64, 1)[1]
    guarded = []

    def step_call(c, what, edit, B=None, out_channels=None):
        c = dict(c, B=B or c["B"], cfg=1 if B else c["cfg"])
        z = hc.inputs(dict(c, cfg=0))                                     # (the inputs of the shape; the CFG duplication is not needed)
        fw = z["final_w"] if out_channels is None else torch.cat([z["final_w"], z["final_w"]])[:out_channels]
        fb = z["final_b"] if out_channels is None else torch.cat([z["final_b"], z["final_b"]])[:out_channels]
        planted = _Planted(c, z, dev, pack, fw, fb)
        if out_channels is not None:
            planted.model.in_channels = c["Cout"]
        step, outs, xbuf, keep = _step_buffers(c, z, dev)
        other = _tail(z["x"], F32, dev)
        edit(step, other)
        snap = {n: t.clone() for n, t in outs.items()}
        r, _ = _forward(c, z, dev, planted, step=step, x_buf=xbuf)
        refused.append((what, r, ERR_BAD_SHAPE))
        guarded.append((what, outs, snap, keep))

    step_call(vel, "velocity with CFG and an odd batch", lambda s, o: None, B=3)
    step_call(eul, "Euler step with CFG and an odd batch", lambda s, o: None, B=3)
    step_call(eul, "state != x", lambda s, o: setattr(s, "state", o.data_ptr()))
    step_call(eul, "missing dt", lambda s, o: setattr(s, "dt", None))
    step_call(eul, "missing state", lambda s, o: setattr(s, "state", None))
    step_call(eul, "missing counter", lambda s, o: setattr(s, "counter", None))
    step_call(vel, "velocity with out_channels != in_channels", lambda s, o: None, out_channels=6)
    step_call(eul, "Euler step with out_channels != in_channels", lambda s, o: None, out_channels=6)
    # ---- ga_dit_pooled_vector
    pc = hc.CASES["pooled"][0]
    pz = hc.inputs(pc)
    pm = _copy(pack["model"])
    pkeep = [_tail(pz[n], BF16 if n == "W" else F32, dev) for n in ("ln_w", "ln_b", "W", "b")]
    pm.hidden, pm.context_dim = pc["D"], pc["ctx"]
    pm.pool_ln_w, pm.pool_ln_b, pm.pool_w, pm.pool_b = (t.data_ptr() for t in pkeep)
    pin = torch.zeros(17 * pc["ctx"], dtype=F32, device=dev)
    pscr, pout = _sentinel(17, pc["ctx"], F32, dev), _sentinel(17, pc["D"], F32, dev)
    for batch in (0, 17):
        refused.append((f"pooled_vector batch {batch}", Lib.ga_dit_pooled_vector(ctypes.byref(pm), batch, pin.data_ptr(), pscr[1:].data_ptr(),
                                                                                   pout[1:].data_ptr(), st), ERR_BAD_SHAPE))
    # ---- ga_dit_cache_context_ws
    cc = hc.CASES["ctxnorm"][2]
    cz = hc.inputs(cc)
    cm, ckeep = _ctx_model(cc, cz, dev)
    rows = cc["B"] * cc["T"]
    need = Lib.ga_dit_context_scratch_bytes(ctypes.byref(cm), cc["B"], cc["T"])
    cscr = torch.full((need // 2 + 256,), BF16_SENTINEL, dtype=torch.int16, device=dev).view(BF16)
    ctx = _tail(cz["x"], BF16, dev, n=cc["ctx"])
    ck = torch.full((rows * 64,), BF16_SENTINEL, dtype=torch.int16, device=dev).view(BF16)
    cvt = torch.full((cc["B"] * 64 * 64,), BF16_SENTINEL, dtype=torch.int16, device=dev).view(BF16)

    def cache(scratch, nbytes):
        return Lib.ga_dit_cache_context_ws(ctypes.byref(cm), cc["B"], cc["T"], ctx.data_ptr(), ck.data_ptr(), cvt.data_ptr(), scratch, nbytes, st)

    refused += [("cache_context_ws without a scratch", cache(None, need), ERR_NULL_ARG),
                ("cache_context_ws with too small a scratch", cache(cscr.data_ptr(), need - 256), ERR_BAD_SHAPE),
                ("cache_context_ws with a misaligned scratch", cache(cscr.data_ptr() + 2, need), ERR_BAD_SHAPE)]
    # ---- ga_dit_sampler_advance
    grid = torch.zeros(80, dtype=F32, device=dev)
    ats, adt, acnt = _sentinel(1, 80, F32, dev), _sentinel(1, 1, F32, dev), _sentinel(1, 1, I32, dev)
    refused += [("sampler_advance batch 65", Lib.ga_dit_sampler_advance(acnt[1:].data_ptr(), grid.data_ptr(), grid.data_ptr(), 9, ats[1:].data_ptr(),
                                                                        65, adt[1:].data_ptr(), st), ERR_BAD_SHAPE),
                ("sampler_advance grid_len 0", Lib.ga_dit_sampler_advance(acnt[1:].data_ptr(), grid.data_ptr(), grid.data_ptr(), 0, ats[1:].data_ptr(),
                                                                          16, adt[1:].data_ptr(), st), ERR_BAD_SHAPE)]
    torch.cuda.synchronize()
    for what, got, want in refused:
        assert got == want, f"{what}: returned {got}, expected {want}"
    for what, outs, snap, keep in guarded:
        for n in outs:
            assert torch.equal(_bits(outs[n]), _bits(snap[n])), f"{what}: the refused call wrote to {n}"
        if len(keep) > 1:
            assert keep[1][1].item() == I32_SENTINEL
    for name, buf, sent in (("pooled scratch", pscr, F32_SENTINEL), ("pooled out", pout, F32_SENTINEL), ("context scratch", cscr, BF16_SENTINEL),
                            ("ca_k", ck, BF16_SENTINEL), ("ca_vt", cvt, BF16_SENTINEL), ("timesteps", ats, F32_SENTINEL), ("dt", adt, F32_SENTINEL),
                            ("counter", acnt, I32_SENTINEL)):
        assert bool((_bits(buf) == sent).all()), f"a refused call wrote to {name}"
