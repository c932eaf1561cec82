"""GPU tests of the SDE sampler steps (include/ga_dit.h: GaSdeStep / ga_sde_step, csrc/ode_sde.hip) and of the device-resident loop built
on them (sample_sde_device, Sampler.sample_sde, cascade.sample(sde=...)).

The phases are compared with the numpy float32 restatement (tests/_sde_ref.py) BIT FOR BIT on caller-supplied noise, the kernel's own
noise with the float64 restatement of Philox4x32-10 and the Box-Muller transform, the captured loop with the eager torch loop on the same
module bit for bit.  Every raw call poisons its outputs first and checks guard words behind every buffer."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _sde_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 64            # 32-bit words behind every buffer
GUARD_WORD = 0x5A5A5A5A
POISON = np.float32(-77.25)
NI = 5                # intervals of the raw-call tables: counter 0, 2 (middle), 4 (last)


class Buf:
    """a float32 device buffer with guard words behind it"""

    def __init__(self, values, device):
        values = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
        self.n = values.size
        self.t = torch.full((self.n + GUARD,), GUARD_WORD, dtype=torch.int32, device=device)
        self.t[:self.n] = torch.from_numpy(values.view(np.int32)).to(device)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def bits(self):
        assert bool((self.t[self.n:] == GUARD_WORD).all()), "guard words overwritten"
        return self.t[:self.n].cpu().numpy()

    def f32(self):
        return self.bits().view(np.float32)


def same_bits(got, want):
    return np.array_equal(np.asarray(got).reshape(-1).view(np.uint32), np.ascontiguousarray(want, dtype=np.float32).reshape(-1).view(np.uint32))


class Raw:
    """the buffers of one GaSdeStep with random contents, and raw calls of ga_sde_step through the C-ABI"""

    def __init__(self, n, pairs, device, seed=0, with_noise=True, batch=3):
        from gaussiananything_amd import dit_ops as ops
        self.ops, self.n, self.pairs, self.dev, self.batch = ops, n, pairs, device, batch
        self.nd = n // 2 if pairs else n
        rng = np.random.default_rng(1000 + n + (7 if pairs else 0))
        half = lambda: np.tile(rng.standard_normal(self.nd).astype(np.float32), 2 if pairs else 1)  # noqa: E731
        self.host = {"state": half(), "velocity": half(), "k1": half(), "xhat": half()}
        self.coef_h = ref.table(rng, NI)
        self.noise_h = rng.standard_normal((NI, self.nd)).astype(np.float32)
        self.seed = seed
        self.with_noise = with_noise
        self.fresh(0)

    def fresh(self, counter):
        dev = self.dev
        self.b = {k: Buf(v, dev) for k, v in self.host.items()}
        self.b["traj"] = Buf(np.full((NI + 1) * self.n, POISON), dev)
        self.b["timesteps"] = Buf(np.full(self.batch, POISON), dev)
        self.b["coef"] = Buf(self.coef_h, dev)
        self.b["noise"] = Buf(self.noise_h, dev)
        self.b["noise_out"] = Buf(np.full(self.nd, POISON), dev)
        self.counter = torch.full((1 + GUARD,), GUARD_WORD, dtype=torch.int32, device=dev)
        self.counter[0] = counter
        s = self.seed & ((1 << 64) - 1)
        self.seed_t = torch.tensor([s - (1 << 64) if s >> 63 else s], dtype=torch.int64, device=dev)
        b = self.b
        self.args = self.ops.GaSdeStep(self.n, self.batch, NI, 1 if self.pairs else 0, b["state"].ptr, b["velocity"].ptr, b["k1"].ptr,
                                       b["xhat"].ptr, b["traj"].ptr, self.counter.data_ptr(), b["timesteps"].ptr, b["coef"].ptr,
                                       self.seed_t.data_ptr(), b["noise"].ptr if self.with_noise else None, b["noise_out"].ptr)

    def call(self, phase):
        with torch.cuda.device(self.dev):
            self.ops.check(self.ops.lib().ga_sde_step(ctypes.byref(self.args), phase,
                                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "ga_sde_step")
            torch.cuda.synchronize()

    def counter_value(self):
        assert bool((self.counter[1:] == GUARD_WORD).all())
        return int(self.counter[0])


N_CASES = [(n, False) for n in (1, 3, 255, 256, 257, 576, 4608)] + [(n, True) for n in (2, 12, 1150, 4608)]


@pytest.mark.parametrize("n,pairs", N_CASES)
def test_g1_every_phase_matches_the_float32_restatement_bit_for_bit(gpu_device, n, pairs):
    """G1.  Caller-supplied noise; counter 0, middle and last; the trajectory slot, the untouched buffers and the guard words."""
    raw = Raw(n, pairs, gpu_device)
    h = raw.host
    for counter in (0, NI // 2, NI - 1):
        for phase in range(ref.EM, ref.LAST_NONE + 1):
            raw.fresh(counter)
            raw.call(phase)
            last = phase >= ref.LAST_MEAN
            row = raw.coef_h[NI if last else counter]
            xi = ref.spread(raw.noise_h[counter], n, pairs)
            want = ref.phase(phase, row, h["state"], h["velocity"], h["xhat"], h["k1"], xi)
            for name in ("state", "xhat", "k1", "velocity"):
                assert same_bits(raw.b[name].bits(), want.get(name, h[name])), (phase, counter, name)
            traj = np.full((NI + 1, n), POISON, dtype=np.float32)
            if "slot" in want:
                traj[NI if last else counter] = want["slot"]
            assert same_bits(raw.b["traj"].bits(), traj), (phase, counter, "traj")
            ts = np.full(raw.batch, row[ref.C_T2] if phase == ref.HEUN_PREDICT else POISON, dtype=np.float32)
            assert same_bits(raw.b["timesteps"].bits(), ts), (phase, counter, "timesteps")
            nout = raw.noise_h[counter] if phase in (ref.EM, ref.HEUN_PERTURB) else np.full(raw.nd, POISON)
            assert same_bits(raw.b["noise_out"].bits(), nout), (phase, counter, "noise_out")
            assert raw.counter_value() == counter
            assert same_bits(raw.b["coef"].bits(), raw.coef_h) and same_bits(raw.b["noise"].bits(), raw.noise_h)
        raw.fresh(counter)
        raw.call(ref.ADVANCE)
        assert raw.counter_value() == counter + 1
        assert same_bits(raw.b["timesteps"].bits(), np.full(raw.batch, raw.coef_h[counter + 1][ref.C_T]))
        assert same_bits(raw.b["state"].bits(), h["state"]) and same_bits(raw.b["traj"].bits(), np.full((NI + 1) * n, POISON))
    raw.fresh(NI)            # a replay past the end: the counter and every index stay inside the table
    raw.call(ref.ADVANCE)
    assert raw.counter_value() == NI and same_bits(raw.b["timesteps"].bits(), np.full(raw.batch, raw.coef_h[NI][ref.C_T]))


@pytest.mark.parametrize("n,pairs", N_CASES)
def test_g2_device_noise_matches_the_float64_restatement(gpu_device, n, pairs):
    """G2.  The normals the kernel draws, read through noise_out, against Philox4x32-10 + Box-Muller in float64 within 1e-5 absolute:
    |z| <= sqrt(48 ln 2) = 5.77; 3 ulp for log and 4 ulp for sin / cos (the OpenCL-profile bounds), plus the fp32 rounding of the angle
    and of the radius, give about 7e-6.  The two CFG halves take the same normals; consecutive counters and the two phases differ."""
    seed = 0x9E3779B97F4A7C15
    raw = Raw(n, pairs, gpu_device, seed=seed, with_noise=False)
    worst, drawn = 0.0, {}
    for phase in (ref.EM, ref.HEUN_PERTURB):
        for counter in (0, 1, NI - 1):
            raw.fresh(counter)
            raw.call(phase)
            z = raw.b["noise_out"].f32().copy()
            drawn[(phase, counter)] = z
            worst = max(worst, float(np.abs(z - ref.normals(seed, counter, phase, raw.nd)).max()))
            # the update used exactly these normals, in both halves
            xi = ref.spread(z, n, pairs)
            h = raw.host
            want = ref.phase(phase, raw.coef_h[counter], h["state"], h["velocity"], h["xhat"], h["k1"], xi)
            name = "state" if phase == ref.EM else "xhat"
            got = raw.b[name].f32()
            assert same_bits(got, want[name]), (phase, counter)
            if pairs:
                assert same_bits(got[:n // 2], got[n // 2:])
    print(f"n = {n}, pairs = {pairs}: max |device normal - float64 restatement| = {worst:.3e}")
    assert worst <= 1e-5
    if raw.nd >= 4:
        assert not np.array_equal(drawn[(ref.EM, 0)], drawn[(ref.EM, 1)])
        assert not np.array_equal(drawn[(ref.EM, 0)], drawn[(ref.HEUN_PERTURB, 0)])


def test_g2_the_stream_does_not_depend_on_the_grid(gpu_device):
    """a call with n = 4608 and one with n = 576 agree on their common prefix"""
    seed = 12345
    a, b = Raw(4608, False, gpu_device, seed=seed, with_noise=False), Raw(576, False, gpu_device, seed=seed, with_noise=False)
    for r in (a, b):
        r.fresh(3)
        r.call(ref.EM)
    assert same_bits(a.b["noise_out"].f32()[:576], b.b["noise_out"].f32())


# ---- the loop on the small golden models -----------------------------------------------------------------------------------------------

_models = {}


def _golden(stage, device):
    if stage not in _models:
        from gaussiananything_amd import synthetic
        from gaussiananything_amd.dit import DiT_I23D_PCD_PixelArt_noclip, DiT_I23D_PCD_PixelArt_noclip_clay_stage2
        z = torch.load(synthetic.fixture_path(f"dit_ref_stage{stage}.pt"))
        kw = dict(z["kwargs"], **({"use_pe_cond": True} if stage == 2 else {}))
        model = (DiT_I23D_PCD_PixelArt_noclip if stage == 1 else DiT_I23D_PCD_PixelArt_noclip_clay_stage2)(**kw)
        model.load_state_dict(z["state_dict"], strict=True)
        model.to(device)
        _models[stage] = (z, model, {k: v.to(device) for k, v in z["context"].items()})
    return _models[stage]


def _sampler():
    from gaussiananything_amd.transport import Sampler, create_transport
    return Sampler(create_transport("GVP", "velocity", None, None, None, snr_type="uniform"))


def _doubled(z, device):
    h = z["x"][:z["x"].shape[0] // 2].to(device)
    return torch.cat([h, h], 0)


@pytest.mark.parametrize("method,last", [("Euler", "Mean"), ("Euler", "Tweedie"), ("Heun", "Euler"), ("Heun", None)])
def test_g3_the_device_loop_equals_the_eager_loop_bit_for_bit(gpu_device, monkeypatch, method, last):
    """G3.  Stage-1 golden, CFG state [4, 48, 3], 7 grid points, the same ``noise=`` tensor: the captured, replayed device loop against
    the eager torch loop over ``forward_with_cfg`` on the same module (GA_ODE_GRAPH=0 in a fresh Sampler call)."""
    z, model, ctx = _golden(1, gpu_device)
    x0 = _doubled(z, gpu_device)
    assert tuple(x0.shape) == (4, 48, 3)
    noise = torch.randn(6, x0.numel() // 2, generator=torch.Generator().manual_seed(21)).to(gpu_device)
    kw = dict(sampling_method=method, last_step=last, num_steps=7, noise=noise)
    smp = _sampler()
    dev_out = smp.sample_sde(**kw)(x0, model.forward_with_cfg, context=ctx, cfg_scale=z["cfg_scale"])
    assert smp.last_sde.last_stats.get("fused") is True
    monkeypatch.setenv("GA_ODE_GRAPH", "0")
    smp2 = _sampler()
    eager = smp2.sample_sde(**kw)(x0, model.forward_with_cfg, context=ctx, cfg_scale=z["cfg_scale"])
    assert "fused" not in smp2.last_sde.last_stats
    assert dev_out.shape == (7, 4, 48, 3) and dev_out.dtype == torch.float32 and bool(dev_out.isfinite().all())
    assert torch.equal(dev_out.view(torch.int32), eager.view(torch.int32))
    assert torch.equal(dev_out[:, :2], dev_out[:, 2:])
    assert not torch.equal(dev_out[0], dev_out[1])


def test_g4_replay_draws_fresh_noise_and_the_cache_serves_any_seed(gpu_device):
    """G4.  Device noise: the same seed replays the cached graph to the same bits, another seed differs, and the normals of step k
    under replay are the restatement's for counter k (a step index baked into the graph would repeat step 0's)."""
    from gaussiananything_amd.transport.sampler import sde_coefficients
    z, model, ctx = _golden(1, gpu_device)
    x0 = _doubled(z, gpu_device)
    call = lambda seed: _sampler().sample_sde(num_steps=7, seed=seed)(x0, model.forward_with_cfg, context=ctx,   # noqa: E731
                                                                      cfg_scale=z["cfg_scale"])
    a = call(77)
    graph = model._samplers.held("sde").graph
    b = call(77)
    assert model._samplers.held("sde").graph is graph
    c = call(78)
    assert model._samplers.held("sde").graph is graph                          # the seed is device data: no re-capture
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and not torch.equal(a, c)
    assert torch.equal(a[:, :2], a[:, 2:]) and bool(a.isfinite().all())
    worst = 0.0
    for method, stream in (("Euler", ref.EM), ("Heun", ref.HEUN_PERTURB)):
        nd = x0.numel() // 2
        nout = torch.full((3, nd), float("nan"), device=gpu_device)
        coef = sde_coefficients("GVP", "sigma", 1.0, torch.linspace(0, 0.96, 4), 0.04)
        model.sample_sde_device(x0, coef, ctx, method=method, cfg_scale=z["cfg_scale"], cfg=True, seed=4242, noise_out=nout)
        got = nout.cpu().numpy()
        for k in range(3):
            worst = max(worst, float(np.abs(got[k] - ref.normals(4242, k, stream, nd)).max()))
        assert not np.array_equal(got[0], got[1])
    print(f"normals under replay vs the restatement at the step's counter: max |diff| = {worst:.3e}")
    assert worst <= 1e-5


def test_g5_stage2_forward_cond_and_the_cascade_option(gpu_device, monkeypatch):
    """G5.  forward_cond on the stage-2 golden ([2, 48, 10], no pairs): device loop == eager loop on supplied noise; cascade.sample(sde=)
    equals the direct sample_sde call; the default cascade.sample output is what it was before any SDE call on the module."""
    from gaussiananything_amd import cascade
    z, model, ctx = _golden(2, gpu_device)
    L, C = z["x"].shape[1], z["x"].shape[2]
    ctx = {k: v[:2].contiguous() for k, v in ctx.items()}
    cond = dict(ctx)
    before = cascade.sample(model, cond, dict(cond), (L, C), 2, 4.0, 3, 6, "euler")
    x0 = z["x"][:2].to(gpu_device)
    assert tuple(x0.shape) == (2, 48, 10)
    noise = torch.randn(5, x0.numel(), generator=torch.Generator().manual_seed(22)).to(gpu_device)
    smp = _sampler()
    dev_out = smp.sample_sde(num_steps=6, noise=noise)(x0, model.forward_cond, context=ctx, cfg_scale=4.0)
    assert smp.last_sde.last_stats.get("fused") is True
    with monkeypatch.context() as m:
        m.setenv("GA_ODE_GRAPH", "0")
        eager = _sampler().sample_sde(num_steps=6, noise=noise)(x0, model.forward_cond, context=ctx, cfg_scale=4.0)
    assert torch.equal(dev_out.view(torch.int32), eager.view(torch.int32))
    assert not torch.equal(dev_out[:, 0], dev_out[:, 1])                 # no pairs: the batch items draw their own noise
    # cascade: the same initial state as cascade.sample draws it
    stats = {}
    got = cascade.sample(model, cond, dict(cond), (L, C), x0.shape[0], 4.0, 3, 6, "euler", stats=stats, sde={"last_step": "Tweedie"})
    torch.manual_seed(3)
    zs = torch.randn(x0.shape[0], L, C).to(gpu_device).to(torch.bfloat16).float()
    want = _sampler().sample_sde(num_steps=6, seed=3, last_step="Tweedie")(zs, model.forward_cond, context=dict(cond), cfg_scale=4.0)[-1]
    assert torch.equal(got, want)
    assert stats["sde"] is True and stats["nfe"] == 6 and stats["steps"] == 6 and stats["noop_cfg_dedup"] is True
    after = cascade.sample(model, cond, dict(cond), (L, C), 2, 4.0, 3, 6, "euler")
    assert torch.equal(before, after)


def test_learn_sigma_models_are_refused(gpu_device):
    from gaussiananything_amd.dit import DiT_I23D_PCD_PixelArt_noclip
    from gaussiananything_amd.transport.sampler import sde_coefficients
    z, _, ctx = _golden(1, gpu_device)
    model = DiT_I23D_PCD_PixelArt_noclip(**dict(z["kwargs"], learn_sigma=True)).to(gpu_device)
    coef = sde_coefficients("GVP", "sigma", 1.0, torch.linspace(0, 0.96, 4), 0.04)
    with pytest.raises(ValueError, match="learn_sigma"):
        model.sample_sde_device(_doubled(z, gpu_device), coef, ctx)
