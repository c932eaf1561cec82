"""CPU tests of the SDE sampler surface (transport/sampler.py: Sampler.sample_sde, its coefficient table, the eager loop and the host
restatement of the kernel's noise) against the reference's own results (tests/golden/sde_ref.pt, written by make_sde_golden.py) and
against the mathematics."""
import math

import numpy as np
import pytest
import torch

from tests import _sde_ref as ref


def _sampler(path_type="GVP"):
    from gaussiananything_amd.transport import Sampler, create_transport
    return Sampler(create_transport(path_type, "velocity", None, None, None, snr_type="uniform"))


def _golden():
    from gaussiananything_amd import synthetic
    return torch.load(synthetic.fixture_path("sde_ref.pt"), weights_only=False)


def _velocity(x, t, scale=1.0):
    return -scale * x * (1 + t.view(-1, 1, 1)) + 0.3


def test_c1_the_two_philox_restatements_agree_and_match_the_published_vector():
    """C1.  The known-answer vector of Random123 for Philox4x32-10 at counter 0, key 0 is written from memory; the two independent
    restatements (Python integers; numpy limbs) must agree on it and on 10 000 random counters and keys."""
    zero = ref.philox_int((0, 0, 0, 0), (0, 0))
    assert tuple(int(v) for v in ref.philox_np([0], [0], [0], [0], [0], [0])[0]) == zero
    assert zero == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    rng = np.random.default_rng(2026)
    cols = rng.integers(0, 1 << 32, size=(6, 10000), dtype=np.uint64).astype(np.uint32)
    got = ref.philox_np(*cols)
    for i in range(cols.shape[1]):
        c = [int(v) for v in cols[:, i]]
        assert tuple(int(v) for v in got[i]) == ref.philox_int(tuple(c[:4]), tuple(c[4:])), i
    # the package's own host restatement draws the same integers: its fp32 normals are the float64 ones to fp32 accuracy
    from gaussiananything_amd.transport.sampler import philox_normals
    for seed, step, stream, n in ((0, 0, 0, 8), (0xDEADBEEF12345678, 7, 1, 1001), (1 << 63, 249, 0, 4096)):
        z = philox_normals(seed, step, stream, n)
        assert z.dtype == np.float32 and z.shape == (n,)
        assert float(np.abs(z - ref.normals(seed, step, stream, n)).max()) < 1e-5


def test_c2_the_eager_loop_reproduces_the_reference_on_its_own_normals():
    """C2.  Every state of every configuration that is finite in the reference, fed the normals the reference's stepper drew, within
    1e-5 absolute (the bound of test_transport_surface_and_reference_plumbing; the states are O(1))."""
    g = _golden()
    assert len(g["configs"]) == 60
    worst = 0.0
    for (path_type, form, method, last), cfg in g["configs"].items():
        calls = []

        def model(x, t, scale=1.0):
            calls.append(1)
            return _velocity(x, t, scale)

        fn = _sampler(path_type).sample_sde(sampling_method=method, diffusion_form=form, last_step=last, num_steps=g["num_steps"],
                                            noise=cfg["noise"])
        got = fn(g["x0"], model, scale=g["scale"])
        assert got.shape == cfg["states"].shape and got.dtype == torch.float32
        err = float((got - cfg["states"]).abs().max())
        worst = max(worst, err)
        assert err <= 1e-5, (path_type, form, method, last, err)
        assert len(calls) == (g["num_steps"] - 1) * (1 if method == "Euler" else 2) + (last is not None)
    print(f"eager SDE loop vs the reference, 60 configurations: max |diff| = {worst:.3e}")


def test_c3_surface():
    """C3.  Refusals, interval, shape, one model call per Euler step, seeds, and the zero-diffusion limit."""
    smp = _sampler("GVP")
    with pytest.raises(ValueError, match="non-finite at t0 = 0"):
        smp.sample_sde(diffusion_form="SBDM")
    with pytest.raises(ValueError, match="divides by 1 - t"):
        _sampler("Linear").sample_sde(sampling_method="Heun", last_step=None)
    smp.sample_sde(sampling_method="Heun", last_step=None)                    # GVP: finite, served
    with pytest.raises(ValueError):
        smp.sample_sde(diffusion_form="quadratic")
    with pytest.raises(ValueError):
        smp.sample_sde(sampling_method="Milstein")
    with pytest.raises(ValueError):
        smp.sample_sde(last_step="Median")
    tr = smp.transport
    assert tr.check_interval(tr.train_eps, tr.sample_eps, sde=True, eval=True, last_step_size=0.04) == (0, 1 - 0.04)
    assert tr.check_interval(tr.train_eps, tr.sample_eps, sde=True, eval=True) == (0, 1)
    assert tr.check_interval(tr.train_eps, tr.sample_eps, sde=False, eval=True) == (0, 1)
    x0 = torch.randn(2, 8, 3, generator=torch.Generator().manual_seed(3))
    calls = []

    def model(x, t, scale=1.0):
        calls.append(t.clone())
        return _velocity(x, t, scale)

    a = smp.sample_sde(num_steps=12, seed=5)(x0, model, scale=0.7)
    assert a.shape == (12, 2, 8, 3) and len(calls) == 12                   # 11 steps + the last step, one call each
    assert smp.last_sde.last_stats == {"nfe": 12, "steps": 12, "sde": True}
    grid = torch.linspace(0, 1 - 0.04, 12)
    assert all(torch.equal(t, torch.ones(2) * grid[k]) for k, t in enumerate(calls))
    b = smp.sample_sde(num_steps=12, seed=5)(x0, model, scale=0.7)
    c = smp.sample_sde(num_steps=12, seed=6)(x0, model, scale=0.7)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert smp.sample_sde(num_steps=12, diffusion_form="constant", diffusion_norm=0.3)(x0, model, scale=0.7).isfinite().all()
    # no diffusion: drift = v, the trajectory is plain Euler on the same grid (v + 0 * score and + 0 * dw round to the same numbers)
    e = smp.sample_sde(num_steps=12, diffusion_norm=0.0, last_step="Euler")(x0, model, scale=0.7)
    x, dt = x0.clone(), grid[1] - grid[0]
    for k in range(11):
        x = x + _velocity(x, torch.ones(2) * grid[k], 0.7) * dt
        assert float((e[k] - x).abs().max()) <= 4 * torch.finfo(torch.float32).eps * float(x.abs().max()), k
    x = x + _velocity(x, torch.ones(2) * grid[11], 0.7) * 0.04
    assert float((e[11] - x).abs().max()) <= 4 * torch.finfo(torch.float32).eps * float(x.abs().max())


def test_c3_cfg_pairs_share_the_noise_on_the_eager_path():
    """a callable named forward_with_cfg takes the doubled state: both halves get the same normals and stay equal"""
    class Twin:
        def forward_with_cfg(self, x, t, scale=1.0):
            return _velocity(x, t, scale)

    h = torch.randn(2, 8, 3, generator=torch.Generator().manual_seed(4))
    out = _sampler().sample_sde(num_steps=9, seed=11)(torch.cat([h, h]), Twin().forward_with_cfg, scale=0.7)
    assert out.shape == (9, 4, 8, 3) and torch.equal(out[:, :2], out[:, 2:])
    single = _sampler().sample_sde(num_steps=9, seed=11)(h, lambda x, t, scale=1.0: _velocity(x, t, scale), scale=0.7)
    assert torch.equal(out[:, :2], single)


def test_c4_gaussian_data_end_variance():
    """C4.  Data N(0, s^2 I), s = 0.5, on GVP has the exact linear velocity ((alpha' alpha s^2 + sigma' sigma) / (alpha^2 s^2 + sigma^2)) x;
    250-step Euler-Maruyama with the sigma form from 4096 x 3 standard normals must end with variance s^2.  The reference was run on
    the same (Philox, seeded) normals when the fixture was made.  Ours must match its end variance within 1e-5, and both must lie
    within five standard errors 5 s^2 sqrt(2 / N) of the variance the scheme reaches exactly (s^2 plus the discretisation bias, a
    float64 recursion over the reference's own noise-free multipliers: make_sde_golden.py).  A sign or sqrt(2 w) error misses this by
    tens of per cent."""
    g = _golden()["gaussian"]
    s = g["s"]

    def velocity(x, t):
        t = t.view(-1, 1)
        a, da = torch.sin(t * math.pi / 2), math.pi / 2 * torch.cos(t * math.pi / 2)
        sg, dsg = torch.cos(t * math.pi / 2), -math.pi / 2 * torch.sin(t * math.pi / 2)
        return (da * a * s * s + dsg * sg) / (a * a * s * s + sg * sg) * x

    end = _sampler("GVP").sample_sde(diffusion_form="sigma", num_steps=g["num_steps"], seed=g["seed"])(g["x0"], velocity)[-1]
    ours = float(end.double().var(unbiased=False))
    n = g["x0"].numel()
    bar = 5 * s * s * math.sqrt(2 / n)
    print(f"end variance: ours {ours:.6f}, reference {g['ref_end_variance']:.6f}, scheme {g['scheme_end_variance']:.6f}, s^2 {s * s}, "
          f"5 standard errors {bar:.6f}")
    assert abs(ours - g["ref_end_variance"]) <= 1e-5
    assert abs(g["scheme_end_variance"] - s * s) < 0.05 * s * s          # the bias is a discretisation bias, not a wrong target
    assert abs(ours - g["scheme_end_variance"]) <= bar and abs(g["ref_end_variance"] - g["scheme_end_variance"]) <= bar


@pytest.mark.parametrize("seed", [0, 1, (1 << 63) + 5])
def test_c5_statistics_of_the_restated_normals(seed):
    """C5.  24 steps x 15 360 elements of the float64 restatement: mean, variance, lag-1 correlation across the steps of an element
    and correlation of neighbouring elements, each within five standard errors of 0 / 1 / 0 / 0.  The kernel draws the same integers
    (test_sde_gpu.py), so on the GPU these can only fail through the kernel."""
    steps, n = 24, 15360
    z = np.stack([ref.normals(seed, k, ref.EM, n) for k in range(steps)])
    N = z.size
    assert abs(z.mean()) <= 5 / math.sqrt(N)
    assert abs(z.var() - 1) <= 5 * math.sqrt(2 / N)
    lag = (z[:-1] * z[1:]).mean()
    assert abs(lag) <= 5 / math.sqrt(z[:-1].size)
    nb = (z[:, :-1] * z[:, 1:]).mean()
    assert abs(nb) <= 5 / math.sqrt(z[:, :-1].size)
    assert float(np.abs(z).max()) <= math.sqrt(48 * math.log(2))


def test_argument_validation_of_the_step_without_a_gpu():
    """ga_sde_step_check: the error code ga_sde_step returns before it launches anything (host only)"""
    import ctypes
    from gaussiananything_amd import dit_ops as ops
    L = ops.lib()
    ok = dict(n=48, batch=2, num_intervals=5, cfg_pairs=1, state=64, velocity=64, k1=64, xhat=64, traj=64, counter=64, timesteps=64,
              coef=64, seed=64, noise=None, noise_out=None)
    check = lambda phase, **kw: L.ga_sde_step_check(ctypes.byref(ops.GaSdeStep(**dict(ok, **kw))), phase)  # noqa: E731
    for phase in range(9):
        assert check(phase) == 0
    assert check(9) == -2 and check(-1) == -2
    assert check(ops.GA_SDE_EM, n=47) == -2                      # cfg_pairs needs an even state
    assert check(ops.GA_SDE_EM, n=47, cfg_pairs=0) == 0
    assert check(ops.GA_SDE_EM, n=0) == -2 and check(ops.GA_SDE_EM, batch=65) == -2 and check(ops.GA_SDE_EM, num_intervals=0) == -2
    assert check(ops.GA_SDE_EM, n=1 << 31) == -2
    assert check(ops.GA_SDE_EM, seed=None) == -1 and check(ops.GA_SDE_EM, seed=None, noise=64) == 0
    assert check(ops.GA_SDE_EM, velocity=None) == -1 and check(ops.GA_SDE_LAST_NONE, velocity=None) == 0
    assert check(ops.GA_SDE_HEUN_PERTURB, xhat=None) == -1 and check(ops.GA_SDE_HEUN_CORRECT, k1=None) == -1
    assert check(ops.GA_SDE_EM, traj=None) == -1 and check(ops.GA_SDE_ADVANCE, timesteps=None) == -1
    assert check(ops.GA_SDE_HEUN_PREDICT, timesteps=None) == -1 and check(ops.GA_SDE_EM, coef=None) == -1
    assert L.ga_sde_step_check(None, 0) == -1
