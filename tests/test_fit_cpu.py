"""The arithmetic of the surfel fitter without a GPU: the float32 restatement of include/ga_fit.h (tests/_fit_ref.py, what the GPU tests
hold the kernels to bit for bit) against torch in float64, the step table, and to_raw against the activation.

Bars.  Each comes from the error torch's OWN float32 evaluation of the same expression makes against float64 (``E``): the restatement
gets 2 E (its products are in the written order, torch's ``lerp`` / ``addcmul`` / fused sigmoid are not) plus a floor of 4 float32 ulp
of the value compared.  The measured E of the Adam loop is in profiles/fit_bounds.txt."""
import numpy as np
import pytest
import torch

from tests import _fit_ref as ref

LR = dict(xyz=(1.6e-4, 1.6e-6), opacity=0.05, scale=0.005, rotation=0.001, rgb=0.0025)
BETAS, EPS = (0.9, 0.999), 1e-15
ULP_FLOOR = 4


def _raw(n, seed):
    rng = np.random.default_rng(seed)
    raw = rng.standard_normal((n, 13)).astype(np.float32)
    raw[:, 4:6] = raw[:, 4:6] - 4.0                       # scales around exp(-4)
    raw[:, 6:10] *= rng.choice([0.3, 1.0, 5.0], size=(n, 1)).astype(np.float32)   # quaternions that are not normalised
    return raw


def _mixed_grads(steps, n, seed):
    """gradients of mixed magnitude: exact zeros, 1e-20, 1e+4 and everything between"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(steps):
        g = rng.standard_normal((n, 13)) * np.power(10.0, rng.uniform(-6, 2, size=(n, 13)))
        pick = rng.integers(0, 8, size=(n, 13))
        g[pick == 0] = 0.0
        g[pick == 1] = 1e-20 * np.sign(g[pick == 1])
        g[pick == 2] = 1e4 * np.sign(g[pick == 2])
        out.append(g.astype(np.float32))
    return out


CASES = {"mixed": (97, 11), "mixed-2": (33, 12), "one-surfel": (1, 13)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_restatement_against_float64_adam(case):
    """10 steps of activation -> chain rule -> Adam: the float32 restatement against autograd + torch.optim.Adam (five param groups) in
    float64, held to 2 E + 4 ulp with E the error of the same torch loop in float32, per case and per column group"""
    n, seed = CASES[case]
    raw0, grads = _raw(n, seed), _mixed_grads(10, n, seed + 100)
    max_steps = 10
    want = ref.torch_loop(raw0, grads, LR, BETAS, EPS, max_steps, torch.float64)
    t32 = ref.torch_loop(raw0, grads, LR, BETAS, EPS, max_steps, torch.float32)
    got = ref.ref_loop(raw0, grads, LR, BETAS, EPS, max_steps).astype(np.float64)
    for name, s in ref.SLICES.items():
        E = float(np.abs(t32[..., s] - want[..., s]).max())
        floor = ULP_FLOOR * ref.ulp(want[..., s])                 # per element: a few ulp of the parameter itself
        err = np.abs(got[..., s] - want[..., s])
        print(f"fit bounds {case:11s} {name:9s} E_torch32 {E:.3e} restatement {float(err.max()):.3e} "
              f"worst err / bar {float((err / (2 * E + floor)).max()):.3f}")
        assert bool((err <= 2 * E + floor).all()), (case, name, float(err.max()), E)


def test_the_zero_gradient_stays_put():
    """exact zeros: m and v stay 0, the update is 0 / eps * step = 0 and the parameter keeps its bits"""
    raw = _raw(5, 3)
    tab = ref.table(LR, BETAS, 4).astype(np.float32)
    r1, m1, v1 = ref.adam_step(raw, np.zeros_like(raw), np.zeros_like(raw), np.zeros_like(raw), tab[0], BETAS, EPS)
    assert np.array_equal(r1, raw) and not m1.any() and not v1.any()


def test_step_table():
    """row t = lr_g(t) / (1 - b1^(t+1)) and sqrt(1 - b2^(t+1)) in double, rounded once; xyz decays log-linearly between its two ends;
    the last row is the one the clamped counter stays on"""
    from gaussiananything_amd import fitting
    max_steps = 257
    tab = fitting.step_table(LR, BETAS, max_steps)
    assert tab.dtype == torch.float32 and tuple(tab.shape) == (max_steps, 8)
    want = ref.table(LR, BETAS, max_steps)
    assert np.array_equal(tab.numpy(), want.astype(np.float32))
    # the definition once more, by hand, for three rows
    for t in (0, 100, max_steps - 1):
        lr_xyz = np.exp(np.log(1.6e-4) + (np.log(1.6e-6) - np.log(1.6e-4)) * t / (max_steps - 1))
        assert tab[t, 0].item() == np.float32(lr_xyz / (1 - 0.9 ** (t + 1)))
        assert tab[t, 1].item() == np.float32(0.05 / (1 - 0.9 ** (t + 1)))
        assert tab[t, 5].item() == np.float32(np.sqrt(1 - 0.999 ** (t + 1)))
    lr_xyz = want[:, 0] * (1 - 0.9 ** (np.arange(max_steps) + 1.0))
    steps = np.diff(np.log(lr_xyz))
    assert np.allclose(steps, steps[0], rtol=1e-9) and abs(lr_xyz[0] - 1.6e-4) < 1e-18 and abs(lr_xyz[-1] - 1.6e-6) < 1e-18
    assert not tab[:, 6:].any()
    assert len({tuple(r) for r in tab.numpy().tolist()}) == max_steps        # every row differs
    one = fitting.step_table(LR, BETAS, 1)
    assert one[0, 0].item() == np.float32(1.6e-4 / (1 - 0.9))


def test_step_table_refuses_bad_learning_rates():
    from gaussiananything_amd import fitting
    with pytest.raises(ValueError):
        fitting.step_table(dict(xyz=1e-4, opacity=0.05), BETAS, 4)
    with pytest.raises(ValueError):
        fitting.step_table(dict(LR, xyz=(1e-4, 0.0)), BETAS, 4)


def test_to_raw_inverts_the_activation():
    """activate(to_raw(g)) == g inside the clamps, measured against float64: the bar is 2 E + 4 ulp with E the error of the same
    composition in float32 torch (logit, then sigmoid; log, then exp)"""
    from gaussiananything_amd import fitting, synthetic
    g = synthetic.random_surfels(500, seed=2)[0]
    g[:5, 3] = torch.tensor([1e-5, 1 - 1e-5, 0.5, 2e-6, 0.999])     # inside the clamps, near their ends
    g[:3, 4] = torch.tensor([1e-7, 1e-3, 3.0])
    raw = fitting.to_raw(g)
    assert raw.dtype == torch.float32 and tuple(raw.shape) == (500, 13)
    assert torch.equal(raw[:, 0:3], g[:, 0:3]) and torch.equal(raw[:, 6:10], g[:, 6:10])
    got = ref.packed(ref.activate(raw.numpy())).astype(np.float64)
    g64 = g.double()
    exact = g64.numpy()
    exact[:, 6:10] = (g64[:, 6:10] / g64[:, 6:10].pow(2).sum(1, keepdim=True).sqrt()).numpy()
    # the float32 torch composition
    p = torch.cat([g[:, 3:4], g[:, 10:13]], 1)
    t32 = torch.sigmoid(torch.logit(p)).double().numpy()
    s32 = torch.exp(torch.log(g[:, 4:6])).double().numpy()
    for name, cols, comp in (("sigmoid", [3, 10, 11, 12], t32), ("exp", [4, 5], s32)):
        E = float(np.abs(comp - exact[:, cols]).max())
        err = np.abs(got[:, cols] - exact[:, cols])
        floor = ULP_FLOOR * ref.ulp(exact[:, cols])                # per element
        print(f"to_raw o activate {name}: E_torch32 {E:.3e} got {float(err.max()):.3e} worst err / bar {float((err / (2 * E + floor)).max()):.3f}")
        assert bool((err <= 2 * E + floor).all()), (name, float(err.max()), E)
    assert np.abs(got[:, 6:10] - exact[:, 6:10]).max() <= 2 * 2 ** -24        # a correctly rounded quotient of a correctly rounded root
    # outside the clamps the value is the clamp's
    h = g.clone()
    h[0, 3], h[1, 3], h[0, 4] = 0.0, 1.0, 0.0
    r = fitting.to_raw(h)
    assert abs(r[0, 3].item() - np.log(1e-6 / (1 - 1e-6))) < 1e-4 and abs(r[1, 3].item() + np.log(1e-6 / (1 - 1e-6))) < 0.2
    assert abs(r[0, 4].item() - np.log(1e-8)) < 1e-5
    assert tuple(fitting.to_raw(g[None]).shape) == (500, 13)


def test_validation_without_a_device():
    """a clear exception before anything is enqueued: CPU tensors, wrong shapes, a zero quaternion"""
    from gaussiananything_amd import fitting, synthetic
    g = synthetic.random_surfels(10, seed=1)
    bad = g.clone()
    bad[0, 3, 6:10] = 0
    with pytest.raises(ValueError, match="zero quaternion"):
        fitting.to_raw(bad)
    with pytest.raises(ValueError, match=r"\[N,13\]"):
        fitting.to_raw(g[0][:, :12])
    with pytest.raises(TypeError):
        fitting.to_raw(g.numpy())
    cams = synthetic.eval_cameras(2)
    with pytest.raises(ValueError, match="no CPU path"):
        fitting.SurfelFitter(g, cams["cam_view"], cams["cam_view_proj"], cams["tanfov"], torch.zeros(2, 3, 32, 32))
