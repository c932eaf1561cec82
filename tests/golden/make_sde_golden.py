#!/usr/bin/env python3
"""Generates tests/golden/sde_ref.pt: results of the REFERENCE'S OWN ``Sampler.sample_sde`` (transport/*.py imported as it stands, with
the stand-ins of make_transport_golden.py for torchdiffeq and sgm.util), so that tests/test_sde_cpu.py runs without the reference tree.

  configs   velocity prediction on GVP and Linear x diffusion form (sigma, linear, decreasing, inccreasing-decreasing) x Euler / Heun x
            last step Mean / Tweedie / Euler / None -- every combination that is finite in the reference (Heun with None on the Linear
            path is not; "SBDM" is NaN and "constant" a TypeError there, asserted below) -- on the analytic velocity
            f(x, t) = -s x (1 + t) + 0.3, state [2, 8, 3], 25 steps: the normals the reference's stepper drew (``th.randn`` wrapped
            inside transport.integrators) and its full list of states
  gaussian  data N(0, s^2 I), s = 0.5, on GVP with its exact linear velocity: 250-step Euler-Maruyama, "sigma" form, from 4096 x 3
            standard normals, the stepper fed the Philox normals of this package (seeded: the test regenerates them); the end variance
            the reference reaches, and the variance the SCHEME reaches exactly (float64 recursion over the reference's own noise-free
            multipliers and diffusion coefficients) -- the discretisation bias the test allows for

Run once:  python tests/golden/make_sde_golden.py <root of the reference tree>
"""
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

FORMS = ("sigma", "linear", "decreasing", "inccreasing-decreasing")
S_DATA, N_POINTS, GAUSS_STEPS, GAUSS_SEED = 0.5, 4096, 250, 20260


class _Randn:
    """stands in for the module ``th`` inside transport.integrators: ``randn`` is recorded or replaced, everything else is torch's"""

    def __init__(self):
        self.drawn, self.feed = [], None

    def __getattr__(self, name):
        return getattr(torch, name)

    def randn(self, *size, **kw):
        z = torch.randn(*size, **kw) if self.feed is None else self.feed(len(self.drawn), *size)
        self.drawn.append(z.clone())
        return z


def gaussian_velocity(x, t, s=S_DATA):
    """the exact velocity of data N(0, s^2 I) on the GVP path: ((alpha' alpha s^2 + sigma' sigma) / (alpha^2 s^2 + sigma^2)) x"""
    t = t.view(-1, *([1] * (x.dim() - 1)))
    a, da = torch.sin(t * math.pi / 2), math.pi / 2 * torch.cos(t * math.pi / 2)
    sg, dsg = torch.cos(t * math.pi / 2), -math.pi / 2 * torch.sin(t * math.pi / 2)
    return (da * a * s * s + dsg * sg) / (a * a * s * s + sg * sg) * x


def main():
    if len(sys.argv) != 2:
        raise SystemExit("usage: python tests/golden/make_sde_golden.py <root of the reference tree>")
    from make_transport_golden import reference_transport
    from gaussiananything_amd.transport.sampler import philox_normals
    rt_mod = reference_transport(sys.argv[1])
    import transport.integrators as ref_int
    rec = _Randn()
    ref_int.th = rec

    scale = 0.7
    f = lambda x, t, scale=1.0: -scale * x * (1 + t.view(-1, 1, 1)) + 0.3  # noqa: E731
    x0 = torch.randn(2, 8, 3, generator=torch.Generator().manual_seed(11))
    out = {"x0": x0, "scale": scale, "num_steps": 25, "configs": {}}
    for path_type in ("GVP", "Linear"):
        sampler = rt_mod.Sampler(rt_mod.create_transport(path_type, "velocity", None, None, None, snr_type="uniform"))
        # what the package refuses or serves differently, established on the reference itself
        nan = torch.stack(sampler.sample_sde(diffusion_form="SBDM", num_steps=25)(x0, f, scale=scale))
        assert not bool(torch.isfinite(nan).all()), "SBDM is expected to be non-finite for a velocity model"
        try:
            sampler.sample_sde(diffusion_form="constant", num_steps=25)(x0, f, scale=scale)
            raise AssertionError("the reference's 'constant' form is expected to fail in the stepper")
        except TypeError:
            pass
        for form in FORMS:
            for method in ("Euler", "Heun"):
                for last in ("Mean", "Tweedie", "Euler", None):
                    rec.drawn = []
                    torch.manual_seed(1000 + len(out["configs"]))
                    xs = torch.stack(sampler.sample_sde(sampling_method=method, diffusion_form=form, last_step=last,
                                                        num_steps=25)(x0, f, scale=scale))
                    finite = bool(torch.isfinite(xs).all())
                    assert finite == (not (method == "Heun" and last is None and path_type == "Linear")), (path_type, form, method, last)
                    if finite:
                        out["configs"][(path_type, form, method, last)] = {"noise": torch.stack(rec.drawn), "states": xs}
    print(len(out["configs"]), "finite configurations")

    # the Gaussian-data case: Philox normals of this package fed to the reference's stepper
    sampler = rt_mod.Sampler(rt_mod.create_transport("GVP", "velocity", None, None, None, snr_type="uniform"))
    g0 = torch.randn(N_POINTS, 3, generator=torch.Generator().manual_seed(12))
    rec.drawn = []
    rec.feed = lambda k, *size: torch.from_numpy(philox_normals(GAUSS_SEED, k, 0, N_POINTS * 3)).reshape(*size)
    end = sampler.sample_sde(diffusion_form="sigma", num_steps=GAUSS_STEPS)(g0, gaussian_velocity)[-1]
    ref_var = float(end.double().var(unbiased=False))
    # the variance the scheme reaches exactly: x' = m_k x + sqrt(2 w_k dt) xi per step, then the noise-free last step -- the multipliers
    # from the reference's own loop run noise-free in float64 on x = 1, the diffusion coefficients from its compute_diffusion
    rec.feed = lambda k, *size: torch.zeros(*size)
    ones = torch.ones(1, 1, dtype=torch.float64)
    path = [ones] + sampler.sample_sde(diffusion_form="sigma", num_steps=GAUSS_STEPS)(ones, gaussian_velocity)
    t1 = 1 - 0.04
    tg = torch.linspace(0, t1, GAUSS_STEPS)
    dt = float(tg[1] - tg[0])
    var = 1.0
    for k in range(GAUSS_STEPS - 1):
        w = float(sampler.transport.path_sampler.compute_diffusion(ones, tg[k].double().view(1), form="sigma", norm=1.0))
        var = float(path[k + 1] / path[k]) ** 2 * var + 2 * w * dt
    var *= float(path[GAUSS_STEPS] / path[GAUSS_STEPS - 1]) ** 2
    n = N_POINTS * 3
    se = S_DATA ** 2 * math.sqrt(2 / n)
    print(f"gaussian: reference end variance {ref_var:.6f}, scheme {var:.6f} (s^2 = {S_DATA ** 2}), 5 standard errors {5 * se:.6f}")
    assert abs(ref_var - var) <= 5 * se, "N too small: the reference alone misses the bar"
    out["gaussian"] = {"x0": g0, "s": S_DATA, "seed": GAUSS_SEED, "num_steps": GAUSS_STEPS, "ref_end_variance": ref_var,
                       "scheme_end_variance": var}
    path = os.path.join(HERE, "sde_ref.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
