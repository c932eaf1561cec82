#!/usr/bin/env python3
"""Generates tests/golden/transport_ref.pt: results of the REFERENCE'S OWN transport package (transport/*.py, imported as it stands,
with the oracle integrator standing in for the absent torchdiffeq and a stub for sgm.util), so that the transport tests of
tests/test_cpu_oracle_and_host.py run without the reference tree:

  plumbing   Sampler(create_transport("GVP", "velocity")).sample_ode(euler, 25 grid points) on a small linear drift
  bound      every path plan (Linear, GVP, VP) x every parametrisation (velocity, score, noise): sample_ode with 9 grid points of a
             small nonlinear model, euler and dopri5 (velocity) or euler and heun3 (score / noise), states at every grid time

Run once:  python tests/golden/make_transport_golden.py <root of the reference tree>
"""
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)


def reference_transport(ref_root):
    from oracle import ode as oo

    def fake_odeint(fn, x, t, method, atol, rtol):
        return torch.from_numpy(oo.odeint(lambda ts, y: fn(torch.tensor(ts, dtype=torch.float32),
                                                            torch.from_numpy(y).float()).numpy(),
                                          x.numpy(), t.numpy(), method=method, atol=atol[0], rtol=rtol[0])).float()

    sys.modules["torchdiffeq"] = types.SimpleNamespace(odeint=fake_odeint)
    sys.modules["sgm"] = types.ModuleType("sgm")
    sys.modules["sgm.util"] = types.SimpleNamespace(instantiate_from_config=lambda *a, **k: None)
    sys.path.insert(0, ref_root)
    import transport
    return transport


def main():
    if len(sys.argv) != 2:
        raise SystemExit("usage: python tests/golden/make_transport_golden.py <root of the reference tree>")
    ref_root = sys.argv[1]
    rt_mod = reference_transport(ref_root)
    out = {"plumbing": {}, "bound": {}}

    # test_transport_surface_and_reference_plumbing
    f = lambda x, t, scale=1.0: -scale * x * (1 + t.view(-1, 1))  # noqa: E731
    x0 = torch.tensor([[1.0, 2.0], [0.5, -1.0]])
    rt = rt_mod.create_transport("GVP", "velocity", None, None, None, snr_type="uniform")
    try:
        sampler = rt_mod.Sampler(rt, guider_config=None)
    except TypeError:
        sampler = rt_mod.Sampler(rt)
    out["plumbing"] = {"x0": x0, "scale": 2.0, "num_steps": 25,
                       "euler": sampler.sample_ode(sampling_method="euler", num_steps=25)(x0, f, scale=2.0)}

    # test_bound_reference_transport_integrates_with_this_package
    model = lambda x, t, scale=1.0: torch.tanh(scale * x) * (0.5 + t.view(-1, 1, 1)) - 0.3 * x  # noqa: E731
    x0 = torch.randn(3, 4, 2, generator=torch.Generator().manual_seed(5))
    for path_type in ("Linear", "GVP", "VP"):
        for prediction in ("velocity", "score", "noise"):
            rt = rt_mod.create_transport(path_type, prediction, None, None, None, snr_type="uniform")
            methods = ("euler", "dopri5") if prediction == "velocity" else ("euler", "heun3")
            out["bound"][f"{path_type}/{prediction}"] = {
                m: rt_mod.Sampler(rt).sample_ode(sampling_method=m, num_steps=9)(x0, model, scale=1.5) for m in methods}
    out["bound_x0"] = x0
    path = os.path.join(HERE, "transport_ref.pt")
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
