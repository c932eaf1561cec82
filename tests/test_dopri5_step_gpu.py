"""GPU tests of the dopri5 step kernels through the C ABI (include/ga_dit.h: GaOdeDopri5, ga_ode_dopri5_stage / ga_ode_dopri5_finish;
csrc/ode_dopri5.hip: stage_kernel, error_kernel, control_kernel, accept_kernel) and of ga_dit_sampler_advance.

One attempted step is a closed function of buffers the caller owns, so no denoiser runs here: the test supplies the k's and holds every
call to the reference of tests/_dopri5_ref.py -- stage inputs and times bit for bit, the sum of squares within 5 * 2^-24, every word of
the controller's head as a float64 value, the dense output element by element within its derived bound P.  The bars are derived there;
tests/test_dopri5_bounds_cpu.py shows that seeded faults of the kernels land over them.  Every buffer has guard words behind it, every
output is poisoned first, and ctl is allocated with exactly GA_ODE_CTL_WORDS + nparts doubles.

`pytest -s` prints one DOPRI5CASE line per case: profiles/dopri5_bounds.txt."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _dopri5_ref as ref
from tests._dopri5_ref import ACCEPT, DONE, DT, JCOUNT, JNEXT, REJECTED, STEPS, T, f32, f64

pytestmark = pytest.mark.gpu

GUARD = 64            # 32-bit words behind every buffer
GUARD_WORD = 0x5A5A5A5A
OK, NULL_ARG, BAD_SHAPE = 0, -1, -2


class Buf:
    """a float32 or float64 device buffer with guard words behind it"""

    def __init__(self, values, device):
        values = np.ascontiguousarray(values)
        assert values.dtype in (np.float32, np.float64)
        self.dtype, self.shape = values.dtype, values.shape
        words = values.reshape(-1).view(np.int32)
        self.n = words.size
        self.t = torch.full((self.n + GUARD,), GUARD_WORD, dtype=torch.int32, device=device)
        self.t[:self.n] = torch.from_numpy(words).to(device)

    @property
    def ptr(self):
        return self.t.data_ptr()

    def tensor(self):
        """the payload as a float tensor on the device (a view)"""
        return self.t[:self.n].view(torch.float32 if self.dtype == np.float32 else torch.float64)

    def get(self):
        assert bool((self.t[self.n:] == GUARD_WORD).all()), "guard words overwritten"
        return self.t[:self.n].cpu().numpy().view(self.dtype).reshape(self.shape)


class Dev:
    """the buffers of one GaOdeDopri5 on the device, and raw calls of the two entry points"""

    def __init__(self, state, device):
        from gaussiananything_amd import dit_ops as ops
        self.ops, self.dev = ops, device
        self.load(state)

    def load(self, s):
        dev = self.dev
        self.n, self.batch = s.n, s.batch
        self.b = {name: Buf(getattr(s, name), dev) for name in ("y", "ystage", "timesteps", "ctl", "t_grid", "out")}
        self.k = [Buf(v, dev) for v in s.k]
        assert s.ctl.size == ref.CTL_WORDS + ref.nparts(s.n)
        b = self.b
        self.args = self.ops.GaOdeDopri5(s.n, s.batch, len(s.t_grid), b["y"].ptr, (ctypes.c_void_p * 7)(*[k.ptr for k in self.k]),
                                         b["ystage"].ptr, b["timesteps"].ptr, b["ctl"].ptr, b["t_grid"].ptr, b["out"].ptr, s.ctl.size)

    def pull(self):
        s = ref.State.__new__(ref.State)
        s.n, s.batch = self.n, self.batch
        for name, buf in self.b.items():
            setattr(s, name, buf.get())
        s.k = [k.get() for k in self.k]
        return s

    def set_k(self, j, values):
        if not torch.is_tensor(values):
            values = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32))
        self.k[j].tensor().copy_(values.to(self.dev))

    def raw(self, what, args, *more):
        with torch.cuda.device(self.dev):
            rc = getattr(self.ops.lib(), what)(ctypes.byref(args) if args is not None else None, *more,
                                               ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
        return rc

    def stage(self, i):
        assert self.raw("ga_ode_dopri5_stage", self.args, i) == OK

    def finish(self):
        assert self.raw("ga_ode_dopri5_finish", self.args) == OK


# ---- (a) one attempted step, every size --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", ref.DTS_A)
@pytest.mark.parametrize("n,batch", ref.SIZES_A)
def test_a_one_attempted_step_at_every_size(gpu_device, n, batch, dt):
    """1 workgroup, the golden size, 64 / 65 / 66 partials, the grid at its cap, one and many threads on a second grid-stride lap; an
    accepted step (dt = 0.05) and a rejected one (dt = 0.3).  k[i + 1] = f(timesteps[0], ystage) by the reference's field after every
    stage call."""
    state, field = ref.case_a(n, batch, dt)
    before, after, fig = ref.attempt(Dev(state, gpu_device), field)
    print(ref.line(f"a_n{n}_b{batch}_dt{dt}", fig))
    accept = dt == ref.DTS_A[0]
    assert fig["accept"] == accept and after.ctl[ACCEPT] == accept and after.ctl[STEPS] == 1
    if accept:
        assert sorted(fig["out"]) == [1, 2, 3] and after.ctl[JNEXT] == 4 and after.ctl[DONE] == 0
        assert bool((after.out[0] == ref.POISON).all() and (after.out[4] == ref.POISON).all())
    else:
        assert after.ctl[T] == before.ctl[T] and after.ctl[REJECTED] == before.ctl[REJECTED] + 1 and after.ctl[JCOUNT] == 0
        assert ref.same_bits(after.out, before.out) and ref.same_bits(after.y, before.y) and ref.same_bits(after.k[0], before.k[0])


# ---- (b) controller branches -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", ref.SIZES_B)
@pytest.mark.parametrize("name", ref.CASES_B)
def test_b_controller_branches(gpu_device, name, n):
    """k set by hand; the stage calls still run, so y1 = ystage is the kernel's own.  ratio == 0, the three clamps of the step factor, the
    two error codes (NaN, +inf, 0 / 0; step underflow), a call on a block that is DONE, and the requested times: none inside the step,
    the last one inside, a grid of one."""
    before, after, fig = ref.attempt(Dev(ref.case_b(name, n), gpu_device), nan_ok=name in ("nan", "inf"))
    print(ref.line(f"b_{name}_n{n}", fig))
    ref.hold_expect_b(name, before, after)
    if ref.EXPECT_B[name].get(ref.ERROR) or name == "done":
        assert ref.same_bits(after.y, before.y) and ref.same_bits(after.k[0], before.k[0]) and ref.same_bits(after.out, before.out)


# ---- (c) entry-point guards --------------------------------------------------------------------------------------------------------------

def test_c_entry_point_guards(gpu_device):
    """nothing is enqueued and every buffer is bit-unchanged"""
    state, _ = ref.case_a(257, 3, 0.05)
    dev = Dev(state, gpu_device)
    ops = dev.ops
    before = dev.pull()

    def variant(**kw):
        a = ops.GaOdeDopri5()
        ctypes.memmove(ctypes.byref(a), ctypes.byref(dev.args), ctypes.sizeof(a))
        for name, v in kw.items():
            setattr(a, name, v)
        return a

    def k_without(j):
        k = (ctypes.c_void_p * 7)(*[b.ptr for b in dev.k])
        k[j] = None
        return k

    for st in (-1, 6):
        assert dev.raw("ga_ode_dopri5_stage", dev.args, st) == BAD_SHAPE
    for bt in (0, 65):
        assert dev.raw("ga_ode_dopri5_stage", variant(batch=bt), 0) == BAD_SHAPE
    assert dev.raw("ga_ode_dopri5_stage", variant(n=0), 0) == BAD_SHAPE
    assert dev.raw("ga_ode_dopri5_finish", variant(n=0)) == BAD_SHAPE
    assert dev.raw("ga_ode_dopri5_finish", variant(grid_len=0)) == BAD_SHAPE
    assert dev.raw("ga_ode_dopri5_finish", variant(ctl_words=ref.CTL_WORDS + ref.nparts(257) - 1)) == BAD_SHAPE
    assert dev.raw("ga_ode_dopri5_stage", None, 0) == NULL_ARG and dev.raw("ga_ode_dopri5_finish", None) == NULL_ARG
    # each pointer in turn, at the entry points that read or write it
    for name, calls in (("y", "sf"), ("ystage", "sf"), ("ctl", "sf"), ("timesteps", "s"), ("t_grid", "f"), ("out", "f")):
        if "s" in calls:
            assert dev.raw("ga_ode_dopri5_stage", variant(**{name: None}), 0) == NULL_ARG, name
        if "f" in calls:
            assert dev.raw("ga_ode_dopri5_finish", variant(**{name: None})) == NULL_ARG, name
    for j in range(7):
        assert dev.raw("ga_ode_dopri5_stage", variant(k=k_without(j)), 5) == NULL_ARG, j
        assert dev.raw("ga_ode_dopri5_finish", variant(k=k_without(j))) == NULL_ARG, j
    after = dev.pull()
    for name in ref.State.FIELDS:
        if name == "k":
            assert all(ref.same_bits(a, b) for a, b in zip(after.k, before.k))
        else:
            assert ref.same_bits(getattr(after, name), getattr(before, name)), name


# ---- (d) a whole integration on an analytic field ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,lam_max", ref.SIZES_D)
def test_d_a_whole_integration_step_by_step(gpu_device, n, lam_max):
    """The test drives the loop: six stage calls, each followed by f = amp cos(3 t) - lam * y evaluated with torch on the device from ystage
    and timesteps[0] (the product a tensor of its own before the subtraction), then finish.  Every attempted step is held to the reference
    of the device's own y, k and ctl as they were before it -- real ratios, rejects and step-size changes, no accumulated divergence.
    At the end the counters are the float64 oracle's, and the dense output is within 4 e_host of it, e_host = max |transport.odeint.odeint
    (fp32, CPU) - oracle| measured here: both are references, the margin is for cosf and the other roundings of the dense output."""
    from gaussiananything_amd.transport import odeint as host
    from oracle import ode as oracle
    field, y0 = ref.case_d(n, lam_max)
    amp_c, lam_c = torch.from_numpy(field.amp), torch.from_numpy(field.lam)
    amp, lam = amp_c.to(gpu_device), lam_c.to(gpu_device)

    def f_torch(a, la):
        def f(t, y):
            drive = a * torch.cos(3 * torch.as_tensor(t, dtype=torch.float32, device=y.device))
            decay = la * y
            return drive - decay
        return f

    f_dev = f_torch(amp, lam)
    y0_dev = torch.from_numpy(y0).to(gpu_device)
    k0 = f_dev(0.0, y0_dev)
    dt0 = host._initial_step(f_dev, 0.0, y0_dev, k0, ref.RTOL_D, ref.ATOL_D)
    state = ref.State(y0.copy(), [k0.cpu().numpy()] + [np.zeros(n, f32) for _ in range(6)],
                      ref.head_of(0.0, dt0, ref.ATOL_D, ref.RTOL_D, n=n), ref.GRID_D, 1)
    state.out[0] = y0
    dev = Dev(state, gpu_device)
    on_device = lambda _t, _y: f_dev(dev.b["timesteps"].tensor()[0], dev.b["ystage"].tensor())      # noqa: E731
    worst = {"sumsq": 0.0, "dt": 0.0, "out": 0.0, "gap": np.inf}
    for _ in range(200):
        before, after, fig = ref.attempt(dev, on_device)
        worst["sumsq"], worst["dt"] = max(worst["sumsq"], fig["sumsq"]), max(worst["dt"], fig["dt"])
        worst["out"] = max([worst["out"]] + list(fig["out"].values()))
        worst["gap"] = min(worst["gap"], abs(fig["ratio"] - 1))
        if after.ctl[DONE]:
            break
    end = dev.pull()
    assert end.ctl[DONE] == 1 and end.ctl[ref.ERROR] == 0 and end.ctl[JNEXT] == len(ref.GRID_D)
    stats = {}
    want = oracle.odeint(field.f64, y0.astype(f64), ref.GRID_D, atol=ref.ATOL_D, rtol=ref.RTOL_D, stats=stats)
    steps, rejected = int(end.ctl[STEPS]), int(end.ctl[REJECTED])
    assert (2 + 6 * steps, steps, rejected) == (stats["nfe"], stats["steps"], stats["rejected"])
    assert worst["gap"] > 1e-3
    assert ref.same_bits(end.out[0], y0)
    hst = host.odeint(f_torch(amp_c, lam_c), torch.from_numpy(y0), torch.from_numpy(ref.GRID_D), atol=ref.ATOL_D, rtol=ref.RTOL_D).numpy()
    e_host = float(np.abs(hst - want).max())
    e_dev = float(np.abs(end.out.astype(f64) - want).max())
    print(f"DOPRI5TRAJ d_n{n} | {steps} steps, {rejected} rejected, min |ratio - 1| {worst['gap']:.3f} | worst over the steps: out {worst['out']:.3f} "
          f"(err / P), SUMSQ rel {worst['sumsq']:.3e}, DT rel {worst['dt']:.3e} | e_host {e_host:.3e}, device to oracle {e_dev:.3e} "
          f"({e_dev / e_host:.2f} e_host)")
    assert e_dev <= 4 * e_host


# ---- (e) ga_dit_sampler_advance ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("batch", [1, 3, 64])
def test_e_sampler_advance(gpu_device, batch):
    """the one-thread kernel that closes every fused Euler step: timesteps[0..batch) and *dt take t_grid / dt_grid at min(counter + 1,
    grid_len - 1), the counter goes up by one also past the end; nothing beyond `batch` and no guard word is touched"""
    from gaussiananything_amd import dit_ops as ops
    L, rng = 5, np.random.default_rng(31)
    tg, dg = rng.uniform(0, 1, L).astype(f32), rng.uniform(0.01, 0.2, L).astype(f32)
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)      # noqa: E731

    def fresh(counter):
        b = {"t": Buf(tg, gpu_device), "d": Buf(dg, gpu_device), "ts": Buf(np.full(batch + 3, ref.POISON), gpu_device),
             "dt": Buf(np.full(1, ref.POISON), gpu_device)}
        c = torch.full((1 + GUARD,), GUARD_WORD, dtype=torch.int32, device=gpu_device)
        c[0] = counter
        return b, c

    def call(c, b, grid_len=L, bt=batch, null=None):
        p = {"c": c.data_ptr(), "t": b["t"].ptr, "d": b["d"].ptr, "ts": b["ts"].ptr, "dt": b["dt"].ptr}
        if null:
            p[null] = None
        with torch.cuda.device(gpu_device):
            rc = ops.lib().ga_dit_sampler_advance(p["c"], p["t"], p["d"], grid_len, p["ts"], bt, p["dt"], stream())
            torch.cuda.synchronize()
        return rc

    for counter in (0, 2, 3, 4, 7):
        b, c = fresh(counter)
        assert call(c, b) == OK
        at = min(counter + 1, L - 1)
        ts = b["ts"].get()
        assert ref.same_bits(ts[:batch], np.full(batch, tg[at])) and ref.same_bits(ts[batch:], np.full(3, ref.POISON)), counter
        assert ref.same_bits(b["dt"].get(), dg[at:at + 1]), counter
        assert int(c[0]) == counter + 1 and bool((c[1:] == GUARD_WORD).all())
        assert ref.same_bits(b["t"].get(), tg) and ref.same_bits(b["d"].get(), dg)
    b, c = fresh(2)
    for kw in (dict(bt=0), dict(bt=65), dict(grid_len=0)):
        assert call(c, b, **kw) == BAD_SHAPE, kw
    for null in ("c", "t", "d", "ts", "dt"):
        assert call(c, b, null=null) == NULL_ARG, null
    assert int(c[0]) == 2 and bool((c[1:] == GUARD_WORD).all())
    assert ref.same_bits(b["ts"].get(), np.full(batch + 3, ref.POISON)) and ref.same_bits(b["dt"].get(), np.full(1, ref.POISON))
