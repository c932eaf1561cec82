"""The bars of tests/test_dopri5_step_gpu.py, kept honest in both directions without a GPU.

`Emu` restates the four kernels of csrc/ode_dopri5.hip in numpy float32: the same operations, products and sums rounded one by one, fl32
of the float64 coefficient products, the grid-stride laps, the wave / workgroup / controller summation order of the error norm.  It is
driven through the same `attempt` and held by the same hold_stage / hold_finish as the device (tests/_dopri5_ref.py):
  * the honest emulation is inside every bar of (2a) and (2b);
  * every seeded mutation is over its bar in every case that claims it;
  * the conditions the bars rest on hold for the inputs (no ratio near 1, no tiny tol, the clamps reached, ...), on the reference alone;
  * the tableau of tests/_dopri5_ref.py equals oracle.ode's exactly."""
import math

import numpy as np
import pytest

from tests import _dopri5_ref as ref
from tests._dopri5_ref import ACCEPT, DONE, DT, DT_USED, ERROR, JBEG, JCOUNT, JNEXT, RATIO, REJECTED, STEPS, SUMSQ, T, TA, TB, f32, f64

ATOL, RTOL = ref.ATOL, ref.RTOL


class Emu:
    """the kernels in numpy fp32; `mut` names one seeded fault"""

    def __init__(self, state, mut=None):
        self.s, self.mut = state.copy(), mut

    def pull(self):
        return self.s.copy()

    def load(self, state):
        self.s = state.copy()

    def set_k(self, j, values):
        self.s.k[j] = np.array(values, f32)

    def reached(self, n):
        """elements the grid-stride loop of a 256-thread launch of grid_for(n) workgroups reaches"""
        return min(n, ref.nparts(n) * 256) if self.mut == "no_second_grid_lap" else n

    def stage(self, i):
        s, m = self.s, self.mut
        t, dt = float(s.ctl[T]), float(s.ctl[DT])
        Bm, Am = [list(r) + [0] * (6 - len(r)) for r in ref.B], list(ref.A)
        if m == "B31_B32_swapped":
            Bm[3][1], Bm[3][2] = Bm[3][2], Bm[3][1]
        if m == "B51_nonzero":
            Bm[5][1] = Bm[4][1]
        if m == "A3_is_A2":
            Am[3] = 4 / 5
        s.timesteps[:] = f32(t + Am[i] * dt)
        v = s.y.copy()
        with np.errstate(all="ignore"):
            for j in range(i + 1):
                if Bm[i][j] != 0:
                    v = v + f32(dt * Bm[i][j]) * s.k[j + 1 if (m == "stage_reads_next_k" and j == i) else j]
        r = self.reached(s.n)
        s.ystage[:r] = v[:r]

    def finish(self):
        s, m, n = self.s, self.mut, self.s.n
        G = ref.nparts(n)
        dt = float(s.ctl[DT])
        y, y1, k = s.y, s.ystage, s.k
        # error_kernel
        Em = list(ref.E)
        if m == "E6_sign":
            Em[6] = -Em[6]
        if m == "E5_without_b5_star":
            Em[5] = 11 / 84
        with np.errstate(all="ignore"):
            err = np.zeros(n, f32)
            for j in range(7):
                if Em[j] != 0:
                    err = err + f32(dt * Em[j]) * k[j]
            atol, rtol = f32(s.ctl[ATOL]), f32(s.ctl[RTOL])
            big = {"tol_min": np.fmin(np.abs(y), np.abs(y1)), "tol_y_alone": np.abs(y)}.get(m, np.fmax(np.abs(y), np.abs(y1)))
            tol = rtol * (atol + big) if m == "tol_rtol_on_all" else atol + rtol * big
            q = err / tol
            sq = (q * q).astype(f64)
            threads = G * 256
            acc = np.zeros(threads, f64)
            for lap in range(0, self.reached(n), threads):
                part = sq[lap:lap + threads]
                acc[:part.size] += part
            a = acc.reshape(G * 4, 64)
            for o in (32, 16, 8, 4, 2, 1):
                a[:, :o] = a[:, :o] + a[:, o:2 * o]
            w = a[:, 0].reshape(G, 4)
            parts = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
            s.ctl[ref.CTL_WORDS:ref.CTL_WORDS + G] = parts
            # control_kernel
            lanes = np.zeros(64, f64)
            for lap in range(0, 64 if m == "no_second_controller_lap" else G, 64):
                part = parts[lap:lap + 64]
                lanes[:part.size] += part
            for o in (32, 16, 8, 4, 2, 1):
                lanes[:o] = lanes[:o] + lanes[o:2 * o]
            sumsq = float(lanes[0])
        c = s.ctl
        c[ACCEPT] = c[JCOUNT] = 0.0
        if c[DONE] != 0.0:
            return
        t = float(c[T])
        with np.errstate(all="ignore"):
            ratio = float(np.sqrt(f64(sumsq)) / n) if m == "ratio_sqrt_over_n" else float(np.sqrt(f64(sumsq) / n))
        c[SUMSQ], c[RATIO] = sumsq, ratio
        c[STEPS] += 1.0
        if not math.isfinite(ratio) or not math.isfinite(dt) or t + dt == t:
            c[ERROR], c[DONE] = (2.0 if math.isfinite(ratio) else 1.0), 1.0
            return
        if ratio == 0.0:
            fac = 10.0
        else:
            safety, expo = (0.8 if m == "safety_0.8" else 0.9), (0.25 if m == "exponent_0.25" else 0.2)
            fac = min(10.0, max(safety / ratio ** expo, 1.0 if (ratio < 1.0 and m != "accepted_floor_0.2") else 0.2))
        c[DT_USED], c[DT] = dt, dt * fac
        if not ratio <= 1.0:
            c[REJECTED] += 1.0
            return
        tb = t + dt
        c[ACCEPT], c[TA], c[TB], c[T] = 1.0, t, tb, tb
        j0 = j1 = int(c[JNEXT])
        beyond = (lambda v: v >= tb) if m == "grid_time_at_tb_is_beyond" else (lambda v: v > tb)
        while j1 < len(s.t_grid) and not beyond(s.t_grid[j1]):
            j1 += 1
        c[JBEG], c[JCOUNT], c[JNEXT] = j0, j1 - j0, j1
        if j1 >= len(s.t_grid):
            c[DONE] = 1.0
        # accept_kernel
        r = self.reached(n)
        Mm = list(ref.MID)
        if m == "MID_without_half":
            Mm = [2 * v for v in Mm]
        if m == "MID2_MID3_swapped":
            Mm[2], Mm[3] = Mm[3], Mm[2]
        if m == "MID6_sign":
            Mm[6] = -Mm[6]
        if m == "MID0_off_by_1e-3":
            Mm[0] *= 1.001
        y0, f0, f1, dtf = y.copy(), k[0].copy(), k[6].copy(), f32(dt)
        if j1 > j0:
            mid = np.zeros(n, f32)
            for j in range(7):
                if Mm[j] != 0:
                    mid = mid + f32(dt * Mm[j]) * k[j]
            ym = y0 + mid
            F = f32
            a = ((F(2) * dtf) * (f1 - f0) - F(8) * (y1 + y0)) + F(16) * ym
            b = ((dtf * (F(5) * f0 - F(3) * f1) + F(18) * y0) + F(18 if m == "b_18_for_14" else 14) * y1) - F(32) * ym
            cc = ((dtf * (f1 - F(4) * f0) - F(11) * y0) - F(5) * y1) + F(16) * ym
            d = dtf * f0
            for j in range(j0, j1):
                x = f32((s.t_grid[j] - t) / (float(c[DT]) if m == "x_over_next_dt" else tb - t))
                s.out[j, :r] = (y0 + x * (d + x * (cc + x * (b + x * a))))[:r]
        s.y[:r] = y1[:r]
        s.k[0][:r] = f1[:r]


def run_a(n, batch, dt, mut=None):
    state, field = ref.case_a(n, batch, dt)
    return ref.attempt(Emu(state, mut), field)


def run_b(name, n, mut=None):
    return ref.attempt(Emu(ref.case_b(name, n), mut), nan_ok=name in ("nan", "inf"))


A_CPU = [(n, b) for n, b in ref.SIZES_A if n <= 16641]


@pytest.mark.parametrize("n,batch,dt", [(n, b, dt) for n, b in A_CPU for dt in ref.DTS_A] + [(524289, 3, ref.DTS_A[0])])
def test_the_honest_emulation_is_inside_every_bar_of_2a(n, batch, dt):
    before, after, fig = run_a(n, batch, dt)
    print(ref.line(f"emulation a_n{n}_b{batch}_dt{dt}", fig))
    assert fig["accept"] == (dt == ref.DTS_A[0])
    assert after.ctl[JCOUNT] == (3 if fig["accept"] else 0) and after.ctl[REJECTED] == (0 if fig["accept"] else 1)
    assert fig["dt"] == 0.0                               # (the emulation's pow is the reference's)


@pytest.mark.parametrize("n", ref.SIZES_B)
@pytest.mark.parametrize("name", ref.CASES_B)
def test_the_honest_emulation_is_inside_every_bar_of_2b(name, n):
    before, after, fig = run_b(name, n)
    ref.hold_expect_b(name, before, after)


# mutation -> the cases that claim it: ("a", n, batch, dt) or ("b", name, n)
A257, A257R = ("a", 257, 64, 0.05), ("a", 257, 64, 0.3)
A4608, A4608R = ("a", 4608, 3, 0.05), ("a", 4608, 3, 0.3)
MUTATIONS = {
    # kB and kA: the stage inputs are bit-exact
    "B31_B32_swapped": [A257, A4608R], "B51_nonzero": [A257, A4608R], "stage_reads_next_k": [A257, A4608R], "A3_is_A2": [A257, A4608R],
    # kCerr and the tolerance: SUMSQ
    "E6_sign": [A4608, A4608R], "E5_without_b5_star": [A4608, A4608R],
    "tol_min": [A4608, A4608R], "tol_y_alone": [A4608, A4608R], "tol_rtol_on_all": [A4608, A4608R],
    "ratio_sqrt_over_n": [A257, A4608R],
    # the dense output: out[1] (x = 1/4) and out[2] (x = 1/2); at x = 1 ymid cancels out of the quartic
    "MID_without_half": [A4608, A257], "MID2_MID3_swapped": [A4608, A257], "MID6_sign": [A4608, A257], "x_over_next_dt": [A4608, A257],
    "b_18_for_14": [A4608, A257], "MID0_off_by_1e-3": [A4608],
    # the controller
    "accepted_floor_0.2": [("b", "clamp1", 257), ("b", "clamp1", 16641)], "safety_0.8": [A257, A257R], "exponent_0.25": [A257, A257R],
    "grid_time_at_tb_is_beyond": [A257, ("b", "last_inside", 257)],
    # (n = 16385 has one element behind the 64th partial, whose share of the sum can be below the SUMSQ bar: not claimed)
    "no_second_controller_lap": [("a", 16641, 3, 0.05), ("a", 16641, 3, 0.3)],
    "no_second_grid_lap": [("a", 524289, 3, 0.05)],
}
OUT_OF_REACH = {}          # mutation -> why no case can see it (none: every mutation above is over a bar in every case that claims it)


@pytest.mark.parametrize("mut", sorted(MUTATIONS))
def test_every_seeded_mutation_is_over_its_bar(mut):
    for case in MUTATIONS[mut]:
        with pytest.raises(AssertionError) as e:
            run_a(*case[1:], mut=mut) if case[0] == "a" else ref.hold_expect_b(case[1], *run_b(case[1], case[2], mut=mut)[:2])
        print(f"MUTATION {mut} in {case}: {str(e.value).splitlines()[0][:150]}")
    assert mut not in OUT_OF_REACH


def test_the_mid_mutations_cannot_show_at_x_equal_1():
    """why the quarter point and the midpoint are in the grid of (2a): at x = 1 ymid cancels out of the quartic (16 - 32 + 16), so out at tb is
    inside P whatever kCmid is; it is out[1] and out[2] that catch them"""
    state, field = ref.case_a(4608, 3, 0.05)
    be = Emu(state, "MID6_sign")
    for i in range(6):
        be.stage(i)
        be.set_k(i + 1, field(be.s.timesteps[0], be.s.ystage))
    before = be.pull()
    be.finish()
    st = ref.Step(before.y, before.ystage, before.k, before.ctl[:ref.CTL_WORDS], before.t_grid)
    over = {j: float((np.abs(be.s.out[j].astype(f64) - st.out[j][0]) / st.out[j][1]).max()) for j in st.out}
    print("MID6_sign, worst err / P:", over)
    assert over[1] > 1 and over[2] > 1 and over[3] <= 1


# ---- conditions on the inputs, on the reference alone --------------------------------------------------------------------------------------

def _reference_step(state, field=None):
    s = state.copy()
    for i in range(6):
        s.ystage, s.timesteps = ref.stage(s.y, s.k, s.ctl[T], s.ctl[DT], i, s.batch)
        if field is not None:
            s.k[i + 1] = field(s.timesteps[0], s.ystage)
    return s, ref.Step(s.y, s.ystage, s.k, s.ctl[:ref.CTL_WORDS], s.t_grid)


@pytest.mark.parametrize("n,batch", A_CPU + [(524289, 3)])
def test_conditions_of_2a(n, batch):
    for dt in ref.DTS_A:
        s, st = _reference_step(*ref.case_a(n, batch, dt))
        assert abs(st.ratio - 1) > 1e-3 and (st.ratio < 1) == (dt == ref.DTS_A[0]), st.ratio
        assert float(st.tol.min()) >= 1e-7 and float(np.abs(st.err / st.tol).max()) <= 1e30
        # the three requested times lie inside (ta, tb] as the controller's comparison sees them
        t, tb = float(s.ctl[T]), float(s.ctl[T]) + float(s.ctl[DT])
        assert s.t_grid[0] < t and all(t < v and not v > tb for v in s.t_grid[1:4]) and s.t_grid[3] == tb and s.t_grid[4] > tb
        if st.head[ACCEPT]:
            assert sorted(st.out) == [1, 2, 3] and st.head[JNEXT] == 4 and st.head[DONE] == 0


@pytest.mark.parametrize("n", ref.SIZES_B)
def test_conditions_of_2b(n):
    for name in ref.CASES_B:
        s, st = _reference_step(ref.case_b(name, n))
        for w, v in ref.EXPECT_B[name].items():
            assert st.head[w] == v, (name, ref.NAMES[w], st.head[w])
        if math.isfinite(st.ratio):
            assert abs(st.ratio - 1) > 1e-3
    r = {name: _reference_step(ref.case_b(name, n))[1].ratio for name in ("tiny", "clamp1", "huge")}
    assert 0 < r["tiny"] and 0.9 / r["tiny"] ** 0.2 > 10          # the clamp at 10, reached by a non-zero ratio
    assert 0.6 < r["clamp1"] < 1 and 0.9 / r["clamp1"] ** 0.2 < 1  # the clamp at 1 of an accepted step
    assert 0.9 / r["huge"] ** 0.2 < 0.2                            # the clamp at 0.2


def _torch_field(field):
    import torch
    amp, lam = torch.from_numpy(field.amp), torch.from_numpy(field.lam)
    return lambda t, y: amp * torch.cos(3 * torch.as_tensor(t, dtype=torch.float32)) - lam * y


@pytest.mark.parametrize("n,lam_max", ref.SIZES_D)
def test_conditions_of_2d(n, lam_max):
    """the trajectory of (2d), by the reference driving itself: no ratio within 1e-3 of 1, the oracle rejects at least once, and the
    reference loop takes the oracle's decisions"""
    import torch
    from gaussiananything_amd.transport import odeint as host
    from oracle import ode as oracle
    field, y0 = ref.case_d(n, lam_max)
    tf = _torch_field(field)
    y0t = torch.from_numpy(y0)
    dt0 = host._initial_step(tf, 0.0, y0t, tf(0.0, y0t), ref.RTOL_D, ref.ATOL_D)
    ratios, steps, rejected, out = ref.trajectory_d(field, y0, dt0)
    stats = {}
    want = oracle.odeint(field.f64, y0.astype(f64), ref.GRID_D, atol=ref.ATOL_D, rtol=ref.RTOL_D, stats=stats)
    gap = min(abs(r - 1) for r in ratios)
    print(f"n = {n}: {steps} steps, {rejected} rejected (oracle: {stats['steps']}, {stats['rejected']}); min |ratio - 1| = {gap:.3f}; "
          f"max |reference loop - oracle| = {float(np.abs(out - want).max()):.3e}")
    assert gap > 1e-3
    assert stats["rejected"] >= 1
    assert (steps, rejected) == (stats["steps"], stats["rejected"])


def test_the_tableau_equals_the_oracles():
    from oracle import ode as oracle
    assert ref.A == oracle.A and ref.B == oracle.B and ref.E == oracle.E and ref.MID == oracle.MID
    assert all(len(r) == i + 1 for i, r in enumerate(ref.B)) and len(ref.E) == len(ref.MID) == 7
