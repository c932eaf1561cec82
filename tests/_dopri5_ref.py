"""The reference of ONE ATTEMPTED STEP of the device-resident Dormand-Prince 5(4) (csrc/ode_dopri5.hip: ga_ode_dopri5_stage /
ga_ode_dopri5_finish), the cases of tests/test_dopri5_step_gpu.py and the bars they are held to.  Numpy only.

An attempted step is a closed function of buffers the caller owns -- y, k[0..6], ctl, t_grid -- so no denoiser is needed: the test
supplies the k's.  The tableau is written out here (not imported from oracle/ode.py, transport/odeint.py or the kernel);
tests/test_dopri5_bounds_cpu.py asserts that it equals oracle.ode's, which is pinned to SciPy.

Determined bits (float32, one rounding per operation):
  ystage_i  = y + sum_j fl(fl32(dt B[i][j]) k_j), in increasing j, zero coefficients skipped; dt B formed in float64, then rounded
  timesteps = fl32(t + A[i] dt) in every one of the `batch` entries
  err       = the same chain from 0 with E;   tol = atol32 + fl(rtol32 max(|y|, |y1|)), y1 = ystage_5;   ymid = fl(y + chain(0, MID))
Float64 from those bits: sumsq = fsum((err / tol)^2), ratio = sqrt(sumsq / n), the controller, and the dense output (torchdiffeq's
quartic through (y0, f0), ymid, (y1, f1)) at the requested times in (ta, tb], from the fp32 values y0, y1, f0 = k[0], f1 = k[6], ymid,
fl32(dt) and x = fl32((t_j - ta) / (tb - ta)).

Bound of the dense output: P = gamma(16) S, S the same Horner expression with every term replaced by its absolute value.  The kernel's
translation unit contracts to FMA and the quartic is not protected; no path from an input to the result passes more than seven roundings
inside a coefficient (2 dt: exact; dt (f1 - f0): 2; 8 (y1 + y0): 1; the two sums of the three terms: 2; 16 ymid: exact -- b and c: a
constant times f, a sum, the product with dt, three more sums, the constants times y: at most 7) and eight in the Horner chain (four
products, four sums); an FMA only removes some.  15 <= 16.

Bars (hold_stage / hold_finish below; the same functions hold the device on the GPU and the fp32 emulation of the kernels on the CPU):
  ystage, timesteps                       bit-identical
  ctl[SUMSQ]                              5 * 2^-24 relative: err and tol have determined bits; the quotient is allowed one ulp of fp32
                                          (2^-23: faithful), doubled by the square, and the square's own rounding 2^-24; the float64
                                          summation error, (n + 70) 2^-53, is far below
  ctl[RATIO]                              sqrt(ctl[SUMSQ] / n) of the device's own SUMSQ within 2^-51 relative
  every other word of the head            equal as float64 values
  ctl[DT]                                 dt * factor(the device's own RATIO) within DT_BAR (the float64 pow is the only inexact operation)
  out[j]                                  within P, element by element
"""
import math

import numpy as np

from tests._bounds import gamma

f32, f64 = np.float32, np.float64

A = [1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0, 1.0]
B = [[1 / 5],
     [3 / 40, 9 / 40],
     [44 / 45, -56 / 15, 32 / 9],
     [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
     [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656],
     [35 / 384, 0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84]]
E = [35 / 384 - 1951 / 21600, 0, 500 / 1113 - 22642 / 50085, 125 / 192 - 451 / 720, -2187 / 6784 + 12231 / 42400,
     11 / 84 - 649 / 6300, -1 / 60]
MID = [6025192743 / 30085553152 / 2, 0, 51252292925 / 65400821598 / 2, -2691868925 / 45128329728 / 2,
       187940372067 / 1594534317056 / 2, -1776094331 / 19743644256 / 2, 11237099 / 235043384 / 2]

# include/ga_dit.h: indices into GaOdeDopri5.ctl
(T, DT, SUMSQ, ATOL, RTOL, DONE, STEPS, REJECTED, ACCEPT, TA, TB, DT_USED, JNEXT, JBEG, JCOUNT, ERROR, RATIO) = range(17)
CTL_WORDS, MAX_PARTIALS = 24, 2048
NAMES = ("T", "DT", "SUMSQ", "ATOL", "RTOL", "DONE", "STEPS", "REJECTED", "ACCEPT", "TA", "TB", "DT_USED", "JNEXT", "JBEG", "JCOUNT",
         "ERROR", "RATIO")

POISON = f32(-77.25)        # outputs before a call
FILL = -1234.5              # head words 17..23 and the partials of ctl before a call
SUMSQ_BAR = 5 * 2.0 ** -24
RATIO_BAR = 2.0 ** -51
# twice the worst |ctl[DT] - dt factor(ctl[RATIO])| / |.| over every case of the GPU run recorded in profiles/dopri5_bounds.txt
# (3.399e-16, in a step of the n = 4608 trajectory: an ulp of the float64 pow, carried through the quotient and the product); it may not
# exceed DT_CAP, below which no mutation of the controller can hide (each moves the factor by more than 1e-3)
DT_WORST = 3.399e-16
DT_BAR = 2 * DT_WORST
DT_CAP = 1e-12


def nparts(n):
    return min((n + 255) // 256, MAX_PARTIALS)


def chain(v, k, dt, cs):
    """v + sum_j fl(fl32(dt c_j) k_j): the product dt c in float64, rounded to fp32; products and sums rounded one by one"""
    with np.errstate(all="ignore"):
        for c, kj in zip(cs, k):
            if c != 0:
                v = v + f32(float(dt) * c) * kj
    return v


def stage(y, k, t, dt, i, batch):
    """(ystage_i, timesteps) from k[0..i]"""
    return chain(y.copy(), k[:i + 1], dt, B[i]), np.full(batch, f32(float(t) + A[i] * float(dt)), f32)


def factor(ratio):
    if ratio == 0.0:
        return 10.0
    return min(10.0, max(0.9 / ratio ** 0.2, 1.0 if ratio < 1.0 else 0.2))


def controller(head, sumsq, ratio, t_grid):
    """the head of ctl after control_kernel, from the head before it"""
    h = np.array(head, f64)
    h[ACCEPT] = h[JCOUNT] = 0.0
    if head[DONE] != 0.0:                    # a replay past the end: nothing else moves
        return h
    t, dt = float(head[T]), float(head[DT])
    h[SUMSQ], h[RATIO] = sumsq, ratio
    h[STEPS] += 1.0
    if not math.isfinite(ratio) or not math.isfinite(dt) or t + dt == t:
        h[ERROR] = 2.0 if math.isfinite(ratio) else 1.0
        h[DONE] = 1.0
        return h
    h[DT_USED] = dt
    h[DT] = dt * factor(ratio)
    if not ratio <= 1.0:
        h[REJECTED] += 1.0
        return h
    tb = t + dt
    h[ACCEPT], h[TA], h[TB], h[T] = 1.0, t, tb, tb
    j0 = j1 = int(head[JNEXT])
    while j1 < len(t_grid) and not t_grid[j1] > tb:
        j1 += 1
    h[JBEG], h[JCOUNT], h[JNEXT] = j0, j1 - j0, j1
    if j1 >= len(t_grid):
        h[DONE] = 1.0
    return h


def dense(y0, y1, f0, f1, ymid, dt, x):
    """(reference, bound P) of the quartic at x, in float64 from fp32 inputs"""
    h, x = float(f32(dt)), float(x)
    y0, y1, f0, f1, ym = (np.asarray(v, f64) for v in (y0, y1, f0, f1, ymid))
    a = 2 * h * (f1 - f0) - 8 * (y1 + y0) + 16 * ym
    b = h * (5 * f0 - 3 * f1) + 18 * y0 + 14 * y1 - 32 * ym
    c = h * (f1 - 4 * f0) - 11 * y0 - 5 * y1 + 16 * ym
    d = h * f0
    ref = y0 + x * (d + x * (c + x * (b + x * a)))
    h, y0, y1, f0, f1, ym = abs(h), abs(y0), abs(y1), abs(f0), abs(f1), abs(ym)
    a = 2 * h * (f1 + f0) + 8 * (y1 + y0) + 16 * ym
    b = h * (5 * f0 + 3 * f1) + 18 * y0 + 14 * y1 + 32 * ym
    c = h * (f1 + 4 * f0) + 11 * y0 + 5 * y1 + 16 * ym
    d = h * f0
    return ref, gamma(16) * (y0 + x * (d + x * (c + x * (b + x * a))))


class Step:
    """everything ga_ode_dopri5_finish computes from (y, y1 = ystage, k, the head of ctl, t_grid)"""

    def __init__(self, y, y1, k, head, t_grid):
        n, dt = y.size, float(head[DT])
        zero = np.zeros(n, f32)
        with np.errstate(all="ignore"):
            self.err = chain(zero, k, dt, E)
            self.tol = f32(head[ATOL]) + f32(head[RTOL]) * np.fmax(np.abs(y), np.abs(y1))     # (fmaxf: a NaN operand is dropped)
            self.ymid = y + chain(zero, k, dt, MID)
            sq = np.square(self.err.astype(f64) / self.tol.astype(f64))
            self.sumsq = math.fsum(sq) if bool(np.isfinite(sq).all()) else float(np.sum(sq))
            self.ratio = math.sqrt(self.sumsq / n) if math.isfinite(self.sumsq) else self.sumsq
        self.head = controller(head, self.sumsq, self.ratio, t_grid)
        self.out = {}
        if self.head[ACCEPT]:
            ta, tb = self.head[TA], self.head[TB]
            for j in range(int(self.head[JBEG]), int(self.head[JBEG] + self.head[JCOUNT])):
                x = f32((float(t_grid[j]) - ta) / (tb - ta))
                self.out[j] = dense(y, y1, k[0], k[6], self.ymid, dt, x)


# ---- the buffers of one GaOdeDopri5 on the host, and the bars ---------------------------------------------------------------------------

class State:
    FIELDS = ("y", "k", "ystage", "timesteps", "ctl", "t_grid", "out")

    def __init__(self, y, k, ctl, t_grid, batch):
        self.n, self.batch = y.size, batch
        self.y, self.k = y, list(k)
        self.ystage, self.timesteps = np.full(self.n, POISON), np.full(batch, POISON)
        self.ctl, self.t_grid = ctl, np.asarray(t_grid, f64)
        self.out = np.full((len(t_grid), self.n), POISON)

    def copy(self):
        s = State.__new__(State)
        s.n, s.batch = self.n, self.batch
        for name in self.FIELDS:
            v = getattr(self, name)
            setattr(s, name, [a.copy() for a in v] if name == "k" else v.copy())
        return s


def head_of(t, dt, atol=1e-6, rtol=1e-3, jnext=1, n=1):
    """ctl with exactly GA_ODE_CTL_WORDS + nparts doubles: words 17..23 and the partials filled"""
    ctl = np.full(CTL_WORDS + nparts(n), FILL, f64)
    ctl[:RATIO + 1] = 0.0
    ctl[T], ctl[DT], ctl[ATOL], ctl[RTOL], ctl[JNEXT] = t, dt, atol, rtol, jnext
    return ctl


def bits(a):
    a = np.ascontiguousarray(a)
    return a.reshape(-1).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want))


def same_bits_or_nan(got, want):
    """bit-identical; where the reference is NaN any NaN will do (sign and payload of a NaN are not the kernel's to keep)"""
    return got.shape == want.shape and bool(((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all())


def rel(got, want):
    return abs(got - want) / abs(want) if want != 0.0 else (0.0 if got == 0.0 else math.inf)


def hold_stage(before, after, i, nan_ok=False):
    """one ga_ode_dopri5_stage(i) call: ystage and timesteps have the reference's bits, nothing else moved"""
    ys, ts = stage(before.y, before.k, before.ctl[T], before.ctl[DT], i, before.batch)
    same = same_bits_or_nan if nan_ok else same_bits
    assert same(after.ystage, ys), f"stage {i}: ystage differs from the reference in {int((bits(after.ystage) != bits(ys)).sum())} elements"
    assert same_bits(after.timesteps, ts), f"stage {i}: timesteps {after.timesteps[:2]} != {ts[:1]}"
    for name in ("y", "ctl", "t_grid", "out"):
        assert same_bits(getattr(after, name), getattr(before, name)), f"stage {i} touched {name}"
    for j in range(7):
        assert same_bits(after.k[j], before.k[j]), f"stage {i} touched k[{j}]"


def hold_finish(before, after):
    """one ga_ode_dopri5_finish call against the reference of the buffers as they were before it.  Returns the figures:
    {"sumsq": relative difference, "dt": relative difference (None where DT does not move), "out": {j: worst err / P}, "ratio": ...}"""
    n, head, got = before.n, before.ctl[:CTL_WORDS], after.ctl[:CTL_WORDS]
    ref = Step(before.y, before.ystage, before.k, head, before.t_grid)
    fig = {"sumsq": 0.0, "dt": None, "out": {}, "ratio": ref.ratio, "accept": bool(ref.head[ACCEPT])}
    assert same_bits(got[RATIO + 1:], head[RATIO + 1:]), "head words 17..23 changed"
    for name in ("k", "ystage", "timesteps", "t_grid"):
        if name == "k":
            for j in range(1, 7):
                assert same_bits(after.k[j], before.k[j]), f"finish touched k[{j}]"
        else:
            assert same_bits(getattr(after, name), getattr(before, name)), f"finish touched {name}"
    exact = [w for w in range(RATIO + 1) if w not in (SUMSQ, RATIO, DT)]
    if head[DONE] != 0.0:                     # only ACCEPT and JCOUNT are written
        exact += [SUMSQ, RATIO, DT]
    else:
        if math.isfinite(ref.sumsq):
            fig["sumsq"] = rel(float(got[SUMSQ]), ref.sumsq)
            assert fig["sumsq"] <= SUMSQ_BAR, f"SUMSQ {got[SUMSQ]!r} against {ref.sumsq!r}: {fig['sumsq']:.3e} relative"
            want = math.sqrt(float(got[SUMSQ]) / n)
            assert rel(float(got[RATIO]), want) <= RATIO_BAR, f"RATIO {got[RATIO]!r} is not sqrt(SUMSQ / n) = {want!r}"
        else:
            assert not math.isfinite(got[SUMSQ]) and not math.isfinite(got[RATIO]), (got[SUMSQ], got[RATIO])
        if ref.head[ERROR] != 0.0:
            exact.append(DT)
        else:
            want = float(head[DT]) * factor(float(got[RATIO]))
            fig["dt"] = rel(float(got[DT]), want)
            assert fig["dt"] <= DT_BAR <= DT_CAP, f"DT {got[DT]!r} against dt factor(RATIO) = {want!r}: {fig['dt']:.3e} relative"
    for w in exact:
        assert got[w] == ref.head[w] and not (got[w] != got[w]), f"ctl[{NAMES[w]}] = {got[w]!r}, reference {ref.head[w]!r}"
    if ref.head[ACCEPT]:
        assert same_bits(after.y, before.ystage), "accepted step: y is not y1"
        assert same_bits(after.k[0], before.k[6]), "accepted step: k[0] is not k[6]"
    else:
        assert same_bits(after.y, before.y) and same_bits(after.k[0], before.k[0]), "y or k[0] moved without an accepted step"
    for j in range(len(before.t_grid)):
        if j in ref.out:
            want, P = ref.out[j]
            err = np.abs(after.out[j].astype(f64) - want)
            with np.errstate(all="ignore"):
                q = np.where(err == 0.0, 0.0, err / P)
            fig["out"][j] = float(q.max())
            assert bool((err <= P).all()), f"out[{j}]: {int((err > P).sum())} elements over P, worst err / P = {fig['out'][j]:.3f}"
        else:
            assert same_bits(after.out[j], before.out[j]), f"out[{j}] was written"
    return fig


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------

class Field:
    """f(t, y) = amp cos(3 t) - lam * y in fp32, the product a value of its own before the subtraction"""

    def __init__(self, n, lam_max, seed):
        rng = np.random.default_rng(seed)
        self.lam = rng.uniform(0.5, lam_max, n).astype(f32)
        self.amp = rng.uniform(0.5, 2.0, n).astype(f32)

    def __call__(self, t, y):
        c = f32(math.cos(float(f32(3.0) * f32(t))))
        return self.amp * c - self.lam * y

    def f64(self, t, y):
        return self.amp.astype(f64) * math.cos(3.0 * t) - self.lam.astype(f64) * y


SIZES_A = [(1, 1), (63, 3), (64, 64), (255, 1), (256, 3), (257, 64), (4608, 3), (16384, 1), (16385, 64), (16641, 3), (524288, 1),
           (524289, 3), (530000, 64)]
DTS_A = [0.05, 0.3]          # accepted (ratio ~ 3e-3), rejected (ratio ~ 35)
T_A = 0.1


def grid_a(t, dt):
    """one before t, t + dt / 4, t + dt / 2, tb = t + dt as the controller forms it, one beyond"""
    return [t - 0.05, t + 0.25 * dt, t + 0.5 * dt, t + dt, t + 2 * dt]


def case_a(n, batch, dt):
    """(state, field): y standard normal, k[0] = f(t, y), k[1..6] random until the test writes them from f of the stage inputs"""
    rng = np.random.default_rng(5000 + n)
    field = Field(n, 8.0, 6000 + n)
    y = rng.standard_normal(n).astype(f32)
    k = [field(f32(T_A), y)] + [rng.standard_normal(n).astype(f32) for _ in range(6)]
    return State(y, k, head_of(T_A, dt, n=n), grid_a(T_A, dt), batch), field


SIZES_B = [257, 16641]
CASES_B = ("zero", "tiny", "clamp1", "huge", "nan", "inf", "zero_over_zero", "underflow", "done", "none_inside", "last_inside",
           "grid_len_1")
# what the reference must say of each case (asserted on the reference in tests/test_dopri5_bounds_cpu.py, on the device on the GPU)
EXPECT_B = {"zero": {ACCEPT: 1, RATIO: 0.0, ERROR: 0}, "tiny": {ACCEPT: 1, ERROR: 0}, "clamp1": {ACCEPT: 1, ERROR: 0},
            "huge": {ACCEPT: 0, REJECTED: 1, ERROR: 0}, "nan": {ACCEPT: 0, ERROR: 1, DONE: 1, STEPS: 1},
            "inf": {ACCEPT: 0, ERROR: 1, DONE: 1, STEPS: 1}, "zero_over_zero": {ACCEPT: 0, ERROR: 1, DONE: 1, STEPS: 1},
            "underflow": {ACCEPT: 0, ERROR: 2, DONE: 1, STEPS: 1}, "done": {ACCEPT: 0, JCOUNT: 0, DONE: 1, STEPS: 3, ERROR: 0},
            "none_inside": {ACCEPT: 1, JCOUNT: 0, JNEXT: 1, DONE: 0}, "last_inside": {ACCEPT: 1, JBEG: 1, JCOUNT: 2, JNEXT: 3, DONE: 1},
            "grid_len_1": {ACCEPT: 1, JCOUNT: 0, JNEXT: 1, DONE: 1}}
FACTOR_B = {"zero": 10.0, "tiny": 10.0, "clamp1": 1.0, "huge": 0.2}       # DT = dt * this, exactly


def _ratio_of(y, k, ctl, grid):
    """the reference ratio of a hand-set case (y1 by the reference's own stage 5)"""
    y1, _ = stage(y, k, ctl[T], ctl[DT], 5, 1)
    return Step(y, y1, k, ctl[:CTL_WORDS], grid).ratio


def case_b(name, n, batch=3):
    """k set by hand.  `clamp1` scales a random k so that the ratio is 0.8 (a fixed point of three sweeps: tol depends on y1)"""
    rng = np.random.default_rng(7000 + n)
    y = rng.standard_normal(n).astype(f32)
    g = [rng.standard_normal(n).astype(f32) for _ in range(7)]
    t, dt, kw = T_A, 0.05, {}
    if name == "underflow":
        t, dt = 1.0, 1e-17
    if name == "huge":
        kw = dict(atol=1e-9, rtol=1e-6)
    if name == "zero_over_zero":
        kw = dict(atol=0.0)
    grid = {"none_inside": [t - 0.05, t + 2 * dt, t + 3 * dt], "last_inside": [t - 0.05, t + 0.5 * dt, t + dt],
            "grid_len_1": [t]}.get(name, grid_a(t, dt))
    ctl = head_of(t, dt, n=n, **kw)
    if name == "zero":
        k = [np.zeros(n, f32) for _ in range(7)]
    elif name == "tiny":
        k = [f32(1e-9) * v for v in g]
    elif name == "huge":
        k = [f32(100.0) * v for v in g]
    elif name == "underflow":
        k = g
    else:
        s = 1.0
        for _ in range(3):
            s *= 0.8 / _ratio_of(y, [f32(s) * v for v in g], ctl, grid)
        k = [f32(s) * v for v in g]
    if name == "nan":
        k[3][-1] = np.nan
    if name == "inf":
        k[3][-1] = np.inf
    if name == "zero_over_zero":
        y[n // 2] = 0.0
        for v in k:
            v[n // 2] = 0.0
    if name == "done":
        ctl[DONE], ctl[STEPS], ctl[ACCEPT], ctl[JCOUNT] = 1.0, 3.0, 1.0, 2.0
    return State(y, k, ctl, grid, batch)


def hold_expect_b(name, before, after):
    """what a case of (2b) names: the branch of the controller it is there for"""
    for w, v in EXPECT_B[name].items():
        assert after.ctl[w] == v, (name, NAMES[w], after.ctl[w], v)
    if name in FACTOR_B:
        assert after.ctl[DT] == before.ctl[DT] * FACTOR_B[name], (name, after.ctl[DT])
    if EXPECT_B[name].get(ERROR):
        assert after.ctl[DT] == before.ctl[DT] and after.ctl[T] == before.ctl[T]
    if name == "done":
        rest = [w for w in range(CTL_WORDS) if w not in (ACCEPT, JCOUNT)]         # only ACCEPT and JCOUNT are written
        assert same_bits(after.ctl[rest], before.ctl[rest])
    if name == "none_inside":
        assert not same_bits(after.y, before.y) and same_bits(after.out, before.out)


# (2d) a whole integration
SIZES_D = [(257, 60.0), (4608, 30.0)]
GRID_D = np.linspace(0.0, 1.0, 9)
ATOL_D, RTOL_D = 1e-6, 1e-3


def case_d(n, lam_max):
    field = Field(n, lam_max, 8000 + n)
    y0 = np.random.default_rng(9000 + n).standard_normal(n).astype(f32)
    return field, y0


def trajectory_d(field, y0, dt0, max_steps=200):
    """the reference driving itself over GRID_D: (ratios of every attempted step, steps, rejected, out)"""
    n = y0.size
    s = State(y0.copy(), [field(f32(0.0), y0)] + [np.zeros(n, f32) for _ in range(6)], head_of(0.0, dt0, ATOL_D, RTOL_D, n=n), GRID_D, 1)
    s.out[0] = y0
    ratios = []
    while s.ctl[DONE] == 0.0 and len(ratios) < max_steps:
        for i in range(6):
            s.ystage, s.timesteps = stage(s.y, s.k, s.ctl[T], s.ctl[DT], i, 1)
            s.k[i + 1] = field(s.timesteps[0], s.ystage)
        st = Step(s.y, s.ystage, s.k, s.ctl[:CTL_WORDS], s.t_grid)
        ratios.append(st.ratio)
        s.ctl[:CTL_WORDS] = st.head
        if st.head[ACCEPT]:
            s.y, s.k[0] = s.ystage, s.k[6]
            for j, (ref, _) in st.out.items():
                s.out[j] = ref.astype(f32)
    return ratios, int(s.ctl[STEPS]), int(s.ctl[REJECTED]), s.out


def attempt(be, field=None, nan_ok=False):
    """one attempted step on a backend (the device, or the emulation of the kernels): six stage calls, each held to hold_stage and, with a
    field, followed by k[i + 1] = f(timesteps[0], ystage); the finish call held to hold_finish; and a second finish from the same buffers
    that must give the same bits.  A backend has pull() -> State, load(State), set_k(j, values), stage(i), finish()."""
    for i in range(6):
        before = be.pull()
        be.stage(i)
        after = be.pull()
        hold_stage(before, after, i, nan_ok)
        if field is not None:
            be.set_k(i + 1, field(after.timesteps[0], after.ystage))
    before = be.pull()
    be.finish()
    after = be.pull()
    fig = hold_finish(before, after)
    be.load(before)
    be.finish()
    again = be.pull()
    for name in ("ctl", "y", "out"):
        assert same_bits(getattr(again, name), getattr(after, name)), f"a second identical finish call gave another {name}"
    return before, after, fig


def line(tag, fig):
    """one line of profiles/dopri5_bounds.txt"""
    outs = ", ".join(f"out[{j}] {v:.3f}" for j, v in sorted(fig["out"].items())) or "no out"
    dt = "DT unchanged" if fig["dt"] is None else f"DT rel {fig['dt']:.3e}"
    return f"DOPRI5CASE {tag} | ratio {fig['ratio']:.4g}, {'accepted' if fig['accept'] else 'not accepted'} | {outs} (err / P) | SUMSQ rel {fig['sumsq']:.3e} | {dt}"
