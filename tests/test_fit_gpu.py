"""The surfel fitter on the device (include/ga_fit.h, gaussiananything_amd/fitting.py).

Kernel level: ``ga_fit_activate``, ``ga_fit_adam`` and ``ga_fit_advance`` against the float32 restatement of tests/_fit_ref.py, bit for bit
where the arithmetic is pinned (everything but exp); ``ga_fit_pack_grads`` bit for bit against autograd through the differentiable
branch of ``GaussianRenderer2DGS.render``.

Fitter level: the YARDSTICK is the loop a user could write before the fitter existed -- ``render`` with grad, ``photometric_loss``,
``geometric_loss``, ``.backward()`` -- run twice, the second time with every raw element moved by one float32 ulp.  The spread between
those two runs is what rounding-level differences and the floating-point atomics of ``ga_surfel_backward`` do to the quantity compared;
the fitter, whose glue differs from autograd's in about four places at rounding level, gets 4 x that spread.  Figures of the last run:
profiles/fit_parity.txt."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _fit_ref as ref

pytestmark = pytest.mark.gpu

LR = dict(xyz=(1.6e-4, 1.6e-6), opacity=(0.05, 0.01), scale=(0.005, 0.001), rotation=(0.001, 0.0002), rgb=(0.0025, 0.0005))
BETAS, EPS = (0.9, 0.999), 1e-15
NS = (1, 63, 65, 257, 1000)
ULP_FLOOR = 4


def _bits(t):
    t = t.detach().cpu().contiguous() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.view(torch.int32)


def _same_bits(got, want, what):
    a, b = _bits(got), _bits(want)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = a != b
    if bool(bad.any()):
        g, w = a.view(torch.float32)[bad], b.view(torch.float32)[bad]
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ in bits, e.g. got {g[0].item()!r} want "
                             f"{w[0].item()!r}; largest |difference| {float((g.double() - w.double()).abs().max()):.3e}")


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _raw(n, seed):
    rng = np.random.default_rng(seed)
    raw = rng.standard_normal((n, 13)).astype(np.float32)
    raw[:, 3] *= 4                                           # opacities into both tails of the sigmoid
    raw[:, 4:6] = raw[:, 4:6] * 2 - 4.0
    raw[:, 6:10] *= rng.choice([0.3, 1.0, 5.0], size=(n, 1)).astype(np.float32)
    return raw


def _mixed(rng, shape):
    g = rng.standard_normal(shape) * np.power(10.0, rng.uniform(-6, 2, size=shape))
    pick = rng.integers(0, 8, size=shape)
    g[pick == 0] = 0.0
    g[pick == 1] = 1e-20 * np.sign(g[pick == 1])
    g[pick == 2] = 1e4 * np.sign(g[pick == 2])
    return g.astype(np.float32)


class _Kernels:
    """the three per-surfel kernels on buffers of their own, through the C-ABI"""

    def __init__(self, dev, raw, num_views=1, max_steps=8, lr=LR, flags=0, radii=None, history_from_raw=False):
        from gaussiananything_amd import _lib, fitting
        self.lib, self.L, self.dev = _lib, _lib.lib(), dev
        n = self.n = raw.shape[0]
        z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        self.raw, self.m, self.v, self.raw_grad = torch.from_numpy(raw).to(dev), z(n, 13), z(n, 13), z(n, 13)
        self.act = {"means": z(n, 3), "opacities": z(n), "colors": z(n, 3), "scales": z(n, 2), "rotations": z(n, 4), "inv_norm": z(n)}
        self.g = {"g_means": z(n, 3), "g_opacities": z(n), "g_colors": z(n, 3), "g_scales": z(n, 2), "g_rotations": z(n, 4)}
        self.table = fitting.step_table(lr, BETAS, max_steps).to(dev)
        self.counter = torch.zeros(1, dtype=torch.int32, device=dev)
        self.history = z(max_steps, 8)
        self.radii = radii if radii is not None else torch.ones(num_views, n, dtype=torch.int32, device=dev)
        self.ones = torch.ones(1, 3, dtype=torch.float32, device=dev)
        a = self.act
        self.a_act = _lib.GaFitActivateArgs(n, 0, self.raw.data_ptr(), a["means"].data_ptr(), a["opacities"].data_ptr(),
                                            a["colors"].data_ptr(), a["scales"].data_ptr(), a["rotations"].data_ptr(), a["inv_norm"].data_ptr())
        g = self.g
        self.a_adam = _lib.GaFitAdamArgs(
            n, num_views, flags, max_steps, g["g_means"].data_ptr(), g["g_opacities"].data_ptr(), g["g_colors"].data_ptr(),
            g["g_scales"].data_ptr(), g["g_rotations"].data_ptr(), a["opacities"].data_ptr(), a["colors"].data_ptr(), a["scales"].data_ptr(),
            a["rotations"].data_ptr(), a["inv_norm"].data_ptr(), self.raw.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
            self.radii.data_ptr(), self.table.data_ptr(), self.counter.data_ptr(), BETAS[0], 1.0 - BETAS[0], BETAS[1], 1.0 - BETAS[1], EPS,
            0, self.raw_grad.data_ptr())
        # history_from_raw: the "loss means" the advance kernel reads are the first three floats of raw, weighted 1: a row per step
        # that differs from every other and that the restatement can predict
        self.a_adv = _lib.GaFitAdvanceArgs(1, max_steps, self.counter.data_ptr(), self.raw.data_ptr() if history_from_raw else None,
                                           None, self.ones.data_ptr(), None, self.history.data_ptr(), 0.0, 0, None, None)

    def set_grads(self, g13):
        """g13 [N,13] float32 (numpy), with respect to the activated values"""
        t = torch.from_numpy(g13).to(self.dev)
        for k, cols in (("g_means", slice(0, 3)), ("g_scales", slice(4, 6)), ("g_rotations", slice(6, 10)), ("g_colors", slice(10, 13))):
            self.g[k].copy_(t[:, cols])
        self.g["g_opacities"].copy_(t[:, 3])

    def activate(self):
        self.lib.check(self.L.ga_fit_activate(ctypes.byref(self.a_act), _stream(self.dev)), "ga_fit_activate")

    def iteration(self):
        s = _stream(self.dev)
        self.lib.check(self.L.ga_fit_activate(ctypes.byref(self.a_act), s), "ga_fit_activate")
        self.lib.check(self.L.ga_fit_adam(ctypes.byref(self.a_adam), s), "ga_fit_adam")
        self.lib.check(self.L.ga_fit_advance(ctypes.byref(self.a_adv), s), "ga_fit_advance")

    def act_numpy(self):
        return {k: t.cpu().numpy() for k, t in self.act.items()}


def _split(g13):
    return {"g_means": g13[:, 0:3], "g_opacities": g13[:, 3], "g_scales": g13[:, 4:6], "g_rotations": g13[:, 6:10], "g_colors": g13[:, 10:13]}


# ---- 4: activation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_activate(gpu_device, n):
    """xyz and the normalised quaternion bit-equal to the restatement; sigmoid and exp against float64 within 2 E + 4 ulp, E the error
    of torch's own float32 sigmoid / exp on the device on the same inputs"""
    raw = _raw(n, 40 + n)
    k = _Kernels(gpu_device, raw)
    k.activate()
    got, want = k.act_numpy(), ref.activate(raw)
    _same_bits(got["means"], want["means"], "means")
    _same_bits(got["rotations"], want["rotations"], "rotations")
    _same_bits(got["inv_norm"], want["inv_norm"], "inv_norm")
    r64 = torch.from_numpy(raw).double()
    rd = torch.from_numpy(raw).to(gpu_device)
    for name, mine, exact, t32 in (
            ("opacities", got["opacities"], torch.sigmoid(r64[:, 3]), torch.sigmoid(rd[:, 3])),
            ("colors", got["colors"], torch.sigmoid(r64[:, 10:13]), torch.sigmoid(rd[:, 10:13])),
            ("scales", got["scales"], torch.exp(r64[:, 4:6]), torch.exp(rd[:, 4:6]))):
        exact = exact.numpy()
        rel = lambda x: np.abs(np.asarray(x, np.float64) - exact) / ref.ulp(exact)     # errors in ulp of the exact value
        E = float(rel(t32.cpu().numpy()).max())
        err = float(rel(mine).max())
        print(f"activate N={n} {name}: E_torch32 {E:.3f} ulp, kernel {err:.3f} ulp")
        assert err <= 2 * E + ULP_FLOOR, (name, err, E)


# ---- 5: chain rule + Adam ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("num_views", (1, 2))
@pytest.mark.parametrize("n", NS)
def test_adam_bit_equal_to_the_restatement(gpu_device, n, num_views):
    """5 steps on synthetic gradients of mixed magnitude (exact zeros, 1e-20, 1e+4): raw, m, v and raw_grad bit-equal to the
    restatement fed with the kernel's own activated values, after every step"""
    rng = np.random.default_rng(500 + n)
    raw = _raw(n, 50 + n)
    k = _Kernels(gpu_device, raw, num_views=num_views)
    tab = k.table.cpu().numpy()
    r, m, v = raw.copy(), np.zeros_like(raw), np.zeros_like(raw)
    for t in range(5):
        g13 = _mixed(rng, (n, 13))
        k.set_grads(g13)
        k.iteration()
        graw = ref.chain_rule(_split(g13), k.act_numpy())
        r, m, v = ref.adam_step(r, m, v, graw, tab[t], BETAS, EPS)
        _same_bits(k.raw_grad, graw, f"raw_grad, step {t}")
        _same_bits(k.raw, r, f"raw, step {t}")
        _same_bits(k.m, m, f"m, step {t}")
        _same_bits(k.v, v, f"v, step {t}")
    assert int(k.counter.cpu()) == 5


# ---- 6: GA_FIT_VISIBLE_ONLY ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (65, 257))
def test_visible_only(gpu_device, n):
    """rows whose radius is 0 in every view keep raw, m and v bit-identical with the flag; without it they take the zero-gradient
    update, in which m and v decay"""
    from gaussiananything_amd import _lib
    rng = np.random.default_rng(600 + n)
    raw = _raw(n, 60 + n)
    radii = torch.from_numpy(rng.integers(0, 3, size=(2, n)).astype(np.int32))
    radii[:, ::3] = 0
    radii[0, 1] = 0; radii[1, 1] = 7                       # seen by the second view only: visible
    hidden = (radii == 0).all(0).numpy()
    assert hidden.any() and not hidden.all() and not hidden[1]
    m0, v0 = np.abs(_mixed(rng, (n, 13))) + 1e-3, np.abs(_mixed(rng, (n, 13))) + 1e-3
    g13 = _mixed(rng, (n, 13))
    g13[hidden] = 0                                            # what the rasterizer's backward hands an unseen surfel
    for flags in (_lib.GA_FIT_VISIBLE_ONLY, 0):
        k = _Kernels(gpu_device, raw, num_views=2, flags=flags, radii=radii.to(gpu_device))
        k.m.copy_(torch.from_numpy(m0)); k.v.copy_(torch.from_numpy(v0))
        k.set_grads(g13)
        k.iteration()
        graw = ref.chain_rule(_split(g13), k.act_numpy())
        r, m, v = ref.adam_step(raw, m0, v0, graw, k.table[0].cpu().numpy(), BETAS, EPS, keep=hidden if flags else None)
        for name, got, want, before in (("raw", k.raw, r, raw), ("m", k.m, m, m0), ("v", k.v, v, v0)):
            _same_bits(got, want, f"{name}, flags {flags}")
            same = (_bits(got) == _bits(before)).all(1).numpy()
            if flags:
                assert same[hidden].all() and not same[~hidden].any(), name
            elif name != "raw":
                assert not same[hidden].any(), name                # m and v decayed
                assert (np.abs(got.cpu().numpy()[hidden]) < np.abs(before[hidden])).all(), name


# ---- 7: device counter and table -----------------------------------------------------------------------------------------------------
def test_graph_replay_advances_the_device_counter(gpu_device):
    """activate + adam + advance captured once and replayed 6 times, the table's rows all different: bit-equal to 6 eager calls and to
    the restatement, and 6 distinct history rows.  A counter frozen into the graph would use row 0 six times and write history row 0
    six times."""
    n, steps = 257, 6
    raw = _raw(n, 70)
    g13 = _mixed(np.random.default_rng(71), (n, 13))
    eager = _Kernels(gpu_device, raw, history_from_raw=True)
    eager.set_grads(g13)
    tab = eager.table.cpu().numpy()
    assert len({tuple(row) for row in tab.tolist()}) == tab.shape[0]
    r, m, v = raw.copy(), np.zeros_like(raw), np.zeros_like(raw)
    hist = np.zeros((steps, 8), np.float32)
    for t in range(steps):
        eager.iteration()
        graw = ref.chain_rule(_split(g13), eager.act_numpy())
        r, m, v = ref.adam_step(r, m, v, graw, tab[t], BETAS, EPS)
        hist[t, 1:4] = r[0, 0:3]
        hist[t, 0] = np.float32(np.float64(r[0, 0]) + np.float64(r[0, 1]) + np.float64(r[0, 2]))
    torch.cuda.synchronize()
    replayed = _Kernels(gpu_device, raw, history_from_raw=True)
    replayed.set_grads(g13)
    side = torch.cuda.Stream(device=gpu_device)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            replayed.iteration()
    torch.cuda.synchronize()
    for _ in range(steps):
        graph.replay()
    torch.cuda.synchronize()
    for name in ("raw", "m", "v", "raw_grad", "history", "counter"):
        _same_bits(getattr(replayed, name).float(), getattr(eager, name).float(), f"replayed {name} against eager")
    _same_bits(replayed.raw, r, "raw against the restatement")
    _same_bits(replayed.m, m, "m against the restatement")
    _same_bits(replayed.v, v, "v against the restatement")
    h = replayed.history.cpu().numpy()
    _same_bits(h[:steps], hist, "history against the restatement")
    assert len({tuple(row) for row in h[:steps].tolist()}) == steps and not h[steps:].any()
    assert int(replayed.counter.cpu()) == steps


def test_counter_stays_on_the_last_row(gpu_device):
    raw = _raw(5, 72)
    k = _Kernels(gpu_device, raw, max_steps=3)
    k.set_grads(_mixed(np.random.default_rng(73), (5, 13)))
    for _ in range(5):
        k.iteration()
    assert int(k.counter.cpu()) == 2


# ---- 8: the adjoint of render's differentiable branch --------------------------------------------------------------------------------
PACK_SHAPES = [(1, 32, 32), (2, 64, 64), (2, 40, 56), (1, 33, 35)]     # 40 x 56: a partly filled last workgroup; 33 x 35: one pixel per lane


@pytest.mark.parametrize("absent", ((), ("g_image",), ("g_rend_normal", "g_depth"), ("g_dist", "g_alpha"),
                                    ("g_image", "g_rend_normal", "g_depth", "g_dist", "g_alpha")))
@pytest.mark.parametrize("shape", PACK_SHAPES)
def test_pack_grads_is_the_adjoint_of_render(gpu_device, shape, absent):
    """bit-equal to autograd through the five lines of the differentiable branch of ``render`` on the same color / allmap: colours
    exactly 0, exactly 1 and beyond, NaN and +-inf in the median depth, absent terms"""
    from gaussiananything_amd import _lib, synthetic
    V, H, W = shape
    gen = torch.Generator().manual_seed(80 + H)
    color = torch.rand(V, 3, H, W, generator=gen) * 1.4 - 0.2
    allmap = torch.randn(V, 7, H, W, generator=gen)
    flat = color.view(-1)
    flat[0], flat[1], flat[2], flat[3], flat[-1] = 0.0, 1.0, 1.0000001, -1e-8, float("nan")
    allmap[0, 5, 0, 0], allmap[0, 5, 0, 5], allmap[0, 5, 0, 6], allmap[-1, 5, -1, -1] = float("nan"), float("inf"), float("-inf"), float("nan")
    view = synthetic.eval_cameras(2)["cam_view"][:V].float()
    grads = {"g_image": torch.randn(V, 3, H, W, generator=gen), "g_rend_normal": torch.randn(V, 3, H, W, generator=gen),
             "g_depth": torch.randn(V, 1, H, W, generator=gen), "g_dist": torch.randn(V, 1, H, W, generator=gen),
             "g_alpha": torch.randn(V, 1, H, W, generator=gen)}
    dev = gpu_device
    color, allmap, view = color.to(dev).requires_grad_(True), allmap.to(dev).requires_grad_(True), view.to(dev)
    vm = view.reshape(V, 16).contiguous()
    grads = {k: (None if k in absent else t.to(dev)) for k, t in grads.items()}
    outs = {"g_image": color.clamp(0, 1), "g_alpha": allmap[:, 1:2],
            "g_rend_normal": torch.einsum("vchw,vdc->vdhw", allmap[:, 2:5], view[:, :3, :3]),
            "g_depth": torch.nan_to_num(allmap[:, 5:6], 0, 0), "g_dist": allmap[:, 6:7]}
    live = [k for k in outs if grads[k] is not None]
    if live:
        want_c, want_a = torch.autograd.grad([outs[k] for k in live], [color, allmap], [grads[k] for k in live], allow_unused=True)
    else:
        want_c = want_a = None
    want_c = torch.zeros_like(color) if want_c is None else want_c
    want_a = torch.zeros_like(allmap) if want_a is None else want_a
    g_color, g_allmap = torch.full_like(want_c, 7.0), torch.full_like(want_a, 7.0)
    ptr = lambda t: None if t is None else t.data_ptr()
    args = _lib.GaFitPackArgs(V, H, W, 0, color.data_ptr(), allmap.data_ptr(), vm.data_ptr(),
                              ptr(grads["g_image"]), ptr(grads["g_rend_normal"]), ptr(grads["g_depth"]), ptr(grads["g_dist"]),
                              ptr(grads["g_alpha"]), g_color.data_ptr(), g_allmap.data_ptr())
    _lib.check(_lib.lib().ga_fit_pack_grads(ctypes.byref(args), _stream(dev)), "ga_fit_pack_grads")
    torch.cuda.synchronize()
    _same_bits(g_color, want_c, "g_color")
    for ch in range(7):
        _same_bits(g_allmap[:, ch], want_a[:, ch], f"g_allmap channel {ch}")
    assert not g_allmap[:, 0].any()


def test_plan(gpu_device):
    from gaussiananything_amd import _lib
    pl = _lib.GaFitPlan()
    assert _lib.lib().ga_fit_plan(1000, 2, 40, 56, ctypes.byref(pl)) == 0
    assert (pl.threads, pl.pack_vec, pl.grid_activate, pl.grid_adam, pl.grid_pack_x, pl.grid_pack_y) == (256, 4, 4, 4, 3, 2)
    offs = [pl.means, pl.opacities, pl.colors, pl.scales, pl.rotations, pl.inv_norm, pl.workspace_bytes]
    assert all(o % 256 == 0 for o in offs) and offs == sorted(offs) and pl.workspace_bytes >= 14 * 1000 * 4
    assert _lib.lib().ga_fit_plan(0, 2, 40, 56, ctypes.byref(pl)) == -2 and _lib.lib().ga_fit_plan(10, 2, 33, 35, ctypes.byref(pl)) == 0
    assert pl.pack_vec == 1


# ---- the fitter against the loop a user could write before it existed ----------------------------------------------------------------
LAMBDAS = dict(l2=0.0, l1=0.8, ssim=0.2, lambda_normal=0.05, lambda_dist=10.0, lambda_alpha=0.1)
SIZE = 64


def _scene(dev, n=1000, views=2, seed=3, size=SIZE, enlarge=6.0):
    """targets: renders of a surfel set g*; start: g* with xyz and rgb perturbed"""
    from gaussiananything_amd import synthetic
    from gaussiananything_amd.gs_surfel import GaussianRenderer2DGS
    cams = synthetic.eval_cameras(8)
    pick = list(range(views))
    g = synthetic.random_surfels(n, seed=seed)
    g[..., 4:6] *= enlarge                                       # larger discs: a thousand surfels cover the views
    cv, cvp, cp = (cams[k][pick].to(dev) for k in ("cam_view", "cam_view_proj", "cam_pos"))
    with torch.no_grad():
        pred = GaussianRenderer2DGS(size, 3, {}).render(g.to(dev), cv[None], cvp[None], cp[None], cams["tanfov"])
    gen = torch.Generator().manual_seed(seed + 1)
    start = g.clone()
    start[..., 0:3] += 0.01 * torch.randn(n, 3, generator=gen)
    start[..., 10:13] = (start[..., 10:13] + 0.2 * torch.randn(n, 3, generator=gen)).clamp(0.02, 0.98)
    return {"cv": cv, "cvp": cvp, "cp": cp, "tanfov": cams["tanfov"], "targets": pred["image"][0].contiguous(),
            "mask": (pred["alpha"][0] > 0.5).float().contiguous(), "start": start.to(dev), "size": size}


def _fitter(sc, gaussians=None, **kw):
    from gaussiananything_amd import fitting
    args = dict(LAMBDAS, mask=sc["mask"], max_steps=64, lr=LR)
    args.update(kw)
    return fitting.SurfelFitter(sc["start"] if gaussians is None else gaussians, sc["cv"], sc["cvp"], sc["tanfov"], sc["targets"], **args)


def _autograd_loss(sc, raw):
    """the parent-style iteration on raw [N,13] (requires grad): activation in torch, render with grad, the two losses"""
    from gaussiananything_amd import losses
    from gaussiananything_amd.gs_surfel import GaussianRenderer2DGS
    act = ref.torch_activate(raw)
    pred = GaussianRenderer2DGS(sc["size"], 3, {}).render(act[None], sc["cv"][None], sc["cvp"][None], sc["cp"][None], sc["tanfov"])
    lp, _ = losses.photometric_loss(pred["image"][0], sc["targets"], LAMBDAS["l2"], LAMBDAS["l1"], LAMBDAS["ssim"])
    lg, _ = losses.geometric_loss(pred, sc["cv"][None], sc["tanfov"], LAMBDAS["lambda_normal"], LAMBDAS["lambda_dist"],
                                  LAMBDAS["lambda_alpha"], mask=sc["mask"][None])
    return lp + lg


def _autograd_grad(sc, raw0):
    raw = raw0.clone().requires_grad_(True)
    loss = _autograd_loss(sc, raw)
    loss.backward()
    return raw.grad.detach(), float(loss.detach())


def _autograd_fit(sc, raw0, steps, max_steps=64):
    """the parent-style loop: five leaves (one per column group, so that torch.optim.Adam has its per-group learning rates), the
    decaying rates set per step -> the loss at the start of every iteration"""
    leaves = {k: raw0[:, s].clone().requires_grad_(True) for k, s in ref.SLICES.items()}
    opt = torch.optim.Adam([{"params": [leaves[k]], "lr": 1.0} for k in ref.SLICES], betas=BETAS, eps=EPS)
    out = []
    for t in range(steps):
        for group, k in zip(opt.param_groups, ref.SLICES):
            group["lr"] = ref.lr_at(LR[k], t, max_steps)
        opt.zero_grad(set_to_none=True)
        loss = _autograd_loss(sc, torch.cat([leaves[k] for k in ref.SLICES], dim=1))
        loss.backward()
        opt.step()
        out.append(float(loss.detach()))
    return out


def _ulp_twin(raw):
    return torch.nextafter(raw, torch.full_like(raw, float("inf")))


def _group_rel(a, b):
    return {k: ref.rel_l2(a[:, s].double().cpu().numpy(), b[:, s].double().cpu().numpy()) for k, s in ref.SLICES.items()}


def _record(lines):
    for line in lines:
        print("fit parity:", line)


@pytest.fixture(scope="module")
def scene(gpu_device):
    return _scene(gpu_device)


@pytest.fixture(scope="module")
def yardstick(gpu_device, scene):
    """one iteration of the fitter and the two parent runs on the same raw input: computed once, shared"""
    f = _fitter(scene)
    raw0 = f.raw.clone()
    f.step(1)
    g_ref, loss_ref = _autograd_grad(scene, raw0)
    g_twin, _ = _autograd_grad(scene, _ulp_twin(raw0))
    return {"fitter": f, "raw0": raw0, "g_fit": f.raw_grad.clone(), "g_ref": g_ref, "loss_ref": loss_ref,
            "spread": _group_rel(g_twin, g_ref)}


def test_one_iteration_against_autograd(yardstick):
    """fitter.raw_grad against the raw-space gradient of the parent-style autograd iteration on the same raw input, per group relative
    L2, held to 4 x the spread between that iteration and its twin on raw moved by one ulp"""
    got = _group_rel(yardstick["g_fit"], yardstick["g_ref"])
    _record([f"one iteration, {k}: fitter vs autograd {got[k]:.3e}, autograd vs its ulp twin {yardstick['spread'][k]:.3e}" for k in got])
    for k in got:
        assert yardstick["spread"][k] > 0, k
        assert got[k] <= 4 * yardstick["spread"][k], (k, got[k], yardstick["spread"][k])
    h = yardstick["fitter"].loss_history()
    assert len(h["loss"]) == 1
    # the history row is the same loss (its means are the same kernels' output; the sum is formed in double here, in fp32 there)
    assert abs(float(h["loss"][0]) - yardstick["loss_ref"]) <= 1e-5 * abs(yardstick["loss_ref"])
    assert abs(sum(float(h[k][0]) for k in h if k != "loss") - float(h["loss"][0])) <= 1e-6 * abs(float(h["loss"][0]))


def test_thirty_iterations(scene, yardstick):
    """the loss falls, for the fitter and for the autograd loop, and the fitter's final loss is within 4 x the spread of the final
    losses of the autograd loop and its ulp twin"""
    steps = 30
    f = _fitter(scene)
    f.step(steps)
    h = f.loss_history()["loss"]
    a = _autograd_fit(scene, yardstick["raw0"], steps)
    b = _autograd_fit(scene, _ulp_twin(yardstick["raw0"]), steps)
    spread = abs(a[-1] - b[-1])
    _record([f"thirty iterations: loss {a[0]:.6e} -> autograd {a[-1]:.6e}, twin {b[-1]:.6e}, fitter {float(h[-1]):.6e}; "
             f"|fitter - autograd| {abs(float(h[-1]) - a[-1]):.3e}, |autograd - twin| {spread:.3e}"])
    assert len(h) == steps and h[-1] < h[0] and a[-1] < a[0]
    assert abs(float(h[-1]) - a[-1]) <= 4 * spread, (float(h[-1]), a[-1], b[-1])


def test_set_views_without_a_new_capture(gpu_device, scene, yardstick):
    """3 steps, then other cameras and targets, then 3 more: equal, within the yardstick of the one-iteration test, to a fresh fitter
    constructed on the swapped views and continued from the intermediate state"""
    other = _scene(gpu_device, seed=3)
    swapped = dict(scene, cv=scene["cv"].flip(0).contiguous(), cvp=scene["cvp"].flip(0).contiguous(),
                   targets=(other["targets"].flip(0) * 0.9).contiguous(), mask=scene["mask"].flip(0).contiguous())
    a = _fitter(scene)
    a.step(3)
    state = a.state_dict()
    graph = a._graph
    a.set_views(swapped["cv"], swapped["cvp"], swapped["targets"], mask=swapped["mask"])
    a.step(3)
    assert a._graph is graph                                   # no new capture
    b = _fitter(swapped).load_state_dict(state)
    b.step(3)
    assert a.steps == b.steps == 6
    for what, x, y in (("raw_grad", a.raw_grad, b.raw_grad), ("raw", a.raw, b.raw)):
        got = _group_rel(x, y)
        _record([f"set_views, {what} {k}: {got[k]:.3e} (bar 4 x {yardstick['spread'][k]:.3e})" for k in got])
        for k in got:
            assert got[k] <= 4 * yardstick["spread"][k], (what, k, got[k])
    assert not torch.equal(a.raw, state["raw"])
    ha, hb = a.loss_history()["loss"], b.loss_history()["loss"]
    assert np.allclose(ha, hb, rtol=1e-4) and abs(ha[3] - ha[2]) > 1e-3 * abs(ha[2])      # the swap shows in the loss


# ---- 12: workspace growth --------------------------------------------------------------------------------------------------------------
def test_a_capacity_far_too_small_is_grown_by_the_warm_up(scene, yardstick):
    small = _fitter(scene, capacity=64)
    assert small.capacity > 64
    small.step(1)
    got = _group_rel(small.raw_grad, yardstick["g_fit"])
    for k in got:
        assert got[k] <= 4 * yardstick["spread"][k], (k, got[k])
    got = _group_rel(small.raw, yardstick["fitter"].raw)
    for k in got:
        assert got[k] <= 4 * yardstick["spread"][k], (k, got[k])
    assert np.allclose(small.loss_history()["loss"], yardstick["fitter"].loss_history()["loss"], rtol=1e-6)


def test_overflow_in_the_middle_of_a_run(gpu_device):
    """200 tiny surfels, one view, targets of large discs, a large scale learning rate: the tile lists outgrow a capacity that was
    just sufficient at the start.  check_every = 4.  The result is that of an ample workspace, within 4 x the spread between the ample
    run and its twin on raw moved by one ulp, and the history has one row per step, none repeated, none missing."""
    from gaussiananything_amd import synthetic
    from gaussiananything_amd.gs_surfel import GaussianRenderer2DGS
    dev, steps = gpu_device, 16
    cams = synthetic.eval_cameras(1)
    cv, cvp, cp = (cams[k].to(dev) for k in ("cam_view", "cam_view_proj", "cam_pos"))
    big = synthetic.random_surfels(200, seed=9)
    big[..., 4:6] *= 12
    with torch.no_grad():
        targets = GaussianRenderer2DGS(64, 3, {}).render(big.to(dev), cv[None], cvp[None], cp[None], cams["tanfov"])["image"][0].contiguous()
    tiny = big.clone()
    tiny[..., 4:6] = big[..., 4:6] / 12
    lr = dict(LR, scale=0.25)
    kw = dict(l1=0.8, ssim=0.2, lambda_normal=0.0, lr=lr, max_steps=32, check_every=4)

    def make(capacity=None):
        from gaussiananything_amd import fitting
        return fitting.SurfelFitter(tiny.to(dev), cv, cvp, cams["tanfov"], targets, capacity=capacity, **kw)

    ample = make()
    raw0 = ample.raw.clone()
    need0 = ample.entries()                                   # the entries of the warm-up forward: what the start needs
    ample.step(steps)
    need1 = ample.entries()
    assert need1 > 2 * need0, (need0, need1)                # the lists did outgrow the start
    twin = make()
    twin.load_state_dict({"raw": _ulp_twin(raw0), "m": torch.zeros_like(raw0), "v": torch.zeros_like(raw0), "steps": 0,
                          "history": torch.zeros(0, 8, device=dev)})
    twin.step(steps)
    tight = make(capacity=need0 + 8)
    assert tight.capacity == need0 + 8                       # the warm-up did not have to grow it
    tight.step(steps)
    assert tight.capacity >= need1 > need0 + 8 and tight.steps == steps
    spread, got = _group_rel(twin.raw, ample.raw), _group_rel(tight.raw, ample.raw)
    _record([f"overflow mid-run, raw {k}: tight vs ample {got[k]:.3e}, ample vs its ulp twin {spread[k]:.3e}" for k in got])
    for k in got:
        assert got[k] <= 4 * spread[k], (k, got[k], spread[k])
    h, ha = tight.loss_history()["loss"], ample.loss_history()["loss"]
    assert len(h) == steps and (h > 0).all() and len(set(h.tolist())) == steps
    assert np.allclose(h, ha, rtol=1e-2), (h, ha)      # a repeated or missing row would shift the sequence


# ---- 13: validation --------------------------------------------------------------------------------------------------------------------
def test_validation(gpu_device, scene):
    from gaussiananything_amd import fitting
    sc = scene
    ok = (sc["start"], sc["cv"], sc["cvp"], sc["tanfov"], sc["targets"])
    with pytest.raises(ValueError, match="no CPU path"):
        fitting.SurfelFitter(sc["start"].cpu(), *ok[1:])
    with pytest.raises(ValueError, match="no CPU path"):
        fitting.SurfelFitter(ok[0], sc["cv"].cpu(), *ok[2:])
    with pytest.raises(ValueError, match="no CPU path"):
        fitting.SurfelFitter(*ok[:4], sc["targets"].cpu())
    with pytest.raises(ValueError, match=r"\[N,13\]"):
        fitting.SurfelFitter(sc["start"][..., :12], *ok[1:])
    with pytest.raises(ValueError, match="cam_view must be"):
        fitting.SurfelFitter(ok[0], sc["cv"][:1], *ok[2:])
    with pytest.raises(ValueError, match="targets must be"):
        fitting.SurfelFitter(*ok[:4], sc["targets"][:, :2])
    with pytest.raises(ValueError, match="mask must be"):
        fitting.SurfelFitter(*ok, mask=sc["mask"][:, :, :32])
    with pytest.raises(ValueError, match="requires grad"):
        fitting.SurfelFitter(*ok[:4], sc["targets"].clone().requires_grad_(True))
    bad = sc["start"].clone()
    bad[0, 5, 6:10] = 0
    with pytest.raises(ValueError, match="zero quaternion"):
        fitting.SurfelFitter(bad, *ok[1:])
    f = fitting.SurfelFitter(*ok, max_steps=3)
    f.step(2)
    with pytest.raises(ValueError, match="max_steps"):
        f.step(2)
    assert f.steps == 2
    f.step(1)
    with pytest.raises(ValueError, match="max_steps"):
        f.step(1)
    with pytest.raises(ValueError, match="targets must be"):
        f.set_views(sc["cv"], sc["cvp"], sc["targets"][:, :, :32])
    with pytest.raises(ValueError, match="without a mask"):
        f.set_views(sc["cv"], sc["cvp"], sc["targets"], mask=sc["mask"])
    g = f.gaussians()
    assert tuple(g.shape) == (1, sc["start"].shape[1], 13) and bool(torch.isfinite(g).all())
    assert float((g[0, :, 6:10].norm(dim=1) - 1).abs().max()) < 1e-6
