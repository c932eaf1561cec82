"""GPU tests of the geometry losses (include/ga_loss.h: ga_geo_loss_*, csrc/geo_loss.hip) and of their Python layer in
gaussiananything_amd/losses.py.

The kernels are compared with the float64 restatement of the reference's route (tests/_geo_ref.py) within bars that come, per case,
from the error of the fp32 restatement of that route on the same input: normals per pixel E_map + 1e-6, per-view means 1e-6 relative,
gradients (relative L2 per tensor) E_grad + 2e-6.  Every raw call poisons its outputs first and checks guard words behind each buffer
and the workspace."""
import ctypes

import pytest
import torch

from tests import _geo_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 64            # fp32 words behind every buffer
GUARD_VALUE = 12345.0
POISON = float("nan")
GRADS = ("grad_rend_normal", "grad_depth", "grad_dist", "grad_alpha")
WORST = {}            # worst ratio to the bar per quantity, over everything this module ran


@pytest.fixture(scope="module", autouse=True)
def _bounds_file():
    """after the module: profiles/geo_loss_bounds.txt gets the worst ratio of a measured error to its bar, per quantity"""
    yield
    if WORST:
        lines = [f"{k:18s} worst measured / bar: {v:.3f}" for k, v in sorted(WORST.items())]
        ref.write_section("GPU (tests/test_geo_loss_gpu.py): kernels and Python layer against the float64 restatement", lines)
        print("\n".join(lines))


def _guarded(n_words, device, fill=None):
    t = torch.full((n_words + GUARD,), GUARD_VALUE, dtype=torch.float32, device=device)
    if fill is None:
        t[:n_words] = POISON
    else:
        t[:n_words] = fill.reshape(-1).float().to(device)
    return t


def _plan(V=1, H=64, W=64):
    from gaussiananything_amd import _lib
    pl = _lib.GaGeoLossPlan()
    assert _lib.lib().ga_geo_loss_plan(V, H, W, ctypes.byref(pl)) == 0
    return pl


def _tile():
    from gaussiananything_amd import losses
    pl = losses.geo_plan(1, 64, 64)
    assert pl["tile_w"] == pl["tile_h"] == _plan().tile_w and pl["grid_x"] == 4 and pl["num_partials"] == 12
    return pl["tile_w"]


class Raw:
    """the C-ABI on guarded buffers.  mode: 'depth' (normals from the depth map), 'target' or 'normals' (GA_GEO_LOSS_NORMALS);
    ``absent``: names of nullable pointers passed as NULL"""

    def __init__(self, inp, device, mode="depth", use_mask=True, absent=()):
        from gaussiananything_amd import _lib
        self._lib, self.L, self.device, self.mode = _lib, _lib.lib(), device, mode
        self.shape = V, H, W = tuple(inp["depth"].shape[0:1]) + tuple(inp["depth"].shape[2:])
        self.hw = H * W
        self.flags = {"depth": 0, "target": _lib.GA_GEO_LOSS_TARGET, "normals": _lib.GA_GEO_LOSS_NORMALS}[mode]
        self.sizes = {"view": V * 16, "rend_normal": 3 * V * self.hw, "depth": V * self.hw, "alpha": V * self.hw, "dist": V * self.hw,
                      "target_normal": 3 * V * self.hw, "mask": V * self.hw, "out": V * 3, "surf_normal_out": 3 * V * self.hw,
                      "grad_out": (3 * V * self.hw if mode == "normals" else V * 3), "grad_rend_normal": 3 * V * self.hw,
                      "grad_depth": V * self.hw, "grad_dist": V * self.hw, "grad_alpha": V * self.hw}
        self.nbytes = int(self.L.ga_geo_loss_workspace_bytes(V, H, W))
        assert self.nbytes > 0 and self.nbytes % 256 == 0 and self.nbytes >= 12 * _plan(V, H, W).grid_x
        self.sizes["workspace"] = self.nbytes // 4
        skip = set(absent)
        if mode != "target":
            skip.add("target_normal")
        if not use_mask or mode == "normals":
            skip.add("mask")
        if mode == "normals":
            skip |= {"rend_normal", "dist", "out", "grad_rend_normal", "grad_dist", "grad_alpha"}
        self.buf = {}
        for name, n in self.sizes.items():
            if name in skip:
                continue
            src = inp["cam_view"] if name == "view" else inp.get(name)
            self.buf[name] = _guarded(n, device, src)
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    def load(self, inp):
        """new contents into the same buffers"""
        for name in ("view", "rend_normal", "depth", "alpha", "dist", "target_normal", "mask"):
            if name in self.buf:
                src = inp["cam_view"] if name == "view" else inp[name]
                self.buf[name][:self.sizes[name]] = src.reshape(-1).float().to(self.device)

    def args(self):
        V, H, W = self.shape
        a = self._lib.GaGeoLossArgs()
        a.num_views, a.height, a.width, a.flags, a.tanfov = V, H, W, self.flags, ref.TANFOV
        for name, t in self.buf.items():
            if name != "workspace":
                setattr(a, name, t.data_ptr())
        a.workspace, a.workspace_bytes = self.buf["workspace"].data_ptr(), self.nbytes
        return a

    def check_guards(self):
        for name, t in self.buf.items():
            assert bool((t[self.sizes[name]:] == GUARD_VALUE).all()), name

    def poison(self, names):
        for name in names:
            if name in self.buf:
                self.buf[name][:self.sizes[name]] = POISON

    def get(self, name, shape):
        if name not in self.buf:
            return None
        t = self.buf[name][:self.sizes[name]].reshape(shape).clone()
        assert bool(torch.isfinite(t).all()), name           # every slot written
        return t

    def forward(self):
        """-> (means [V,3] or None, s [V,3,H,W] or None), fresh tensors"""
        V, H, W = self.shape
        self.poison(("out", "surf_normal_out"))
        with torch.cuda.device(self.device):
            self._lib.check(self.L.ga_geo_loss_forward(ctypes.byref(self.args()), self.stream), "ga_geo_loss_forward")
            torch.cuda.synchronize()
        self.check_guards()
        return self.get("out", (V, 3)), self.get("surf_normal_out", (V, 3, H, W))

    def backward(self, grad_out):
        """-> dict of the gradient tensors that are present"""
        V, H, W = self.shape
        self.buf["grad_out"][:self.sizes["grad_out"]] = grad_out.reshape(-1).float().to(self.device)
        self.poison(GRADS)
        with torch.cuda.device(self.device):
            self._lib.check(self.L.ga_geo_loss_backward(ctypes.byref(self.args()), self.stream), "ga_geo_loss_backward")
            torch.cuda.synchronize()
        self.check_guards()
        return {k: self.get(k, (V, 3 if k == "grad_rend_normal" else 1, H, W)) for k in GRADS if k in self.buf}


def _same_bits(a, b):
    return bool((a.view(torch.int32) == b.view(torch.int32)).all())


def _hold(got, bar, what):
    for k in got:
        WORST[k] = max(WORST.get(k, 0.0), got[k] / bar[k])
        assert got[k] <= bar[k], (what, k, got[k], bar[k])


def _case_id(case):
    return f"{case[0]}-{'x'.join(map(str, case[1]))}"


def _cases():
    return ref.cases(_plan().tile_w)      # the tile is a build constant reported by the plan (host only)


MODES = (("depth", True), ("depth", False), ("target", True), ("target", False))


@pytest.mark.parametrize("case", _cases(), ids=_case_id)
def test_kernels_against_float64_within_the_bars_of_the_case(gpu_device, case):
    family, shape, seed = case
    V, H, W = shape
    inp = ref.make_inputs(family, shape, seed)
    w = ref.grad_weights(V)
    for mode, use_mask in MODES:
        raw = Raw(inp, gpu_device, mode, use_mask)
        means, s = raw.forward()
        means2, s2 = raw.forward()
        assert _same_bits(means, means2) and _same_bits(s, s2)                 # no atomics: the same bits every time
        grads = raw.backward(w)
        again = raw.backward(w)
        assert all(_same_bits(grads[k], again[k]) for k in GRADS)              # the backward twice on one forward
        r = ref.reference_errors(inp, w, target=(mode == "target"), use_mask=use_mask)
        got = ref.measured(r, dict(grads, s=s, means=means))
        print(mode, use_mask, {k: (got[k], ref.bars(r)[k]) for k in got})
        _hold(got, ref.bars(r), (mode, use_mask))
        if mode == "depth":
            assert bool((s[:, :, 0] == 0).all() and (s[:, :, -1] == 0).all() and (s[:, :, :, 0] == 0).all() and (s[:, :, :, -1] == 0).all())
            if H < 3 or W < 3:                                                  # no interior: no normals, no depth gradient
                assert bool((s == 0).all()) and bool((grads["grad_depth"] == 0).all())
            elif family != "holes":
                assert float(s.abs().max()) > 0 and float(grads["grad_depth"].abs().max()) > 0
        else:
            assert bool((grads["grad_depth"] == 0).all())
        if not use_mask:                                                        # the alpha term is off
            assert bool((means[:, 2] == 0).all()) and bool((grads["grad_alpha"] == 0).all())
        if V == 2:                                                              # a zero weight gives an exactly zero gradient
            assert bool((grads["grad_rend_normal"][1] == 0).all()) and bool((grads["grad_depth"][1] == 0).all())


def test_absent_outputs_change_nothing_else(gpu_device):
    """each nullable output absent in turn: the others keep their bits; NULL required pointers are refused on the host"""
    from gaussiananything_amd import _lib
    inp = ref.make_inputs("noisy", (2, 37, 70), 7)
    w = ref.grad_weights(2)
    full = Raw(inp, gpu_device)
    means, _ = full.forward()
    grads = full.backward(w)
    for name in ("surf_normal_out",) + GRADS:
        raw = Raw(inp, gpu_device, absent=(name,))
        m, s = raw.forward()
        assert _same_bits(m, means) and (s is None) == (name == "surf_normal_out")
        g = raw.backward(w)
        assert set(g) == set(GRADS) - {name}
        assert all(_same_bits(g[k], grads[k]) for k in g)
    for name, fn in (("depth", "forward"), ("out", "forward"), ("alpha", "backward"), ("grad_out", "backward")):
        a = full.args()
        setattr(a, name, None)
        assert getattr(full.L, "ga_geo_loss_" + fn)(ctypes.byref(a), full.stream) == -1          # GA_ERR_NULL_ARG
    a = full.args()
    a.flags = 3
    assert full.L.ga_geo_loss_forward(ctypes.byref(a), full.stream) == -5                         # GA_ERR_BAD_FLAGS
    a = full.args()
    a.workspace_bytes = full.nbytes - 1
    assert full.L.ga_geo_loss_forward(ctypes.byref(a), full.stream) == -3                         # GA_ERR_WORKSPACE
    assert _lib.lib().ga_geo_loss_workspace_bytes(0, 4, 4) == 0
    torch.cuda.synchronize()
    full.check_guards()


def test_depth_gradient_crosses_tile_edges(gpu_device):
    """a one-hot grad_out per term and a one-hot rend_normal at tile corners: the depth gradient lands on the four neighbours of that
    pixel, three of which another workgroup owns"""
    T = _tile()
    H, W = 2 * T + 1, T + 2
    inp = ref.make_inputs("plane", (1, H, W), 9)
    for (y, x) in ((T, T), (T - 1, T - 1), (2 * T - 1, T), (T, 1), (2 * T - 1, T - 1)):
        one = dict(inp, rend_normal=torch.zeros(1, 3, H, W))
        one["rend_normal"][0, :, y, x] = torch.tensor([0.3, -0.8, 0.5])
        raw = Raw(one, gpu_device, "depth", True)
        raw.forward()
        for term in range(3):
            w = torch.zeros(1, 3)
            w[0, term] = 1.7
            g = raw.backward(w)
            r = ref.reference_errors(one, w, use_mask=True)
            _hold(ref.measured(r, g), ref.bars(r), ((y, x), term))
            nz = g["grad_depth"][0, 0].nonzero().tolist()
            if term == 0:
                assert sorted(nz) == sorted([[y - 1, x], [y + 1, x], [y, x - 1], [y, x + 1]]), nz
                assert bool((g["grad_dist"] == 0).all()) and bool((g["grad_alpha"] == 0).all())
            else:
                assert nz == [] and bool((g["grad_rend_normal"] == 0).all())
                other = g["grad_dist" if term == 2 else "grad_alpha"]
                assert bool((other == 0).all())
            if term == 1:
                assert bool((g["grad_dist"] == g["grad_dist"][0, 0, 0, 0]).all()) and float(g["grad_dist"][0, 0, 0, 0]) > 0


def _island_inputs():
    d = ref.island_depth().float()[None]                       # [1,1,12,12]
    inp = ref.make_inputs("noisy", (1, 12, 12), 4)
    inp["depth"] = d
    inp["alpha"] = 0.5 + 0.5 * inp["alpha"]                    # alpha > 0 everywhere, the island and the holes around it included
    return inp


def test_zero_gradient_departure_on_an_isolated_pixel(gpu_device):
    inp = _island_inputs()
    assert float(inp["alpha"].min()) > 0
    w = torch.tensor([[1.0, 0.0, 0.0]])
    raw = Raw(inp, gpu_device, "depth", False)
    means, s = raw.forward()
    g = raw.backward(w)                                        # finite: checked by Raw.get
    assert bool((s[0, :, 4, 5] == 0).all() and (s[0, :, 5, 4] == 0).all())       # the vanishing cross products
    r = ref.reference_errors(inp, w)
    _hold(ref.measured(r, dict(g, s=s, means=means)), ref.bars(r), "island")
    assert float(g["grad_depth"].abs().max()) < 1.0            # torch's autograd gives 1e9 and more here (tests/test_geo_loss_cpu.py)


def test_normals_only_mode(gpu_device):
    """GA_GEO_LOSS_NORMALS: the map alone, with and without alpha, and the gradient of an arbitrary map gradient to depth"""
    T = _tile()
    for family, shape, seed in (("sphere", (2, T + 1, T + 2), 21), ("holes", (1, 37, 70), 22), ("plane", (1, 2, 5), 23)):
        inp = ref.make_inputs(family, shape, seed)
        V, H, W = shape
        gmap = torch.randn(V, 3, H, W, generator=torch.Generator().manual_seed(seed))
        for with_alpha in (True, False):
            raw = Raw(inp, gpu_device, "normals", absent=() if with_alpha else ("alpha",))
            _, s = raw.forward()
            g = raw.backward(gmap)["grad_depth"]
            assert _same_bits(g, raw.backward(gmap)["grad_depth"])
            err = {}
            want = {}
            for dtype in (torch.float64, torch.float32):
                d = inp["depth"].detach().to(dtype).clone().requires_grad_(True)
                n = ref.normal_maps(dict(inp, depth=d), "reference", dtype) * (inp["alpha"].to(dtype) if with_alpha else 1)
                (n * gmap.to(dtype)).sum().backward()
                want[dtype] = (n.detach(), d.grad)
            e_map = float((want[torch.float32][0].double() - want[torch.float64][0]).abs().max())
            e_grad = ref.rel_l2(want[torch.float32][1], want[torch.float64][1])
            err["map"] = float((s.double().cpu() - want[torch.float64][0]).abs().max())
            err["grad_depth"] = ref.rel_l2(g, want[torch.float64][1])
            _hold(err, {"map": e_map + 1e-6, "grad_depth": e_grad + 2e-6}, (family, with_alpha))


def test_captured_graph_replays_with_new_maps_view_and_weights(gpu_device):
    """forward + backward captured once as a single chain; replays read the maps, the view matrix and grad_out from the same buffers,
    so new contents give the eager result bit for bit"""
    from gaussiananything_amd import _lib
    shape = (2, 37, 70)
    inp = ref.make_inputs("sphere", shape, 31)
    raw = Raw(inp, gpu_device, "depth", True)
    raw.buf["grad_out"][:6] = torch.tensor([1.0, 0.5, 0.25, 0.3, 0.0, 2.0], device=gpu_device)
    L = _lib.lib()
    side = torch.cuda.Stream(device=gpu_device)

    def enqueue(stream):
        s = ctypes.c_void_p(stream.cuda_stream)
        _lib.check(L.ga_geo_loss_forward(ctypes.byref(raw.args()), s), "ga_geo_loss_forward")
        _lib.check(L.ga_geo_loss_backward(ctypes.byref(raw.args()), s), "ga_geo_loss_backward")

    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        enqueue(side)          # warm-up on the capture stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            enqueue(side)
    torch.cuda.synchronize()
    inp2 = ref.make_inputs("holes", shape, 32)
    w2 = torch.tensor([[0.0, 0.0, 0.0], [0.8, 1.5, 0.1]])
    raw.load(inp2)
    raw.buf["grad_out"][:6] = w2.reshape(-1).to(gpu_device)
    raw.poison(("out", "surf_normal_out") + GRADS)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    raw.check_guards()
    V, H, W = shape
    got = {k: raw.get(k, (V, 3 if k == "grad_rend_normal" else 1, H, W)) for k in GRADS}
    got_means, got_s = raw.get("out", (V, 3)), raw.get("surf_normal_out", (V, 3, H, W))
    eager = Raw(inp2, gpu_device, "depth", True)
    want_means, want_s = eager.forward()
    want = eager.backward(w2)
    assert _same_bits(got_means, want_means) and _same_bits(got_s, want_s)
    assert all(_same_bits(got[k], want[k]) for k in GRADS)
    assert bool((got["grad_depth"][0] == 0).all()) and float(got["grad_depth"][1].abs().max()) > 0


def _on(inp, device):
    return {k: v.to(device) for k, v in inp.items()}


def _batched(inp, B, V):
    return {k: v.unflatten(0, (B, V)) for k, v in inp.items()}


@pytest.mark.parametrize("target", [False, True], ids=["from-depth", "target"])
def test_geometric_loss_matches_the_terms_composed_in_torch(gpu_device, target):
    from gaussiananything_amd import losses
    B, V, H, W = 2, 2, 37, 70
    inp = _on(ref.make_inputs("sphere", (B * V, H, W), 41), gpu_device)
    lam = dict(lambda_normal=0.7, lambda_dist=100.0, lambda_alpha=0.3)
    w = torch.tensor([[lam["lambda_normal"], lam["lambda_dist"], lam["lambda_alpha"]]] * (B * V)) / (B * V)
    r = ref.reference_errors(inp, w, target=target, use_mask=True)              # float64 and fp32, composed in torch on the device
    b = _batched(inp, B, V)
    leaves = {k: b[k].clone().requires_grad_(True) for k in ("rend_normal", "depth", "dist", "alpha")}
    kw = dict(normal=b["target_normal"], mask=b["mask"]) if target else dict(mask=b["mask"])
    loss, d = losses.geometric_loss(leaves, b["cam_view"], ref.TANFOV, **lam, **kw)
    assert set(d) == {"loss", "loss_normal", "loss_dist", "loss_alpha"} and d["loss"] is loss
    loss.backward()
    want = (r["means"] * w.to(gpu_device).double()).sum(0)
    for key, value in zip(("loss_normal", "loss_dist", "loss_alpha"), want):
        assert abs(float(d[key].detach()) - float(value)) <= 1e-6 * abs(float(value)) + 1e-9, key
    assert abs(float(loss.detach()) - float(want.sum())) <= 1e-6 * float(want.abs().sum())
    got = {"grad_" + k: t.grad.flatten(0, 1) for k, t in leaves.items()}
    assert all(got[k].shape == r[k].shape for k in got)
    _hold(ref.measured(r, got), ref.bars(r), ("geometric_loss", target))
    # lambdas of 0 take their terms out of the loss and hand no gradient on
    leaves0 = {k: b[k].clone().requires_grad_(True) for k in leaves}
    loss0, d0 = losses.geometric_loss(leaves0, b["cam_view"], ref.TANFOV, lambda_dist=1.0, **kw)
    loss0.backward()
    assert float(d0["loss_normal"].detach()) == 0 and bool((leaves0["depth"].grad == 0).all()) and float(leaves0["dist"].grad.abs().max()) > 0
    # strided no-grad views (what render hands out under no_grad) and other dtypes are taken as .float().contiguous()
    allmap = torch.randn(B, V, 7, H, W, device=gpu_device)
    allmap[:, :, 1:2] = b["alpha"]
    allmap[:, :, 6:7] = b["dist"]
    strided = dict(b, alpha=allmap[:, :, 1:2], dist=allmap[:, :, 6:7], depth=b["depth"].double())
    assert not strided["alpha"].is_contiguous()
    with torch.no_grad():
        loss1, _ = losses.geometric_loss(strided, b["cam_view"], ref.TANFOV, **lam, **kw)
    assert abs(float(loss1) - float(loss.detach())) <= 1e-6 * abs(float(loss.detach()))


def test_depth_to_normal_and_surface_normal(gpu_device):
    """depth_to_normal takes the reference's matrix convention and reproduces the reference's own normals (the golden);
    surface_normal takes render's and multiplies by alpha; both hand a gradient to depth"""
    from gaussiananything_amd import losses
    golden = torch.load(ref.GOLDEN)
    for c in golden["cases"]:
        H, W = c["shape"]
        inp = ref.make_inputs(c["family"], (1, H, W), c["seed"])
        n64 = ref.normals_reference_route(c["w2c"].double(), c["tanfov"], inp["depth"][0].double(), torch.float64)
        e_map = float((c["normal"].double() - n64).abs().max())                  # the reference's own fp32 error on this case
        got = losses.depth_to_normal(c["w2c"][None].to(gpu_device), c["tanfov"], inp["depth"].to(gpu_device))
        assert got.shape == (1, 3, H, W) and got.dtype == torch.float32
        _hold({"map": float((got[0].permute(1, 2, 0).double().cpu() - n64).abs().max())}, {"map": e_map + 1e-6}, c["family"])
    inp = _on(ref.make_inputs("sphere", (4, 33, 31), 51), gpu_device)
    b = _batched(inp, 2, 2)
    depth = b["depth"].clone().requires_grad_(True)
    s = losses.surface_normal(depth, b["alpha"], b["cam_view"], ref.TANFOV)
    assert s.shape == (2, 2, 3, 33, 31)
    gmap = torch.randn(s.shape, device=gpu_device, generator=torch.Generator(device=gpu_device).manual_seed(1))
    (s * gmap).sum().backward()
    want = {}
    for dtype in (torch.float64, torch.float32):
        d = inp["depth"].detach().to(dtype).clone().requires_grad_(True)
        n = ref.normal_maps(dict(inp, depth=d), "reference", dtype) * inp["alpha"].to(dtype)
        (n * gmap.flatten(0, 1).to(dtype)).sum().backward()
        want[dtype] = (n.detach(), d.grad)
    e_map = float((want[torch.float32][0].double() - want[torch.float64][0]).abs().max())
    e_grad = ref.rel_l2(want[torch.float32][1], want[torch.float64][1])
    _hold({"map": float((s.detach().flatten(0, 1).double() - want[torch.float64][0]).abs().max()),
           "grad_depth": ref.rel_l2(depth.grad.flatten(0, 1), want[torch.float64][1])},
          {"map": e_map + 1e-6, "grad_depth": e_grad + 2e-6}, "surface_normal")


def test_validation_errors(gpu_device):
    from gaussiananything_amd import losses
    inp = ref.make_inputs("plane", (2, 8, 9), 61)
    dev = _on(inp, gpu_device)
    args = lambda d: (d["rend_normal"], d["depth"], d["alpha"], d["dist"], d["cam_view"], ref.TANFOV)   # noqa: E731
    assert losses.geo_means(*args(dev)).shape == (2, 3)
    with pytest.raises(ValueError, match="GPU"):
        losses.geo_means(*args(inp))                                            # CPU tensors: no fallback
    with pytest.raises(ValueError, match="GPU"):
        losses.geo_means(*args(dict(dev, alpha=inp["alpha"])))
    with pytest.raises(ValueError, match="must be"):
        losses.geo_means(*args(dict(dev, depth=dev["depth"][:, :, :-1])))
    with pytest.raises(ValueError, match="must be"):
        losses.geo_means(*args(dict(dev, rend_normal=dev["rend_normal"][:, :2])))
    with pytest.raises(ValueError, match="view"):
        losses.geo_means(*args(dict(dev, cam_view=dev["cam_view"][:1])))
    with pytest.raises(ValueError, match="requires grad"):
        losses.geo_means(*args(dev), normal=dev["target_normal"].clone().requires_grad_(True))
    with pytest.raises(ValueError, match="requires grad"):
        losses.geo_means(*args(dev), mask=dev["mask"].clone().requires_grad_(True))
    with pytest.raises(ValueError, match="tanfov"):
        losses.geo_means(*args(dev)[:5], 0.0)
    with pytest.raises(TypeError):
        losses.geo_means(*args(dict(dev, depth=inp["depth"].numpy())))
    with pytest.raises(TypeError):
        losses.geometric_loss({"depth": dev["depth"]}, dev["cam_view"][None], ref.TANFOV)
    with pytest.raises(ValueError):
        losses.depth_to_normal(dev["w2c"], ref.TANFOV, dev["depth"][0])
    with pytest.raises(ValueError, match="GPU"):
        losses.surface_normal(inp["depth"][None], inp["alpha"][None], inp["cam_view"][None], ref.TANFOV)


def _camera_inputs(pred, cam_view, tanfov):
    """the maps of a render [1,V,...] and its cam_view [1,V,4,4] as the dict the restatement takes"""
    out = {k: pred[k][0].detach().float() for k in ("rend_normal", "depth", "alpha", "dist")}
    out["cam_view"] = cam_view[0].float()
    out["w2c"] = cam_view[0].float().transpose(1, 2).contiguous()
    out["mask"] = (out["alpha"] > 0.5).float()
    out["target_normal"] = torch.zeros_like(out["rend_normal"])
    out["tanfov"] = tanfov
    return out


def test_behind_the_renderer(gpu_device):
    """300 surfels, 2 views, 32 x 32, rendered with grad: geometric_loss(...).backward() hands the rendered maps the gradients of the
    torch composition on the same maps (compared with retain_grad, so the rasterizer's own backward stays out of the comparison) and
    reaches the Gaussian tensor"""
    from gaussiananything_amd import losses, synthetic
    from gaussiananything_amd.gs_surfel import GaussianRenderer2DGS
    cams = synthetic.eval_cameras(2)
    g = synthetic.random_surfels(300, seed=5)
    g[..., 4:6] *= 6                                            # larger discs: a few hundred surfels still cover the views
    leaf = g.to(gpu_device).requires_grad_(True)
    cv, cvp, cp = (cams[k][None].to(gpu_device) for k in ("cam_view", "cam_view_proj", "cam_pos"))
    r = GaussianRenderer2DGS(32, 3, {})
    pred = r.render(leaf, cv, cvp, cp, cams["tanfov"])
    for k in ("rend_normal", "depth", "alpha", "dist"):
        pred[k].retain_grad()
    inp = _camera_inputs(pred, cv, cams["tanfov"])
    lam = dict(lambda_normal=0.05, lambda_dist=100.0, lambda_alpha=1.0)
    loss, d = losses.geometric_loss(pred, cv, cams["tanfov"], mask=inp["mask"][None], **lam)
    loss.backward()
    w = torch.tensor([[lam["lambda_normal"], lam["lambda_dist"], lam["lambda_alpha"]]] * 2) / 2
    res = ref.reference_errors(inp, w, use_mask=True)
    assert float(res["s"].abs().max()) > 0.5                    # the render has surface in it
    assert abs(float(loss.detach()) - float((res["means"] * w.to(gpu_device).double()).sum())) <= 1e-6 * abs(float(loss.detach()))
    got = {"grad_" + k: pred[k].grad[0] for k in ("rend_normal", "depth", "dist", "alpha")}
    _hold(ref.measured(res, got), ref.bars(res), "behind the renderer")
    assert bool(torch.isfinite(leaf.grad).all()) and float(leaf.grad.abs().max()) > 0


def test_sign_and_convention_on_one_surfel_facing_the_camera(gpu_device):
    """one opaque surfel facing the camera: wherever alpha > 0.9 the rasterizer's normal and surface_normal agree in sign.  At such a
    pixel the dot product is at least 0.81 times the cosine, which is about 1 for a planar splat; in camera space rows x columns gives
    (0, 1, 0) x (1, 0, 0) = (0, 0, -1), which faces the camera as the rasterizer's normals do.  A wrong transpose in surface_normal
    fails this."""
    from gaussiananything_amd import losses, synthetic
    from gaussiananything_amd.gs_surfel import GaussianRenderer2DGS
    cams = synthetic.eval_cameras(1)
    cv, cvp, cp = (cams[k][None].to(gpu_device) for k in ("cam_view", "cam_view_proj", "cam_pos"))
    to_cam = torch.nn.functional.normalize(cams["cam_pos"][0].float(), dim=0)
    z = torch.tensor([0.0, 0.0, 1.0])
    quat = torch.nn.functional.normalize(torch.cat([(1 + z @ to_cam)[None], torch.linalg.cross(z, to_cam)]), dim=0)   # wxyz: z -> to_cam
    g = torch.cat([torch.zeros(3), torch.ones(1), torch.full((2,), 0.15), quat, torch.tensor([0.2, 0.6, 0.9])])[None, None]
    with torch.no_grad():
        pred = GaussianRenderer2DGS(32, 3, {}).render(g.to(gpu_device), cv, cvp, cp, cams["tanfov"])
        s = losses.surface_normal(pred["depth"], pred["alpha"], cv, cams["tanfov"])
    dot = (pred["rend_normal"] * s).sum(2, keepdim=True)
    solid = pred["alpha"] > 0.9
    assert int(solid.sum()) >= 1
    assert not bool(solid[..., 0, :].any() or solid[..., -1, :].any() or solid[..., 0].any() or solid[..., -1].any())   # the disc is inside
    assert float(dot[solid].min()) > 0.5, float(dot[solid].min())
