"""GPU tests of the photometric loss (include/ga_loss.h, csrc/photo_loss.hip) and of gaussiananything_amd/losses.py.

The kernels are compared with the float64 restatement (tests/_ssim_ref.py) within bars that come, per case, from the error of the
fp32 restatement of the reference on that case's input: per-pixel S 2 E_map + 2e-6, mean 2 E_mean + 1e-6, gradient (relative L2)
2 E_grad + 2e-6, L1 and L2 sums 1e-6 relative.  Every raw call poisons its outputs first and checks guard words behind each buffer
and the workspace."""
import ctypes
import os

import pytest
import torch

from tests import _ssim_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 64            # fp32 words behind every buffer
GUARD_VALUE = 12345.0
POISON = float("nan")


def _guarded(n_words, device, fill=None):
    t = torch.full((n_words + GUARD,), GUARD_VALUE, dtype=torch.float32, device=device)
    if fill is None:
        t[:n_words] = POISON
    else:
        t[:n_words] = fill.reshape(-1).to(device)
    return t


def _intact(t, n_words):
    return bool((t[n_words:] == GUARD_VALUE).all())


def _tile():
    from gaussiananything_amd import losses
    pl = losses.plan(1, 1, 64, 64)
    assert pl["tile_w"] == pl["tile_h"]
    return pl["tile_w"]


class Raw:
    """one forward (SAVE, with the S map) through the C-ABI on guarded buffers; ``backward(grad_out)`` as often as wanted"""

    def __init__(self, img1, img2, device, save=True, want_map=True):
        from gaussiananything_amd import _lib
        self._lib, self.L, self.device = _lib, _lib.lib(), device
        self.shape = N, C, H, W = tuple(img1.shape)
        self.count = N * C * H * W
        self.flags = _lib.GA_PHOTO_LOSS_SAVE if save else 0
        self.x, self.y = _guarded(self.count, device, img1), _guarded(self.count, device, img2)
        self.nbytes = int(self.L.ga_photo_loss_workspace_bytes(N, C, H, W, self.flags))
        assert self.nbytes > 0 and self.nbytes % 4 == 0
        self.ws = _guarded(self.nbytes // 4, device)
        self.out = _guarded(N * 3, device)
        self.map = _guarded(self.count, device) if want_map else None
        self.grad = _guarded(self.count, device)
        self.stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    def _args(self, grad_out=None):
        N, C, H, W = self.shape
        return self._lib.GaPhotoLossArgs(N, C, H, W, self.flags, 0, self.x.data_ptr(), self.y.data_ptr(), self.out.data_ptr(),
                                         self.map.data_ptr() if self.map is not None else None,
                                         grad_out.data_ptr() if grad_out is not None else None, self.grad.data_ptr(),
                                         self.ws.data_ptr(), self.nbytes)

    def check_guards(self):
        assert _intact(self.x, self.count) and _intact(self.y, self.count) and _intact(self.ws, self.nbytes // 4)
        assert _intact(self.out, self.shape[0] * 3) and _intact(self.grad, self.count)
        assert self.map is None or _intact(self.map, self.count)

    def forward(self):
        """-> (means [N,3], map [N,C,H,W] or None), fresh tensors"""
        self.out[:self.shape[0] * 3] = POISON
        with torch.cuda.device(self.device):
            self._lib.check(self.L.ga_photo_loss_forward(ctypes.byref(self._args()), self.stream), "ga_photo_loss_forward")
            torch.cuda.synchronize()
        self.check_guards()
        means = self.out[:self.shape[0] * 3].reshape(-1, 3).clone()
        m = self.map[:self.count].reshape(self.shape).clone() if self.map is not None else None
        assert bool(torch.isfinite(means).all()) and (m is None or bool(torch.isfinite(m).all()))   # every slot written
        return means, m

    def backward(self, grad_out):
        g = _guarded(self.shape[0] * 3, self.device, grad_out.float())
        self.grad[:self.count] = POISON
        with torch.cuda.device(self.device):
            self._lib.check(self.L.ga_photo_loss_backward(ctypes.byref(self._args(g)), self.stream), "ga_photo_loss_backward")
            torch.cuda.synchronize()
        self.check_guards()
        assert _intact(g, self.shape[0] * 3)
        out = self.grad[:self.count].reshape(self.shape).clone()
        assert bool(torch.isfinite(out).all())
        return out


def _same_bits(a, b):
    return bool((a.view(torch.int32) == b.view(torch.int32)).all())


def _case_id(case):
    return f"{case[0]}-{'x'.join(map(str, case[1]))}-{case[2]}"


def _cases():
    # the tile is a build constant reported by the plan (host only, no GPU needed to collect)
    from gaussiananything_amd import _lib
    pl = _lib.GaPhotoLossPlan()
    assert _lib.lib().ga_photo_loss_plan(1, 1, 64, 64, ctypes.byref(pl)) == 0
    return ref.cases(pl.tile_w)


@pytest.mark.parametrize("case", _cases(), ids=_case_id)
def test_kernels_against_float64_within_the_bars_of_the_case(gpu_device, case):
    family, shape, seed = case
    a, b = ref.make_inputs(family, shape, seed)
    raw = Raw(a, b, gpu_device)
    means, smap = raw.forward()
    means2, smap2 = raw.forward()
    assert _same_bits(means, means2) and _same_bits(smap, smap2)               # no atomics: the same bits every time
    plain = Raw(a, b, gpu_device, save=False, want_map=False)                  # without SAVE and without the map: the same means
    assert _same_bits(plain.forward()[0], means)
    for which in ("ssim", "mixed"):
        w = ref.grad_weights(shape[0], which)
        r = ref.reference_errors(a, b, w)
        grad = raw.backward(w)
        assert _same_bits(grad, raw.backward(w))
        got, bar = ref.measured(r, smap, means, grad), ref.bars(r)
        print(which, {k: (got[k], bar[k]) for k in got})
        for key in ("map", "mean", "grad", "l1l2"):
            assert got[key] <= bar[key], (which, key, got[key], bar[key])
        if which == "mixed" and shape[0] == 2:
            assert bool((grad[1] == 0).all()) and float(grad[0].abs().max()) > 0  # a zero weight gives an exactly zero gradient


@pytest.mark.parametrize("shape", [(2, 3, 37, 70), (1, 1, 5, 33), (1, 4, 67, 31)])
def test_equal_images_give_ssim_one_and_no_l1_l2_gradient(gpu_device, shape):
    a, _ = ref.make_inputs("uniform11", shape, 5)
    raw = Raw(a, a.clone(), gpu_device)
    means, _ = raw.forward()
    w = torch.tensor([[0.0, 0.9, 1.7]] * shape[0])
    r = ref.reference_errors(a, a, w)
    assert float((means[:, 0].double().cpu() - 1).abs().max()) <= ref.bars(r)["mean"]
    assert bool((means[:, 1:] == 0).all())
    assert bool((raw.backward(w) == 0).all())        # sign(0) = 0 and 2 (x - y) = 0


def test_python_surface_matches_the_restatement(gpu_device):
    from gaussiananything_amd import losses
    a, b = ref.make_inputs("near", (2, 3, 37, 70), 21)
    x, y = (a * 2 - 1).to(gpu_device), (b * 2 - 1).to(gpu_device)
    w = torch.tensor([[1.0, 0.0, 0.0]] * 2)
    r = ref.reference_errors(x.cpu(), y.cpu(), w)
    bar = ref.bars(r)
    want = r["means"][:, 0]
    got = losses.ssim(x, y, size_average=False)
    assert got.shape == (2,) and float((got.double().cpu() - want).abs().max()) <= bar["mean"]
    assert abs(float(losses.ssim(x, y)) - float(want.mean())) <= bar["mean"]
    assert abs(float(losses.ssim_loss(x, y)) - float(1 - want.mean())) <= bar["mean"] + 1e-7
    assert float((losses.ssim_loss(x, y, 11, False).double().cpu() - (1 - want)).abs().max()) <= bar["mean"] + 1e-7
    # with gradients: d mean(ssim) / d img1 is the 'ssim' gradient with weights 1 / N
    xg = x.clone().requires_grad_(True)
    losses.ssim(xg, y).backward()
    r2 = ref.reference_errors(x.cpu(), y.cpu(), w / 2)
    assert ref.rel_l2(xg.grad, r2["grad"]) <= ref.bars(r2)["grad"]
    # photometric_loss: keys, values, PSNR by its formula
    lam = dict(l2_lambda=1.0, l1_lambda=0.5, ssim_lambda=0.2)
    loss, d = losses.photometric_loss(x, y, **lam)
    want_loss, want_d = ref.photometric_loss(x.cpu(), y.cpu(), dtype=torch.float64, **lam)
    assert set(d) == {"loss", "loss_l2", "loss_ssim", "mae", "PSNR", "SSIM"} and d["loss"] is loss
    for k in d:
        tol = bar["mean"] + 1e-6 * abs(float(want_d[k])) + 1e-7
        assert abs(float(d[k]) - float(want_d[k])) <= (tol if k != "PSNR" else 1e-4), k
    mse = float(((x.double() - y.double()) ** 2).mean())
    assert abs(float(d["PSNR"]) - 10 * torch.log10(torch.tensor(4.0 / mse, dtype=torch.float64)).item()) <= 1e-4
    # lambdas of 0 take their terms out of the loss, the metrics stay true (the documented departure)
    loss0, d0 = losses.photometric_loss(x, y)
    assert abs(float(loss0) - mse) <= 1e-6 * mse and float(d0["mae"]) > 0 and float(d0["SSIM"]) < 1
    # other dtypes and layouts are taken as .float().contiguous(); the gradient comes back in the prediction's dtype
    xh = x.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2).double().requires_grad_(True)
    assert not xh.is_contiguous()
    l2, _ = losses.photometric_loss(xh, y, **lam)
    l2.backward()
    assert xh.grad.dtype == torch.float64 and abs(float(l2.detach()) - float(loss)) <= 1e-6
    with torch.no_grad():                                  # forward only: no derivative maps are stored
        assert not losses.photo_means(x.clone().requires_grad_(True), y).requires_grad


def _e2e(device):
    from gaussiananything_amd import synthetic
    from gaussiananything_amd.gs_surfel import GaussianRenderer2DGS
    cams = synthetic.eval_cameras(2)
    g = synthetic.random_surfels(1000, seed=3).to(device)
    cv, cvp, cp = (cams[k][None].to(device) for k in ("cam_view", "cam_view_proj", "cam_pos"))
    r = GaussianRenderer2DGS(64, 3, {})
    gen = torch.Generator().manual_seed(8)
    g_target = g.clone()
    g_target[..., 10:13] = (g[..., 10:13] + 0.2 * torch.randn(g[..., 10:13].shape, generator=gen).to(device)).clamp(0, 1)
    with torch.no_grad():
        target = r.render(g_target, cv, cvp, cp, cams["tanfov"])["image"].reshape(-1, 3, 64, 64) * 2 - 1

    def render(leaf):
        return r.render(leaf, cv, cvp, cp, cams["tanfov"])["image"].reshape(-1, 3, 64, 64) * 2 - 1

    return g, target, render


def test_end_to_end_through_the_renderer(gpu_device):
    """1000 surfels, 2 views, 64 x 64, the target rendered from the same surfels with perturbed colours: the gradient of
    photometric_loss reaches the Gaussian tensor and equals the one obtained with the torch restatement of the loss on the same
    rendered image (both go through ga_surfel_backward, so only the loss gradient differs)."""
    from gaussiananything_amd import losses, synthetic
    g, target, render = _e2e(gpu_device)
    lam = dict(l2_lambda=1.0, l1_lambda=1.0, ssim_lambda=0.2)
    leaf = g.clone().requires_grad_(True)
    loss, d = losses.photometric_loss(render(leaf), target, **lam)
    loss.backward()
    leaf_ref = g.clone().requires_grad_(True)
    image = render(leaf_ref)
    image_cpu = image.detach().cpu().requires_grad_(True)      # the restatement runs on the CPU; its gradient goes back to the device
    loss_ref, _ = ref.photometric_loss(image_cpu, target.cpu(), **lam)
    loss_ref.backward()
    image.backward(image_cpu.grad.to(gpu_device))
    assert abs(float(loss) - float(loss_ref)) <= 1e-5 * abs(float(loss_ref))
    names = ("means3D", "opacity", "scales", "rotations", "rgb")
    got, want = synthetic.split_gaussians(leaf.grad[0]), synthetic.split_gaussians(leaf_ref.grad[0])
    lines, worst = [], 0.0
    for name, a, b in zip(names, got, want):
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0, name
        err = ref.rel_l2(a, b)
        lines.append(f"{name:10s} relative L2 of the gradient against the torch loss on the same render: {err:.3e}")
        worst = max(worst, err)
    ref.write_section("end to end (tests/test_photo_loss_gpu.py): 1000 surfels, 2 views, 64 x 64, lambdas 1 / 1 / 0.2", lines)
    print("\n".join(lines))
    assert worst <= E2E_BAR, worst


# relative L2 of each leaf gradient against the torch restatement of the loss: 4 x the largest measured value (2.65e-6:
# means3D 2.6e-6, opacity 2.5e-6, scales 2.6e-6, rotations 2.7e-7, rgb 1.6e-6; profiles/photo_loss_bounds.txt),
# which is below the 1e-4 the check starts from
E2E_BAR = 1.1e-5


def test_captured_graph_replays_with_new_images_and_weights(gpu_device):
    """forward + backward captured once as a single chain; replays read the images and grad_out from the same buffers, so new
    contents give the eager result bit for bit (nothing of them is frozen into the graph)"""
    from gaussiananything_amd import _lib
    shape = (2, 3, 37, 70)
    a, b = ref.make_inputs("uniform01", shape, 31)
    raw = Raw(a, b, gpu_device)
    g = _guarded(6, gpu_device, torch.tensor([[1.0, 0.5, 0.25], [0.3, 0.0, 2.0]]))
    L = _lib.lib()
    side = torch.cuda.Stream(device=gpu_device)

    def enqueue(stream):
        s = ctypes.c_void_p(stream.cuda_stream)
        _lib.check(L.ga_photo_loss_forward(ctypes.byref(raw._args()), s), "ga_photo_loss_forward")
        _lib.check(L.ga_photo_loss_backward(ctypes.byref(raw._args(g)), s), "ga_photo_loss_backward")

    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        enqueue(side)          # warm-up on the capture stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            enqueue(side)
    torch.cuda.synchronize()
    a2, b2 = ref.make_inputs("near", shape, 32)
    w2 = torch.tensor([[0.0, 0.0, 0.0], [0.8, 1.5, 0.1]])
    raw.x[:raw.count] = a2.reshape(-1).to(gpu_device)
    raw.y[:raw.count] = b2.reshape(-1).to(gpu_device)
    g[:6] = w2.reshape(-1).to(gpu_device)
    raw.out[:6] = POISON
    raw.grad[:raw.count] = POISON
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    raw.check_guards()
    means, grad = raw.out[:6].reshape(2, 3).clone(), raw.grad[:raw.count].reshape(shape).clone()
    eager = Raw(a2, b2, gpu_device)
    want_means, _ = eager.forward()
    want_grad = eager.backward(w2)
    assert _same_bits(means, want_means) and _same_bits(grad, want_grad)
    assert bool((grad[0] == 0).all()) and float(grad[1].abs().max()) > 0
