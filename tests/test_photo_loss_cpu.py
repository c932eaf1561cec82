"""CPU tests of the photometric loss (include/ga_loss.h): the restatement against the golden recorded from the reference's own
functions, the struct layouts, the host validation of the C-ABI and of the Python front end (no launch happens for a rejected call, so
no GPU is needed), the derivative formulas of the header, and the confirmation that a separable fp32 evaluation stays within the bars
of every GPU case."""
import ctypes
import os
import subprocess

import pytest
import torch

from tests import _ssim_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GA_ERR_NULL_ARG, GA_ERR_BAD_SHAPE, GA_ERR_WORKSPACE, GA_ERR_BAD_FLAGS = -1, -2, -3, -5


def _lib():
    from gaussiananything_amd import _lib
    return _lib, _lib.lib()


def _tile():
    _l, L = _lib()
    pl = _l.GaPhotoLossPlan()
    assert L.ga_photo_loss_plan(1, 1, 64, 64, ctypes.byref(pl)) == 0 and pl.tile_w == pl.tile_h
    return pl.tile_w


def test_restatement_reproduces_the_golden_of_the_reference():
    """tests/golden/photo_loss_ref.pt was recorded from the reference's gaussian / create_window / _ssim: on the same torch the fp32
    restatement gives the same values; 1e-6 absorbs a different convolution order of another build"""
    z = torch.load(os.path.join(ROOT, "tests", "golden", "photo_loss_ref.pt"))
    assert len(z["cases"]) >= 4
    worst = 0.0
    for case in z["cases"]:
        a, b = ref.make_inputs(case["family"], tuple(case["shape"]), case["seed"])
        x = a.clone().requires_grad_(True)
        mean = ref.ssim(x, b, True)
        mean.backward()
        per_image = ref.ssim(a, b, False)
        assert per_image.shape == (case["shape"][0],)
        diffs = (float((mean.detach() - case["ssim"]).abs()), float((per_image - case["ssim_per_image"]).abs().max()),
                 float((x.grad - case["grad_img1"]).abs().max()))
        print(case["family"], tuple(case["shape"]), "max differences (mean, per image, gradient)", diffs)
        worst = max(worst, *diffs)
    assert worst <= 1e-6, worst


def test_photo_loss_ctypes_mirrors_have_the_layout_of_the_header(tmp_path):
    from gaussiananything_amd import _lib as _l
    mirrors = [_l.GaPhotoLossArgs, _l.GaPhotoLossPlan]
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "ga_loss.h"', "int main(void) {",
             '  printf("GA_PHOTO_LOSS_SAVE %d\\n", GA_PHOTO_LOSS_SAVE);']
    for cls in mirrors:
        lines.append(f'  printf("{cls.__name__} %zu\\n", sizeof({cls.__name__}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cls.__name__}.{fname} %zu\\n", offsetof({cls.__name__}, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["GA_PHOTO_LOSS_SAVE"]) == _l.GA_PHOTO_LOSS_SAVE
    for cls in mirrors:
        assert int(got[cls.__name__]) == ctypes.sizeof(cls), cls.__name__
        for fname, _ in cls._fields_:
            assert int(got[f"{cls.__name__}.{fname}"]) == getattr(cls, fname).offset, (cls.__name__, fname)


def test_plan_and_workspace_are_consistent():
    _l, L = _lib()
    pl = _l.GaPhotoLossPlan()
    assert L.ga_photo_loss_plan(1, 1, 8, 8, None) == GA_ERR_NULL_ARG
    for bad in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, -1), (1, 3, 65537, 8), (1 << 20, 1 << 11, 8, 8), (1 << 15, 1, 65536, 65536)):
        assert L.ga_photo_loss_plan(*bad, ctypes.byref(pl)) == GA_ERR_BAD_SHAPE, bad
        assert L.ga_photo_loss_workspace_bytes(*bad, 0) == 0 and L.ga_photo_loss_workspace_bytes(*bad, 1) == 0
    for N, C, H, W in ((1, 1, 1, 1), (2, 3, 37, 70), (8, 3, 512, 512), (50, 3, 128, 128), (1, 4, 33, 31)):
        assert L.ga_photo_loss_plan(N, C, H, W, ctypes.byref(pl)) == 0
        T = pl.tile_w
        assert pl.tile_h == T and pl.threads == 256 and pl.tiles_x == -(-W // T) and pl.tiles_y == -(-H // T)
        assert pl.grid_x == N * C * pl.tiles_x * pl.tiles_y and pl.num_partials == 3 * pl.grid_x
        assert 0 < pl.lds_bytes <= 160 * 1024 // 3      # three workgroups per CU
        plain, save = L.ga_photo_loss_workspace_bytes(N, C, H, W, 0), L.ga_photo_loss_workspace_bytes(N, C, H, W, 1)
        assert plain >= 4 * pl.num_partials and plain % 256 == 0 and save == plain + 3 * 4 * N * C * H * W


def test_host_validation_rejects_before_any_launch():
    """Fake, non-NULL device addresses: a call that got past validation would fault; every one here must be turned away."""
    _l, L = _lib()
    P = 0x1000   # never dereferenced
    need = L.ga_photo_loss_workspace_bytes(2, 3, 37, 70, 1)

    def args(N=2, C=3, H=37, W=70, flags=1, img1=P, img2=P, out=P, grad_out=P, grad_img1=P, workspace=P, nbytes=need):
        return _l.GaPhotoLossArgs(N, C, H, W, flags, 0, img1, img2, out, None, grad_out, grad_img1, workspace, nbytes)

    for fn in (L.ga_photo_loss_forward, L.ga_photo_loss_backward):
        assert fn(None, None) == GA_ERR_NULL_ARG
        for kw in (dict(img1=None), dict(img2=None), dict(workspace=None)):
            assert fn(ctypes.byref(args(**kw)), None) == GA_ERR_NULL_ARG, kw
        for kw in (dict(N=0), dict(C=0), dict(H=0), dict(W=-3), dict(H=65537)):
            assert fn(ctypes.byref(args(**kw)), None) == GA_ERR_BAD_SHAPE, kw
        for kw in (dict(flags=2), dict(flags=3), dict(flags=-1)):
            assert fn(ctypes.byref(args(**kw)), None) == GA_ERR_BAD_FLAGS, kw
        assert fn(ctypes.byref(args(nbytes=need - 1)), None) == GA_ERR_WORKSPACE
        assert fn(ctypes.byref(args(nbytes=0)), None) == GA_ERR_WORKSPACE
    assert L.ga_photo_loss_forward(ctypes.byref(args(out=None)), None) == GA_ERR_NULL_ARG
    assert L.ga_photo_loss_backward(ctypes.byref(args(grad_out=None)), None) == GA_ERR_NULL_ARG
    assert L.ga_photo_loss_backward(ctypes.byref(args(grad_img1=None)), None) == GA_ERR_NULL_ARG
    assert L.ga_photo_loss_backward(ctypes.byref(args(flags=0)), None) == GA_ERR_BAD_FLAGS   # no saved maps to read
    small = L.ga_photo_loss_workspace_bytes(2, 3, 37, 70, 0)
    assert L.ga_photo_loss_forward(ctypes.byref(args(flags=1, nbytes=small)), None) == GA_ERR_WORKSPACE


def test_python_front_end_validates_on_the_host(monkeypatch):
    from gaussiananything_amd import _lib as _l, losses
    a, b = torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8)

    def no_launch(*args, **kw):
        raise AssertionError("a rejected call reached the library")

    monkeypatch.setattr(losses, "_forward", no_launch)
    for fn in (losses.ssim, losses.ssim_loss, losses.photometric_loss, losses.photo_means):
        with pytest.raises(ValueError, match="no CPU fallback"):
            fn(a, b)
        with pytest.raises(TypeError):
            fn(a.numpy(), b)
        with pytest.raises(TypeError):
            fn(a, b.long())
    with pytest.raises(ValueError, match="window_size"):
        losses.ssim(a, b, window_size=7)
    with pytest.raises(ValueError, match="window_size"):
        losses.ssim_loss(a, b, 9)
    with pytest.raises(ValueError, match="one shape"):
        losses.ssim(a, torch.zeros(1, 3, 8, 9))
    with pytest.raises(ValueError, match="one shape"):
        losses.photometric_loss(a[0], b[0])
    with pytest.raises(ValueError, match="requires grad"):
        losses.ssim(a, torch.zeros(1, 3, 8, 8, requires_grad=True))
    with pytest.raises(ValueError, match="requires grad"):
        losses.photometric_loss(a, torch.zeros(1, 3, 8, 8, requires_grad=True), ssim_lambda=0.2)
    # a missing library raises, with nothing enqueued
    monkeypatch.setattr(_l, "_lib", None)
    monkeypatch.setattr(_l, "LIB_PATH", os.path.join(str(ROOT), "no_such_dir", "libga_mi355.so"))
    with pytest.raises(RuntimeError):
        losses._validate(_CudaLike(a), _CudaLike(b))


class _CudaLike(torch.Tensor):
    """a CPU tensor that reports a GPU device: reaches the library lookup of the validation, and nothing behind it is called"""

    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    @property
    def device(self):
        return torch.device("cuda", 0)


def test_derivative_formulas_of_the_header_match_autograd_in_float64():
    """dS/dmu1 (E11, E12 held fixed), dS/dE11, dS/dE12 as include/ga_loss.h states them, and the composition
    grad = conv(dS/dmu1) + 2 x conv(dS/dE11) + y conv(dS/dE12), against autograd of the float64 restatement"""
    dt = torch.float64
    worst = 0.0
    for family, shape, seed in (("uniform01", (2, 3, 17, 23), 1), ("uniform11", (1, 1, 5, 40), 2), ("white", (1, 4, 13, 12), 3)):
        a, b = ref.make_inputs(family, shape, seed)
        x, y = a.to(dt), b.to(dt)
        leaves = [t.detach().clone().requires_grad_(True) for t in ref.moments(x, y, dt)]
        S = ref.ssim_from_moments(*leaves)
        S.sum().backward()
        mu1, mu2, e11, e22, e12 = [t.detach() for t in leaves]
        A1, A2 = 2 * mu1 * mu2 + ref.C1, 2 * (e12 - mu1 * mu2) + ref.C2
        B1, B2 = mu1 ** 2 + mu2 ** 2 + ref.C1, (e11 - mu1 ** 2) + (e22 - mu2 ** 2) + ref.C2
        d_e11 = -A1 * A2 / (B1 * B2 ** 2)
        d_e12 = 2 * A1 / (B1 * B2)
        d_mu1 = 2 * mu2 * A2 / (B1 * B2) - 2 * mu1 * A1 * A2 / (B1 ** 2 * B2) + 2 * mu1 * A1 * A2 / (B1 * B2 ** 2) - 2 * mu2 * A1 / (B1 * B2)
        for got, want in ((d_e11, leaves[2].grad), (d_e12, leaves[4].grad), (d_mu1, leaves[0].grad)):
            worst = max(worst, ref.rel_l2(got, want))
        xg = x.clone().requires_grad_(True)
        ref.ssim_map(xg, y, dt).sum().backward()
        C = shape[1]
        composed = ref._conv2d(d_mu1, C, dt) + 2 * x * ref._conv2d(d_e11, C, dt) + y * ref._conv2d(d_e12, C, dt)
        worst = max(worst, ref.rel_l2(composed, xg.grad))
    print("worst relative L2 difference", worst)
    assert worst <= 1e-12


def test_a_separable_fp32_evaluation_stays_within_the_bars_of_every_gpu_case():
    """'Numerics' of the issue, repeated for every case the GPU test runs: E_map, E_mean, E_grad of the fp32 2-D-window restatement
    against float64 set the bars, and an fp32 rows-then-columns model (what the kernel does) must fit them.  The table goes to
    profiles/photo_loss_bounds.txt."""
    T = _tile()
    cases = ref.cases(T)
    sides = set(ref.shapes_hw(T))
    assert 35 <= len(cases) <= 48
    assert {c[1][2] for c in cases} >= sides and {c[1][3] for c in cases} >= sides and any(c[1][2:] == (37, 70) for c in cases)
    assert {c[0] for c in cases} == set(ref.FAMILIES) and {c[1][1] for c in cases} == {1, 3, 4} and {c[1][0] for c in cases} == {1, 2}
    lines = [f"tile {T}; per case the errors of the fp32 2-D-window restatement against float64 (E_*), the bars 2 E + floor, and the",
             "errors of the fp32 separable model against float64 (sep_*); gradient columns are relative L2, weights 'ssim' / 'mixed'",
             f"{'family':10s} {'shape':16s} {'E_map':>9s} {'sep_map':>9s} {'E_mean':>9s} {'sep_mean':>9s} {'E_grad':>9s} {'sep_grad':>9s} "
             f"{'E_grad_mx':>9s} {'sep_gr_mx':>9s} {'sep_l1l2':>9s}"]
    failures = []
    for family, shape, seed in cases:
        a, b = ref.make_inputs(family, shape, seed)
        row = []
        for which in ("ssim", "mixed"):
            w = ref.grad_weights(shape[0], which)
            r = ref.reference_errors(a, b, w)
            got = ref.measured(r, *ref.evaluate(a, b, w, torch.float32, separable=True))
            bar = ref.bars(r)
            for key in ("map", "mean", "grad", "l1l2"):
                if not got[key] <= bar[key]:
                    failures.append((family, shape, which, key, got[key], bar[key]))
            row.append((r, got))
        (r0, g0), (r1, g1) = row
        lines.append(f"{family:10s} {'x'.join(map(str, shape)):16s} {r0['E_map']:9.2e} {g0['map']:9.2e} {r0['E_mean']:9.2e} {g0['mean']:9.2e} "
                     f"{r0['E_grad']:9.2e} {g0['grad']:9.2e} {r1['E_grad']:9.2e} {g1['grad']:9.2e} {g1['l1l2']:9.2e}")
    ref.write_section("bars per GPU case (tests/test_photo_loss_cpu.py)", lines)
    print("\n".join(lines))
    assert not failures, failures
