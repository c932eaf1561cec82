"""CPU tests of the depth-view unprojection (include/ga_pointcloud.h: ga_pc_unproject; csrc/pc_unproject.hip): the float32 restatement
the GPU tests hold the kernels to bit for bit (tests/_unproject_ref.py) against the reference's own result (tests/golden/
unproject_ref.pt, written by make_unproject_golden.py from the reference's ray sampler and the tensor lines of its save_pcd script) and
against float64, the pixel-centre convention against the rasterizer's projection, and what the Python front end refuses before it
touches the library.

Bars.  (b) 4 x the reference's own largest deviation from the float64 geometry, recorded in the fixture (2.066e-7 -> 8.26e-7): the
restatement's chain of roundings is as long as the reference's but ordered differently.  (c) 1e-3 px and 1e-5 relative: fp32 on
coordinates <= 2 is 1.2e-7 relative per operation, a dozen operations and a projection of focal length ~1.4 image widths of 16 px
stay under 1e-4 px and 2e-6 relative."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import _unproject_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
CLIP, DEPTH_MIN = 0.45, 1.05


@pytest.fixture(scope="module")
def golden():
    z = torch.load(os.path.join(ROOT, "tests", "golden", "unproject_ref.pt"))
    return {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in z.items()}


@pytest.fixture(scope="module")
def restated(golden):
    """the restatement under the reference's rules on the golden inputs: computed once, shared, left unchanged"""
    cam = ref.cameras_from_pose25(golden["c"])
    lo = float(np.nextafter(F(DEPTH_MIN), F(-np.inf)))          # `depth < 1.05` dropped, 1.05 itself kept
    out = ref.unproject_f32(golden["depth"], cam, mask=(golden["alpha_mask"] == 1).astype(F), depth_kind=ref.DEPTH_RAY, depth_min=lo,
                            mask_threshold=0.5, clip=CLIP, drop_zero=True)
    return cam, out


def test_restatement_keeps_the_pixels_the_reference_keeps(golden, restated):
    cam, out = restated
    n = out["count"]
    mine, theirs = out["source"][:n], golden["source"]
    assert (np.diff(mine) > 0).all() and (np.diff(theirs) > 0).all()                    # both in ascending pixel order
    differ = np.setxor1d(mine, theirs)
    print(f"restatement keeps {n} pixels, the reference {len(theirs)}; {len(differ)} differ")
    if len(differ):
        exact = ref.lift_f64(golden["depth"], cam, ref.DEPTH_RAY).reshape(-1, 3)[differ]
        gap = np.abs(np.abs(exact) - CLIP).min(1)
        assert len(differ) <= 2 and (gap <= np.spacing(F(CLIP))).all(), (differ, gap)
    else:
        assert n == len(theirs) and np.array_equal(mine, theirs)
        assert (out["view_counts"] == np.bincount(theirs // (24 * 24), minlength=3)).all()
    assert (out["source"][n:] == -1).all() and not out["points"][n:].any()


def test_restated_coordinates_against_float64(golden, restated):
    cam, out = restated
    n = out["count"]
    exact = ref.lift_f64(golden["depth"], cam, ref.DEPTH_RAY).reshape(-1, 3)
    bar = 4 * golden["deviation_from_float64"]
    err = np.abs(out["points"][:n].astype(np.float64) - exact[out["source"][:n]]).max()
    ref_err = np.abs(golden["points"].astype(np.float64) - exact[golden["source"]]).max()
    print(f"restatement vs float64 {err:.3e}, reference vs float64 {ref_err:.3e} (recorded {golden['deviation_from_float64']:.3e}), bar {bar:.3e}")
    assert abs(ref_err - golden["deviation_from_float64"]) <= 1e-12 and 0 < bar < 2e-6      # the recorded figure is reproducible
    assert err <= bar
    # camera-z depth: the same bar on the same inputs (the chain is shorter: no normalisation)
    z32 = ref.lift_f32(golden["depth"], cam, ref.DEPTH_Z).astype(np.float64)
    z64 = ref.lift_f64(golden["depth"], cam, ref.DEPTH_Z)
    assert np.abs(z32 - z64).max() <= bar


def test_pixel_centres_round_trip_through_the_rasterizer_projection():
    """every pixel centre of a 16 x 16 image, every camera of cameras_eval8.npz: the restated point for camera-z depth through
    cameras_from_view's formulas, projected in float64 with cam_view_proj, lands on (x, y) -- pixel = ((ndc + 1) * S - 1) / 2, the
    rasterizer's ndc2Pix -- and its view-space z is the depth"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "cameras_eval8.npz"))
    S, V = 16, z["cam_view"].shape[0]
    cam = ref.cameras_from_view(z["cam_view"], float(z["tanfov"]))
    rng = np.random.default_rng(5)
    depth = rng.uniform(1.0, 2.5, size=(V, S, S)).astype(F)
    p = ref.lift_f32(depth, cam, ref.DEPTH_Z).astype(np.float64)
    hom = np.concatenate([p, np.ones((V, S, S, 1))], -1)
    clip = np.einsum("vyxa,vab->vyxb", hom, z["cam_view_proj"].astype(np.float64))
    view = np.einsum("vyxa,vab->vyxb", hom, z["cam_view"].astype(np.float64))
    pix = ((clip[..., :2] / clip[..., 3:4] + 1) * S - 1) / 2
    yy, xx = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    off = max(np.abs(pix[..., 0] - xx).max(), np.abs(pix[..., 1] - yy).max())
    rel = (np.abs(view[..., 2] - depth) / depth).max()
    print(f"pixel-centre round trip: {off:.3e} px, view-space z {rel:.3e} relative")
    assert off <= 1e-3 and rel <= 1e-5
    # the torch helper states the same formulas
    from gaussiananything_amd import cameras
    got = cameras.cameras_from_view(torch.from_numpy(z["cam_view"]), float(z["tanfov"])).numpy()
    assert got.shape == (V, 21) and np.abs(got - cam).max() <= 4 * 2.0 ** -24 * 2 and np.array_equal(got[:, :9], cam[:, :9])
    assert np.array_equal(got[:, 12:], cam[:, 12:]) and not got[:, 17:].any()
    assert np.array_equal(cameras.cameras_from_pose25(torch.from_numpy(z["poses"])).numpy(), ref.cameras_from_pose25(z["poses"]))


def test_restated_erosion_is_the_iterated_cross():
    """the diamond the kernel tests directly equals e iterations of the cross, borders included"""
    rng = np.random.default_rng(9)
    m = (rng.uniform(size=(2, 13, 17)) < 0.85).astype(F)
    for e in (1, 2, 3, 4):
        it = ref.eroded_foreground(m, 0.5, e)
        fg = m >= 0.5
        want = np.ones_like(fg)
        for dy in range(-e, e + 1):
            for dx in range(-(e - abs(dy)), e - abs(dy) + 1):
                sh = np.ones_like(fg)
                ys, xs = slice(max(0, -dy), 13 - max(0, dy)), slice(max(0, -dx), 17 - max(0, dx))
                yd, xd = slice(max(0, dy), 13 - max(0, -dy)), slice(max(0, dx), 17 - max(0, -dx))
                sh[:, ys, xs] = fg[:, yd, xd]
                want &= sh
        assert np.array_equal(it, want), e


def test_c_abi_rejects_before_any_launch():
    """Fake, non-NULL device addresses: a call that got past validation would fault; every one here must be turned away."""
    from gaussiananything_amd import _lib as _l
    L = _l.lib()
    P = 0x1000   # never dereferenced, 16-byte aligned
    NULL_ARG, BAD_SHAPE, WORKSPACE, BAD_FLAGS = -1, -2, -3, -5
    fields = [n for n, _ in _l.GaUnprojectArgs._fields_]

    def call(**kw):
        v = dict(num_views=2, height=8, width=8, depth_kind=0, color_kind=0, erode=0, drop_zero=0, pixel_stride=1, capacity=128,
                 depth_min=0.0, depth_max=float("inf"), mask_threshold=0.5, clip=0.0, reserved=0, depth=P, mask=P, color=P, normal=P,
                 cameras=P, points=P, colors=P, normals=P, source=P, count=P, view_counts=P, workspace=P, workspace_bytes=1 << 20)
        v.update(kw)
        return L.ga_pc_unproject(ctypes.byref(_l.GaUnprojectArgs(*[v[n] for n in fields])), None)

    assert L.ga_pc_unproject(None, None) == NULL_ARG
    for kw in (dict(num_views=0), dict(height=0), dict(width=0), dict(width=4097), dict(num_views=1 << 15, height=1 << 8, width=1 << 8),
               dict(capacity=0), dict(capacity=-1)):
        assert call(**kw) == BAD_SHAPE, kw
    nan = float("nan")
    for kw in (dict(depth_kind=2), dict(depth_kind=-1), dict(color_kind=2), dict(erode=5), dict(erode=-1), dict(drop_zero=2),
               dict(pixel_stride=0), dict(reserved=1), dict(depth_min=nan), dict(depth_max=nan), dict(mask_threshold=nan),
               dict(clip=nan), dict(clip=-0.5), dict(clip=float("inf"))):
        assert call(**kw) == BAD_FLAGS, kw
    for name in ("depth", "cameras", "points", "source", "count", "view_counts", "workspace", "colors", "normals", "color", "normal"):
        assert call(**{name: None}) == NULL_ARG, name                  # (a colour or normal map without its output, and the reverse)
    need = L.ga_pc_unproject_workspace_bytes(2, 8, 8)
    assert need > 0 and need % 16 == 0
    assert call(workspace_bytes=need - 1) == WORKSPACE and call(workspace=P + 4) == WORKSPACE
    assert L.ga_pc_unproject_workspace_bytes(0, 8, 8) == 0 and L.ga_pc_unproject_workspace_bytes(2, 8, 4097) == 0
    # num_blocks + 1 int32 padded to 16 bytes, then one byte per pixel padded to 16
    r, bpv, nb = ref.plan(3, 40, 56)
    assert L.ga_pc_unproject_workspace_bytes(3, 40, 56) == -(-(nb + 1) // 4) * 16 + -(-(3 * 40 * 56) // 16) * 16


def test_front_end_validates_on_the_host():
    """CPU tensors: everything is refused before the library is loaded (GPU only, no fallback)"""
    from gaussiananything_amd import cameras, fitting, io_formats, pointcloud
    d, c = torch.ones(2, 8, 8), torch.zeros(2, 25)
    U = pointcloud.unproject_depth_views
    with pytest.raises(RuntimeError, match="GPU"):
        U(d, c)
    with pytest.raises(RuntimeError, match="GPU"):
        U(d[:, None], torch.zeros(2, 21), mask=d, color=torch.zeros(2, 3, 8, 8, dtype=torch.uint8), normal=torch.zeros(2, 3, 8, 8))
    for bad in (dict(depth_kind="x"), dict(erode=5), dict(erode=-1), dict(erode=1), dict(pixel_stride=0), dict(clip=0.0 - 1), dict(clip=float("inf")),
                dict(depth_range=(1.0, 1.0)), dict(depth_range=(float("nan"), 1.0)), dict(mask_threshold=float("nan")), dict(capacity=0),
                dict(capacity=2 ** 31)):
        with pytest.raises(ValueError):
            U(d, c, **bad)
    for depth, cam in ((torch.ones(8, 8), c), (torch.ones(2, 2, 8, 8), c), (d, torch.zeros(3, 25)), (d, torch.zeros(2, 16)),
                       (np.ones((2, 8, 8), F), c), (torch.ones(2, 8, 5000), c)):
        with pytest.raises(ValueError):
            U(depth, cam)
    with pytest.raises(TypeError):
        U(d.long(), c)
    with pytest.raises(ValueError):
        U(d, c, mask=torch.ones(2, 8, 7))
    with pytest.raises(ValueError):
        U(d, c, color=torch.ones(2, 4, 8, 8))
    with pytest.raises(TypeError):
        U(d, c, normal=torch.ones(2, 3, 8, 8, dtype=torch.uint8))
    assert pointcloud.unproject_candidates(3, 40, 56, 3) == 3 * 14 * 19
    with pytest.raises(ValueError):
        cameras.cameras_from_view(torch.zeros(4, 4), 0.5)
    with pytest.raises(ValueError):
        cameras.cameras_from_view(torch.zeros(2, 4, 4), 0.0)
    with pytest.raises(ValueError):
        pointcloud.cloud_from_render({"depth": d}, torch.zeros(2, 4, 4), 0.5)
    out = {k: torch.zeros(1, 2, ch, 8, 8) for k, ch in (("depth", 1), ("alpha", 1), ("image", 3), ("rend_normal", 3))}
    with pytest.raises(RuntimeError, match="GPU"):
        pointcloud.cloud_from_render(out, torch.eye(4).repeat(1, 2, 1, 1), 0.5)
    with pytest.raises(ValueError):
        pointcloud.cloud_from_render(out, torch.eye(4).repeat(1, 2, 1, 1), 0.5, depth_kind="ray")
    with pytest.raises(RuntimeError, match="GPU"):
        fitting.SurfelFitter.from_rgbd(d, torch.eye(4).repeat(2, 1, 1), torch.eye(4).repeat(2, 1, 1), 0.5, torch.zeros(2, 3, 8, 8))
    with pytest.raises(ValueError):
        fitting.SurfelFitter.from_rgbd(d, torch.eye(4).repeat(2, 1, 1), torch.eye(4).repeat(2, 1, 1), 0.5, torch.zeros(2, 3, 8, 9))
    with pytest.raises(ValueError):
        fitting.SurfelFitter.from_rgbd(d, torch.eye(4).repeat(2, 1, 1), torch.eye(4).repeat(2, 1, 1), 0.5, torch.zeros(2, 3, 8, 8), max_points=3)
    with pytest.raises(ValueError):
        io_formats.export_fps_points_from_depth(np.ones((2, 8, 8), F), np.zeros((3, 25), F), "unused.ply")
