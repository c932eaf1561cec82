"""GPU tests of the TSDF kernels (csrc/tsdf.hip behind include/ga_tsdf.h) where the sphere of tests/test_tsdf_gpu.py does not reach:
every marching-cubes case, holes, units never opened, more than 1024 units (the carry of the unit scan), exact zeros and saturated
values, the emit contract under smaller counts, and fusion with other strides, intrinsics, camera positions, depth and colour
values than the in-tree evaluation cameras give.

Bars as in tests/test_tsdf_gpu.py (tests/_tsdf_util.py: check_volume, check_mesh, check_units; tests/test_tsdf_cpu.py shows that each
of them fails on a planted defect): integer artefacts identical; tsdf, vertices and vertex colours 1e-6; the colour volume 1e-4.  No
voxel is exempt.  The mesh calls go through the C-ABI on poisoned buffers with guard words behind each of them."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import tsdf as otsdf
from tests import _tsdf_util as tu

pytestmark = pytest.mark.gpu

GUARD = 64                                   # 32-bit words behind every buffer
GUARD_F, GUARD_I, GUARD_B = 12345.0, 0x5A5A5A5A, 0xA5
BOX = dict(units=(3, 4, 5), unit0=(-1, -2, -3), voxel=0.0125, trunc=0.075)     # x [-0.2, 0.4], y [-0.4, 0.4], z [-0.6, 0.4]
CENTRE = (0.1, 0.0, -0.1)


class RawMesh:
    """ga_tsdf_mesh_count / ga_tsdf_mesh_emit of one TSDFVolume on guarded buffers"""

    def __init__(self, hvol):
        from gaussiananything_amd import _lib
        self._lib, self.L, self.hvol, self.dev = _lib, _lib.lib(), hvol, hvol.device
        self.nbytes = int(self.L.ga_tsdf_mesh_scratch_bytes(ctypes.byref(hvol._c)))
        assert self.nbytes > 0
        self.scratch = torch.full((self.nbytes + 4 * GUARD,), GUARD_B, dtype=torch.uint8, device=self.dev)
        self.counts = torch.full((2 + GUARD,), GUARD_I, dtype=torch.int64, device=self.dev)

    def count(self):
        with torch.cuda.device(self.dev):
            rc = self.L.ga_tsdf_mesh_count(ctypes.byref(self.hvol._c), self.scratch.data_ptr(), self.nbytes, self.counts.data_ptr(),
                                           self.hvol._stream())
            torch.cuda.synchronize()
        assert rc == 0, rc
        assert bool((self.scratch[self.nbytes:] == GUARD_B).all()) and bool((self.counts[2:] == GUARD_I).all())
        return tuple(int(x) for x in self.counts[:2].cpu().tolist())

    def emit(self, nv, nt, room_v, room_t):
        """pass the counts (nv, nt) with buffers that have room for (room_v, room_t); -> host (vertices, colours, triangles) as
        [room, 3] arrays, NaN / -1 where nothing was written"""
        v = torch.full((3 * room_v + GUARD,), float("nan"), dtype=torch.float32, device=self.dev)
        c = torch.full((3 * room_v + GUARD,), float("nan"), dtype=torch.float32, device=self.dev)
        t = torch.full((3 * room_t + GUARD,), -1, dtype=torch.int32, device=self.dev)
        v[3 * room_v:], c[3 * room_v:], t[3 * room_t:] = GUARD_F, GUARD_F, GUARD_I
        with torch.cuda.device(self.dev):
            rc = self.L.ga_tsdf_mesh_emit(ctypes.byref(self.hvol._c), self.scratch.data_ptr(), self.nbytes, nv, nt, v.data_ptr(), c.data_ptr(),
                                          t.data_ptr(), self.hvol._stream())
            torch.cuda.synchronize()
        assert rc == 0, rc
        assert bool((v[3 * room_v:] == GUARD_F).all()) and bool((c[3 * room_v:] == GUARD_F).all()) and bool((t[3 * room_t:] == GUARD_I).all())
        assert bool((self.scratch[self.nbytes:] == GUARD_B).all())
        return (v[:3 * room_v].reshape(-1, 3).cpu().numpy(), c[:3 * room_v].reshape(-1, 3).cpu().numpy(),
                t[:3 * room_t].reshape(-1, 3).cpu().numpy())


def _same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _mesh_against_oracle(hvol, want):
    """count + emit twice over: counts, index lists, positions and colours against the oracle, every slot written, guards intact,
    the same bits on the second run"""
    raw = RawMesh(hvol)
    nv, nt = raw.count()
    assert (nv, nt) == (len(want[0]), len(want[2])), ((nv, nt), (len(want[0]), len(want[2])))
    got = raw.emit(nv, nt, nv, nt)
    figures = tu.check_mesh(got, want)
    tu.check_mesh_invariants(got[2], nv)
    assert raw.count() == (nv, nt)
    again = raw.emit(nv, nt, nv, nt)
    assert all(_same_bits(a, b) for a, b in zip(got, again))
    return raw, got, figures


def _loaded(dev, name):
    vol = tu.mc_volume(name)
    hvol = tu.hip_volume_like(vol, dev)
    tu.load_dense(hvol, vol.tsdf, vol.weight, vol.color, vol.allocated)
    return vol, hvol


def test_dense_after_load_dense_returns_the_input(gpu_device):
    vol, hvol = _loaded(gpu_device, "M2")
    t, w, c = hvol.dense()
    assert _same_bits(t, vol.tsdf) and _same_bits(w, vol.weight) and _same_bits(c, vol.color)
    assert np.array_equal(hvol.allocated.cpu().numpy().reshape(vol.units).astype(bool), vol.allocated)


@pytest.mark.parametrize("name", tu.MC_NAMES)
def test_marching_cubes_of_the_named_volumes_against_the_oracle(gpu_device, name):
    """M1 every cube case; M2 holes, a unit never opened, a unit opened and empty; M3 the scan's carry past 1024 units; M4 exact
    zeros of both signs and saturated values; M5 a sign change on the first / last voxel of the box, and none at all."""
    vol, hvol = _loaded(gpu_device, name)
    want = tu.mc_oracle_mesh(name)
    _mesh_against_oracle(hvol, want)
    if name == "M3":
        assert int(np.prod(vol.units)) > 1024 and len(want[2]) > 0


def test_emit_writes_nothing_at_or_past_the_counts_it_is_given(gpu_device):
    """include/ga_tsdf.h: "nothing is written past" the counts.  A vertex is written iff its index is below the count; the triangles
    of a cube are written iff all of them fit; what is written is the full mesh's value."""
    vol, hvol = _loaded(gpu_device, "M2")
    ov, oc, ot = tu.mc_oracle_mesh("M2")
    raw, (fv, fc, ft), _ = _mesh_against_oracle(hvol, (ov, oc, ot))
    nv, nt = len(fv), len(ft)
    for pv, pt in ((nv - 1, nt - 1), (0, nt), (nv, 0)):
        fresh = RawMesh(hvol)                                          # (a scratch no earlier emit has left anything in)
        assert fresh.count() == (nv, nt)
        v, c, t = fresh.emit(pv, pt, nv, nt)
        assert np.isnan(v[pv:]).all() and np.isnan(c[pv:]).all() and (t[pt:] == -1).all(), (pv, pt)
        assert _same_bits(v[:pv], fv[:pv]) and _same_bits(c[:pv], fc[:pv]), (pv, pt)
        written = (t != -1).all(1)
        assert np.array_equal(written, (t != -1).any(1)) and np.array_equal(t[written], ft[written]), (pv, pt)
        # all of a cube's triangles or none: at most the four before the last cube's last one are held back
        assert written[:max(pt - 5, 0)].all(), (pv, pt)


# ---- integration ---------------------------------------------------------------------------------------------------------------
def _volume_against_oracle(ovol, hvol):
    t, w, c = hvol.dense()
    alloc = hvol.allocated.cpu().numpy().reshape(ovol.units).astype(bool)
    return tu.check_volume((t, w, c, alloc), (ovol.tsdf, ovol.weight, ovol.color, ovol.allocated))


def _mesh_of_fused_volume_against_oracle(ovol, hvol):
    # same volume on both sides, so that a last-bit difference of the fusion cannot flip a sign: the HIP volume is the input
    t, w, c = hvol.dense()
    ovol.tsdf[:], ovol.weight[:], ovol.color[:] = t, w, c
    want = otsdf.extract_mesh(ovol)
    assert len(want[2]) > 500
    _mesh_against_oracle(hvol, want)


def _scene_frames(eyes, H=48, W=80, fx=70.0, fy=62.0, off=(3.5, -3.25), **kw):
    kw.setdefault("sphere", (CENTRE, 0.15))
    kw.setdefault("plane", ((0.0, 0.0, -0.3), (0.0, 0.0, 1.0)))
    return tu.analytic_frames(eyes, kw.pop("target", CENTRE), H, W, fx, fy, (W - 1) / 2 + off[0], (H - 1) / 2 + off[1], **kw)


EYES = [(1.0, 0.3, 0.7), (-0.6, 0.9, 0.5), (0.2, -1.1, 0.6), (-0.8, -0.5, 0.9), (0.9, -0.6, 0.3), (0.1, 0.2, 1.3)]


def _fuse(dev, frames, **kw):
    return tu.fuse_both(dev, frames, BOX["units"], BOX["unit0"], BOX["voxel"], BOX["trunc"], **kw)


@pytest.mark.parametrize("stride", (3, 1, 7))
def test_fusion_with_other_strides_intrinsics_and_no_alpha(gpu_device, stride):
    """H != W, fx != fy, the principal point 3-4 px off the centre, alpha = NULL; every stride-th pixel opens units"""
    frames = _scene_frames(EYES[:2])
    for f in frames:
        f["alpha"] = None
    ovol, hvol = _fuse(gpu_device, frames, stride=stride)
    assert ovol.weight.max() == 2 and 4 < ovol.allocated.sum() < 60
    _volume_against_oracle(ovol, hvol)
    if stride == 3:
        _mesh_of_fused_volume_against_oracle(ovol, hvol)


def test_fusion_from_a_camera_inside_the_box(gpu_device):
    """the camera sits in a unit its own frame opens: voxels behind it (pc[2] <= 0) and voxels that project outside the image"""
    H, W, fx, fy = 64, 64, 40.0, 40.0
    frames = tu.analytic_frames([(0.3, 0.02, -0.1)], (0.4, 0.0, -0.16), H, W, fx, fy, 31.5, 31.5, plane=((0.36, 0.0, 0.0), (-1.0, 0.0, 0.0)))
    ovol, hvol = _fuse(gpu_device, frames)
    # on the host, from the extrinsic: the voxel centres of the opened units in camera space
    ext = frames[0]["ext"]
    idx = [(np.arange(16 * n) + 0.5) * BOX["voxel"] + u0 * 16 * BOX["voxel"] for n, u0 in zip(BOX["units"], BOX["unit0"])]
    p = np.stack(np.meshgrid(*idx, indexing="ij"), -1)
    opened = np.repeat(np.repeat(np.repeat(ovol.allocated, 16, 0), 16, 1), 16, 2)
    pc = p[opened] @ ext[:3, :3].T + ext[:3, 3]
    front = pc[:, 2] > 1e-3
    u = pc[front, 0] * fx / pc[front, 2] + 31.5
    assert ovol.allocated.any() and (pc[:, 2] < -1e-3).sum() > 100 and ((u < -1) | (u > W + 1)).sum() > 100
    assert ovol.weight.max() == 1
    _volume_against_oracle(ovol, hvol)


def test_fusion_with_degenerate_depth_and_alpha_at_the_threshold(gpu_device):
    """patches of depth 0, -1, NaN, +inf, depth_trunc itself and the float below it; alpha at alpha_thres and one ulp below"""
    frames = _scene_frames(EYES[:2], depth_trunc=1.25)                 # (the truncation depth cuts through the scene)
    thres = np.float32(0.08)
    for k, f in enumerate(frames):
        d, a = f["depth"], f["alpha"]
        assert (d > 1.25).any() and ((d > 0) & (d < 1.25)).any()
        a[:] = 1.0
        for i, val in enumerate((0.0, -1.0, np.nan, np.inf, np.float32(1.25), np.nextafter(np.float32(1.25), np.float32(0)))):
            d[4 + 7 * i:9 + 7 * i, 6 + 9 * k:30 + 9 * k] = val
        d[8:40, 50:53] = np.float32(1.25)
        d[8:40, 53:56] = np.nextafter(np.float32(1.25), np.float32(0))
        a[6:44, 58:64] = thres
        a[6:44, 64:70] = np.nextafter(thres, np.float32(0))
    with np.errstate(invalid="ignore", over="ignore"):
        ovol, hvol = _fuse(gpu_device, frames, alpha_thres=0.08)
    assert np.isfinite(ovol.tsdf).all() and np.isfinite(ovol.color).all() and ovol.weight.max() == 2
    _volume_against_oracle(ovol, hvol)


def test_fusion_of_colours_outside_the_unit_interval_and_on_8_bit_boundaries(gpu_device):
    frames = _scene_frames(EYES[:2])
    ks = np.array([0, 1, 2, 3, 7, 64, 127, 128, 200, 254, 255], np.float32)
    for f in frames:
        rgb = f["rgb"]
        rgb[:] = np.float32(1.7) * rgb - np.float32(0.3)
        assert rgb.min() < 0 and rgb.max() > 1
        on = (ks / np.float32(255.0)).astype(np.float32)
        band = np.concatenate([np.nextafter(on, np.float32(-1)), on, np.nextafter(on, np.float32(2))])      # k/255 and its two neighbours
        rows = slice(12, 36)
        rgb[:, rows, 20:20 + len(band)] = band[None, None, :]
        rgb[1, rows, 20:20 + len(band)] = band[None, ::-1]
    ovol, hvol = _fuse(gpu_device, frames)
    assert len(np.unique(ovol.color[:, ovol.weight == 1])) > 50
    _volume_against_oracle(ovol, hvol)


def test_fusion_of_a_scene_larger_than_the_box_on_all_six_sides(gpu_device):
    """depth points beyond every face of the box (the clipping of the unit range), truncation bands that only reach in from outside,
    and a frame that sees nothing inside: it opens no unit and changes nothing"""
    wide = dict(H=64, W=64, fx=30.0, fy=34.0, off=(1.0, -2.0), sphere=None)
    frames = _scene_frames([(0.1, 0.05, 1.0)], plane=((0, 0, -0.1), (0, 0, 1.0)), **wide)                      # beyond -x +x -y +y
    frames += _scene_frames([(1.1, 0.05, -0.1)], plane=((0.1, 0, 0), (1.0, 0, 0)), **wide)                     # beyond -y +y -z +z
    frames += _scene_frames([(0.1, 0.05, 1.4)], plane=((0, 0, 0.45), (0, 0, 1.0)), **wide)                     # above the box, band reaches in
    frames += _scene_frames([(-1.2, 0.05, -0.1)], plane=((-0.23, 0, 0), (-1.0, 0, 0)), **wide)                 # beside it, band reaches in
    for f, axes in zip(frames[:2], ((0, 1), (1, 2))):
        z = f["depth"].astype(np.float64)
        v, u = np.meshgrid(np.arange(64.0), np.arange(64.0), indexing="ij")
        fx, fy, cx, cy = f["intr"]
        pw = (np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z, np.ones_like(z)], -1) @ np.linalg.inv(f["ext"]).T)[..., :3][z > 0]
        lo = [u0 * 0.2 for u0 in BOX["unit0"]]
        hi = [(u0 + n) * 0.2 for u0, n in zip(BOX["unit0"], BOX["units"])]
        for k in axes:
            assert (pw[:, k] < lo[k] - 0.1).any() and (pw[:, k] > hi[k] + 0.1).any(), k
    ovol, hvol = _fuse(gpu_device, frames)
    assert ovol.allocated[:, :, 4].any() and ovol.allocated[0].any() and not ovol.allocated.all()
    figures = _volume_against_oracle(ovol, hvol)
    before = [x.copy() for x in hvol.dense()] + [hvol.allocated.cpu().numpy().copy()]
    nothing = _scene_frames([(0.1, 0.05, 1.0)], plane=((0, 0, -2.0), (0, 0, 1.0)), depth_trunc=10.0, **wide)
    assert (nothing[0]["depth"] > 0).sum() > 1000
    touched = otsdf.integrate(ovol, nothing[0]["rgb"], nothing[0]["depth"], nothing[0]["alpha"], 0.08, 10.0, nothing[0]["intr"], nothing[0]["ext"])
    f = nothing[0]
    hvol.integrate(torch.from_numpy(f["rgb"]), torch.from_numpy(f["depth"]), f["intr"], f["ext"], 10.0, alpha=torch.from_numpy(f["alpha"]),
                   alpha_thres=0.08)
    assert not touched.any() and int(hvol.touched.sum()) == 0
    after = list(hvol.dense()) + [hvol.allocated.cpu().numpy()]
    assert all(_same_bits(a, b) for a, b in zip(before, after))
    assert figures["tsdf"] <= tu.TSDF_BAR


def test_fusion_of_six_frames_of_one_scene_and_its_mesh(gpu_device):
    frames = _scene_frames(EYES, H=64, W=64, fx=75.0, fy=75.0, off=(0.0, 0.0))
    ovol, hvol = _fuse(gpu_device, frames)
    assert ovol.weight.max() == 6
    _volume_against_oracle(ovol, hvol)
    _mesh_of_fused_volume_against_oracle(ovol, hvol)
