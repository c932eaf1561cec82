"""The cache policy of the forward's global stores (GaSurfelForwardArgs.flags bits 4..11, include/ga_surfel.h) must not change a
single bit: every case renders the same input with all sites plain and with the policy under test -- every site write-through,
every site non-temporal, and the library's default combination -- and compares colour, radii, allmap, tile ranges, point lists and
tile rects with torch.equal; the result under the policy is also held to the CPU oracle with the bars of tests/test_surfel_gpu.py
(bit-identical bins, pixel MSE <= 1e-5).

Shapes are the smallest that reach every store site: 16-byte and per-lane background stores of the sort launch (whole and partial
tiles, empty tiles), wave-sorted and LDS-sorted lists, unsegmented, wrapping and segmented items of the blend (the last writer of a
segmented tile), the transmittance table of a differentiable forward, and the workspace head a forward leaves for the next one."""
import functools

import numpy as np
import pytest
import torch

from gaussiananything_amd import _lib, synthetic
from tests import _util
from tests.test_surfel_gpu import _compare_view

pytestmark = pytest.mark.gpu

PLAIN = _lib.store_flags(0, 0, 0, 0)
POLICIES = {"write_through": _lib.store_flags(1, 1, 1, 1), "nontemporal": _lib.store_flags(2, 2, 2, 2),
            "default": _lib.GA_SURFEL_STORE_DEFAULT}
BG = (0.25, 0.5, 0.75)


def _small_object(n, seed):
    g = synthetic.random_surfels(n, seed=seed)[0].clone()
    g[:, :3] = g[:, :3] * 0.3 + 0.1           # most of the image is background: empty tiles
    return g


def _segmented_scene():
    """the 'very long lists beside short ones' scene of tests/test_surfel_gpu.py at a third of its size: one clump with lists of
    2048 entries and more (blended in segments), a neighbouring one with lists of 513 .. 2047 (the wrapping ring), a sparse rest"""
    dense = synthetic.random_surfels(3600, seed=21)[0].clone()
    dense[:, 0:3] *= 0.04
    mid = synthetic.random_surfels(1500, seed=22)[0].clone()
    mid[:, 0:3] = mid[:, 0:3] * 0.08 + torch.tensor([0.25, 0.2, 0.0])
    sparse = synthetic.random_surfels(500, seed=23)[0].clone()
    g = torch.cat([dense, mid, sparse], 0)
    g[:, 3] = 0.004 + 0.02 * torch.rand(g.shape[0], generator=torch.Generator().manual_seed(17))
    return g


SCENES = {
    "surface_64x64": (lambda: synthetic.surface_surfels(4096, seed=1)[0], [0, 3], 64, 64),
    "surface_72x40": (lambda: synthetic.surface_surfels(4096, seed=1)[0], [0, 3], 40, 72),     # partial tiles at both edges
    "small_object_72x40": (lambda: _small_object(400, 4), [0, 2], 40, 72),                    # empty tiles, whole and partial
    "segmented_96x96": (_segmented_scene, [0, 3], 96, 96),
}


def _render(g, views, H, W, device, flags):
    from gaussiananything_amd.diff_surfel_rasterization import SurfelForwardPlan
    cams = synthetic.eval_cameras(8)
    m, o, s, r, c = [t.to(device) for t in synthetic.split_gaussians(g)]
    plan = SurfelForwardPlan(m, o, c, s, r, cams["cam_view"][views].to(device), cams["cam_view_proj"][views].to(device),
                             torch.tensor(BG, device=device), H, W, flags=flags)
    plan.color.fill_(-7.0)
    plan.allmap.fill_(-7.0)
    plan.run()
    plan.ensure_capacity()
    torch.cuda.synchronize()
    return plan


def _outputs(plan):
    """what a forward leaves: (colour, radii, allmap, tile_start, point_list[:D], rect), status words"""
    st = plan.ws.status().cpu()
    assert int(st[_lib.GA_STATUS_OVERFLOW]) == 0
    tiles = ((plan.w + 15) // 16) * ((plan.h + 15) // 16)
    D = int(st[_lib.GA_STATUS_NUM_RENDERED])
    out = (plan.color.clone(), plan.radii.clone(), plan.allmap.clone(),
           plan.ws.section("tile_start", torch.int32, plan.v * tiles + 1).clone(),
           plan.ws.section("point_list", torch.int32, max(D, 1))[:D].clone(),
           plan.ws.section("rect", torch.int16, plan.v * plan.n * 4).clone())
    return out, st


NAMES = ("color", "radii", "allmap", "tile_start", "point_list", "rect")


def _assert_same(a, b, what):
    for name, x, y in zip(NAMES, a, b):
        assert x.shape == y.shape and torch.equal(x, y), f"{what}: {name} differs"


@functools.lru_cache(maxsize=None)
def _reference(scene, device):
    """the all-plain render and the oracle's views of a scene: computed once, shared by the policies, never modified"""
    make, views, H, W = SCENES[scene]
    g = make()
    out, st = _outputs(_render(g, views, H, W, device, PLAIN))
    cams = synthetic.eval_cameras(8)
    oracle = [_util.oracle_view(g, cams, v, H, W, bg=BG) for v in views]
    return g, out, st, oracle


@pytest.mark.parametrize("policy", list(POLICIES))
@pytest.mark.parametrize("scene", list(SCENES))
def test_store_policy_changes_no_bit_and_matches_the_oracle(gpu_device, scene, policy):
    make, views, H, W = SCENES[scene]
    g, ref, st, oracle = _reference(scene, gpu_device)
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    counts = np.diff(ref[3].cpu().numpy().astype(np.int64))
    if scene == "small_object_72x40":
        assert int((counts == 0).sum()) > 0, "no empty tile: the background stores of the sort launch are not reached"
    if scene == "segmented_96x96":
        assert int(st[7]) > 0 and int(st[_lib.GA_STATUS_SEG_WORK]) > 0, "no tile was blended in segments"   # GA_STATUS_LONG_TILES
        assert int(counts.max()) >= 2048 and int(((counts > 512) & (counts < 2048)).sum()) > 0
    plan = _render(g, views, H, W, gpu_device, POLICIES[policy])
    got, st2 = _outputs(plan)
    _assert_same(got, ref, f"{scene} / {policy}")
    assert torch.equal(st2[:4], st[:4])
    assert float((got[2] == -7.0).sum()) == 0 and float((got[0] == -7.0).sum()) == 0          # every pixel written
    art = _util.ws_artifacts(plan.ws, g.shape[0], len(views), H, W)
    color, radii, allmap = got[0].cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy()
    for k in range(len(views)):
        _compare_view(oracle[k], color[k], radii[k], allmap[k], art, k, g.shape[0], tiles)


def _differentiable_forward(g, vm, pm, bg, H, W, device, monkeypatch, flags):
    """forward with the transmittance table (the blend's STORE instantiation) on a workspace of the test's own, whose table is
    pre-filled so that the rows no segment owns compare equal; then one backward through the autograd path under the same flags"""
    from gaussiananything_amd import diff_surfel_rasterization as dsr
    monkeypatch.setattr(dsr, "EXTRA_FLAGS", flags)
    m, op, sc, rot, rgb = [t.to(device) for t in synthetic.split_gaussians(g)]
    n, v = m.shape[0], vm.shape[0]
    ws = dsr.SurfelWorkspace(device, n, v, H, W, dsr.default_capacity(n, v))
    dsr._seg_T(ws).fill_(-9.0)
    with torch.no_grad():
        color, radii, allmap, _ = dsr._rasterize_views_nograd(m, op, rgb, sc, rot, vm, pm, bg, H, W, workspace=ws, for_backward=True)
    torch.cuda.synchronize()
    seg_T = ws.seg_T.clone()
    leaves = [t.detach().clone().requires_grad_(True) for t in (m, op, rgb, sc, rot)]
    c1, r1, a1, _ = dsr.rasterize_views(*leaves, vm, pm, bg, H, W)
    assert torch.equal(c1, color) and torch.equal(a1, allmap) and torch.equal(r1, radii)
    gen = torch.Generator(device="cpu").manual_seed(5)
    wc = torch.rand(c1.shape, generator=gen).to(device)
    wo = torch.rand(a1.shape, generator=gen).to(device)
    ((c1 * wc).sum() + (a1 * wo).sum()).backward()
    torch.cuda.synchronize()
    return color, radii, allmap, seg_T, [t.grad.clone() for t in leaves]


@functools.lru_cache(maxsize=None)
def _differentiable_reference(device):
    """two all-plain differentiable forwards + backwards of the same scene (the second one tells whether the backward repeats itself)"""
    cams = synthetic.eval_cameras(8)
    g = synthetic.surface_surfels(4096, seed=1)[0]
    vm, pm = cams["cam_view"][[0, 3]].to(device), cams["cam_view_proj"][[0, 3]].to(device)
    bg = torch.tensor(BG, device=device)
    with pytest.MonkeyPatch.context() as mp:
        runs = [_differentiable_forward(g, vm, pm, bg, 64, 64, device, mp, PLAIN) for _ in range(2)]
    return g, vm, pm, bg, runs


@pytest.mark.parametrize("policy", list(POLICIES))
def test_differentiable_forward_hands_over_the_same_transmittances_and_gradients(gpu_device, monkeypatch, policy):
    """seg_T (the 4-byte stores of the blend's STORE instantiation) and everything else the backward reads are bit-identical, and one
    backward from them gives the gradients of the all-plain run.

    Bit-identical gradients are asserted whenever the backward repeats itself bit for bit on two all-plain runs.  It does not
    always: ga_surfel_backward sums a Gaussian's contributions with fp32 atomics (LDS and global), in the order the waves arrive
    -- measured on an MI355X, this scene: two runs on bit-identical inputs differ by up to 7.6e-06 in grad means3D, one ulp of its
    largest elements (87).  The backward is outside this change.  When the two all-plain runs differ, the gradients under the
    policy are held to the same sums in another order instead: every element within 8 ulp of the tensor's largest magnitude
    (2^-23 * 8 * max |gradient|: a wrong or missing contribution of this scene is five orders of magnitude above that)."""
    g, vm, pm, bg, (ref, ref2) = _differentiable_reference(gpu_device)
    got = _differentiable_forward(g, vm, pm, bg, 64, 64, gpu_device, monkeypatch, POLICIES[policy])
    assert float((ref[3] != -9.0).sum()) > 0
    for name, a, b in zip(("color", "radii", "allmap", "seg_T"), got[:4], ref[:4]):
        assert torch.equal(a, b), name
    repeats = all(torch.equal(a, b) for a, b in zip(ref[4], ref2[4]))
    for name, a, b, b2 in zip(("means3D", "opacities", "colors", "scales", "rotations"), got[4], ref[4], ref2[4]):
        assert torch.isfinite(a).all()
        print(f"{policy}: grad {name} max |policy - plain| {float((a - b).abs().max()):.3e}, max |plain - plain again| "
              f"{float((b2 - b).abs().max()):.3e}, max |gradient| {float(b.abs().max()):.3e}")
        if repeats:
            assert torch.equal(a, b), f"gradient of {name} differs"
        else:
            assert float((a - b).abs().max()) <= 8 * 2.0 ** -23 * float(b.abs().max()), f"gradient of {name} differs"


@pytest.mark.parametrize("policy", list(POLICIES))
def test_second_forward_on_a_clean_workspace_equals_a_fresh_workspace(gpu_device, policy):
    """Two forwards on one workspace, the second with GA_SURFEL_FLAG_WORKSPACE_CLEAN (no clearing memset) and on different
    Gaussians: every store of the first -- the words its sort launch leaves cleared included -- must have landed before the second
    one's first launch reads the workspace head."""
    views, H, W = [0, 3], 72, 72
    g1 = synthetic.surface_surfels(4096, seed=1)[0]
    g2 = _small_object(4096, 8)
    fresh, _ = _outputs(_render(g2, views, H, W, gpu_device, PLAIN))
    plan = _render(g1, views, H, W, gpu_device, POLICIES[policy])
    first, _ = _outputs(plan)
    _assert_same(first, _outputs(_render(g1, views, H, W, gpu_device, PLAIN))[0], f"first forward / {policy}")
    for dst, src in zip((plan.means3D, plan.opacities, plan.colors, plan.scales, plan.rotations),
                        [synthetic.split_gaussians(g2)[i] for i in (0, 1, 4, 2, 3)]):
        dst.copy_(src.to(gpu_device).reshape(dst.shape))
    assert plan._args.flags & _lib.GA_SURFEL_FLAG_WORKSPACE_CLEAN
    plan.color.fill_(-7.0)
    plan.allmap.fill_(-7.0)
    plan.run()
    torch.cuda.synchronize()
    second, _ = _outputs(plan)
    _assert_same(second, fresh, f"second forward on the used workspace / {policy}")
