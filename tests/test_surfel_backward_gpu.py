"""ga_surfel_backward held row by row to the float64 autograd oracle (oracle/surfel_autograd.py), on every kernel path.

The bars are those of tests/_bwd_bars.py: per surfel err_i <= 1e-3 (|ref_i| + s) on each of the five gradient tensors, no unnamed
exception, beside the whole-tensor relative L2 bar of 2e-4 the backward has always had.  Every case asserts from the forward's integer
artefacts (list lengths, the status word, the cull boxes) that it is on the path it names.  What each case is for:

  one output-channel group at a time     colour, depth, alpha, normal, median depth, distortion: the small terms (gDist (m^2 W - 2 m M1
                                         + M2), the cross-segment prefix P_start, gMedian) are not hidden inside the colour term's norm
  opaque                                 the 0.99 clamp (no gradient above it), walks that end at T (1 - alpha) < 1e-4, lists of 460 ..
                                         600 entries (the forward's wrapping LDS image, beyond 512)
  long_transparent / long_mixed          2200 entries in one list: the forward blends in segments across workgroups (from 2048 on)
                                         and its STORE instantiation writes seg_T per segment; both with and without that table
                                         (GA_SURFEL_SEG_T=0: the trans and prefix_T launches of the backward)
  seams                                  lists of exactly 127, 128, 129, 256, 257 entries: slot 127 / 128 of a segment, a last segment
                                         of one entry
  kernel selection                       pair-major surfel_bwd_grad_kernel against surfel_bwd_grad_big_kernel, and the lane-major
                                         against the entry-major walk of a wave inside the latter, asserted by a host restatement
  chain rule                             scale_modifier != 1, three views with surfels culled in some of them, N = 1 and N = 257
  linearity, repeatability               twice the upstream gradient, a zero one, two backwards through one retained node
"""
import numpy as np
import pytest
import torch

from gaussiananything_amd import synthetic
from tests import _bwd_bars as bb
from tests import _util
from tests.test_surfel_gpu import _backward_case

pytestmark = pytest.mark.gpu


def _case(gpu_device, name, **kw):
    args, edit = bb.SCENES[name]
    return _backward_case(gpu_device, **args, edit=edit, label=name, **kw)


def _forward_facts(gpu_device, name, scale_modifier=1.0):
    """The scene through the inference forward (same lists and images as the differentiable call, bit for bit --
    test_forward_of_a_differentiable_call_equals_...): the workspace artefacts, radii, allmap, and the C oracle's view records."""
    sc = bb.named_scene(name)
    g, cams = bb.gaussians(sc), synthetic.eval_cameras(8)
    color, radii, allmap, ws = _util.hip_views(g, cams, sc["views"], sc["H"], sc["W"], gpu_device, bg=(0.3, 0.6, 0.1),
                                               scale_modifier=scale_modifier)
    art = _util.ws_artifacts(ws, sc["n"], len(sc["views"]), sc["H"], sc["W"])
    assert art["overflow"] == 0
    oracle = [_util.oracle_view(g, cams, v, sc["H"], sc["W"], bg=(0.3, 0.6, 0.1), scale_modifier=scale_modifier) for v in sc["views"]]
    return sc, art, radii.cpu().numpy(), allmap.cpu().numpy(), oracle


def _walks_that_ended_early(o):
    """pixels of one oracle view whose walk stopped (T (1 - alpha) < 1e-4) before the end of their tile's list"""
    H, W = o["n_walked"].shape
    gx = (W + 15) // 16
    ys, xs = np.mgrid[0:H, 0:W]
    length = (o["ranges"][:, 1].astype(np.int64) - o["ranges"][:, 0].astype(np.int64))[(ys // 16) * gx + xs // 16]
    return int(np.count_nonzero(o["n_walked"] < length))


# ---- a. one output-channel group at a time --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["six", "medium"])
def test_backward_one_output_channel_group_at_a_time(gpu_device, name):
    """One oracle forward and one HIP forward, six backwards through each: every group of upstream gradients on its own, so that
    the distortion and median-depth terms (orders of magnitude below the colour term) answer for themselves.  Where a group cannot
    reach a tensor (the colours under anything but the colour gradient, the opacities under the median depth) it must stay zero."""
    refs, _, figures = _case(gpu_device, name, masks=tuple(bb.GROUPS.values()))
    for group, (_, ref) in zip(bb.GROUPS, refs):
        zero = {n for n, g in zip(bb.NAMES, ref) if float(g.abs().max()) == 0.0}
        assert zero == ({"colors"} if group not in ("colour", "median") else {"opacities", "colors"} if group == "median" else set())
        if group == "median":     # (and no scale moves the depth at which a ray meets the splat's plane: 1e-16 in float64, not 0)
            assert float(ref[3].abs().max()) <= bb.ZERO_REF * float(ref[0].norm(dim=1).max())
        assert float(ref[0].abs().max()) > 0


# ---- b. opaque surfels: the clamp and the end of a walk ----------------------------------------------------------------------------
def test_backward_opaque_surfels_clamp_and_walk_end(gpu_device):
    """600 surfels of opacity 0.2 .. 1.0 in four tiles, two views, eight of them at opacity exactly 1.0: lists of 460 .. 600 entries
    (the wrapping forward path above 512), pairs above the 0.99 clamp that do take part in the blend, walks that end early."""
    sc, art, radii, allmap, oracle = _forward_facts(gpu_device, "opaque")
    lengths = np.diff(art["tile_start"])
    assert lengths.min() >= 460 and lengths.max() <= 600 and (lengths > 512).sum() >= 6, lengths
    clamped = [p for o in oracle for p in bb.contributing_pairs_above_the_clamp(o, bb.EIGHT_OPAQUE, sc["W"])]
    assert len(clamped) >= 1, "no pair above the 0.99 clamp takes part in the blend"
    assert sum(_walks_that_ended_early(o) for o in oracle) >= 16
    # a walk that ends leaves T in [1e-4, 1e-4 / (1 - alpha)): alpha = 1 - T comes to 0.9999 from below and, T >= 1e-4 being what the
    # stop rule keeps, never reaches the fp32 number 0.9999 itself -- the oracle's maximum here is 0.99989975
    assert float(allmap[:, 1].max()) > 0.99989 and max(float(o["allmap"][1].max()) for o in oracle) > 0.99989
    _case(gpu_device, "opaque")


# ---- c. lists beyond 2048 entries ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg_t", ["1", "0"])
@pytest.mark.parametrize("name", bb.LONG)
def test_backward_lists_beyond_2048_entries_with_and_without_the_transmittance_table(gpu_device, monkeypatch, name, seg_t):
    """One tile, 2200 surfels, all in its list: the forward blends it in segments across workgroups and (GA_SURFEL_SEG_T=1) leaves
    the per-segment transmittances for the backward, which otherwise (=0) forms them in two launches of its own.  Both against the
    same frozen float64 reference (tests/golden/surfel_bwd_long_ref.pt).  "transparent": every segment seam is crossed alive by every
    pixel; "mixed": walks end inside early segments."""
    from gaussiananything_amd import diff_surfel_rasterization as dsr
    monkeypatch.setenv("GA_SURFEL_SEG_T", seg_t)
    dsr.clear_workspaces()                       # (a pooled workspace keeps the table it was given under another setting)
    sc, art, radii, allmap, (o,) = _forward_facts(gpu_device, name)
    assert np.diff(art["tile_start"]).tolist() == [2200] and art["max_tile"] >= 2048
    if name == "long_transparent":
        assert float(allmap[0, 1].max()) < 0.9999 and _walks_that_ended_early(o) == 0
    else:
        assert float(allmap[0, 1].max()) > 0.99989 and int(o["n_walked"].min()) < 128      # a walk that ends inside the first segment
    z = torch.load(synthetic.fixture_path(bb.LONG_FIXTURE))[name]
    assert z["args"] == bb.SCENES[name][0]
    _case(gpu_device, name, refs=[(z["loss"], z["grads"])])
    dsr.clear_workspaces()


# ---- d. segment seams --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [127, 128, 129, 256, 257])
def test_backward_segment_seams(gpu_device, n):
    """Lists of exactly n entries in one tile: the last slot of a 128-entry segment, a segment that is exactly full, a last segment
    of one entry -- transparent enough (max alpha below 0.9) that every pixel crosses the seams alive."""
    sc, art, radii, allmap, (o,) = _forward_facts(gpu_device, f"seam{n}")
    assert np.diff(art["tile_start"]).tolist() == [n]
    assert float(allmap[0, 1].max()) < 0.95 and _walks_that_ended_early(o) == 0
    _case(gpu_device, f"seam{n}")


# ---- e. which gradient kernel ran ----------------------------------------------------------------------------------------------------
def _segments(gpu_device, name):
    sc, art, _, allmap, _ = _forward_facts(gpu_device, name)
    segs = bb.segment_pair_counts(art, (sc["W"] + 15) // 16)
    for s in segs:
        print(name, {k: s[k] for k in ("view", "tile", "k", "entries", "pairs", "big")}, s["waves"] if s["big"] else "")
    return segs, allmap


def test_which_gradient_kernel_the_segments_of_the_backward_scenes_take(gpu_device):
    """The host restatement of the rule of surfel_bwd_sums_kernel (a segment whose cull boxes hold more than 2528 (pixel, entry)
    pairs goes to surfel_bwd_grad_big_kernel) on the scenes whose docstrings name a path: the six large surfels are pair-major, the
    60 large ones take grad_big only.  The 300 medium surfels are pair-major throughout: 1045 list entries of 6 pairs each on
    average, no segment beyond 900 pairs -- their test's docstring claimed both kernels, counting a surfel's ~25 pairs as an entry's.
    "both_kernels" is the scene that has segments on either side of the capacity in one launch."""
    six, _ = _segments(gpu_device, "six")
    assert six and not any(s["big"] for s in six)
    large, _ = _segments(gpu_device, "large60")
    assert len(large) == 4 and all(s["big"] for s in large)
    medium, _ = _segments(gpu_device, "medium")
    assert len(medium) >= 8 and not any(s["big"] for s in medium) and max(s["pairs"] for s in medium) < 1000
    both, _ = _segments(gpu_device, "both_kernels")
    assert any(s["big"] for s in both) and any(not s["big"] and s["pairs"] > 2000 for s in both)
    # away from the capacity by more than the few pairs a cull box's rounding can move
    assert all(abs(s["pairs"] - bb.PAIR_CAP) > 32 for s in six + large + medium + both)


@pytest.mark.parametrize("name", ["large60", "both_kernels"])
def test_backward_waves_of_grad_big_walk_lane_major_and_entry_major(gpu_device, name):
    """Inside surfel_bwd_grad_big_kernel a wave (an 8 x 8 quadrant of the tile) walks a 64-entry half entry-major when its pixels
    evaluate an entry 12 at a time on average, lane-major otherwise.  Both walks occur in these scenes, by the restatement (valid
    while no pixel has finished: lists of at most 64 entries, entered with T = 1), and their gradients keep the bars."""
    segs, allmap = _segments(gpu_device, name)
    assert max(s["entries"] for s in segs) <= 64
    walks = [w for s in segs if s["big"] for w in s["waves"]]
    # (counted only where a cull box's rounding cannot move the wave across the switch: 16 pairs or more away from it)
    clear = {w[2] for w in walks if abs(w[3] - bb.WAVE_MAJOR_LANES * w[4]) >= 16}
    assert clear == {"entry", "lane"}, walks
    _case(gpu_device, name)


# ---- f. the chain-rule kernel --------------------------------------------------------------------------------------------------------
def test_backward_with_a_scale_modifier(gpu_device):
    refs, _, _ = _case(gpu_device, "six", scale_modifier=1.7)
    plain, _ = bb.oracle_gradients(bb.named_scene("six"))
    assert bb.whole_tensor_error(plain[0][1][3], refs[0][1][3]) > 0.1      # (the modifier does reach the reference)


def test_backward_sums_three_views_with_surfels_culled_in_some(gpu_device):
    """Views 0, 3, 6 of a ragged 40 x 24 image, 200 surfels; the first 20 lie where at least one view culls them (radius 0) and at
    least one renders them: surfel_preprocess_bwd_kernel sums the views in registers and must skip exactly the culled ones."""
    sc, art, radii, allmap, oracle = _forward_facts(gpu_device, "three_views")
    seen = radii[:, :bb.CULLED] > 0
    assert bool((seen.any(0) & ~seen.all(0)).all()), seen.sum(0)
    assert bool((radii[:, bb.CULLED:] > 0).sum(0).min() >= 1)
    refs, _, _ = _case(gpu_device, "three_views")
    assert bool((refs[0][1][0][:bb.CULLED].norm(dim=1) > 0).all())             # each of them does receive a gradient


@pytest.mark.parametrize("name", ["one", "n257"])
def test_backward_grid_edges_of_the_per_surfel_launches(gpu_device, name):
    """N = 1 and N = 257: a first block with one thread in use, and a second block of the 256-thread chain-rule launch with one."""
    _case(gpu_device, name)


# ---- g. linearity and repeatability --------------------------------------------------------------------------------------------------
def test_backward_is_linear_in_the_upstream_gradient_and_repeatable(gpu_device):
    """On the 300-surfel scene: twice the upstream gradient gives twice every gradient and a second backward through the retained
    node gives the first one's, both to 1e-5 (|g_i| + s) per row (the float atomics' summation order allows no more); a zero
    upstream gradient gives exactly zero."""
    from gaussiananything_amd.diff_surfel_rasterization import rasterize_views
    args, _ = bb.SCENES["medium"]
    sc, cams = bb.named_scene("medium"), synthetic.eval_cameras(8)
    n, views = sc["n"], sc["views"]
    dins = [sc[k].float().to(gpu_device).requires_grad_(True) for k in ("means", "opac", "rgb", "scales", "quats")]
    color, _, allmap, _ = rasterize_views(dins[0], dins[1][:, None], dins[2], dins[3], dins[4], cams["cam_view"][views].to(gpu_device),
                                          cams["cam_view_proj"][views].to(gpu_device), sc["bg"].float().to(gpu_device), sc["H"], sc["W"])
    wc, wa = sc["wc"].float().to(gpu_device), sc["wa"].float().to(gpu_device)
    back = lambda f: torch.autograd.grad([color, allmap], dins, [f * wc, f * wa], retain_graph=True)    # noqa: E731
    once, again, twice, nothing = back(1.0), back(1.0), back(2.0), back(0.0)
    for name, a, b, c, z in zip(bb.NAMES, once, again, twice, nothing):
        assert float(a.abs().max()) > 0
        r_again, r_twice = float(bb.row_ratios(b, a, n).max()), float(bb.row_ratios(c, 2.0 * a, n).max())
        print(f"backward medium {name}: repeated {r_again:.2e}, doubled {r_twice:.2e} (|g_i| + s)")
        assert r_again <= 1e-5 and r_twice <= 1e-5, (name, r_again, r_twice)
        assert float(z.abs().max()) == 0.0, name
