"""The row-by-row bars of the surfel backward (tests/_bwd_bars.py), without a GPU: the helper catches what the whole-tensor bar lets
through, the oracle alone stays well inside the bar, the frozen long-scene references are the oracle's, and the host restatement of
the gradient kernels' selection rule counts what it says.

Calibration (test_float32_oracle_...): oracle/surfel_autograd.py evaluated in float32 against its float64 run, per-row maxima of
err_i / (|ref_i| + s), measured here as means3D / opacities / colors / scales / rotations (no row of any scene beyond 4.1e-5):

    six                 1.2e-06 / 2.2e-07 / 2.1e-07 / 2.5e-07 / 4.1e-07        (scale_modifier 1.7: 4.6e-07 / 2.2e-07 / 2.6e-07 / 2.1e-07 / 2.7e-07)
    small400            2.2e-05 / 7.1e-06 / 4.8e-06 / 2.0e-05 / 2.7e-05
    large60             9.5e-06 / 5.6e-07 / 3.8e-07 / 5.7e-07 / 1.0e-05
    medium              6.4e-06 / 7.9e-06 / 2.6e-06 / 3.1e-06 / 1.0e-05
    both_kernels        1.9e-05 / 1.8e-06 / 5.7e-07 / 1.9e-06 / 6.8e-06
    opaque              2.4e-05 / 1.7e-05 / 3.8e-06 / 5.7e-06 / 2.4e-05
    three_views         3.8e-05 / 1.6e-06 / 1.1e-06 / 1.1e-05 / 4.0e-05
    one                 9.7e-08 / 1.7e-08 / 8.6e-08 / 9.5e-08 / 2.8e-07
    n257                5.6e-06 / 3.3e-06 / 1.5e-06 / 5.1e-06 / 4.8e-06
    seam127             3.2e-06 / 5.1e-07 / 3.2e-07 / 5.1e-06 / 6.9e-07
    seam128             2.3e-06 / 5.3e-07 / 3.2e-07 / 8.0e-06 / 1.1e-06
    seam129             3.1e-06 / 8.9e-07 / 2.8e-07 / 7.8e-06 / 5.4e-07
    seam256             2.3e-06 / 7.7e-07 / 4.1e-07 / 3.4e-06 / 5.7e-07
    seam257             2.5e-06 / 1.1e-06 / 7.7e-07 / 5.4e-06 / 7.3e-07
    long_transparent    1.6e-05 / 1.3e-06 / 5.8e-07 / 1.8e-05 / 1.0e-06
    long_mixed          6.0e-06 / 2.0e-05 / 4.2e-06 / 4.1e-05 / 3.5e-06        (not asserted here: ten more seconds)

These are runs with all ten output channels weighted at once.  With the distortion channel ALONE a plain fp32 evaluation does not
stay inside the bar: its raw moments m^2 W - 2 m M1 + M2 cancel to 1e-4 of their terms (six: 7.2e-4 on the worst row, medium:
2.1e-1).  The HIP backward takes the moments about the tile's front depth instead and is held to the bar on that channel alone by
tests/test_surfel_backward_gpu.py.
The bar of the GPU tests is 1e-3 with at most max(1, n // 500) rows beyond it; this file holds the fp32 oracle to 5e-4 with none.
"""
import functools

import numpy as np
import pytest
import torch

from gaussiananything_amd import synthetic
from tests import _bwd_bars as bb

CALIBRATION_TOL = 5e-4
CALIBRATED = ["six", "small400", "large60", "medium", "both_kernels", "opaque", "three_views", "one", "n257", "seam127", "seam128",
              "seam129", "seam256", "seam257", "long_transparent"]


@functools.lru_cache(maxsize=None)
def _reference(name, scale_modifier=1.0):
    ((loss, grads),), _ = bb.oracle_gradients(bb.named_scene(name), scale_modifier=scale_modifier)
    return loss, grads


def test_row_bars_catch_one_wrong_row_that_the_whole_tensor_bar_lets_through():
    """The gap, demonstrated on the float64 reference gradients of the 400-surfel scene: one surfel's position gradient scaled by
    1.01 passes the whole-tensor 2e-4 bar and fails the rows; so does one wrong by 10 % (the hard cap, even for a row a case names);
    n // 500 + 1 rows fail the cap on excepted rows although the case names them all; the unchanged gradients pass."""
    n = 400
    _, grads = _reference("small400")
    ref = grads[0]
    by_size = ref.norm(dim=1).argsort()
    row = int(by_size[n // 2])                                      # a row of median size
    bad = ref.clone()
    bad[row] *= 1.01
    assert bb.whole_tensor_error(bad, ref) < bb.WHOLE_TOL           # the old bar passes ...
    assert float(bb.row_ratios(bad, ref, n)[row]) > 4 * bb.ROW_TOL
    with pytest.raises(AssertionError, match="does not name"):      # ... the rows do not
        bb.row_bars(bad, ref, n)
    with pytest.raises(AssertionError, match="does not name"):
        bb.check_gradients([bad] + list(grads[1:]), grads, n)
    assert bb.row_bars(bad, ref, n, named=(row,)) == (float(bb.row_ratios(bad, ref, n)[row]), row, 1)   # a named flip is the one exception
    worse = ref.clone()
    worse[row] *= 1.1
    with pytest.raises(AssertionError, match="beyond the cap"):
        bb.row_bars(worse, ref, n, named=(row,))
    rows = by_size[n // 2:n // 2 + n // 500 + 2].tolist()
    assert len(rows) == bb.allowed_rows(n) + 1
    more = ref.clone()
    more[rows] *= 1.01
    assert bb.whole_tensor_error(more, ref) < bb.WHOLE_TOL
    with pytest.raises(AssertionError, match="rows beyond"):
        bb.row_bars(more, ref, n, named=rows)
    assert bb.row_bars(ref.clone(), ref, n) == (0.0, 0, 0)
    # the zero rule: a reference that is entirely zero admits 1e-7 of the case's largest reference row, no more
    zero = torch.zeros_like(grads[1])
    scale = max(float(g.reshape(n, -1).norm(dim=1).max()) for g in grads)
    leak = zero.clone()
    leak[7] = 2e-7 * scale
    refs = [grads[0], zero, grads[2], grads[3], grads[4]]
    bb.check_gradients([grads[0], zero.clone(), grads[2], grads[3], grads[4]], refs, n)
    with pytest.raises(AssertionError):
        bb.check_gradients([grads[0], leak, grads[2], grads[3], grads[4]], refs, n)


@pytest.mark.parametrize("name", CALIBRATED)
def test_float32_oracle_stays_inside_half_the_row_bar_without_exceptions(name):
    """oracle/surfel_autograd.py in float32 against float64 on the scenes of the GPU cases of at most 600 surfels and on one long
    scene: every row of every tensor within 5e-4 (|ref_i| + s) -- the reference alone needs neither the bar's margin nor its cap."""
    sc = bb.named_scene(name)
    _, ref = _reference(name)
    ((_, got),), _ = bb.oracle_gradients(sc, dtype=torch.float32)
    ratios = [float(bb.row_ratios(a, b, sc["n"]).max()) for a, b in zip(got, ref)]
    print(name, " / ".join(f"{r:.1e}" for r in ratios))
    assert max(ratios) <= CALIBRATION_TOL, dict(zip(bb.NAMES, ratios))
    assert all(g.dtype == torch.float32 for g in got)


def test_float32_oracle_with_a_scale_modifier():
    sc = bb.named_scene("six")
    _, ref = _reference("six", 1.7)
    ((_, got),), _ = bb.oracle_gradients(sc, scale_modifier=1.7, dtype=torch.float32)
    assert max(float(bb.row_ratios(a, b, 6).max()) for a, b in zip(got, ref)) <= CALIBRATION_TOL
    _, plain = _reference("six")
    assert bb.whole_tensor_error(plain[3], ref[3]) > 0.1           # (the modifier does reach the gradients)


def test_autograd_oracle_ends_a_walk_where_the_rasterizer_does():
    """The stop rule of the blend in oracle/surfel_autograd.py against oracle/surfel_raster.c where walks do end (the opaque scene,
    view 3): a pixel's walk ends at the first pair that would take T below 1e-4 and nothing behind it takes part.  (Skipping that
    pair alone and going on, as the autograd oracle did before the opaque cases existed, is 3.3e-3 off in alpha and 2e-3 in colour
    here; the gradients of occluded surfels moved by up to 15 %.)"""
    from oracle import surfel_autograd as oag
    from tests import _util
    sc, cams = bb.named_scene("opaque"), synthetic.eval_cameras(8)
    with torch.no_grad():
        col, am = oag.render(sc["means"], sc["opac"], sc["rgb"], sc["scales"], sc["quats"], cams["cam_view"][3].double(),
                             cams["cam_view_proj"][3].double(), sc["bg"], sc["H"], sc["W"])
    o = _util.oracle_view(bb.gaussians(sc), cams, 3, sc["H"], sc["W"], bg=(0.3, 0.6, 0.1))
    ended = o["n_walked"].reshape(2, 16, 2, 16) < (o["ranges"][:, 1] - o["ranges"][:, 0]).reshape(2, 1, 2, 1)
    assert int(ended.sum()) >= 16
    assert float(np.abs(am[1].numpy() - o["allmap"][1]).max()) < 2e-5
    assert float(np.abs(col.numpy() - o["color"]).max()) < 2e-5
    assert bb.contributing_pairs_above_the_clamp(o, bb.EIGHT_OPAQUE, sc["W"]) == [(158, 15, 15), (86, 17, 14)]


def test_frozen_long_scene_references_are_the_oracles():
    """tests/golden/surfel_bwd_long_ref.pt (make_surfel_bwd_golden.py) against a fresh float64 run of one of its two scenes."""
    z = torch.load(synthetic.fixture_path(bb.LONG_FIXTURE))
    assert set(z) == set(bb.LONG)
    for name in bb.LONG:
        assert z[name]["args"] == bb.SCENES[name][0]
        assert [tuple(g.shape) for g in z[name]["grads"]] == [(2200, 3), (2200,), (2200, 3), (2200, 2), (2200, 4)]
        assert all(g.dtype == torch.float64 and bool(torch.isfinite(g).all()) for g in z[name]["grads"])
    loss, grads = _reference("long_transparent")
    assert abs(float(loss) - z["long_transparent"]["loss"]) <= 1e-12 * abs(float(loss))
    for a, b in zip(grads, z["long_transparent"]["grads"]):
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())


def test_segment_pair_counts_restate_the_selection_rule_on_hand_made_boxes():
    """segment_pair_counts on one 16 x 16 tile with boxes whose pairs can be counted by hand: full-tile boxes (256 pairs each) on
    either side of the pair table's 2528 slots, a second segment from entry 128 on, and the per-wave rule (a wave = an 8 x 8 quadrant;
    entry-major from 12 lanes per entry on average)."""
    def art(boxes):       # boxes: (cx, cy, rx, ry) per entry, in list order
        b = np.asarray(boxes, np.float32)
        return dict(tile_start=np.array([0, len(b)]), tiles=1, point_list=np.arange(len(b)),
                    cull_centre=b[None, :, 0:2], cull_half=b[None, :, 2:4])
    full, dot = (7.5, 7.5, 8.0, 8.0), (3.0, 3.0, 0.4, 0.4)          # 16 x 16 pixels; the one pixel (3, 3)
    (s,) = bb.segment_pair_counts(art([full] * 9 + [dot] * 100), 1)
    assert (s["entries"], s["pairs"], s["big"]) == (109, 9 * 256 + 100, False)
    (s,) = bb.segment_pair_counts(art([full] * 9 + [(7.5, 7.0, 8.0, 7.0)]), 1)     # 16 columns x rows 0 .. 14: 2304 + 240 = 2544 > 2528
    assert (s["pairs"], s["big"]) == (2544, True)
    (s,) = bb.segment_pair_counts(art([full] * 9 + [(7.5, 7.5, 8.0, 7.0)]), 1)     # rows 1 .. 14: 2304 + 224 = 2528, the table is full
    assert (s["pairs"], s["big"]) == (2528, False)
    a, b = bb.segment_pair_counts(art([dot] * 128 + [full] * 10), 1)
    assert (a["entries"], a["pairs"], a["big"], b["k"], b["entries"], b["pairs"], b["big"]) == (128, 128, False, 1, 10, 2560, True)
    # waves: ten full boxes and 60 single pixels in quadrant 0, in one 64-entry half and a bit: quadrant 0 of half 0 meets 64 entries
    # with 10 x 64 + 54 pairs = 694 < 12 x 64 -- lane-major; the other quadrants meet the ten boxes only, 64 lanes each -- entry-major
    (s,) = bb.segment_pair_counts(art([full] * 10 + [dot] * 60), 1)
    assert s["big"] and s["waves"] == [(0, 0, "lane", 694, 64), (0, 1, "entry", 640, 10), (0, 2, "entry", 640, 10),
                                       (0, 3, "entry", 640, 10), (1, 0, "lane", 6, 6)]
    # a box outside the tile and a surfel below the alpha threshold (half-extents -1) count nothing
    (s,) = bb.segment_pair_counts(art([(40.0, 7.5, 3.0, 3.0), (7.5, 7.5, -1.0, -1.0), dot]), 1)
    assert (s["entries"], s["pairs"], s["waves"]) == (3, 1, [(0, 0, "lane", 1, 1)])
