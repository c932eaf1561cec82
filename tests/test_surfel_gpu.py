"""GPU parity of the HIP surfel rasterizer (through the C-ABI) against the CPU oracle.

Bars (BASELINE.json north_star): integer artefacts -- radii, tile rects, per-tile ranges and depth-ordered index
lists -- BIT-IDENTICAL; pixels MSE <= 1e-5 per output (colour and each allmap channel).
"""
import numpy as np
import os

import pytest
import torch

from gaussiananything_amd import synthetic
from tests import _bwd_bars, _util

pytestmark = pytest.mark.gpu

MSE_TOL = 1e-5
# Beside the MSE bar of north_star: the ABSOLUTE pixel differences.  An MSE alone lets a whole wrong 16 x 16 tile through at 512^2
# (error 0.1 on 256 pixels = MSE 1e-5).  A plain "max abs <= 1e-4" is not a property any fp32 evaluation order of this algorithm has:
# a pixel's walk takes threshold decisions (alpha >= 1/255, T (1 - alpha) < 1e-4 stops the walk, T > 0.5 picks the median depth,
# rho3d <= rho2d picks the depth) and the cross product of a nearly edge-on splat cancels, so a few pixels in a million move by
# 1e-3 ... 1e-2 (the median-depth channel by a whole depth) when the operations are ordered differently -- measured
# (tools/parity_maxabs.py, all scenes below): the fp32 oracle against ITS OWN blend loop in double differs beyond 1e-4 on as many
# pixels as the HIP kernel does against the fp32 oracle (stress scene, 2.1 M pixels: 123 vs 180 on the worst channel; 80-90 % of them
# the same pixels; never more than 11 in one tile).  So the bars are: per output channel at most max(4, 3e-4 P) of the P pixels beyond
# 1e-4, at most 24 of them inside one 16 x 16 tile (a wrong tile is 256), and nothing beyond 0.25 outside the median-depth channel.
MAXABS_TOL = 1e-4
OUTLIER_FRACTION = 3e-4
OUTLIERS_PER_TILE = 24
MAXABS_CAP = 0.25


def _pixel_bars(color, allmap, o):
    d = np.concatenate([np.abs(color - o["color"]), np.abs(allmap - o["allmap"])], 0)        # [10, H, W]; 8 = median depth
    H, W = d.shape[1:]
    out = d > MAXABS_TOL
    allowed = max(4, int(np.ceil(OUTLIER_FRACTION * H * W)))
    per_channel = out.reshape(10, -1).sum(1)
    assert int(per_channel.max()) <= allowed, f"pixels beyond {MAXABS_TOL} per channel {per_channel.tolist()} (allowed {allowed})"
    Hp, Wp = (H + 15) // 16 * 16, (W + 15) // 16 * 16
    pad = np.zeros((10, Hp, Wp), bool)
    pad[:, :H, :W] = out
    per_tile = int(pad.reshape(10, Hp // 16, 16, Wp // 16, 16).sum((2, 4)).max())
    assert per_tile <= OUTLIERS_PER_TILE, f"{per_tile} pixels beyond {MAXABS_TOL} inside one tile"
    cap = float(np.delete(d, 8, 0).max())
    assert cap <= MAXABS_CAP, f"max abs {cap}"


def _compare_view(o, color, radii, allmap, art, v, N, tiles):
    assert np.array_equal(radii, o["radii"]), "radii differ"
    assert np.array_equal(art["rect"][v].astype(np.uint32), o["rect"]), "tile rects differ"
    ts = art["tile_start"][v * tiles:(v + 1) * tiles + 1]
    base = ts[0]
    cnt_o = (o["ranges"][:, 1].astype(np.int64) - o["ranges"][:, 0].astype(np.int64))
    assert np.array_equal(np.diff(ts), cnt_o), "per-tile list lengths differ"
    nz = cnt_o > 0
    assert np.array_equal((ts[:-1] - base)[nz], o["ranges"][nz, 0].astype(np.int64)), "tile range starts differ"
    pl = art["point_list"][base:base + o["D"]]
    assert np.array_equal(pl.astype(np.uint32), o["point_list"]), "depth-ordered point lists differ"
    mse_c = float(np.mean((color - o["color"]) ** 2))
    assert mse_c <= MSE_TOL, f"colour MSE {mse_c}"
    for ch in range(7):
        mse = float(np.mean((allmap[ch] - o["allmap"][ch]) ** 2))
        assert mse <= MSE_TOL, f"allmap[{ch}] MSE {mse}"
    _pixel_bars(color, allmap, o)
    return mse_c


def _run_case(g, cams, views, H, W, device, scale_modifier=1.0, bg=(1.0, 1.0, 1.0)):
    N = g.shape[0]
    color, radii, allmap, ws = _util.hip_views(g, cams, views, H, W, device, bg=bg, scale_modifier=scale_modifier)
    art = _util.ws_artifacts(ws, N, len(views), H, W)
    assert art["overflow"] == 0
    color, radii, allmap = color.cpu().numpy(), radii.cpu().numpy(), allmap.cpu().numpy()
    total = 0
    for k, v in enumerate(views):
        o = _util.oracle_view(g, cams, v, H, W, bg=bg, scale_modifier=scale_modifier)
        _compare_view(o, color[k], radii[k], allmap[k], art, k, N, art["tiles"])
        total += o["D"]
    assert total == art["D"]
    return art


def test_config1_1k_256(gpu_device):
    cams = synthetic.eval_cameras(8)
    g = synthetic.random_surfels(1000, seed=0)[0]
    _run_case(g, cams, [0], 256, 256, gpu_device)


@pytest.mark.parametrize("scene", ["surface", "stress", "small"])
def test_split_walk_of_the_blend_matches_the_oracle(gpu_device, monkeypatch, scene):
    """GA_SURFEL_FLAG_SPLIT_WALK (round 4; opt-in: measured slower than the fused walk): unsegmented lists evaluated with lanes =
    (entry, pixel) pairs and composited with lanes = pixels from per-pixel LDS lists -- same pixels as the oracle (the lists' order is
    the depth order), full lists (the small scene's big splats fill them: composite passes in the middle of a pair instruction),
    ragged image, and the default walk's images to 1e-5."""
    from gaussiananything_amd import _lib, diff_surfel_rasterization as dsr
    cams = synthetic.eval_cameras(8)
    if scene == "small":
        g, views, H, W, sm = synthetic.random_surfels(3000, seed=5)[0], [0, 5], 200, 296, 3.0
    else:
        g = synthetic.surface_surfels(100_000, seed=1)[0] if scene == "surface" else synthetic.random_surfels(100_000, seed=0)[0]
        views, H, W, sm = [0, 3], 512, 512, 1.0
    ref = _util.hip_views(g, cams, views, H, W, gpu_device, scale_modifier=sm)
    dsr.clear_workspaces()
    monkeypatch.setattr(dsr, "EXTRA_FLAGS", _lib.GA_SURFEL_FLAG_SPLIT_WALK)
    _run_case(g, cams, views, H, W, gpu_device, scale_modifier=sm)
    got = _util.hip_views(g, cams, views, H, W, gpu_device, scale_modifier=sm)
    assert float((got[0] - ref[0]).abs().max()) < 1e-5 and float((got[2] - ref[2]).abs().max()) < 1e-4
    dsr.clear_workspaces()


def test_lds_atomics_serve_the_lanes_of_an_instruction_in_lane_order(gpu_device):
    """what the split walk's list append relies on (one returning ds_add per passing pair): tools/lds_atomic_order.hip"""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "_build", "lds_atomic_order")
    if not os.path.exists(exe):
        pytest.skip("tools/_build/lds_atomic_order not built (__graft_entry__.build() compiles it)")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120).stdout
    assert "lane order held in every case" in out, out


def test_config1_matches_frozen_golden(gpu_device):
    """HIP output against the committed fixture (tests/golden/surfel_cfg1_oracle.npz), without running the oracle."""
    z = np.load(synthetic.fixture_path("surfel_cfg1_oracle.npz"))
    cams = synthetic.eval_cameras(1)
    g = synthetic.random_surfels(1000, seed=0)[0]
    color, radii, allmap, ws = _util.hip_views(g, cams, [0], 256, 256, gpu_device)
    art = _util.ws_artifacts(ws, 1000, 1, 256, 256)
    assert np.array_equal(radii[0].cpu().numpy(), z["radii"])
    assert np.array_equal(art["point_list"].astype(np.uint32), z["point_list"])
    assert np.array_equal(art["rect"][0].astype(np.uint32), z["rect"])
    assert float(np.mean((color[0].cpu().numpy() - z["color_f16"].astype(np.float32)) ** 2)) < 1e-5
    assert np.allclose(color[0].double().sum((1, 2)).cpu().numpy(), z["color_sum"], rtol=1e-4)


@pytest.mark.parametrize("scene", ["surface", "stress"])
def test_baseline_config2_100k_surfels_8_views_512(gpu_device, scene):
    """BASELINE.json configs[1] -- the configuration bench.py times (SURVEY.md 8d 'Config #2 input'; call site
    /root/reference/nsr/gs_surfel.py:85-114): 100 000 surfels x eval_pose[:8] x 512^2, the surface-like scene (sub-pixel
    splats at the filter floor, tile lists up to ~5 k entries: cull boxes, segmented blend and the merge path all
    matter) and the uniform-random stress scene.  Bit-identical radii / rects / ranges / point lists, MSE <= 1e-5 per
    channel, every view against the C oracle."""
    cams = synthetic.eval_cameras(8)
    g = synthetic.surface_surfels(100_000, seed=1)[0] if scene == "surface" else synthetic.random_surfels(100_000, seed=0)[0]
    art = _run_case(g, cams, list(range(8)), 512, 512, gpu_device)
    assert art["D"] > 100_000 * 8


def test_unnormalised_quaternions_are_renormalised(gpu_device):
    """the rasterizer re-normalises the quaternion; a direct caller handing over scaled rotations
    gets the same splats (same integer artefacts, pixels to rounding) and parity with the oracle holds for them."""
    cams = synthetic.eval_cameras(8)
    g = synthetic.random_surfels(3000, seed=9)[0].clone()
    gen = torch.Generator().manual_seed(5)
    g2 = g.clone()
    g2[:, 6:10] *= torch.exp(2.0 * torch.randn(3000, 1, generator=gen))      # |q| from ~0.02 to ~50
    _run_case(g2, cams, [0, 6], 160, 160, gpu_device)
    c1, r1, a1, _ = _util.hip_views(g, cams, [0, 6], 160, 160, gpu_device)
    c2, r2, a2, _ = _util.hip_views(g2, cams, [0, 6], 160, 160, gpu_device)
    assert float((r1 != r2).float().mean()) < 0.01          # a radius may move by one where ceil() sits on an integer
    assert float(((c1 - c2) ** 2).mean()) < 1e-6


@pytest.mark.parametrize("H,W", [(250, 300), (16, 16), (33, 17)])
def test_ragged_image_sizes(gpu_device, H, W):
    cams = synthetic.eval_cameras(8)
    g = synthetic.random_surfels(2000, seed=3)[0]
    _run_case(g, cams, [1, 5], H, W, gpu_device)


def test_more_than_8192_tiles_take_the_chunked_scan(gpu_device):
    """3 views of 1024 x 1024 = 12 288 (view, tile) counters: beyond the single-pass register scan of the tile-scan
    kernel (and beyond the per-view LDS histograms of preprocess / fill at 4096 tiles? no: those hold 8192)."""
    cams = synthetic.eval_cameras(8)
    g = synthetic.random_surfels(1500, seed=21)[0]
    _run_case(g, cams, [1, 4, 6], 1024, 1024, gpu_device)


def test_sizes_beyond_the_fused_binning_launch_take_the_scan_in_front_of_the_fill(gpu_device):
    """The fill launch that carries the schedule (round 4) covers views of at most 8192 tiles and fewer than 65536 (view, tile)
    counters; beyond either the single-workgroup scan runs in front of the fill: (i) one view of 1552 x 1552 = 9409 tiles (global
    cursors, no LDS histogram), (ii) 264 views of 256 x 256 = 67 584 counters (LDS histograms, absolute cursors).  Same bins, same
    pixels as the oracle, and the workspace is left clean for the next forward either way (second forward on the same workspace)."""
    cams = synthetic.eval_cameras(8)
    g = synthetic.random_surfels(1200, seed=33)[0]
    _run_case(g, cams, [2], 1552, 1552, gpu_device)
    _run_case(g, cams, [2], 1552, 1552, gpu_device)
    g2 = synthetic.random_surfels(400, seed=34)[0]
    views = [v % 8 for v in range(264)]
    _run_case(g2, cams, views, 256, 256, gpu_device)
    _run_case(g2, cams, views, 256, 256, gpu_device)


@pytest.mark.parametrize("H,W,views", [(1080, 1920, [0, 3]), (1024, 2048, [1]), (1088, 1920, [2, 5, 7])])
def test_views_of_7681_to_8192_tiles_through_the_fused_binning_launch(gpu_device, H, W, views):
    """Full HD (120 x 68 = 8160 tiles), exactly kLdsTiles = 8192 tiles (2048 x 1024) and 8160 tiles with a ragged last row: the fill
    rows of surfel_fill_sched_kernel scan 16 consecutive tile counters per thread at these sizes and need 64 KiB of dynamic LDS
    beside the kernel's static LDS (opted into with hipFuncSetAttribute).  Round 4 computed the counters per thread as
    (T + 1023) / 512 = 17 there: the 17th counter of every thread was never scanned and the list begins of the fill disagreed with
    the schedule's.  Same bins and pixels as the oracle, twice on the same workspace (it must be left clean)."""
    cams = synthetic.eval_cameras(8)
    g = synthetic.random_surfels(4000, seed=41)[0]
    _run_case(g, cams, views, H, W, gpu_device)
    _run_case(g, cams, views, H, W, gpu_device, scale_modifier=2.0)


def test_multi_view_batch_equals_oracle_per_view(gpu_device):
    cams = synthetic.eval_cameras(8)
    g = synthetic.random_surfels(20000, seed=5)[0]
    _run_case(g, cams, list(range(8)), 256, 256, gpu_device, bg=(0.2, 0.5, 0.9))


def test_scale_modifier_and_big_splats(gpu_device):
    cams = synthetic.eval_cameras(8)
    g = synthetic.random_surfels(3000, seed=7)[0].clone()
    g[:, 4:6] *= 8.0  # large splats: hundreds of tiles each
    _run_case(g, cams, [2], 128, 128, gpu_device, scale_modifier=1.5)


def test_long_tile_lists_take_the_run_merge_path(gpu_device):
    """> 8192 entries in one tile (several LDS runs): exercises the multi-run rank-merge of the per-tile sort."""
    cams = synthetic.eval_cameras(8)
    g = synthetic.random_surfels(30000, seed=11)[0].clone()
    g[:, 0:3] *= 0.05  # everything lands in a couple of tiles
    art = _run_case(g, cams, [0], 64, 64, gpu_device)
    assert art["max_tile"] > 8192


def test_segmented_blend_of_transparent_long_lists(gpu_device):
    """Lists >= 1024 pairs are blended four segments at a time (transmittance pre-pass, ordered merge with the
    distortion cross terms).  Nearly transparent splats keep every segment alive down to the last pair, so colour,
    depth, median depth and distortion all cross the segment seams; an opaque variant stops inside the first segment."""
    cams = synthetic.eval_cameras(8)
    for lo, hi in ((0.005, 0.02), (0.3, 1.0)):
        g = synthetic.random_surfels(6000, seed=13)[0].clone()
        g[:, 0:3] *= 0.05
        g[:, 3] = lo + (hi - lo) * torch.rand(6000, generator=torch.Generator().manual_seed(3))
        art = _run_case(g, cams, [0, 5], 64, 64, gpu_device)
        assert art["max_tile"] >= 1024
        if lo < 0.1:
            _, _, allmap, _ = _util.hip_views(g, cams, [0], 64, 64, gpu_device)
            alpha = allmap[0, 1].cpu().numpy()
            assert 0.2 < float(alpha.max()) < 0.9999, "scene should stay short of the stop rule"


def test_segmented_blend_of_very_long_lists_beside_short_ones(gpu_device):
    """Tiles with > 4096, with 1-2 k and with a handful of pairs in one launch (the schedule puts the long ones first, four
    quadrant workgroups each), transparent so that every segment seam is crossed; one and several views; repeated calls
    are bit-identical."""
    cams = synthetic.eval_cameras(8)
    gen = torch.Generator().manual_seed(17)
    dense = synthetic.random_surfels(9000, seed=21)[0].clone()
    dense[:, 0:3] *= 0.04                      # a few tiles with thousands of entries
    mid = synthetic.random_surfels(3000, seed=22)[0].clone()
    mid[:, 0:3] = mid[:, 0:3] * 0.08 + torch.tensor([0.25, 0.2, 0.0])   # a neighbouring clump with ~1-2 k per tile
    sparse = synthetic.random_surfels(1500, seed=23)[0].clone()
    g = torch.cat([dense, mid, sparse], 0)
    g[:, 3] = 0.004 + 0.02 * torch.rand(g.shape[0], generator=gen)
    for views in ([0], [0, 3, 6]):
        art = _run_case(g, cams, views, 96, 96, gpu_device)
        assert art["max_tile"] >= 4096
    a1 = _util.hip_views(g, cams, [0, 3], 96, 96, gpu_device)
    a2 = _util.hip_views(g, cams, [0, 3], 96, 96, gpu_device)
    assert torch.equal(a1[0], a2[0]) and torch.equal(a1[2], a2[2])


def _long_list_scene(seed, n=9000, spread=0.04, lo=0.004, hi=0.024):
    g = synthetic.random_surfels(n, seed=seed)[0].clone()
    g[:, 0:3] *= spread
    g[:, 3] = lo + (hi - lo) * torch.rand(n, generator=torch.Generator().manual_seed(seed + 100))
    return g


def test_graph_replay_of_the_segmented_blend_on_changing_inputs(gpu_device):
    """SurfelForwardPlan.run() captured in a HIP graph and replayed on DIFFERENT Gaussian sets with lists >= 2048 entries: the
    cross-workgroup exchange words of the segmented blend carry the launch epoch, which has to advance per REPLAY (it is a device
    word the tile scan bumps; a host counter passed as a kernel argument would be frozen in the graph and the words of the
    previous replay would validate).  Every replay is held to the oracle on its own inputs."""
    from gaussiananything_amd.diff_surfel_rasterization import SurfelForwardPlan
    cams = synthetic.eval_cameras(8)
    views, H, W = [0, 3], 96, 96
    scenes = [_long_list_scene(31), _long_list_scene(32, spread=0.05, lo=0.01, hi=0.05), _long_list_scene(33, lo=0.3, hi=1.0),
              _long_list_scene(31)]
    m, o, sc, r, c = [t.to(gpu_device) for t in synthetic.split_gaussians(scenes[0])]
    plan = SurfelForwardPlan(m, o, c, sc, r, cams["cam_view"][views].to(gpu_device), cams["cam_view_proj"][views].to(gpu_device),
                             torch.ones(3, device=gpu_device), H, W)
    plan.run()
    assert plan.ensure_capacity() > 0
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=gpu_device)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        plan.run()          # warm-up on the capture stream
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            plan.run()
    torch.cuda.synchronize()
    for k, g in enumerate(scenes):
        mm, oo, ss, rr, cc = synthetic.split_gaussians(g)
        plan.means3D.copy_(mm.to(gpu_device)); plan.opacities.copy_(oo.to(gpu_device).reshape(-1)); plan.colors.copy_(cc.to(gpu_device))
        plan.scales.copy_(ss.to(gpu_device)); plan.rotations.copy_(rr.to(gpu_device))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        st = plan.ws.status().cpu()
        assert int(st[1]) == 0 and int(st[2]) >= 2048, (k, st[:3])
        color, allmap = plan.color.cpu().numpy(), plan.allmap.cpu().numpy()
        for j, v in enumerate(views):
            ref = _util.oracle_view(g, cams, v, H, W)
            assert float(np.mean((color[j] - ref["color"]) ** 2)) <= MSE_TOL, (k, v)
            for ch in range(7):
                assert float(np.mean((allmap[j, ch] - ref["allmap"][ch]) ** 2)) <= MSE_TOL, (k, v, ch)


def test_segment_scratch_overflow_is_reported_and_regrown(gpu_device):
    """The exchange scratch of the segmented blend is sized for seg_capacity work items, not for the worst case: a launch that
    needs more reports an overflow (nothing rendered, the number needed in the status words) and the host re-sizes."""
    from gaussiananything_amd import _lib
    from gaussiananything_amd.diff_surfel_rasterization import SurfelWorkspace, rasterize_views
    cams = synthetic.eval_cameras(8)
    g = _long_list_scene(41, n=12000)
    H = W = 96
    m, o, sc, r, c = [t.to(gpu_device) for t in synthetic.split_gaussians(g)]
    vm, pm = cams["cam_view"][[0, 2]].to(gpu_device), cams["cam_view_proj"][[0, 2]].to(gpu_device)
    small = SurfelWorkspace(gpu_device, g.shape[0], 2, H, W, 1 << 18, seg_capacity=2)
    bg = torch.ones(3, device=gpu_device)
    with pytest.raises(RuntimeError, match="segment work items"):
        rasterize_views(m, o, c, sc, r, vm, pm, bg, H, W, workspace=small)
    st = small.status().cpu()
    assert int(st[_lib.GA_STATUS_OVERFLOW]) == 1 and int(st[_lib.GA_STATUS_SEG_WORK]) > 2
    assert int(st[_lib.GA_STATUS_NUM_RENDERED]) <= small.capacity      # the lists themselves fit
    big = small.grown(st)
    assert big.seg_items >= int(st[_lib.GA_STATUS_SEG_WORK]) and big.capacity == small.capacity
    color, radii, allmap, _ = rasterize_views(m, o, c, sc, r, vm, pm, bg, H, W, workspace=big)
    ref_color, _, ref_allmap, _ = rasterize_views(m, o, c, sc, r, vm, pm, bg, H, W)   # cached default workspace
    assert torch.equal(color, ref_color) and torch.equal(allmap, ref_allmap)
    ref = _util.oracle_view(g, cams, 0, H, W)
    assert float(np.mean((color[0].cpu().numpy() - ref["color"]) ** 2)) <= MSE_TOL


def test_degenerate_inputs(gpu_device):
    """behind-camera, zero-scale, zero / tiny opacity, duplicate depths (tie-break by index), edge-on splats."""
    cams = synthetic.eval_cameras(8)
    g = synthetic.random_surfels(512, seed=13)[0].clone()
    g[0:32, 0:3] = torch.tensor([5.0, 5.0, 5.0])      # far off / behind for some views
    g[32:64, 4:6] = 0.0                                # zero scale
    g[64:96, 3] = 0.0                                  # zero opacity
    g[96:128, 3] = 1.0 / 300.0                         # below the alpha threshold
    g[128:192, 0:3] = g[128:129, 0:3]                  # identical centres -> identical depth keys
    g[192:224, 6:10] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    for v in (0, 3):
        _run_case(g, cams, [v], 128, 128, gpu_device)


def test_empty_scene(gpu_device):
    cams = synthetic.eval_cameras(8)
    g = synthetic.random_surfels(8, seed=1)[0].clone()
    g[:, 0:3] = 100.0
    color, radii, allmap, ws = _util.hip_views(g, cams, [0], 64, 64, gpu_device, bg=(0.1, 0.2, 0.3))
    assert int(ws.status().cpu()[0]) == 0
    assert torch.all(radii == 0)
    assert torch.allclose(color[0, 1], torch.full((64, 64), 0.2, device=gpu_device))
    assert torch.all(allmap == 0)


def test_cull_box_is_conservative(gpu_device):
    """Every (pixel, splat) pair the oracle blends (alpha >= 1/255) lies inside the HIP path's cull box."""
    from oracle import surfel as osurf  # noqa: F401
    cams = synthetic.eval_cameras(8)
    g = synthetic.random_surfels(4000, seed=17)[0]
    H = W = 128
    _, _, _, ws = _util.hip_views(g, cams, [4], H, W, gpu_device)
    art = _util.ws_artifacts(ws, 4000, 1, H, W)
    o = _util.oracle_view(g, cams, 4, H, W)
    vis = np.nonzero(o["radii"] > 0)[0]
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    bad = 0
    for i in vis[:600]:
        Tu, Tv, Tw = o["trans"][i, 0:3], o["trans"][i, 3:6], o["trans"][i, 6:9]
        k = xs[..., None] * Tw - Tu
        l = ys[..., None] * Tw - Tv
        p = np.cross(k, l)
        with np.errstate(divide="ignore", invalid="ignore"):
            s = p[..., :2] / p[..., 2:3]
        rho3d = (s ** 2).sum(-1)
        d = o["xy"][i] - np.stack([xs, ys], -1)
        rho = np.fmin(rho3d, 2.0 * (d ** 2).sum(-1))
        alpha = np.minimum(0.99, o["normal_opacity"][i, 3] * np.exp(-0.5 * rho))
        live = alpha >= 1.0 / 255.0
        # restrict to the tiles the splat is binned into (the only pixels that can see it)
        rc = o["rect"][i].astype(int)
        tmask = (xs >= rc[0] * 16) & (xs < rc[2] * 16) & (ys >= rc[1] * 16) & (ys < rc[3] * 16)
        live &= tmask
        bb = art["bbox"][0, i]
        inside = (xs >= bb[0]) & (xs <= bb[2]) & (ys >= bb[1]) & (ys <= bb[3])
        bad += int(np.count_nonzero(live & ~inside))
    assert bad == 0


def test_drop_in_rasterizer_call(gpu_device):
    """The reference's exact call sequence (nsr/gs_surfel.py:85-114) through the import shim."""
    from diff_surfel_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    cams = synthetic.eval_cameras(8)
    g = synthetic.random_surfels(1000, seed=0)[0].to(gpu_device)
    m, op, sc, rot, rgb = synthetic.split_gaussians(g)
    rs = GaussianRasterizationSettings(
        image_height=256, image_width=256, tanfovx=cams["tanfov"], tanfovy=cams["tanfov"],
        bg=torch.ones(3, device=gpu_device), scale_modifier=1, viewmatrix=cams["cam_view"][0].to(gpu_device),
        projmatrix=cams["cam_view_proj"][0].to(gpu_device), sh_degree=0, campos=cams["cam_pos"][0].to(gpu_device),
        prefiltered=False, debug=False)
    image, radii, allmap = GaussianRasterizer(raster_settings=rs)(
        means3D=m, means2D=torch.zeros_like(m), shs=None, colors_precomp=rgb, opacities=op, scales=sc,
        rotations=rot, cov3D_precomp=None)
    assert image.shape == (3, 256, 256) and allmap.shape == (7, 256, 256) and radii.shape == (1000,)
    o = _util.oracle_view(g.cpu(), cams, 0, 256, 256)
    assert float(np.mean((image.cpu().numpy() - o["color"]) ** 2)) <= MSE_TOL
    with pytest.raises(Exception):
        GaussianRasterizer(raster_settings=rs)(means3D=m, means2D=None, opacities=op, scales=sc, rotations=rot)
    with pytest.raises(RuntimeError):
        GaussianRasterizer(raster_settings=rs)(means3D=m.cpu(), means2D=None, opacities=op, colors_precomp=rgb,
                                               scales=sc, rotations=rot)


def test_renderer_2dgs_dict(gpu_device):
    """GaussianRenderer2DGS.render: same keys/shapes/post-processing as nsr/gs_surfel.py:41-202."""
    from gaussiananything_amd.gs_surfel import GaussianRenderer2DGS
    cams = synthetic.eval_cameras(4)
    g = synthetic.random_surfels(3000, seed=2).to(gpu_device)
    r = GaussianRenderer2DGS(128, 3, {})
    out = r.render(g, cams["cam_view"][None].to(gpu_device), cams["cam_view_proj"][None].to(gpu_device),
                   cams["cam_pos"][None].to(gpu_device), cams["tanfov"])
    assert out["image"].shape == (1, 4, 3, 128, 128) and out["rend_normal"].shape == (1, 4, 3, 128, 128)
    for v in range(4):
        o = _util.oracle_view(g[0].cpu(), cams, v, 128, 128)
        view = cams["cam_view"][v].numpy()
        nrm = np.einsum("chw,dc->dhw", o["allmap"][2:5], view[:3, :3])
        assert float(np.mean((out["rend_normal"][0, v].cpu().numpy() - nrm) ** 2)) <= MSE_TOL
        assert float(np.mean((out["image"][0, v].cpu().numpy() - np.clip(o["color"], 0, 1)) ** 2)) <= MSE_TOL
        assert float(np.mean((out["depth"][0, v, 0].cpu().numpy() - np.nan_to_num(o["allmap"][5], nan=0.0, posinf=0.0)) ** 2)) <= MSE_TOL
        assert float(np.mean((out["alpha"][0, v, 0].cpu().numpy() - o["allmap"][1]) ** 2)) <= MSE_TOL
        assert float(np.mean((out["dist"][0, v, 0].cpu().numpy() - o["allmap"][6]) ** 2)) <= MSE_TOL


def test_render_levels_overlapped_on_two_streams_equals_one_render_per_set(gpu_device):
    """GaussianRenderer2DGS.render_levels (the four levels of triplane_decode, vit/vit_triplane.py:1550-1591): independent surfel
    sets on two side streams with ONE overflow read-back -- every tensor bit-identical to render() set by set; a set whose
    workspace overflows (splats much larger than the default capacity expects) is rendered again the ordinary way; repeated
    calls (workspaces now 'clean') and two sets of one shape (one shared workspace, one stream) included -- also where the set
    that overflows shares its workspace with a later set that fits: that set's forward overwrites the workspace's status words,
    and the overflow must be found all the same (both orders of the two)."""
    from gaussiananything_amd import diff_surfel_rasterization as dsr
    from gaussiananything_amd.gs_surfel import GaussianRenderer2DGS
    cams = synthetic.eval_cameras(6)
    cv, cvp, cp = (cams[k][None].to(gpu_device) for k in ("cam_view", "cam_view_proj", "cam_pos"))
    big = synthetic.random_surfels(2500, seed=9)
    big[0, :, 4:6] *= 12.0                                   # hundreds of tiles per splat: far beyond 2 N V entries
    sets = [synthetic.random_surfels(700, seed=5), synthetic.surface_surfels(9000, seed=6), big, synthetic.random_surfels(700, seed=7),
            synthetic.surface_surfels(30000, seed=8), synthetic.random_surfels(2500, seed=10)]
    sets = [g.to(gpu_device) for g in sets]
    sizes = [64, 128, 96, 64, 256, 96]
    r = GaussianRenderer2DGS(512, 3, {})
    key = (str(gpu_device), 2500, 6, 96, 96)
    dsr._ws_cache.clear()
    r.render(sets[5], cv, cvp, cp, cams["tanfov"], output_size=96)      # the precondition: the last set alone fits the default capacity
    assert dsr._ws_cache[key].capacity == dsr.default_capacity(2500, 6)
    dsr._ws_cache.clear()
    for rep, order in enumerate(([0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5], [5, 2])):
        if rep in (1, 3):
            dsr._ws_cache.clear()                            # the overflow is found again on fresh workspaces
        got = r.render_levels([sets[i] for i in order], [sizes[i] for i in order], cv, cvp, cp, cams["tanfov"])
        torch.cuda.synchronize()
        for i, res in zip(order, got):
            want = r.render(sets[i], cv, cvp, cp, cams["tanfov"], output_size=sizes[i])
            assert set(res) == set(want)
            for k in want:
                assert res[k].shape == want[k].shape and torch.equal(res[k], want[k]), (rep, i, k)
    assert key in dsr._ws_cache and dsr._ws_cache[key].capacity > dsr.default_capacity(2500, 6)     # it did overflow and grow


def test_background_of_empty_tiles_written_by_the_sort_launch_is_bit_identical(gpu_device):
    """Round 6: the background pixels of the empty tiles come from the waves of the per-tile sort launch that find an empty list
    (surfel_bin.hip) instead of from blend workgroups; GA_SURFEL_FLAG_BG_IN_BLEND restores the old placement.  Same bits, on a scene
    that leaves most tiles empty, with ragged image sizes (16-byte and scalar store paths), a clean and a reused workspace."""
    from gaussiananything_amd import _lib
    from gaussiananything_amd.diff_surfel_rasterization import SurfelForwardPlan
    cams = synthetic.eval_cameras(3)
    g = synthetic.random_surfels(400, seed=4)[0]
    g[:, :3] = g[:, :3] * 0.3 + 0.1                      # a small object: most of the image is background
    m, o, s, r, c = [t.to(gpu_device) for t in synthetic.split_gaussians(g)]
    bg = torch.tensor([0.25, 0.5, 0.75], device=gpu_device)
    for H, W in ((256, 256), (130, 250), (33, 17)):
        outs = []
        for flags in (0, _lib.GA_SURFEL_FLAG_BG_IN_BLEND):
            plan = SurfelForwardPlan(m, o, c, s, r, cams["cam_view"].to(gpu_device), cams["cam_view_proj"].to(gpu_device), bg, H, W, flags=flags)
            for _ in range(2):                            # second run: GA_SURFEL_FLAG_WORKSPACE_CLEAN
                plan.color.fill_(-7.0)
                plan.allmap.fill_(-7.0)
                plan.run()
            torch.cuda.synchronize()
            outs.append((plan.color.clone(), plan.allmap.clone()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), (H, W)
        assert float(outs[0][0].min()) >= 0.0 and float((outs[0][1] == -7.0).sum()) == 0      # every pixel written
        bgpix = (outs[0][1][:, 1] == 0)                   # alpha exactly 0: background
        assert int(bgpix.sum()) > 0.5 * bgpix.numel()
        for ch in range(3):
            assert torch.equal(outs[0][0][:, ch][bgpix], torch.full_like(outs[0][0][:, ch][bgpix], float(bg[ch])))


def test_postprocess_kernel_exact(gpu_device):
    """ga_surfel_postprocess against the torch formulation of nsr/gs_surfel.py:121-163, NaN / inf / out-of-range included,
    image sizes with and without the 16-byte path; batch of two through the renderer."""
    from gaussiananything_amd.diff_surfel_rasterization import postprocess_views
    from gaussiananything_amd.gs_surfel import GaussianRenderer2DGS
    g0 = torch.Generator().manual_seed(11)
    for (V, H, W) in ((3, 32, 32), (2, 15, 17)):
        color = (torch.randn(V, 3, H, W, generator=g0) * 0.8 + 0.5).to(gpu_device)
        allmap = torch.randn(V, 7, H, W, generator=g0).to(gpu_device)
        allmap[0, 5, 0, :4] = torch.tensor([float("nan"), float("inf"), float("-inf"), 2.5], device=gpu_device)
        view = torch.randn(V, 4, 4, generator=g0).to(gpu_device)
        image, normal, depth = postprocess_views(color, allmap, view)
        assert torch.equal(image, color.clamp(0, 1))
        assert torch.equal(depth, torch.nan_to_num(allmap[:, 5:6], 0, 0))
        ref = torch.einsum("vchw,vdc->vdhw", allmap[:, 2:5].double(), view[:, :3, :3].double())
        assert (normal.double() - ref).abs().max().item() < 1e-5
    cams = synthetic.eval_cameras(2)
    gs = torch.stack([synthetic.random_surfels(500, seed=s)[0] for s in (3, 4)]).to(gpu_device)
    r = GaussianRenderer2DGS(64, 3, {})
    cv, cvp, cp = (cams[k][None].expand(2, *cams[k].shape).to(gpu_device) for k in ("cam_view", "cam_view_proj", "cam_pos"))
    both = r.render(gs, cv, cvp, cp, cams["tanfov"])
    for b in range(2):
        one = r.render(gs[b:b + 1], cv[b:b + 1], cvp[b:b + 1], cp[b:b + 1], cams["tanfov"])
        for k in ("image", "alpha", "depth", "rend_normal", "dist"):
            assert both[k].shape[0] == 2 and torch.equal(both[k][b], one[k][0]), k


# ---- backward: ga_surfel_backward against oracle/surfel_autograd.py -----------------------------
def _backward_case(gpu_device, n, H, W, views, seed, scale_lo, scale_hi, spread, opac_lo=0.08, opac_hi=0.33, scale_modifier=1.0,
                   masks=(_bwd_bars.ALL_CHANNELS,), edit=None, refs=None, label="", named=None):
    """One scene of tests/_bwd_bars.py (``scene``: means, opacity, rgb, scales, quaternions, then the weights; ``edit`` changes it after
    the draw) through the HIP path and through autograd of oracle/surfel_autograd.py in float64: ONE forward each, one backward per
    upstream-gradient mask = (colour?, allmap channels) -- the HIP node retained between them.  Per mask: the losses agree, every
    gradient tensor keeps the whole-tensor bar (relative L2 < 2e-4) and the row-by-row bar of tests/_bwd_bars.py (``named``: the rows
    a case excepts as threshold flips); a tensor whose reference is entirely zero stays at zero.  ``refs``: [(loss, gradients)] per
    mask from a fixture instead of the oracle run.  Returns (refs, [gradients of the HIP path per mask], the figures per mask).

    Measured on the MI355X, worst row of any tensor as err_i / (|ref_i| + s) and the tensor it is in (0 rows beyond 1e-3 everywhere):
    six 1.6e-6 rotations (scale_modifier 1.7: the same), small400 2.2e-5 means3D, large60 1.8e-5 means3D, medium 2.5e-5 rotations,
    both_kernels 1.8e-5 means3D, opaque 4.6e-5 rotations, three_views 2.6e-5 rotations, one 6.1e-7 rotations, n257 1.4e-5 scales,
    seam127 / 128 / 129 / 256 / 257 4.5e-6 / 7.5e-6 / 4.4e-6 / 5.9e-6 / 6.5e-6 scales, long_transparent 1.4e-5 scales,
    long_mixed 9.4e-5 opacities (the same with and without the transmittance table); one output-channel group at a time, colour /
    depth / alpha / normal / median / distortion: six 3.0e-6 / 3.9e-6 / 5.0e-6 / 5.8e-6 / 9.3e-6 / 1.4e-6, medium 3.1e-5 / 4.5e-5 /
    4.4e-5 / 1.6e-5 / 2.6e-6 / 1.1e-4 (rotations throughout; the distortion group was 6.4e-1 before the backward took its depth
    moments about the tile's front depth, csrc/surfel_backward.hip tile_rd0)."""
    from gaussiananything_amd.diff_surfel_rasterization import rasterize_views
    cams = synthetic.eval_cameras(8)
    sc = _bwd_bars.scene(n, H, W, views, seed, scale_lo, scale_hi, spread, opac_lo, opac_hi)
    if edit is not None:
        edit(sc)
    if refs is None:       # oracle: autograd through the float64 restatement, view by view
        refs, _ = _bwd_bars.oracle_gradients(sc, masks, scale_modifier)
    # HIP path
    bg = sc["bg"]
    dins = [sc[k].float().to(gpu_device).requires_grad_(True) for k in ("means", "opac", "rgb", "scales", "quats")]
    color, radii, allmap, _ = rasterize_views(dins[0], dins[1][:, None], dins[2], dins[3], dins[4],
                                              cams["cam_view"][views].to(gpu_device), cams["cam_view_proj"][views].to(gpu_device),
                                              bg.float().to(gpu_device), H, W, scale_modifier)
    assert color.requires_grad and allmap.requires_grad and not radii.requires_grad
    gots, figures = [], []
    for j, (mask, (loss, ref)) in enumerate(zip(masks, refs)):
        wc, wa = _bwd_bars.masked_weights(sc, mask)
        dloss = (color.double() * wc.to(gpu_device)).sum() + (allmap.double() * wa.to(gpu_device)).sum()
        assert abs(float(dloss.detach()) - float(loss)) <= 2e-4 * abs(float(loss)) + 1e-3
        got = torch.autograd.grad(dloss, dins, retain_graph=j + 1 < len(masks))
        figures.append(_bwd_bars.check_gradients(got, ref, n, f"{label} {mask}".strip(), named=named))
        gots.append(got)
    return refs, gots, figures


def test_backward_small_scene_against_the_autograd_oracle(gpu_device):
    """Six large surfels, 48 x 48, two views at once: every gradient path (plane intersection, low-pass filter centre,
    distortion, normal rotation, quaternion normalisation; quaternions deliberately not unit) against autograd through
    oracle/surfel_autograd.py."""
    _backward_case(gpu_device, 6, 48, 48, [1, 4], seed=5, scale_lo=0.04, scale_hi=0.12, spread=0.3, label="six")


def test_backward_many_small_surfels_long_lists(gpu_device):
    """400 surfels in a few tiles (lists of several 128-entry chunks in the backward kernel, sub-pixel and larger splats:
    both branches of min(rho3d, rho2d))."""
    _backward_case(gpu_device, 400, 40, 40, [0], seed=9, scale_lo=0.002, scale_hi=0.05, spread=0.25, label="small400")


def test_backward_many_large_surfels_take_the_walk_with_the_lds_gradient_image(gpu_device):
    """60 surfels that each cover most of a 32 x 32 image: 60 x ~256 pairs per tile, more than the pair table of the gradient
    kernel holds (kPairCap = 2528), so this is the former walk -- entry-major waves with the cross-lane sums -- while the six
    surfels of the small scene (at most 6 x 256 pairs) always take the pair-major path."""
    _backward_case(gpu_device, 60, 32, 32, [2], seed=11, scale_lo=0.08, scale_hi=0.2, spread=0.2, label="large60")


def test_backward_medium_surfels(gpu_device):
    """300 surfels of 3 .. 8 pixels across in a 32 x 32 image: lists of 226 .. 300 entries, two full 128-entry segments and a short
    one per tile, and splats whose radius reaches over a tile edge that getRect leaves out (the autograd oracle restates that
    rule).  All eleven segments are pair-major: a surfel has ~21 pairs but they are spread over its 3.5 tiles, 6 per list entry, and
    no segment holds more than 878 of the 2528 the pair table takes (asserted in tests/test_surfel_backward_gpu.py, where the scene
    with both gradient kernels in one launch is "both_kernels"; this docstring used to claim that for this scene)."""
    _backward_case(gpu_device, 300, 32, 32, [3], seed=13, scale_lo=0.02, scale_hi=0.05, spread=0.2, label="medium")


def test_forward_of_a_differentiable_call_equals_the_inference_forward_and_hands_over_the_transmittances(gpu_device, monkeypatch):
    """The blend instantiation that records the per-segment transmittances for the backward (GaSurfelForwardArgs.seg_T: no
    run-ahead across 128-entry boundaries) composites the same pairs in the same order -- its images are the inference call's
    bit for bit -- and the gradients that start from its table agree with those of the backward that forms the products itself
    (GA_SURFEL_SEG_T=0: two more launches).  The two differ in how alpha is evaluated -- the blend's plane form against the
    backward's cross product -- and a product of up to 2 300 factors (1 - alpha) carries that: measured 4.6e-5 relative L2, bar
    2e-4 as for the oracle parity.  Unsegmented, wrapping and segmented items of the blend are all in this scene."""
    from gaussiananything_amd.diff_surfel_rasterization import rasterize_views
    cams = synthetic.eval_cameras(8)
    g = synthetic.surface_surfels(60_000, seed=3)[0].to(gpu_device)
    m, op, sc, rot, rgb = synthetic.split_gaussians(g)
    vm, pm = cams["cam_view"][:3].to(gpu_device), cams["cam_view_proj"][:3].to(gpu_device)
    bg = torch.tensor([0.2, 0.5, 0.9], device=gpu_device)
    gen = torch.Generator(device="cpu").manual_seed(5)
    wc = torch.rand(3, 3, 256, 256, generator=gen).to(gpu_device)
    wo = torch.rand(3, 7, 256, 256, generator=gen).to(gpu_device)
    wo[:, 5] = 0     # (which pair crosses T = 0.5 can differ between the two where a T lies within rounding of 0.5)
    with torch.no_grad():
        c0, r0, a0, ws = rasterize_views(m, op, rgb, sc, rot, vm, pm, bg, 256, 256)
    assert int(ws.status()[2]) > 2048            # the longest list is blended in segments
    grads = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("GA_SURFEL_SEG_T", flag)
        leaves = [t.detach().clone().requires_grad_(True) for t in (m, op, rgb, sc, rot)]
        c1, r1, a1, _ = rasterize_views(*leaves, vm, pm, bg, 256, 256)
        assert torch.equal(c1, c0) and torch.equal(a1, a0) and torch.equal(r1, r0)
        ((c1 * wc).sum() + (a1 * wo).sum()).backward()
        grads[flag] = [t.grad.double() for t in leaves]
    for a, b in zip(grads["1"], grads["0"]):
        assert torch.isfinite(a).all() and float((a - b).norm() / b.norm()) < 2e-4


def test_rasterizer_module_is_differentiable(gpu_device):
    """The reference's call sequence (nsr/gs_surfel.py:85-114) with tensors that require grad: gradients arrive."""
    from diff_surfel_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    cams = synthetic.eval_cameras(8)
    g = synthetic.random_surfels(500, seed=0)[0].to(gpu_device)
    m, op, sc, rot, rgb = [t.clone().requires_grad_(True) for t in synthetic.split_gaussians(g)]
    rs = GaussianRasterizationSettings(
        image_height=64, image_width=64, tanfovx=cams["tanfov"], tanfovy=cams["tanfov"], bg=torch.ones(3, device=gpu_device),
        scale_modifier=1, viewmatrix=cams["cam_view"][0].to(gpu_device), projmatrix=cams["cam_view_proj"][0].to(gpu_device),
        sh_degree=0, campos=cams["cam_pos"][0].to(gpu_device), prefiltered=False, debug=False)
    image, radii, allmap = GaussianRasterizer(raster_settings=rs)(
        means3D=m, means2D=torch.zeros_like(m), shs=None, colors_precomp=rgb, opacities=op, scales=sc, rotations=rot,
        cov3D_precomp=None)
    (image.mean() + allmap[1].mean() + 0.1 * allmap[6].mean()).backward()
    for t in (m, op, sc, rot, rgb):
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0


def test_retained_graphs_and_forwards_in_flight_keep_their_own_workspaces(gpu_device):
    """The reference's training step (dnnlib/util.py calculate_adaptive_weight) runs autograd.grad(..., retain_graph=True) on one
    render before the final backward, with other renders of the step alive: every differentiable forward owns its workspace until
    its autograd node is freed -- several backwards through one node, and forwards issued between them, all see their own lists."""
    from gaussiananything_amd import diff_surfel_rasterization as dsr
    cams = synthetic.eval_cameras(2)
    vm, pm = cams["cam_view"].to(gpu_device), cams["cam_view_proj"].to(gpu_device)
    bg = torch.ones(3, device=gpu_device)
    dsr.clear_workspaces()

    def scene(seed):
        g = synthetic.random_surfels(700, seed=seed)[0].to(gpu_device)
        return [t.clone().requires_grad_(True) for t in synthetic.split_gaussians(g)]

    def render(ins):
        m, op, sc, rot, rgb = ins
        color, _, allmap, _ = dsr.rasterize_views(m, op, rgb, sc, rot, vm, pm, bg, 64, 64)
        return color.mean() + allmap[:, 1].mean() + 0.1 * allmap[:, 6].mean()

    a, b = scene(1), scene(2)
    want_a = torch.autograd.grad(render(a), a)
    want_b = torch.autograd.grad(render(b), b)
    la = render(a)                                            # forward A in flight
    g1 = torch.autograd.grad(la, a, retain_graph=True)        # first backward through A
    lb = render(b)                                            # forward B between two backwards of A
    g2 = torch.autograd.grad(la, a, retain_graph=True)        # second backward through A
    gb = torch.autograd.grad(lb, b)
    g3 = torch.autograd.grad(la, a)                           # final backward through A
    close = lambda x, y: float((x - y).norm()) <= 1e-5 * float(y.norm()) + 1e-12   # noqa: E731  (float atomics: summation order)
    for got in (g1, g2, g3):
        for x, y in zip(got, want_a):
            assert close(x, y)
    for x, y in zip(gb, want_b):
        assert close(x, y)
    del la, lb
    import gc
    gc.collect()
    pool = dsr._autograd_pool[(str(a[0].device), 700, 2, 64, 64)]
    assert 1 <= len(pool) <= 2 and len({id(w) for w in pool}) == len(pool)     # returned once each, bounded


def test_renderer_is_differentiable_end_to_end(gpu_device):
    """GaussianRenderer2DGS.render with a Gaussian tensor that requires grad (training call sites, nsr/gs_surfel.py:41-202):
    same outputs as the inference path, and the gradient of a loss on image + alpha + normal + distortion reaches it."""
    from gaussiananything_amd.gs_surfel import GaussianRenderer2DGS
    cams = synthetic.eval_cameras(3)
    g = synthetic.random_surfels(800, seed=4).to(gpu_device)
    r = GaussianRenderer2DGS(64, 3, {})
    cv, cvp, cp = (cams[k][None].to(gpu_device) for k in ("cam_view", "cam_view_proj", "cam_pos"))
    ref = r.render(g, cv, cvp, cp, cams["tanfov"])
    gg = g.clone().requires_grad_(True)
    out = r.render(gg, cv, cvp, cp, cams["tanfov"])
    for k in ("image", "alpha", "depth", "rend_normal", "dist"):
        assert out[k].shape == ref[k].shape and float((out[k] - ref[k]).abs().max()) < 1e-5, k
    (out["image"].mean() + out["alpha"].mean() + out["rend_normal"].square().mean() + out["dist"].mean()).backward()
    assert gg.grad is not None and bool(torch.isfinite(gg.grad).all()) and float(gg.grad.abs().max()) > 0


def test_backward_directional_derivatives_at_baseline_config2(gpu_device):
    """BASELINE configs[1] size (100 k surfels x 8 views x 512^2), where the autograd oracle cannot go: the gradient against
    central differences of the HIP forward along random directions.  The loss is linear in the colours (the quotient must be
    exact up to fp32 rounding) and smooth in the opacities.  (Geometry is not compared this way: moving 100 k sub-pixel
    surfels carries pairs across the alpha >= 1/255 test, jumps that a difference quotient sees and that the gradient -- by
    the convention of the reference's backward and of oracle/surfel_autograd.py -- treats as constants: measured -4.1e4
    against -7.7e4 along a random direction of the means.  The geometric chain is covered by the oracle tests above.)"""
    from gaussiananything_amd.diff_surfel_rasterization import rasterize_views
    cams = synthetic.eval_cameras(8)
    g = synthetic.surface_surfels(100_000, seed=1)[0].to(gpu_device)
    m, op, sc, rot, rgb = synthetic.split_gaussians(g)
    vm, pm = cams["cam_view"].to(gpu_device), cams["cam_view_proj"].to(gpu_device)
    bg = torch.ones(3, device=gpu_device)
    gen = torch.Generator(device="cpu").manual_seed(11)
    wc = torch.rand(8, 3, 512, 512, generator=gen).to(gpu_device)
    wo = (torch.rand(8, 7, 512, 512, generator=gen) * 0.1).to(gpu_device)
    wo[:, 5] = 0                                            # (the median contributor changes under steps of this size)

    def loss(m_, op_, sc_, rot_, rgb_):
        color, _, allmap, _ = rasterize_views(m_, op_, rgb_, sc_, rot_, vm, pm, bg, 512, 512)
        return ((color.double() * wc).sum() + (allmap.double() * wo).sum())

    leaves = [t.detach().clone().requires_grad_(True) for t in (m, op, sc, rot, rgb)]
    loss(*leaves).backward()
    grads = [t.grad.double() for t in leaves]
    assert all(bool(torch.isfinite(gr).all()) for gr in grads)
    with torch.no_grad():
        for idx, eps, tol in ((4, 1e-2, 2e-3), (1, 1e-3, 3e-2)):
            d = torch.randn(leaves[idx].shape, generator=gen).to(gpu_device)
            args_p = [t.detach() for t in leaves]
            args_m = list(args_p)
            args_p[idx] = args_p[idx] + eps * d
            args_m[idx] = args_m[idx] - eps * d
            fd = float(loss(*args_p) - loss(*args_m)) / (2 * eps)
            an = float((grads[idx] * d.double()).sum())
            assert abs(fd - an) <= tol * max(abs(an), abs(fd)), (idx, fd, an)


def test_backward_edge_cases_nothing_rendered_single_surfel_and_ragged_image(gpu_device):
    """Edge cases of ga_surfel_backward: every surfel behind the cameras (no list entries: all gradients exactly zero), a
    single surfel, and an image whose size is not a multiple of the 16-pixel tiles (pixels outside the image take no part)."""
    from gaussiananything_amd.diff_surfel_rasterization import rasterize_views
    cams = synthetic.eval_cameras(2)
    vm, pm = cams["cam_view"].to(gpu_device), cams["cam_view_proj"].to(gpu_device)
    bg = torch.ones(3, device=gpu_device)

    def run(g, H, W):
        leaves = [t.to(gpu_device).clone().requires_grad_(True) for t in synthetic.split_gaussians(g)]
        color, radii, allmap, _ = rasterize_views(leaves[0], leaves[1], leaves[4], leaves[2], leaves[3], vm, pm, bg, H, W)
        (color.sum() + allmap[:, :5].sum() + allmap[:, 6].sum()).backward()
        return leaves, radii

    g = synthetic.random_surfels(64, seed=2)[0]
    far = g.clone()
    far[:, :3] = far[:, :3] * 0.01 + torch.tensor([0.0, 0.0, 50.0])     # far outside every frustum
    leaves, radii = run(far, 64, 64)
    if int((radii > 0).sum()) == 0:
        assert all(float(t.grad.abs().max()) == 0.0 for t in leaves)
    one = synthetic.random_surfels(1, seed=3)[0]
    one[:, :3] = 0.0
    one[:, 4:6] = 0.05
    leaves, radii = run(one, 64, 64)
    assert int((radii > 0).sum()) == 2 and all(bool(torch.isfinite(t.grad).all()) for t in leaves)
    assert float(leaves[4].grad.abs().max()) > 0 and float(leaves[1].grad.abs().max()) > 0
    # ragged image: same gradients as the oracle path would give is covered above; here: finite, and equal to the gradients of
    # the same scene rendered on the padded size with zero weight outside (the loss only sums inside pixels either way)
    g2 = synthetic.random_surfels(300, seed=4)[0]
    la, _ = run(g2, 50, 70)
    assert all(bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0 for t in la)
