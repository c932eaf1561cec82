"""Row-by-row bars for the gradients of the surfel rasterizer's backward, the seeded scenes they are measured on, and a host
restatement of which gradient kernel a list segment takes (csrc/surfel_backward.hip).

Why rows: the bugs that kernel can have damage a few surfels -- the entry at slot 127 or 128 of a segment, a run of pair-table slots
that straddles a row of 16 lanes, the last entry before a pixel's walk ends -- and a whole-tensor norm over thousands of exact rows
does not move (tests/test_surfel_backward_cpu.py plants such an error and shows it pass the old bar).

The bar, for one input tensor reshaped to [n, k]:  err_i = |got_i - ref_i| <= ROW_TOL (|ref_i| + s),  s = the median of the non-zero
|ref_i|.  ROW_TOL = 1e-3 comes from the oracle itself: oracle/surfel_autograd.py evaluated in float32 against its float64 run stays
below 5e-5 on every row of every scene used here (the figures are in the header of tests/test_surfel_backward_cpu.py, which holds
it to 5e-4 without exceptions), so 1e-3 leaves a factor of twenty for the kernel's v_rcp_f32 / v_exp_f32 and its cross-product form of
the ray-splat intersection, and still catches a row that is off by 0.2 %.  At most max(1, n // 500) rows may exceed it -- a pair within
rounding of alpha = 1/255 or T = 0.5 that falls on the other side in fp32 -- none may exceed ROW_CAP (|ref_i| + s), and a case that needs
such an exception names the row (and, in its comment, the pair): an unnamed row beyond the bar fails.
"""
import numpy as np
import torch

from gaussiananything_amd import synthetic

NAMES = ("means3D", "opacities", "colors", "scales", "rotations")
ROW_TOL = 1e-3
ROW_CAP = 3e-2
ZERO_TOL = 1e-7          # a tensor whose reference is entirely zero: |got_i| below this times the case's largest reference row norm
# A gradient that vanishes identically without being exactly zero in either arithmetic: the median depth is the depth at which a ray
# meets the splat's plane, which no scale moves, but both autograd and the kernel arrive there as a sum of cancelling terms (the
# gradient of the scaled axis, which turns the plane, projected on the axis itself).  Float64 leaves 1e-16 of the terms, recognised
# as below ZERO_REF of the case's largest reference row; fp32 leaves a few roundings of 2^-24 of terms that are as large as the
# position gradient times the |u|, |v| <= 3 of a contributing pixel: held to 32 roundings, 2e-6 of the case's largest row (measured
# on the MI355X: 4.9e-8 and 9.4e-8).
ZERO_REF = 1e-10
CANCEL_TOL = 32 * 2.0 ** -24
WHOLE_TOL = 2e-4         # the whole-tensor relative L2 bar the backward tests have always had; kept beside the rows

# upstream-gradient groups: (colour?, allmap channels)
GROUPS = {"colour": (True, ()), "depth": (False, (0,)), "alpha": (False, (1,)), "normal": (False, (2, 3, 4)),
          "median": (False, (5,)), "distortion": (False, (6,))}
ALL_CHANNELS = (True, (0, 1, 2, 3, 4, 5, 6))


def allowed_rows(n):
    return max(1, n // 500)


def row_ratios(got, ref, n):
    """err_i / (|ref_i| + s) for every row of one tensor; s as in the module docstring (1 when the reference is entirely zero)."""
    got, ref = got.detach().double().cpu().reshape(n, -1), ref.detach().double().cpu().reshape(n, -1)
    rn = ref.norm(dim=1)
    nz = rn[rn > 0]
    s = float(nz.median()) if nz.numel() else 1.0
    return (got - ref).norm(dim=1) / (rn + s)


def row_bars(got, ref, n, name="", named=(), tol=ROW_TOL, cap=ROW_CAP):
    """Assert the per-row bar on one tensor with a non-zero reference: no row beyond ``cap``, at most allowed_rows(n) rows beyond
    ``tol``, and every one of those among ``named`` -- the rows a case has traced to a threshold flip and names in its comment.
    Returns (worst ratio, its row, rows beyond ``tol``)."""
    assert bool(torch.isfinite(got).all()), name
    r = row_ratios(got, ref, n)
    over = torch.nonzero(r > tol).reshape(-1).tolist()
    worst = int(r.argmax())
    listed = [(i, float(r[i])) for i in over[:8]]
    assert float(r.max()) <= cap, f"{name}: row {worst} at {float(r.max()):.2e} (|ref_i| + s), beyond the cap {cap}"
    assert len(over) <= allowed_rows(n), f"{name}: {len(over)} rows beyond {tol} (|ref_i| + s) (allowed {allowed_rows(n)}): {listed}"
    assert set(over) <= set(named), f"{name}: rows beyond {tol} (|ref_i| + s) that the case does not name as threshold flips: {listed}"
    return float(r.max()), worst, len(over)


def whole_tensor_error(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float((got - ref).norm() / (ref.norm() + 1e-30))


def check_gradients(got, ref, n, label="", named=None):
    """All five tensors of one case: the per-row bar and the whole-tensor bar where the reference is non-zero, the zero rule where it
    is entirely zero.  ``named``: {tensor name: rows} a case excepts (see row_bars).  Prints every figure before it asserts; returns
    {name: (worst ratio, row, excepted rows, whole-tensor error)}."""
    scale = max(float(b.detach().double().reshape(n, -1).norm(dim=1).max()) for b in ref)
    out, zero, bound = {}, {}, {}
    for name, a, b in zip(NAMES, got, ref):
        if float(b.detach().double().reshape(n, -1).norm(dim=1).max()) <= ZERO_REF * scale:
            zero[name] = float(a.detach().double().cpu().reshape(n, -1).norm(dim=1).max())
            bound[name] = (ZERO_TOL if float(b.abs().max()) == 0.0 else CANCEL_TOL) * scale
            print(f"backward {label} {name}: reference entirely zero, largest row {zero[name]:.2e} (case scale {scale:.2e})")
            out[name] = (0.0, -1, 0, 0.0)
            continue
        r = row_ratios(a, b, n)
        out[name] = (float(r.max()), int(r.argmax()), int((r > ROW_TOL).sum()), whole_tensor_error(a, b))
        print(f"backward {label} {name}: worst row {out[name][1]} at {out[name][0]:.2e} (|ref_i| + s), {out[name][2]} rows beyond "
              f"{ROW_TOL}; whole tensor {out[name][3]:.2e}")
    for name, a, b in zip(NAMES, got, ref):
        assert bool(torch.isfinite(a).all()), (label, name)
        if name in zero:
            assert zero[name] <= bound[name], (label, name, zero[name], bound[name])
        else:
            row_bars(a, b, n, f"{label} {name}", named=(named or {}).get(name, ()))
            assert out[name][3] < WHOLE_TOL, (label, name, out[name][3])
    return out


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def scene(n, H, W, views, seed, scale_lo, scale_hi, spread, opac_lo=0.08, opac_hi=0.33):
    """The seeded scene of a backward case, drawn in this order: means, opacity, rgb, scales, quaternions x (0.5 + U) (deliberately not
    unit), then the upstream-gradient weights of the colour and of the seven allmap channels.  float64 tensors of float32 values.
    The default opacities stay below 0.35: nothing outside the 3-sigma box reaches 1/255."""
    g = torch.Generator().manual_seed(seed)
    means = ((torch.rand(n, 3, generator=g) - 0.5) * spread).double()
    opac = (opac_lo + (opac_hi - opac_lo) * torch.rand(n, generator=g)).double()
    rgb = torch.rand(n, 3, generator=g).double()
    scales = (scale_lo + (scale_hi - scale_lo) * torch.rand(n, 2, generator=g)).double()
    quats = (torch.nn.functional.normalize(torch.randn(n, 4, generator=g), dim=-1) * (0.5 + torch.rand(n, 1, generator=g))).double()
    bg = torch.tensor([0.3, 0.6, 0.1], dtype=torch.float64)
    wc = torch.rand(len(views), 3, H, W, generator=g).double()
    wa = torch.rand(len(views), 7, H, W, generator=g).double()
    return dict(n=n, H=H, W=W, views=list(views), means=means, opac=opac, rgb=rgb, scales=scales, quats=quats, bg=bg, wc=wc, wa=wa)


def masked_weights(sc, mask):
    """the scene's upstream-gradient weights with everything outside ``mask`` = (colour?, allmap channels) set to zero"""
    colour, channels = mask
    wc = sc["wc"] if colour else torch.zeros_like(sc["wc"])
    wa = torch.zeros_like(sc["wa"])
    for ch in channels:
        wa[:, ch] = sc["wa"][:, ch]
    return wc, wa


def gaussians(sc):
    """the scene as the [n, 13] float32 tensor of gaussiananything_amd.synthetic (xyz, opacity, scales, rotation, rgb)"""
    return torch.cat([sc["means"], sc["opac"][:, None], sc["scales"], sc["quats"], sc["rgb"]], 1).float()


def oracle_gradients(sc, masks=(ALL_CHANNELS,), scale_modifier=1.0, dtype=torch.float64):
    """Autograd through oracle/surfel_autograd.py, view by view, ONE forward and one backward per mask.  Returns a list of
    (loss, five gradients) and the rendered (colour, allmap) per view, detached."""
    from oracle import surfel_autograd as oag
    cams = synthetic.eval_cameras(8)
    ins = [sc[k].to(dtype).clone().requires_grad_(True) for k in ("means", "opac", "rgb", "scales", "quats")]
    outs = [oag.render(*ins, cams["cam_view"][v].to(dtype), cams["cam_view_proj"][v].to(dtype), sc["bg"].to(dtype), sc["H"], sc["W"],
                       scale_modifier=scale_modifier, dtype=dtype) for v in sc["views"]]
    res = []
    for j, mask in enumerate(masks):
        wc, wa = masked_weights(sc, mask)
        loss = sum((col * wc[k].to(dtype)).sum() + (am * wa[k].to(dtype)).sum() for k, (col, am) in enumerate(outs))
        res.append((loss.detach(), torch.autograd.grad(loss, ins, retain_graph=j + 1 < len(masks))))
    return res, [(c.detach(), a.detach()) for c, a in outs]


# Raw alpha = opacity exp(-rho / 2) passes the 0.99 clamp only where rho < 0.02: at a pixel centre within a tenth of a pixel (or of a
# sigma) of the splat's centre.  These eight are the surfels of the "opaque" scene that have such a pixel in one of its two views
# (found with the C oracle's records); 86 and 158 are reached by their pixels' walks before those end.
EIGHT_OPAQUE = [86, 135, 158, 374, 383, 427, 440, 459]


def _eight_opaque(sc):
    sc["opac"][torch.tensor(EIGHT_OPAQUE)] = 1.0      # opacity exactly 1: above the clamp there is no gradient


CULLED = 20      # surfels of the three-view scene that are moved off some views' images


def _move_off_some_views(sc):
    """the first CULLED surfels go to seeded places up to 0.8 from the origin, where the narrow cameras (tan fov 0.36) of the three
    views do not all see them: a splat whose tile rectangle misses a view's image is culled there (radius 0)"""
    cand = ((torch.rand(400, 3, generator=torch.Generator().manual_seed(7)) - 0.5) * 1.6).double()
    sc["means"][:CULLED] = cand[torch.tensor(CULLED_PLACES)]


CULLED_PLACES = [6, 16, 17, 25, 33, 44, 52, 60, 64, 66, 67, 71, 78, 83, 84, 87, 89, 99, 103, 105]

# name -> (arguments of scene(), edit applied after the draw or None)
SCENES = {
    "six": (dict(n=6, H=48, W=48, views=[1, 4], seed=5, scale_lo=0.04, scale_hi=0.12, spread=0.3), None),
    "small400": (dict(n=400, H=40, W=40, views=[0], seed=9, scale_lo=0.002, scale_hi=0.05, spread=0.25), None),
    "large60": (dict(n=60, H=32, W=32, views=[2], seed=11, scale_lo=0.08, scale_hi=0.2, spread=0.2), None),
    "medium": (dict(n=300, H=32, W=32, views=[3], seed=13, scale_lo=0.02, scale_hi=0.05, spread=0.2), None),
    "opaque": (dict(n=600, H=32, W=32, views=[0, 3], seed=22, scale_lo=0.005, scale_hi=0.06, spread=0.2, opac_lo=0.2, opac_hi=1.0),
               _eight_opaque),
    "long_transparent": (dict(n=2200, H=16, W=16, views=[0], seed=21, scale_lo=0.002, scale_hi=0.02, spread=0.6, opac_lo=0.005,
                              opac_hi=0.02), None),
    "long_mixed": (dict(n=2200, H=16, W=16, views=[3], seed=24, scale_lo=0.002, scale_hi=0.05, spread=0.6, opac_lo=0.02, opac_hi=0.9),
                   None),
    # 60 surfels from sub-pixel to most of the image: segments on either side of the pair table's capacity in one launch
    "both_kernels": (dict(n=60, H=32, W=32, views=[2], seed=12, scale_lo=0.01, scale_hi=0.2, spread=0.2), None),
    "three_views": (dict(n=200, H=40, W=24, views=[0, 3, 6], seed=31, scale_lo=0.01, scale_hi=0.06, spread=0.25), _move_off_some_views),
    "one": (dict(n=1, H=32, W=32, views=[0], seed=41, scale_lo=0.04, scale_hi=0.08, spread=0.1), None),
    "n257": (dict(n=257, H=32, W=32, views=[1], seed=42, scale_lo=0.01, scale_hi=0.05, spread=0.25), None),
}
SEAM_SEED = 40       # the seam scenes: seed SEAM_SEED + n
for _n in (127, 128, 129, 256, 257):
    SCENES[f"seam{_n}"] = (dict(n=_n, H=16, W=16, views=[0], seed=SEAM_SEED + _n, scale_lo=0.002, scale_hi=0.03, spread=0.6,
                                opac_lo=0.02, opac_hi=0.2), None)
LONG = ("long_transparent", "long_mixed")        # references frozen in tests/golden/surfel_bwd_long_ref.pt (10 s of oracle each)
LONG_FIXTURE = "surfel_bwd_long_ref.pt"


def named_scene(name):
    kw, edit = SCENES[name]
    sc = scene(**kw)
    if edit is not None:
        edit(sc)
    return sc


def contributing_pairs_above_the_clamp(o, ids, W):
    """From the C oracle's records of one view (oracle.surfel.rasterize): the (pixel, entry) pairs of the surfels ``ids`` whose raw
    alpha exceeds 0.99 AND that take part in their pixel's blend -- the pixel's walk down the tile's depth-ordered list (the
    forward's arithmetic, in double) reaches them with T (1 - 0.99) >= 1e-4.  Returns them as (surfel, x, y)."""
    gx = (W + 15) // 16
    ids = set(int(i) for i in ids)
    found = []
    for tile, (beg, end) in enumerate(o["ranges"].astype(np.int64)):
        lst = o["point_list"][beg:end].astype(np.int64)
        if not ids & set(lst.tolist()):
            continue
        ys, xs = np.mgrid[0:16, 0:16].astype(np.float64)
        x0, y0 = 16 * (tile % gx), 16 * (tile // gx)
        xs, ys = xs + x0, ys + y0
        T, live = np.ones((16, 16)), np.ones((16, 16), bool)
        for i in lst:
            tr = o["trans"][i].astype(np.float64)
            Tu, Tv, Tw = tr[0:3], tr[3:6], tr[6:9]
            k, l = xs[..., None] * Tw - Tu, ys[..., None] * Tw - Tv
            p = np.cross(k, l)
            with np.errstate(divide="ignore", invalid="ignore"):
                s = p[..., :2] / p[..., 2:3]
            rho3d = (s ** 2).sum(-1)
            rho2d = 2.0 * ((o["xy"][i, 0] - xs) ** 2 + (o["xy"][i, 1] - ys) ** 2)
            use3d = rho3d <= rho2d
            depth = np.where(use3d, s[..., 0] * Tw[0] + s[..., 1] * Tw[1] + Tw[2], Tw[2])
            raw = o["normal_opacity"][i, 3] * np.exp(-0.5 * np.fmin(rho3d, rho2d))
            alpha = np.minimum(0.99, raw)
            ok = live & (p[..., 2] != 0) & (depth >= 0.2) & (alpha >= 1.0 / 255.0)
            stop = ok & (T * (1 - alpha) < 1e-4)
            live &= ~stop
            ok &= ~stop
            if int(i) in ids:
                found += [(int(i), int(x) + x0, int(y) + y0) for y, x in zip(*np.nonzero(ok & (raw > 0.99)))]
            T = np.where(ok, T * (1 - alpha), T)
    return found


# ---- which gradient kernel a segment takes ----------------------------------------------------------------------------------------
PAIR_CAP = 2528          # GA_BWD_PAIR_CAP: slots of the pair table of surfel_bwd_grad_kernel
WAVE_MAJOR_LANES = 12    # GA_BWD_WAVE_MAJOR_LANES
SEG = 128                # kBwdSeg


def _intervals(art, v, ids, tx, ty):
    """[len(ids), 16] bool each: the tile columns / rows q with |q - (centre - 16 tile)| <= half-extent, in the kernel's fp32
    (stage_segment: fabsf((float)q - ox) <= rx with ox = bx - (float)(16 tx))"""
    c, h = art["cull_centre"][v, ids].astype(np.float32), art["cull_half"][v, ids].astype(np.float32)
    q = np.arange(16, dtype=np.float32)[None, :]
    ox, oy = c[:, 0:1] - np.float32(16 * tx), c[:, 1:2] - np.float32(16 * ty)
    with np.errstate(invalid="ignore"):
        return np.abs(q - ox) <= h[:, 0:1], np.abs(q - oy) <= h[:, 1:2]


def segment_pair_counts(art, gx):
    """Host restatement of the rule of surfel_bwd_sums_kernel: every (view, tile) list of ``ws_artifacts`` cut into 128-entry
    segments; the pairs of a segment are the sum over its entries of (tile columns inside the cull box) x (tile rows inside it); the
    segment goes to surfel_bwd_grad_big_kernel when they exceed PAIR_CAP, to the pair-major surfel_bwd_grad_kernel otherwise.
    ``gx``: tiles per image row.  Returns a list of dicts (view, tile, k, entries, pairs, big, waves); ``waves`` restates the
    per-wave rule of grad_big for a segment on which no pixel has finished: a wave is an 8 x 8 quadrant of the tile; per 64-entry
    half, with the entries whose box meets the quadrant, it walks entry-major ('entry') when the quadrant's (pixel, entry) pairs
    are at least WAVE_MAJOR_LANES times the number of those entries, lane-major ('lane') otherwise, and not at all when there are
    none -- [(half, wave, 'entry' | 'lane', pairs, entries)]."""
    ts, tiles = art["tile_start"], art["tiles"]
    segs = []
    for vt in range(len(ts) - 1):
        v, tile = divmod(vt, tiles)
        tx, ty = tile % gx, tile // gx
        for k, beg in enumerate(range(int(ts[vt]), int(ts[vt + 1]), SEG)):
            ids = art["point_list"][beg:min(beg + SEG, int(ts[vt + 1]))]
            cols, rows = _intervals(art, v, ids, tx, ty)
            pairs = int((cols.sum(1) * rows.sum(1)).sum())
            waves = []
            for h in range(0, len(ids), 64):
                for wv in range(4):
                    cq = cols[h:h + 64, 8 * (wv & 1):8 * (wv & 1) + 8].sum(1)
                    rq = rows[h:h + 64, 8 * (wv >> 1):8 * (wv >> 1) + 8].sum(1)
                    ne, npairs = int(((cq > 0) & (rq > 0)).sum()), int((cq * rq).sum())
                    if ne:
                        waves.append((h // 64, wv, "entry" if npairs >= WAVE_MAJOR_LANES * ne else "lane", npairs, ne))
            segs.append(dict(view=v, tile=tile, k=k, entries=len(ids), pairs=pairs, big=pairs > PAIR_CAP, waves=waves))
    return segs
