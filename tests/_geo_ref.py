"""Restatement of the geometry losses (include/ga_loss.h, ga_geo_loss_*) for the tests, written from the formulas of the reference's
``depths_to_points_2`` / ``depth_to_normal_2`` and of its trainer, parametrised by dtype, gradients through torch autograd.  Runs on
whatever device its inputs are on.

    normals_reference_route   the reference's route: general inverse of the column-vector world-to-camera matrix, fp32 intrinsics and
                              their inverse, points in WORLD space (rotated, origin added), then the differences, cross, normalise
    normals_camera_model      the route of the kernel: camera space, the cross product in its closed form, one rotation at the end
    pullback_depth            the kernel's hand-written backward of that closed form (a gather), checked against autograd on the CPU

Both routes normalise with the project's zero-gradient rule (``normalize_ruled``): the forward of ``F.normalize``, no gradient through a
pixel whose cross product is shorter than 1e-12.  Also the seeded input families and cameras, the per-case bars of the GPU tests and
the section writer of profiles/geo_loss_bounds.txt."""
import math
import os

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_FILE = os.path.join(ROOT, "profiles", "geo_loss_bounds.txt")
GOLDEN = os.path.join(ROOT, "tests", "golden", "geo_loss_ref.pt")
TANFOV = 0.36
RADIUS = 1.7
EPS = 1e-12
FAMILIES = ("sphere", "plane", "noisy", "holes")


# ---- cameras and inputs --------------------------------------------------------------------------------------------------------
def look_at_w2c(seed):
    """column-vector world-to-camera matrix [4,4] fp32 of a camera at radius 1.7 looking at the origin (rigid to fp32 rounding)"""
    g = torch.Generator().manual_seed(1000 + int(seed))
    pos = F.normalize(torch.randn(3, generator=g, dtype=torch.float64), dim=0) * RADIUS
    fwd = F.normalize(-pos, dim=0)                                   # camera z looks at the origin
    up = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)
    if abs(float(fwd @ up)) > 0.95:
        up = torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64)
    right = F.normalize(torch.linalg.cross(fwd, up), dim=0)
    down = torch.linalg.cross(fwd, right)
    R = torch.stack([right, down, fwd])                              # rows: the camera axes in world coordinates
    m = torch.eye(4, dtype=torch.float64)
    m[:3, :3] = R
    m[:3, 3] = -R @ pos
    return m.float()


def make_depth(family, H, W, seed):
    """[H,W] fp32 depth map, a function of (family, H, W, seed) alone"""
    g = torch.Generator().manual_seed(int(seed))
    fx, fy = W / (2 * TANFOV), H / (2 * TANFOV)
    u = ((torch.arange(W, dtype=torch.float64) - W / 2) / fx)[None, :].expand(H, W)
    v = ((torch.arange(H, dtype=torch.float64) - H / 2) / fy)[:, None].expand(H, W)
    if family == "sphere":       # a ray-cast ball at the origin, seen from RADIUS, on a zero background
        rad = 0.45 + 0.1 * float(torch.rand(1, generator=g))
        rr = u * u + v * v + 1
        disc = (2 * RADIUS) ** 2 - 4 * rr * (RADIUS ** 2 - rad ** 2)
        t = (2 * RADIUS - disc.clamp_min(0).sqrt()) / (2 * rr)
        return torch.where(disc > 0, t, torch.zeros_like(t)).float()
    if family == "plane":        # a tilted plane through the origin
        a, b = (torch.rand(2, generator=g, dtype=torch.float64) - 0.5).tolist()
        return (RADIUS / (1 + a * u + b * v)).float()
    if family == "noisy":
        return 1.7 + 0.3 * torch.rand(H, W, generator=g)
    if family == "holes":        # a smooth surface with 30 % of the pixels zeroed
        ph = torch.rand(2, generator=g, dtype=torch.float64) * 6.28
        d = (RADIUS + 0.2 * torch.sin(5 * u + ph[0]) * torch.cos(4 * v + ph[1])).float()
        return torch.where(torch.rand(H, W, generator=g) < 0.3, torch.zeros_like(d), d)
    raise ValueError(family)


def make_inputs(family, shape, seed):
    """shape (V,H,W) -> dict of fp32 CPU tensors: depth, alpha, dist, mask [V,1,H,W]; rend_normal, target_normal [V,3,H,W];
    w2c [V,4,4] (column-vector world-to-camera, what depth_to_normal_2 takes) and cam_view, its transpose (what render takes)"""
    V, H, W = shape
    g = torch.Generator().manual_seed(7919 * int(seed) + 13)
    depth = torch.stack([make_depth(family, H, W, 31 * seed + v) for v in range(V)])[:, None]
    w2c = torch.stack([look_at_w2c(31 * seed + v) for v in range(V)])
    alpha = (0.1 + 0.9 * torch.rand(V, 1, H, W, generator=g)) * (depth > 0)            # holes carry no alpha, as in a render
    alpha = torch.where(torch.rand(V, 1, H, W, generator=g) < 0.05, torch.ones_like(alpha), alpha)   # some exactly 1, for sign(0)
    mask = (torch.rand(V, 1, H, W, generator=g) < 0.6).float()
    rend_normal = F.normalize(torch.randn(V, 3, H, W, generator=g), dim=1) * (0.2 + 0.8 * torch.rand(V, 1, H, W, generator=g))
    target_normal = F.normalize(torch.randn(V, 3, H, W, generator=g), dim=1)
    dist = 0.05 * torch.rand(V, 1, H, W, generator=g)
    return {"depth": depth.contiguous(), "alpha": alpha, "dist": dist, "mask": mask, "rend_normal": rend_normal,
            "target_normal": target_normal, "w2c": w2c, "cam_view": w2c.transpose(1, 2).contiguous()}


def island_depth():
    """[1,12,12] float64: a smooth surface, a 5 x 5 block of holes in it, one valid pixel in the middle of the block.  The normals of
    that pixel's four neighbours have a vanishing cross product: the zero-gradient rule decides their gradient."""
    H = W = 12
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    d = 1.7 + 0.05 * torch.sin(0.7 * x) + 0.04 * torch.cos(0.5 * y)
    d[3:8, 3:8] = 0
    d[5, 5] = 1.6
    return d[None]


def shapes(T):
    """(V,H,W): the smallest shapes at which the kernel can go wrong; T is the tile edge"""
    return [(1, 2, 2), (1, 1, 5), (1, 3, 3), (1, T, T), (1, T + 1, T - 1), (1, 37, 70), (2, 2 * T + 1, T + 2), (1, 129, 65)]


def cases(T):
    """(family, (V,H,W), seed): every family on every shape"""
    out = []
    for si, shape in enumerate(shapes(T)):
        for fi, fam in enumerate(FAMILIES):
            out.append((fam, shape, 100 + 10 * si + fi))
    return out


# ---- normals -------------------------------------------------------------------------------------------------------------------
def normalize_ruled(c):
    """F.normalize(c, dim=-1) in the forward; no gradient through a vector shorter than 1e-12 (torch returns G / 1e-12 there)"""
    length = c.detach().norm(dim=-1, keepdim=True)
    ok = length >= EPS
    safe = torch.where(ok, c, torch.ones_like(c))                    # keeps 0 / 0 out of the branch that is not taken
    return torch.where(ok, safe / safe.norm(dim=-1, keepdim=True).clamp_min(EPS), (c / EPS).detach())


def _border(normal_map, H, W):
    out = torch.zeros(H, W, 3, dtype=normal_map.dtype, device=normal_map.device)
    out[1:-1, 1:-1] = normal_map
    return out


def _no_interior(depth, dtype):
    """a map without interior pixels: all zero, still a function of depth for autograd"""
    H, W = depth.shape[-2:]
    return torch.zeros(H, W, 3, dtype=dtype, device=depth.device) + 0 * depth.to(dtype).sum()


def normals_reference_route(w2c, tanfov, depth, dtype=torch.float32, normalize=normalize_ruled):
    """one view: w2c [4,4] column-vector world-to-camera, depth [1,H,W] -> [H,W,3] in ``dtype``.  In fp32 the steps and their order are
    the reference's (fp32 intrinsics, fp32 inverses, ((grid K^-T) R^T) d + o); in float64 everything is float64."""
    H, W = depth.shape[-2:]
    dev = depth.device
    c2w = torch.linalg.inv(w2c.to(dtype))
    fx, fy = W / (2 * tanfov), H / (2 * tanfov)
    intrins = torch.tensor([[fx, 0.0, W / 2.0], [0.0, fy, H / 2.0], [0.0, 0.0, 1.0]], dtype=dtype, device=dev)
    gx, gy = torch.meshgrid(torch.arange(W, device=dev).to(dtype), torch.arange(H, device=dev).to(dtype), indexing="xy")
    pix = torch.stack([gx, gy, torch.ones_like(gx)], dim=-1).reshape(-1, 3)
    rays_d = pix @ torch.linalg.inv(intrins).T @ c2w[:3, :3].T
    points = (depth.to(dtype).reshape(-1, 1) * rays_d + c2w[:3, 3]).reshape(H, W, 3)
    if H < 3 or W < 3:
        return _no_interior(depth, dtype)
    dx = points[2:, 1:-1] - points[:-2, 1:-1]                        # along the rows
    dy = points[1:-1, 2:] - points[1:-1, :-2]
    return _border(normalize(torch.linalg.cross(dx, dy, dim=-1)), H, W)


def camera_cross(tanfov, depth, dtype=torch.float32):
    """depth [H,W] -> (c [H-2,W-2,3], parts) of the interior pixels: the closed form of ga_loss.h, every operation in ``dtype``"""
    H, W = depth.shape
    dev = depth.device
    d = depth.to(dtype)
    ifx = torch.tensor(2.0 * tanfov / W, dtype=dtype, device=dev)
    ify = torch.tensor(2.0 * tanfov / H, dtype=dtype, device=dev)
    u = ((torch.arange(W, device=dev).to(dtype) - W / 2.0) * ifx)[None, 1:-1]
    v = ((torch.arange(H, device=dev).to(dtype) - H / 2.0) * ify)[1:-1, None]
    dN, dS, dW, dE = d[:-2, 1:-1], d[2:, 1:-1], d[1:-1, :-2], d[1:-1, 2:]
    dv, dh = dS - dN, dE - dW
    p, q = (dS + dN) * ify, (dE + dW) * ifx
    c = torch.stack([p * dh, q * dv, -(v * dv * q + u * dh * p + p * q)], dim=-1)
    return c, dict(u=u, v=v, dv=dv, dh=dh, p=p, q=q, ifx=ifx, ify=ify)


def normals_camera_model(cam_view, tanfov, depth, dtype=torch.float32):
    """one view: cam_view [4,4] (render's convention: rotation block = camera to world), depth [1,H,W] -> [H,W,3]"""
    H, W = depth.shape[-2:]
    if H < 3 or W < 3:
        return _no_interior(depth, dtype)
    c, _ = camera_cross(tanfov, depth[0], dtype)
    n = normalize_ruled(c)
    return _border(n @ cam_view[:3, :3].to(dtype).T, H, W)


def pullback_depth(cam_view, tanfov, depth, grad_normal):
    """the kernel's backward by hand, fp32: depth [H,W], grad_normal [H,W,3] (with respect to the world normal) -> grad depth [H,W]"""
    H, W = depth.shape
    out = torch.zeros(H, W, dtype=torch.float32)
    if H < 3 or W < 3:
        return out
    c, k = camera_cross(tanfov, depth, torch.float32)
    length = c.norm(dim=-1, keepdim=True)
    ok = (length >= EPS)[..., 0]
    h = grad_normal[1:-1, 1:-1].float() @ cam_view[:3, :3].float()                       # R^T G per pixel
    n = c / length.clamp_min(EPS)
    gc = (h - n * (n * h).sum(-1, keepdim=True)) / length.clamp_min(EPS)
    gcx, gcy, gcz = gc.unbind(-1)
    g_dv = k["q"] * (gcy - gcz * k["v"])
    g_dh = k["p"] * (gcx - gcz * k["u"])
    g_sv = k["ify"] * (gcx * k["dh"] - gcz * (k["u"] * k["dh"] + k["q"]))
    g_sh = k["ifx"] * (gcy * k["dv"] - gcz * (k["v"] * k["dv"] + k["p"]))
    zero = torch.zeros_like(g_dv)
    gS, gN, gE, gW = (torch.where(ok, t, zero) for t in (g_sv + g_dv, g_sv - g_dv, g_sh + g_dh, g_sh - g_dh))
    out[2:, 1:-1] += gS
    out[:-2, 1:-1] += gN
    out[1:-1, 2:] += gE
    out[1:-1, :-2] += gW
    return out


def normal_maps(inp, route, dtype):
    """[V,3,H,W] world normals of every view of ``inp`` by ``route`` ('reference' or 'camera'); ``inp['tanfov']`` overrides TANFOV"""
    maps = []
    tanfov = inp.get("tanfov", TANFOV)
    for v in range(inp["depth"].shape[0]):
        if route == "reference":
            n = normals_reference_route(inp["w2c"][v], tanfov, inp["depth"][v], dtype)
        else:
            n = normals_camera_model(inp["cam_view"][v], tanfov, inp["depth"][v], dtype)
        maps.append(n.permute(2, 0, 1))
    return torch.stack(maps)


# ---- the loss terms --------------------------------------------------------------------------------------------------------------
def evaluate(inp, grad_out, route="reference", dtype=torch.float64, target=False, use_mask=False):
    """-> dict: 's' [V,3,H,W] (the surf normal of the normal term), 'means' [V,3], and the gradients of sum(grad_out * means) with
    respect to rend_normal, depth, dist and alpha, all in ``dtype``.  ``inp`` as make_inputs returns it (any device)."""
    leaves = {k: inp[k].detach().to(dtype).requires_grad_(True) for k in ("rend_normal", "depth", "dist", "alpha")}
    work = dict(inp, depth=leaves["depth"])
    mask = inp["mask"].to(dtype) if use_mask else None
    if target:
        s = inp["target_normal"].to(dtype) * (mask if mask is not None else 1)
    else:
        s = normal_maps(work, route, dtype) * leaves["alpha"].detach()
    normal_term = (1 - (leaves["rend_normal"] * s).sum(1)).mean((1, 2))
    dist_term = leaves["dist"].mean((1, 2, 3))
    alpha_term = (leaves["alpha"] - mask).abs().mean((1, 2, 3)) if mask is not None else 0 * leaves["alpha"].sum((1, 2, 3))
    means = torch.stack([normal_term, dist_term, alpha_term], 1)
    total = (means * grad_out.to(device=means.device, dtype=dtype)).sum() + 0 * sum(t.sum() for t in leaves.values())
    total.backward()
    out = {"s": s.detach(), "means": means.detach()}
    out.update({"grad_" + k: t.grad.detach() for k, t in leaves.items()})
    return out


GRAD_KEYS = ("grad_rend_normal", "grad_depth", "grad_dist", "grad_alpha")


def rel_l2(a, b):
    """|a - b| / |b| in float64 (0 / 0 = 0)"""
    a, b = a.double().cpu(), b.double().cpu()
    n = float(b.norm())
    d = float((a - b).norm())
    return d / n if n > 0 else d


def reference_errors(inp, grad_out, target=False, use_mask=False):
    """float64 reference route (the truth of the tests) and the errors of the reference's own fp32 route against it"""
    r64 = evaluate(inp, grad_out, "reference", torch.float64, target, use_mask)
    r32 = evaluate(inp, grad_out, "reference", torch.float32, target, use_mask)
    r64["E_map"] = float((r32["s"].double() - r64["s"]).abs().max())
    for k in GRAD_KEYS:
        r64["E_" + k] = rel_l2(r32[k], r64[k])
    return r64


def bars(ref):
    """the bars of the GPU tests: map E_map + 1e-6 per pixel, means 1e-6 relative, gradients E_grad + 2e-6 relative L2 per tensor"""
    out = {"map": ref["E_map"] + 1e-6, "means": 1e-6}
    out.update({k: ref["E_" + k] + 2e-6 for k in GRAD_KEYS})
    return out


def measured(ref, got):
    """errors of a candidate (kernel or model) against the float64 results of ``ref``; ``got`` may lack keys"""
    out = {}
    if got.get("s") is not None:
        out["map"] = float((got["s"].double().cpu() - ref["s"].cpu()).abs().max())
    if got.get("means") is not None:
        want = ref["means"].cpu()
        err = (got["means"].double().cpu() - want).abs()
        out["means"] = float(torch.where(want != 0, err / want.abs().clamp_min(1e-300), err).max())
    for k in GRAD_KEYS:
        if got.get(k) is not None:
            out[k] = rel_l2(got[k], ref[k])
    return out


def grad_weights(V):
    """[V,3] weights of the per-view means; for V = 2 the second view's normal weight is exactly 0"""
    return torch.tensor([[1.3, 0.4, 0.7], [0.0, 1.1, 0.5]][:V])


def write_section(name, lines):
    """replace (or append) the section ``name`` of profiles/geo_loss_bounds.txt; a read-only tree is not an error"""
    head = f"## {name}"
    try:
        old = open(BOUNDS_FILE).read().split("\n") if os.path.exists(BOUNDS_FILE) else []
        while old and old[-1] == "":
            old.pop()
        starts = [i for i, ln in enumerate(old) if ln.startswith("## ")]
        begin = next((i for i in starts if old[i].strip() == head), None)
        if begin is None:
            new = old + ([""] if old else []) + [head] + list(lines)
        else:
            end = next((i for i in starts if i > begin), len(old))
            new = old[:begin] + [head] + list(lines) + ([""] if end < len(old) else []) + old[end:]
        os.makedirs(os.path.dirname(BOUNDS_FILE), exist_ok=True)
        with open(BOUNDS_FILE, "w") as f:
            f.write("\n".join(new) + "\n")
    except OSError:
        pass
