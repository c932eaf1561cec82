"""Restatement of the photometric loss (include/ga_loss.h) for the tests: the reference's ``gaussian`` / ``create_window`` / ``_ssim``
and the loss composition, written from their formulas, parametrised by dtype, with the gradient through torch autograd.  Runs on
whatever device its inputs are on.  Also the seeded input families, the case list the CPU and GPU tests share, the error bars of the
issue ('Numerics') and the section writer of profiles/photo_loss_bounds.txt."""
import math
import os

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_FILE = os.path.join(ROOT, "profiles", "photo_loss_bounds.txt")
WINDOW, SIGMA = 11, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def gaussian(window_size=WINDOW, sigma=SIGMA):
    """fp32 taps from double exponentials, normalised by their fp32 sum"""
    g = torch.tensor([math.exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2)) for x in range(window_size)], dtype=torch.float32)
    return g / g.sum()


def create_window(channel, dtype=torch.float32, device="cpu"):
    """[C,1,11,11]: the fp32 outer product of the taps (rounded in fp32, as the reference builds it), then cast"""
    g = gaussian().unsqueeze(1)
    w2 = g.mm(g.t()).float()
    return w2.expand(channel, 1, WINDOW, WINDOW).contiguous().to(device=device, dtype=dtype)


def _conv2d(x, channel, dtype):
    return F.conv2d(x, create_window(channel, dtype, x.device), padding=WINDOW // 2, groups=channel)


def _conv_separable(x, channel, dtype):
    """rows, then columns, with the 1-D taps: the model of a separable kernel"""
    g = gaussian().to(device=x.device, dtype=dtype)
    x = F.conv2d(x, g.view(1, 1, 1, WINDOW).expand(channel, 1, 1, WINDOW).contiguous(), padding=(0, WINDOW // 2), groups=channel)
    return F.conv2d(x, g.view(1, 1, WINDOW, 1).expand(channel, 1, WINDOW, 1).contiguous(), padding=(WINDOW // 2, 0), groups=channel)


def moments(img1, img2, dtype=torch.float32, separable=False):
    conv = _conv_separable if separable else _conv2d
    c = img1.shape[1]
    return (conv(img1, c, dtype), conv(img2, c, dtype), conv(img1 * img1, c, dtype), conv(img2 * img2, c, dtype),
            conv(img1 * img2, c, dtype))


def ssim_from_moments(mu1, mu2, e11, e22, e12):
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq, sigma2_sq, sigma12 = e11 - mu1_sq, e22 - mu2_sq, e12 - mu1_mu2
    return ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))


def ssim_map(img1, img2, dtype=torch.float32, separable=False):
    return ssim_from_moments(*moments(img1.to(dtype), img2.to(dtype), dtype, separable))


def photo_means(img1, img2, dtype=torch.float32, separable=False):
    """-> (map [N,C,H,W], means [N,3]: SSIM, L1, L2 per image)"""
    x, y = img1.to(dtype), img2.to(dtype)
    m = ssim_map(x, y, dtype, separable)
    d = x - y
    return m, torch.stack([m.mean((1, 2, 3)), d.abs().mean((1, 2, 3)), (d * d).mean((1, 2, 3))], 1)


def evaluate(img1, img2, grad_out, dtype=torch.float32, separable=False):
    """-> (map, means [N,3], gradient of sum(grad_out * means) with respect to img1), all in ``dtype``"""
    x = img1.detach().to(dtype).requires_grad_(True)
    m, means = photo_means(x, img2.detach(), dtype, separable)
    (means * grad_out.to(device=x.device, dtype=dtype)).sum().backward()
    return m.detach(), means.detach(), x.grad.detach()


def ssim(img1, img2, size_average=True, dtype=torch.float32):
    m = ssim_map(img1, img2, dtype)
    return m.mean() if size_average else m.mean(1).mean(1).mean(1)


def photometric_loss(inp, gt, l2_lambda=1.0, l1_lambda=0.0, ssim_lambda=0.0, dtype=torch.float32):
    """the composition of the reference's ``calc_2d_rec_loss`` (MSE criterion, no LPIPS / identity terms), every term always evaluated"""
    x, y = inp.to(dtype), gt.to(dtype)
    mse, l1, s = F.mse_loss(x, y), F.l1_loss(x, y), ssim(x, y, True, dtype)
    loss = mse * l2_lambda + (1 - s) * ssim_lambda + l1_lambda * l1
    return loss, {"loss": loss, "loss_l2": mse * l2_lambda, "loss_ssim": 1 - s, "mae": l1, "PSNR": 10 * torch.log10(4 / mse.detach()),
                  "SSIM": s}


# ---- inputs --------------------------------------------------------------------------------------------------------------------
FAMILIES = ("uniform01", "uniform11", "near", "smooth", "const", "white")


def make_inputs(family, shape, seed):
    """-> (img1, img2) fp32 CPU tensors of ``shape`` [N,C,H,W], a function of (family, shape, seed) alone"""
    g = torch.Generator().manual_seed(int(seed))
    N, C, H, W = shape

    def u():
        return torch.rand(shape, generator=g)

    if family == "uniform01":
        return u(), u()
    if family == "uniform11":
        return u() * 2 - 1, u() * 2 - 1
    if family == "near":
        a = u()
        return a, a + 0.02 * torch.randn(shape, generator=g)
    if family == "smooth":
        def s():
            coarse = torch.rand(N, C, 3, 4, generator=g)
            return F.interpolate(coarse, size=(H, W), mode="bilinear", align_corners=True).contiguous()
        return s(), s()
    if family == "const":
        return 0.7 + 1e-3 * torch.randn(shape, generator=g), torch.full(shape, 0.7)
    if family == "white":
        return 1 - 0.05 * u(), torch.ones(shape)
    raise ValueError(family)


def shapes_hw(T):
    return [1, 5, 7, 10, 11, T - 1, T, T + 1, 2 * T + 3]


def cases(T):
    """about 40 (family, (N,C,H,W), seed): every side length of ``shapes_hw`` as a height and as a width, 37 x 70, every family, every C
    of {1, 3, 4} and N of {1, 2}.  The shape list walks H up and W down, so nearly every case is non-square."""
    sides = shapes_hw(T)
    out = []
    k = 0
    hw = [(h, sides[-1 - i]) for i, h in enumerate(sides)]                      # 9: H ascending against W descending
    hw += [(sides[(i + 3) % len(sides)], w) for i, w in enumerate(sides)]       # 9: another pairing
    hw += [(37, 70), (70, 37), (T, T), (2 * T + 3, 2 * T + 3), (1, 1), (T + 1, 1)]
    for h, w in hw:
        for rep in range(2 if (h, w) in ((37, 70), (2 * T + 3, 2 * T + 3)) else 1):
            out.append((FAMILIES[k % 6], ((1, 2)[(k // 2) % 2], (1, 3, 4)[k % 3], h, w), 100 + k))
            k += 1
    # every family on the one shape with several tiles both ways and on a sub-window image
    for fam in FAMILIES:
        out.append((fam, (2, 3, 37, 70), 200 + len(out)))
        out.append((fam, (1, 1, 7, T + 1), 200 + len(out)))
    return out


def grad_weights(N, which):
    """[N,3] weights of the per-image means. 'ssim': SSIM only; 'mixed': all three, and for N = 2 the second image at exactly 0"""
    if which == "ssim":
        return torch.tensor([[1.3, 0.0, 0.0], [0.6, 0.0, 0.0]][:N])
    return torch.tensor([[0.7, 0.3, 1.1], [0.0, 0.0, 0.0]][:N])


# ---- bars ('Numerics' of the issue) -------------------------------------------------------------------------------------------------
def rel_l2(a, b):
    """|a - b| / |b| in float64 (0 / 0 = 0)"""
    a, b = a.double().cpu(), b.double().cpu()
    n = float(b.norm())
    d = float((a - b).norm())
    return d / n if n > 0 else d


def reference_errors(img1, img2, grad_out):
    """the fp32 restatement (2-D window) against the float64 one on this input -> dict with the float64 results and E_map, E_mean,
    E_grad; computed on the CPU"""
    m64, mean64, g64 = evaluate(img1.cpu(), img2.cpu(), grad_out.cpu(), torch.float64)
    m32, mean32, g32 = evaluate(img1.cpu(), img2.cpu(), grad_out.cpu(), torch.float32)
    return {"map": m64, "means": mean64, "grad": g64,
            "E_map": float((m32.double() - m64).abs().max()),
            "E_mean": float((mean32[:, 0].double() - mean64[:, 0]).abs().max()),
            "E_grad": rel_l2(g32, g64)}


def bars(ref):
    return {"map": 2 * ref["E_map"] + 2e-6, "mean": 2 * ref["E_mean"] + 1e-6, "grad": 2 * ref["E_grad"] + 2e-6, "l1l2": 1e-6}


def measured(ref, got_map, got_means, got_grad):
    """errors of a candidate (kernel or model) against the float64 results of ``ref``"""
    gm = got_means.double().cpu()
    out = {"map": float((got_map.double().cpu() - ref["map"]).abs().max()) if got_map is not None else 0.0,
           "mean": float((gm[:, 0] - ref["means"][:, 0]).abs().max()),
           "grad": rel_l2(got_grad, ref["grad"]) if got_grad is not None else 0.0,
           "l1l2": float(((gm[:, 1:] - ref["means"][:, 1:]).abs() / ref["means"][:, 1:].abs().clamp_min(1e-300)).max())}
    return out


def write_section(name, lines):
    """replace (or append) the section ``name`` of profiles/photo_loss_bounds.txt; a read-only tree is not an error"""
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
        text = "\n".join(new) + "\n"
        os.makedirs(os.path.dirname(BOUNDS_FILE), exist_ok=True)
        with open(BOUNDS_FILE, "w") as f:
            f.write(text)
    except OSError:
        pass
