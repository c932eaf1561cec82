"""Restatement of include/ga_fit.h in numpy float32, operation by operation (every product, quotient, sum and square root a float32
operation of its own, in the written order), plus the float64 / float32 torch loops the CPU tests measure it against.  Shared by
tests/test_fit_cpu.py and tests/test_fit_gpu.py; nothing here touches the device."""
import numpy as np
import torch

F = np.float32
GROUP_OF_COLUMN = (0, 0, 0, 1, 2, 2, 3, 3, 3, 3, 4, 4, 4)   # xyz, opacity, scale, rotation, rgb
SLICES = {"xyz": slice(0, 3), "opacity": slice(3, 4), "scale": slice(4, 6), "rotation": slice(6, 10), "rgb": slice(10, 13)}


def sigmoid(r):
    r = np.asarray(r, F)
    return F(1) / (F(1) + np.exp(-r))


def quat_norm(q):
    """sqrt(w*w + x*x + y*y + z*z), the sum taken in that order; q [N,4] float32"""
    q = np.asarray(q, F)
    return np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])


def activate(raw):
    """raw [N,13] float32 -> dict of means [N,3], opacities [N], colors [N,3], scales [N,2], rotations [N,4], inv_norm [N]"""
    raw = np.asarray(raw, F)
    norm = quat_norm(raw[:, 6:10])
    return {"means": raw[:, 0:3].copy(), "opacities": sigmoid(raw[:, 3]), "scales": np.exp(raw[:, 4:6]),
            "rotations": raw[:, 6:10] / norm[:, None], "inv_norm": F(1) / norm, "colors": sigmoid(raw[:, 10:13])}


def packed(act):
    """the [N,13] Gaussian tensor of the activated arrays"""
    return np.concatenate([act["means"], act["opacities"][:, None], act["scales"], act["rotations"], act["colors"]], axis=1)


def chain_rule(grads, act):
    """grads: dict of g_means [N,3], g_opacities [N], g_colors [N,3], g_scales [N,2], g_rotations [N,4] with respect to the ACTIVATED
    values; act: what ``activate`` (or the kernel) returned -> the gradient in raw space [N,13]"""
    g = {k: np.asarray(v, F) for k, v in grads.items()}
    o, c, s, q, inv = act["opacities"], act["colors"], act["scales"], act["rotations"], act["inv_norm"]
    out = np.empty((o.shape[0], 13), F)
    out[:, 0:3] = g["g_means"]
    out[:, 3] = g["g_opacities"] * (o * (F(1) - o))
    out[:, 4:6] = g["g_scales"] * s
    gq = g["g_rotations"]
    dot = ((q[:, 0] * gq[:, 0] + q[:, 1] * gq[:, 1]) + q[:, 2] * gq[:, 2]) + q[:, 3] * gq[:, 3]
    out[:, 6:10] = (gq - q * dot[:, None]) * inv[:, None]
    out[:, 10:13] = g["g_colors"] * (c * (F(1) - c))
    return out


def adam_step(raw, m, v, g, row, betas=(0.9, 0.999), eps=1e-15, keep=None):
    """one step on float32 arrays [N,13]; ``row`` is one row of the step table (float32 [8]); ``keep`` [N] bool: rows left untouched
    (GA_FIT_VISIBLE_ONLY) -> (raw', m', v')"""
    b1, omb1, b2, omb2, e = F(betas[0]), F(1.0 - betas[0]), F(betas[1]), F(1.0 - betas[1]), F(eps)
    row = np.asarray(row, F)
    step = row[np.asarray(GROUP_OF_COLUMN)][None, :]
    sbc2 = row[5]
    with np.errstate(all="ignore"):
        m1 = b1 * m + omb1 * g
        v1 = b2 * v + (omb2 * g) * g
        denom = np.sqrt(v1) / sbc2 + e
        raw1 = raw - step * (m1 / denom)
    if keep is not None:
        k = np.asarray(keep, bool)[:, None]
        raw1, m1, v1 = np.where(k, raw, raw1), np.where(k, m, m1), np.where(k, v, v1)
    return raw1.astype(F), m1.astype(F), v1.astype(F)


def lr_at(spec, t, max_steps):
    """double: a constant, or a (first, last) pair decaying log-linearly from step 0 to step max_steps - 1"""
    if isinstance(spec, (tuple, list)):
        a, b = float(spec[0]), float(spec[1])
        if max_steps == 1:
            return a
        return float(np.exp(np.log(a) + (np.log(b) - np.log(a)) * (t / (max_steps - 1))))
    return float(spec)


def table(lr, betas, max_steps):
    """the step table in double [max_steps, 8]: five step sizes lr_g(t) / (1 - b1^(t+1)), sqrt(1 - b2^(t+1)), two zeros"""
    out = np.zeros((max_steps, 8), np.float64)
    for t in range(max_steps):
        for k, name in enumerate(("xyz", "opacity", "scale", "rotation", "rgb")):
            out[t, k] = lr_at(lr[name], t, max_steps) / (1.0 - float(betas[0]) ** (t + 1))
        out[t, 5] = np.sqrt(1.0 - float(betas[1]) ** (t + 1))
    return out


# ---- the torch loops the restatement is measured against (CPU) -------------------------------------------------------------------
def torch_activate(raw):
    """autograd-visible activation of raw [N,13] (any float dtype) -> the packed [N,13] Gaussian tensor"""
    q = raw[:, 6:10]
    return torch.cat([raw[:, 0:3], torch.sigmoid(raw[:, 3:4]), torch.exp(raw[:, 4:6]), q / q.pow(2).sum(1, keepdim=True).sqrt(),
                      torch.sigmoid(raw[:, 10:13])], dim=1)


def torch_loop(raw0, grads, lr, betas, eps, max_steps, dtype):
    """``len(grads)`` steps of torch.optim.Adam with five param groups on the five column groups of raw0 [N,13]; grads[t] is the [N,13]
    gradient with respect to the ACTIVATED values, taken through ``torch_activate`` by autograd -> raw after every step [T,N,13]"""
    leaves = {k: torch.tensor(np.asarray(raw0)[:, s], dtype=dtype).requires_grad_(True) for k, s in SLICES.items()}
    opt = torch.optim.Adam([{"params": [leaves[k]], "lr": lr_at(lr[k], 0, max_steps)} for k in SLICES], betas=betas, eps=eps)
    out = []
    for t, g in enumerate(grads):
        for group, k in zip(opt.param_groups, SLICES):
            group["lr"] = lr_at(lr[k], t, max_steps)
        opt.zero_grad(set_to_none=True)
        act = torch_activate(torch.cat([leaves[k] for k in SLICES], dim=1))
        (act * torch.tensor(np.asarray(g), dtype=dtype)).sum().backward()
        opt.step()
        out.append(torch.cat([leaves[k].detach() for k in SLICES], dim=1).double().numpy().copy())
    return np.stack(out)


def ref_loop(raw0, grads, lr, betas, eps, max_steps):
    """the same steps through the float32 restatement, with the float32-rounded table -> raw after every step [T,N,13] (float32)"""
    tab = table(lr, betas, max_steps).astype(F)
    raw = np.asarray(raw0, F).copy()
    m, v = np.zeros_like(raw), np.zeros_like(raw)
    out = []
    for t, g in enumerate(grads):
        act = activate(raw)
        g = np.asarray(g, F)
        graw = chain_rule({"g_means": g[:, 0:3], "g_opacities": g[:, 3], "g_scales": g[:, 4:6], "g_rotations": g[:, 6:10],
                           "g_colors": g[:, 10:13]}, act)
        raw, m, v = adam_step(raw, m, v, graw, tab[t], betas, eps)
        out.append(raw.copy())
    return np.stack(out)


def ulp(x):
    """float32 spacing at |x| (float64 array)"""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(F)).astype(np.float64)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))
