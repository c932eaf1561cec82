"""Writes tests/golden/geo_loss_ref.pt from the REFERENCE's own ``depths_to_points_2`` and ``depth_to_normal_2``
(utils/point_utils.py of the reference checkout named by GA_REFERENCE, default /root/reference).

The module cannot be imported whole here (it needs cv2, matplotlib and point_cloud_utils), so, as make_photo_loss_golden.py does, the
two function definitions are read out of the reference file at run time and exec'd; none of their text is committed.  They hard-code
``.cuda()`` and ``device='cuda'``; on a machine without a GPU they run on the CPU with ``torch.Tensor.cuda`` patched to the identity
for the duration of the calls and, inside the exec namespace only, a thin proxy of ``torch`` whose ``arange`` drops ``device=``.

The inputs are the seeded families and look-at cameras of tests/_geo_ref.py, one view per case.  Recorded per case: family, seed,
shape, the view matrix (column-vector world-to-camera, as the function takes it), tanfov, the normal map [H,W,3], and the autograd
gradient with respect to depth of ``mean(1 - sum_c rend_normal_c * normal_c * alpha)`` for the seeded rend_normal and alpha of that
case.  alpha is set to 0 wherever the reference's normal is 0 (asserted), so torch's G / 1e-12 through ``F.normalize`` of a vanishing
cross product never enters the fixture; the alpha used is recorded too.

    python tests/golden/make_geo_loss_golden.py
"""
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import _geo_ref as ref  # noqa: E402

REF = os.environ.get("GA_REFERENCE", "/root/reference")
CASES = [("sphere", (37, 70), 11), ("plane", (37, 70), 12), ("noisy", (37, 70), 13), ("holes", (37, 70), 14), ("holes", (16, 16), 15),
         ("sphere", (3, 3), 16), ("plane", (33, 31), 17), ("noisy", (65, 34), 18)]


class _TorchOnCpu:
    """``torch`` for the exec namespace: everything is torch's, except that ``arange`` ignores ``device=``"""

    def __getattr__(self, name):
        return getattr(torch, name)

    @staticmethod
    def arange(*args, **kwargs):
        kwargs.pop("device", None)
        return torch.arange(*args, **kwargs)


def reference_functions():
    src = open(os.path.join(REF, "utils", "point_utils.py")).read().split("\n")
    ns = {"torch": _TorchOnCpu(), "math": math}
    for name in ("depths_to_points_2", "depth_to_normal_2"):
        start = next(i for i, l in enumerate(src) if l.startswith(f"def {name}("))
        end = next((i for i in range(start + 1, len(src)) if src[i] and not src[i][0].isspace()), len(src))
        exec("\n".join(src[start:end]), ns)
    return ns["depth_to_normal_2"]


def main():
    depth_to_normal_2 = reference_functions()
    out = []
    saved_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        for family, (H, W), seed in CASES:
            inp = ref.make_inputs(family, (1, H, W), seed)
            w2c, depth = inp["w2c"][0], inp["depth"][0]                     # [4,4], [1,H,W]
            with torch.no_grad():
                normal = depth_to_normal_2(w2c, ref.TANFOV, W, H, depth)    # [H,W,3]
            zero = (normal == 0).all(-1)
            alpha = torch.where(zero, torch.zeros(H, W), inp["alpha"][0, 0])
            assert bool((alpha[zero] == 0).all()) and bool(zero[0].all() and zero[-1].all() and zero[:, 0].all() and zero[:, -1].all())
            d = depth.clone().requires_grad_(True)
            n = depth_to_normal_2(w2c, ref.TANFOV, W, H, d).permute(2, 0, 1)
            (1 - (inp["rend_normal"][0] * n * alpha[None]).sum(0)).mean().backward()
            assert bool(torch.isfinite(d.grad).all())
            out.append({"family": family, "seed": seed, "shape": [H, W], "w2c": w2c.clone(), "tanfov": ref.TANFOV,
                        "normal": normal.clone(), "alpha": alpha.clone(), "grad_depth": d.grad.detach().clone()})
    finally:
        torch.Tensor.cuda = saved_cuda
    path = os.path.join(HERE, "geo_loss_ref.pt")
    torch.save({"torch": str(torch.__version__), "cases": out}, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
