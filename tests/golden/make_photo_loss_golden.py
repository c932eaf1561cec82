"""Writes tests/golden/photo_loss_ref.pt from the REFERENCE's own ``gaussian``, ``create_window`` and ``_ssim``
(nsr/losses/builder.py of the reference checkout named by GA_REFERENCE, default /root/reference).

The module cannot be imported whole here (it needs lpips and kornia), so, as ref_dit_loader.py does for ``XYZPosEmbed``, the three
function definitions are read out of the reference file at run time and exec'd; none of their text is committed.  The inputs are the
seeded families of tests/_ssim_ref.py; recorded are the family, seed and shape, both ``size_average`` outputs and the autograd
gradient of the ``size_average=True`` value with respect to img1.

    python tests/golden/make_photo_loss_golden.py
"""
import os
import sys
from math import exp

import torch
import torch.nn.functional as F
from torch.autograd import Variable

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import _ssim_ref as ref  # noqa: E402

REF = os.environ.get("GA_REFERENCE", "/root/reference")
CASES = [("uniform01", (2, 3, 37, 70), 11), ("uniform11", (1, 1, 11, 13), 12), ("near", (1, 4, 5, 23), 13), ("smooth", (2, 3, 33, 31), 14),
         ("const", (1, 3, 12, 40), 15), ("white", (2, 1, 37, 34), 16)]


def reference_functions():
    src = open(os.path.join(REF, "nsr", "losses", "builder.py")).read().split("\n")
    ns = {"torch": torch, "F": F, "Variable": Variable, "exp": exp}
    for name in ("gaussian", "create_window", "_ssim"):
        start = next(i for i, l in enumerate(src) if l.startswith(f"def {name}("))
        end = next(i for i in range(start + 1, len(src)) if src[i] and not src[i][0].isspace())
        exec("\n".join(src[start:end]), ns)
    return ns["create_window"], ns["_ssim"]


def main():
    create_window, _ssim = reference_functions()
    out = []
    for family, shape, seed in CASES:
        a, b = ref.make_inputs(family, shape, seed)
        window = create_window(11, shape[1]).type_as(a)
        x = a.clone().requires_grad_(True)
        mean = _ssim(x, b, window, 11, shape[1], True)
        mean.backward()
        per_image = _ssim(a, b, window, 11, shape[1], False)
        out.append({"family": family, "shape": list(shape), "seed": seed, "ssim": mean.detach().clone(), "ssim_per_image": per_image.detach().clone(),
                    "grad_img1": x.grad.detach().clone()})
    path = os.path.join(HERE, "photo_loss_ref.pt")
    torch.save({"torch": str(torch.__version__), "cases": out}, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
