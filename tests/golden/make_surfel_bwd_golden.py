"""Writes tests/golden/surfel_bwd_long_ref.pt: the float64 gradients of oracle/surfel_autograd.py (this repository's own backward
oracle) for the two one-tile scenes of 2200 surfels of tests/_bwd_bars.py ("long_transparent", "long_mixed"), whose lists lie beyond
the 2048 entries at which the forward blends in segments.  The oracle needs about ten seconds per scene, too long for a GPU test, so
its results are frozen here; tests/test_surfel_backward_cpu.py regenerates one of the two and compares.

Recorded per scene: the arguments of ``_bwd_bars.scene`` (the inputs and the upstream-gradient weights are regenerated from the seed),
the loss, and the five gradient tensors (means3D, opacities, colors, scales, rotations) as float64.

    python tests/golden/make_surfel_bwd_golden.py
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import _bwd_bars as bb  # noqa: E402


def main():
    out = {}
    for name in bb.LONG:
        ((loss, grads),), _ = bb.oracle_gradients(bb.named_scene(name))
        out[name] = dict(args=dict(bb.SCENES[name][0]), loss=float(loss), grads=[g.double().contiguous() for g in grads])
        print(name, "loss", float(loss), [tuple(g.shape) for g in grads])
    path = os.path.join(HERE, bb.LONG_FIXTURE)
    torch.save(out, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
