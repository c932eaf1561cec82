"""Writes tests/golden/unproject_ref.pt from the REFERENCE's own ray sampler and the tensor lines of its depth -> ``fps-K.ply`` script
(nsr/volumetric_rendering/ray_sampler.py and scripts/save_pcd.py:325-395 of the reference checkout named by GA_REFERENCE, default
/root/reference).

``RaySampler`` is imported from its file (the module needs torch alone).  The script cannot be imported (it is a training entry point
with a dozen absent dependencies), so, as make_geo_loss_golden.py does, the statements are read out of the reference file at run time
and exec'd one by one; none of their text is committed.  Each is located by its line number and checked against the name it assigns,
so a reference that moved fails loudly here.

Inputs: 3 views x 24 x 24, the first three poses of cameras_eval8.npz, a seeded synthetic ray-distance depth in [1.2, 2.4] around the
object with holes (0) and a few values under the reference's 1.05 filter, and an alpha mask with the values 0, 0.5 and 1.  Recorded:
the inputs, the points the reference keeps and their pixels, and the reference's own largest deviation from the float64 geometry
(tests/_unproject_ref.py: lift_f64) over the kept points.  Before writing, the script checks what tests/test_unproject_cpu.py (a)
needs of the fixture: the reference keeps the pixels float64 keeps, up to at most 2 that lie within one fp32 ulp of the clip boundary.

    python tests/golden/make_unproject_golden.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import _unproject_ref as ref  # noqa: E402

REF = os.environ.get("GA_REFERENCE", "/root/reference")
V, S = 3, 24
# (first line, last line, the name the statement assigns) in scripts/save_pcd.py
STATEMENTS = [(325, 325, "cam2world_matrix"), (326, 326, "intrinsics"), (328, 329, "ray_origins, ray_directions"), (344, 344, "fg_mask"),
              (359, 359, "fg_mask"), (361, 361, "depth"), (362, 362, "depth"), (363, 363, "depth[depth == 0]"), (381, 381, "gt_pos"),
              (382, 382, "gt_pos"), (388, 388, "gt_pos"), (389, 389, "gt_pos"), (390, 390, "gt_pos"), (394, 394, "nonzero_mask"),
              (395, 395, "nonzero_gt_pos")]


def inputs():
    rng = np.random.default_rng(20261020)
    z = np.load(os.path.join(HERE, "cameras_eval8.npz"))
    c = z["poses"][:V].astype(np.float32)
    dist = np.linalg.norm(c[:, [3, 7, 11]].astype(np.float64), axis=1)                     # camera to the origin
    yy, xx = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    bump = 0.22 * np.sin(0.7 * xx + 0.3)[None] * np.cos(0.5 * yy - 0.2)[None] + rng.uniform(-0.12, 0.12, size=(V, S, S))
    depth = np.clip(dist[:, None, None] - 0.2 + bump, 1.2, 2.4).astype(np.float32)
    depth[rng.uniform(size=depth.shape) < 0.08] = 0.0                                        # holes
    depth[rng.uniform(size=depth.shape) < 0.03] = np.float32(0.9)                            # under the reference's 1.05 filter
    alpha = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), size=(V, S, S), p=[0.15, 0.15, 0.7]).astype(np.float32)
    return c, depth, alpha


def reference_kept(c, depth, alpha):
    spec = importlib.util.spec_from_file_location("ref_ray_sampler", os.path.join(REF, "nsr", "volumetric_rendering", "ray_sampler.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lines = open(os.path.join(REF, "scripts", "save_pcd.py")).read().split("\n")

    class _Dist:
        @staticmethod
        def dev():
            return "cpu"

    ns = {"th": torch, "dist_util": _Dist, "ray_sampler": mod.RaySampler(), "B": V, "img_size": S,
          "sample": {"c": torch.from_numpy(c), "depth": torch.from_numpy(depth.copy()), "alpha_mask": torch.from_numpy(alpha)}}
    ns["micro"] = ns["sample"]
    for first, last, name in STATEMENTS:
        text = "\n    ".join(l.strip() for l in lines[first - 1:last])      # (a continuation line may be indented freely inside brackets)
        assert text.startswith(name + " ="), f"scripts/save_pcd.py:{first} no longer assigns {name}: {text[:60]!r}"
        exec(text, ns)
    keep = ns["nonzero_mask"].numpy()
    return ns["nonzero_gt_pos"].numpy().astype(np.float32), np.flatnonzero(keep).astype(np.int32)


def main():
    c, depth, alpha = inputs()
    points, source = reference_kept(c, depth, alpha)
    cam = ref.cameras_from_pose25(c)
    exact = ref.lift_f64(depth, cam, ref.DEPTH_RAY).reshape(-1, 3)
    deviation = float(np.abs(points.astype(np.float64) - exact[source]).max())
    # what float64 keeps under the reference's rules
    ok64 = ((depth >= np.float32(1.05)) & (alpha == 1)).reshape(-1) & (np.abs(exact) < 0.45).all(1) & (exact != 0).all(1)
    differ = np.flatnonzero(ok64 != np.isin(np.arange(ok64.size), source))
    ulp = float(np.spacing(np.float32(0.45)))
    near = np.abs(np.abs(exact[differ]) - 0.45).min(1) <= ulp if len(differ) else np.zeros(0, bool)
    assert len(differ) <= 2 and near.all(), f"{len(differ)} pixels kept differently by the reference and float64: choose other inputs"
    inside = int(len(source))
    assert 200 <= inside <= V * S * S - 200, f"{inside} kept points: the inputs should keep some and drop some"
    torch.save({"c": torch.from_numpy(c), "depth": torch.from_numpy(depth), "alpha_mask": torch.from_numpy(alpha),
                "points": torch.from_numpy(points), "source": torch.from_numpy(source), "deviation_from_float64": deviation,
                "K": 64}, os.path.join(HERE, "unproject_ref.pt"))
    print(f"kept {inside} of {V * S * S} pixels; reference vs float64: largest deviation {deviation:.3e}, {len(differ)} pixels kept differently")


if __name__ == "__main__":
    main()
