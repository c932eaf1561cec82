"""Fits the synthetic scene of profiles/densify_fit.txt from its POINTS and writes profiles/fit_from_points.txt: the loss curve of
``SurfelFitter.from_points`` (PCA frames) beside the same start with 2DGS's random rotations.

    python tools/fit_from_points.py [--out profiles/fit_from_points.txt]

The scene is that of tools/bench_densify.py's sparse fit: targets rendered from 400 surfels (4 views, 128^2), 400 iterations, the same
loss weights, no density control.  The cloud is the 400 surfel centres with their colours.  Both starts share positions, colours,
opacity and the scales of the distance rule; they differ in the rotation alone: the PCA frame of ``surfels_from_points`` against
``torch.rand(N, 4)``, which is what 2DGS's ``create_from_pcd`` draws.  One scene, one seed: a result, not a claim."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gaussiananything_amd import fitting, synthetic  # noqa: E402
from gaussiananything_amd.gs_surfel import GaussianRenderer2DGS  # noqa: E402

LAMBDAS = dict(l2=0.0, l1=0.8, ssim=0.2, lambda_normal=0.05, lambda_dist=0.0, lambda_alpha=0.0)      # tools/bench_densify.py's
STEPS, SIZE, VIEWS, K = 400, 128, 4, 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_from_points.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/fit_from_points.py needs the GPU: the fitter has no CPU path")
    dev = torch.device("cuda:0")
    cams = synthetic.eval_cameras(8)
    cv, cvp, cp = (cams[k][:VIEWS].to(dev) for k in ("cam_view", "cam_view_proj", "cam_pos"))
    g = synthetic.random_surfels(400, seed=3)
    g[..., 4:6] *= 8.0
    with torch.no_grad():
        targets = GaussianRenderer2DGS(SIZE, 3, {}).render(g.to(dev), cv[None], cvp[None], cp[None], cams["tanfov"])["image"][0].contiguous()
    points, colors = g[0, :, 0:3].to(dev), g[0, :, 10:13].clamp(0.02, 0.98).to(dev)
    kw = dict(max_steps=STEPS, **LAMBDAS)
    start = fitting.surfels_from_points(points, colors=colors, K=K)
    random_rot = start.clone()
    random_rot[:, 6:10] = torch.rand(400, 4, generator=torch.Generator().manual_seed(0)).to(dev)
    runs = [("from_points: PCA frames", fitting.SurfelFitter.from_points(points, cv, cvp, cams["tanfov"], targets, colors=colors, K=K, **kw)),
            ("the same scales, 2DGS's random rotations (torch.rand(N, 4), seed 0)", fitting.SurfelFitter(random_rot, cv, cvp, cams["tanfov"], targets, **kw))]
    marks = list(range(0, STEPS, 50)) + [STEPS - 1]
    lines = [f"# tools/fit_from_points.py: targets rendered from 400 surfels ({VIEWS} views, {SIZE}^2), the fit started from their 400 centres and",
             f"# colours; {STEPS} iterations, no density control, K = {K}, opacity 0.1, scale_factor 1.0; initial scale: median "
             f"{float(start[:, 4].median()):.4f}, min {float(start[:, 4].min()):.4f}, max {float(start[:, 4].max()):.4f}; "
             f"rows with opacity 0 (invalid): {int((start[:, 3] == 0).sum())}",
             "# loss at iteration:  " + "  ".join(f"{t:>9}" for t in marks)]
    final = []
    for name, f in runs:
        f.step(STEPS)
        h = f.loss_history()["loss"]
        final.append(float(h[-1]))
        lines.append(f"{name}\n    loss             " + "  ".join(f"{float(h[t]):9.5f}" for t in marks))
        print("\n".join(lines[-1:]), flush=True)
    better = "PCA frames end lower" if final[0] < final[1] else "random rotations end lower"
    lines.append(f"# final loss: PCA frames {final[0]:.5f}, random rotations {final[1]:.5f}: {better} by {abs(final[0] - final[1]):.5f} "
                 f"({100 * abs(final[0] - final[1]) / max(final):.1f} %).  The cloud is 400 points drawn uniformly in a box, not samples of a "
                 "surface: its PCA planes describe no geometry the targets show.  One scene, one seed.")
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
