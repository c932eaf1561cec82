"""Times ``mesh.sample_points_from_mesh`` (ga_mesh_sample) and ``mesh.point_mesh_distance`` (ga_mesh_point_distance) against what a user
composes in torch today, on the same device in the same process, and writes profiles/mesh_ops_bench.txt.

    python tools/bench_mesh_ops.py [--rounds 9] [--out profiles/mesh_ops_bench.txt]

The meshes are triangulated height fields (a sine bump over a regular grid): 999 698, 20 480 and 1 280 faces.  The torch side of the
sampling: face areas -> ``cumsum`` -> ``torch.rand`` + ``searchsorted`` -> barycentric weights -> gathers, in fp32 (what
pytorch3d's sampler does with ``multinomial`` in place of the search).  The torch side of the distance: the same region test written
with broadcasting over [queries, faces] blocks of at most 2^26 pairs, ``min`` per block, merged with ``where`` -- there is no
point-to-triangle operator in torch.  The sides are timed alternately with device events around the whole Python call after a warm-up
of each; the table reports the median and the range.  The two sides of the distance are compared before they are timed."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from gaussiananything_amd import mesh  # noqa: E402

PAIRS_PER_BLOCK = 1 << 26


def height_field(nx, ny, dev):
    """2 (nx - 1) (ny - 1) triangles over [-0.45, 0.45]^2 with z = 0.1 sin(7 x) cos(5 y) -> (vertices [V,3], faces [F,3] int32)"""
    x, y = torch.meshgrid(torch.linspace(-0.45, 0.45, nx, device=dev), torch.linspace(-0.45, 0.45, ny, device=dev), indexing="ij")
    v = torch.stack([x, y, 0.1 * torch.sin(7 * x) * torch.cos(5 * y)], -1).reshape(-1, 3)
    i, j = torch.meshgrid(torch.arange(nx - 1, device=dev), torch.arange(ny - 1, device=dev), indexing="ij")
    a = (i * ny + j).reshape(-1)
    f = torch.cat([torch.stack([a, a + ny, a + 1], 1), torch.stack([a + 1, a + ny, a + ny + 1], 1)])
    return v.contiguous(), f.to(torch.int32).contiguous()


def torch_sample(v, f, S, gen):
    tri = v[f.long()]
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    area = torch.linalg.cross(b - a, c - a).norm(dim=1)
    cum = torch.cumsum(area, 0)
    u = torch.rand(S, device=v.device, generator=gen) * cum[-1]
    face = torch.searchsorted(cum, u, right=True).clamp(max=f.shape[0] - 1)
    r = torch.rand(S, 2, device=v.device, generator=gen)
    s = r[:, 0].sqrt()
    w0, w1, w2 = 1 - s, s * (1 - r[:, 1]), s * r[:, 1]
    return w0[:, None] * a[face] + w1[:, None] * b[face] + w2[:, None] * c[face], face


def _block_dist2(p, a, ab, ac):
    """[n, m] squared distances of queries p [n,1,3] to triangles (a, ab, ac) [1,m,3]: Ericson 5.1.5 with ``where``"""
    dot = lambda x, y: (x * y).sum(-1)   # noqa: E731
    ap = p - a
    d1, d2 = dot(ab, ap), dot(ac, ap)
    abab, abac, acac = dot(ab, ab), dot(ab, ac), dot(ac, ac)
    d3, d4, d5, d6 = d1 - abab, d2 - abac, d1 - abac, d2 - acac
    vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
    e, g = d4 - d3, d5 - d6
    zero, one = torch.zeros_like(d1), torch.ones_like(d1)
    r = 1 / ((va + vb) + vc)
    v, w = vb * r, vc * r                                                     # interior, then the regions from last to first
    t = e / (e + g)
    m = (va <= 0) & (e >= 0) & (g >= 0)
    v, w = torch.where(m, 1 - t, v), torch.where(m, t, w)
    m = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
    v, w = torch.where(m, zero, v), torch.where(m, d2 / (d2 - d6), w)
    m = (d6 >= 0) & (d5 <= d6)
    v, w = torch.where(m, zero, v), torch.where(m, one, w)
    m = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
    v, w = torch.where(m, d1 / (d1 - d3), v), torch.where(m, zero, w)
    m = (d3 >= 0) & (d4 <= d3)
    v, w = torch.where(m, one, v), torch.where(m, zero, w)
    m = (d1 <= 0) & (d2 <= 0)
    v, w = torch.where(m, zero, v), torch.where(m, zero, w)
    d = ap - ab * v[..., None] - ac * w[..., None]
    return dot(d, d)


def torch_distance(p, v, f):
    tri = v[f.long()]
    a, ab, ac = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    N, F = p.shape[0], f.shape[0]
    qn = min(N, 4096)
    fm = max(1, PAIRS_PER_BLOCK // qn)
    best = torch.full((N,), float("inf"), device=p.device)
    face = torch.full((N,), -1, dtype=torch.int64, device=p.device)
    for q0 in range(0, N, qn):
        pq = p[q0:q0 + qn, None, :]
        for f0 in range(0, F, fm):
            d, j = _block_dist2(pq, a[None, f0:f0 + fm], ab[None, f0:f0 + fm], ac[None, f0:f0 + fm]).min(dim=1)
            better = d < best[q0:q0 + qn]
            best[q0:q0 + qn] = torch.where(better, d, best[q0:q0 + qn])
            face[q0:q0 + qn] = torch.where(better, j + f0, face[q0:q0 + qn])
    return best, face


def time_many(fns, rounds):
    """alternating timings of the callables -> one list of times in ms per callable"""
    out = [[] for _ in fns]
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    for _ in range(rounds):
        for fn, acc in zip(fns, out):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            acc.append(start.elapsed_time(stop))
    return out


def cell(times):
    return f"{statistics.median(times):9.3f} [{min(times):8.3f} ..{max(times):8.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_ops_bench.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mesh_ops.py needs the GPU: a timing on anything else says nothing")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    big, mid, small = height_field(708, 708, dev), height_field(81, 129, dev), height_field(21, 33, dev)
    queries = lambda n: (torch.rand(n, 3, device=dev, generator=gen) - 0.5) * torch.tensor([0.9, 0.9, 0.4], device=dev)   # noqa: E731
    lines = [f"# tools/bench_mesh_ops.py --rounds {a.rounds}   device: {torch.cuda.get_device_name(0)}",
             "# times in ms: median [min .. max] of alternating rounds, device events around the whole Python call, allocations included.",
             "# HIP = mesh.sample_points_from_mesh (ga_mesh_sample, three launches) / mesh.point_mesh_distance (ga_mesh_point_distance,",
             "# three launches, brute force over all faces); torch = the composition described at the top of the tool, fp32.",
             "# pairs/s = rows x faces over the HIP median: each pair is about 90 fp32 operations, none of them fused.",
             f"{'operation':<10} {'rows':>8} {'faces':>9} {'HIP':>9} {'':<21} {'torch':>9} {'':<21} {'torch / HIP':>11}  note"]
    jobs = [("sample", 100000, big), ("sample", 100000, small), ("distance", 4096, big), ("distance", 100000, mid)]
    for op, rows, (v, f) in jobs:
        F = f.shape[0]
        if op == "sample":
            hip, ref = (lambda v=v, f=f: mesh.sample_points_from_mesh(v, f, rows, seed=1)), (lambda v=v, f=f: torch_sample(v, f, rows, gen))
            note = ""
        else:
            p = queries(rows)
            hip, ref = (lambda p=p, v=v, f=f: mesh.point_mesh_distance(p, v, f)), (lambda p=p, v=v, f=f: torch_distance(p, v, f))
            got, want = hip(), ref()
            worst = float((got.dist2 - want[0]).abs().max())
            note = f"max |dist2 - torch's| {worst:.2e}, {int((got.face != want[1]).sum())} of {rows} faces differ"
        t = time_many([hip, ref], a.rounds)
        mh, mt = statistics.median(t[0]), statistics.median(t[1])
        verdict = "HIP faster" if mh < mt else "HIP LOSES at this shape"
        if op == "distance":
            note = f"{rows * F / (mh * 1e-3):.3e} pairs/s; " + note
        lines.append(f"{op:<10} {rows:>8} {F:>9} {cell(t[0])}  {cell(t[1])}  {mt / mh:10.2f}x  {verdict}{'; ' + note if note else ''}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
