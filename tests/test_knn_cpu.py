"""CPU tests of the k-nearest-neighbour operations (include/ga_pointcloud.h): the restatements against each other, the host
validation of the C-ABI (no launch happens for a rejected call, so no GPU is needed), the plan, the ctypes mirrors and the host-side
checks of the Python front end."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import _knn_ref as kref
from tests import _pointcloud_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GA_ERR_NULL_ARG, GA_ERR_BAD_SHAPE = -1, -2


@pytest.mark.parametrize("nq,nt,distinct,K", [(65, 63, 20, 32), (130, 1025, 300, 17), (40, 40, 1, 8)])
def test_fp32_knn_agrees_with_float64_brute_force_on_lattice_clouds(nq, nt, distinct, K):
    """Coordinates k/64: every operation is exact in fp32, so the stable argsort and the sort of explicit (distance, index) tuples
    must agree index for index and distance for distance; duplicated targets make most adjacent list entries exact ties."""
    q = ref.lattice_cloud(nq, seed=nq + 2)
    t = ref.lattice_cloud(nt, seed=nt + 3, distinct=distinct)
    d32, i32 = kref.knn_f32(q, t, K)
    d64, i64 = kref.knn_f64(q, t, K)
    assert d32.dtype == np.float32 and i32.shape == (nq, min(K, nt))
    assert np.array_equal(i32, i64) and np.array_equal(d32.astype(np.float64), d64)
    ties = float(np.mean(d32[:, 1:] == d32[:, :-1]))
    print(f"knn lattice {nq} x {nt} ({distinct} distinct) K {K}: {ties:.2f} of adjacent entries tie")
    assert ties > 0.2   # the tie rule is exercised
    assert (np.diff(d32, axis=1) >= 0).all() and (np.diff(i32, axis=1)[d32[:, 1:] == d32[:, :-1]] > 0).all()
    if distinct == 1:
        assert np.array_equal(i32, np.tile(np.arange(K), (nq, 1)))


def test_fp32_gradient_restatement_is_within_the_derived_bound_of_float64():
    q, t = ref.uniform_cloud((300,), seed=43), ref.uniform_cloud((1025,), seed=143)
    K = 16
    _, idx = kref.knn_f32(q, t, K)
    w = np.random.default_rng(5).uniform(-1, 1, size=(300, K)).astype(np.float32)
    gq32, gt32 = kref.knn_backward_f32(q, t, idx, w)
    gq64, gt64, (mq, aq), (mt, at) = kref.knn_backward_f64(q, t, idx, w)
    assert gq32.dtype == np.float32 and gt32.dtype == np.float32
    assert mq.min() == K and mq.max() == K and mt.sum() == 3 * 300 * K and mt.max() > 4
    bq, bt = kref.grad_bound(mq, aq), kref.grad_bound(mt, at)
    eq, et = np.abs(gq32.astype(np.float64) - gq64), np.abs(gt32.astype(np.float64) - gt64)
    print(f"worst error / bound: query {np.max(eq / bq):.3f}, target {np.max(et[mt > 0] / bt[mt > 0]):.3f}, fan-in up to {mt[:, 0].max()}")
    assert (eq <= bq).all() and (et <= bt).all()
    assert not gt32[mt == 0].any()   # targets nobody selected: exactly 0 (the bound there is 0 as well)


def _lib():
    from gaussiananything_amd import _lib
    return _lib, _lib.lib()


def test_knn_host_validation_rejects_before_any_launch():
    """Fake, non-NULL device addresses: a call that got past validation would fault; every one here must be turned away."""
    _l, L = _lib()
    P = 0x1000   # never dereferenced

    def call(B=2, Nq=10, Nt=20, k=4, query=P, target=P, out_d=P, out_i=P):
        a = _l.GaKnnArgs(B, Nq, Nt, k, query, target, None, None, out_d, out_i)
        return L.ga_pc_knn(ctypes.byref(a), None)

    assert L.ga_pc_knn(None, None) == GA_ERR_NULL_ARG
    for kw in (dict(query=None), dict(target=None), dict(out_d=None), dict(out_i=None)):
        assert call(**kw) == GA_ERR_NULL_ARG, kw
    for kw in (dict(B=0), dict(B=65536), dict(Nq=0), dict(Nt=0), dict(Nq=-1), dict(Nt=-1), dict(k=0), dict(k=-1), dict(k=33),
               dict(Nq=(1 << 31) // 3 + 1, k=1), dict(Nt=(1 << 31) // 3 + 1), dict(Nq=1 << 26, k=32), dict(Nq=(1 << 27), k=16)):
        assert call(**kw) == GA_ERR_BAD_SHAPE, kw


def test_knn_backward_host_validation_rejects_before_any_launch():
    _l, L = _lib()
    P = 0x1000

    def call(B=2, Nq=10, Nt=20, k=4, query=P, target=P, idx=P, grad=P, gq=P, gt=P):
        a = _l.GaKnnBackwardArgs(B, Nq, Nt, k, query, target, None, None, idx, grad, gq, gt)
        return L.ga_pc_knn_backward(ctypes.byref(a), None)

    assert L.ga_pc_knn_backward(None, None) == GA_ERR_NULL_ARG
    for kw in (dict(query=None), dict(target=None), dict(idx=None), dict(grad=None)):
        assert call(**kw) == GA_ERR_NULL_ARG, kw
    for kw in (dict(B=0), dict(B=65536), dict(Nq=0), dict(Nt=0), dict(k=0), dict(k=-3), dict(Nq=(1 << 31) // 3 + 1, k=1),
               dict(Nt=(1 << 31) // 3 + 1), dict(Nq=1 << 26, k=32)):
        assert call(**kw) == GA_ERR_BAD_SHAPE, kw
    assert call(gq=None, gt=None) == 0   # nothing asked for: nothing launched


def test_knn_plan_is_host_only_and_monotone_in_k():
    _l, L = _lib()
    pl = _l.GaKnnPlan()
    assert L.ga_pc_knn_plan(100, 100, 4, None) == GA_ERR_NULL_ARG
    for bad in ((0, 100, 4), (100, 0, 4), (100, 100, 0), (100, 100, 33), (1 << 26, 100, 32), ((1 << 31) // 3 + 1, 100, 1)):
        assert L.ga_pc_knn_plan(*bad, ctypes.byref(pl)) == GA_ERR_BAD_SHAPE, bad
    prev = 0
    classes = set()
    for k in range(1, 33):
        assert L.ga_pc_knn_plan(1000, 5000, k, ctypes.byref(pl)) == 0
        assert pl.k_slots >= k and pl.k_slots >= prev and pl.k_slots <= 32
        assert pl.threads > 0 and pl.threads % 64 == 0 and pl.tile > 0 and pl.tile % 4 == 0
        assert pl.grid_x == -(-1000 // pl.threads) and pl.grid_y == 1
        prev = pl.k_slots
        classes.add(pl.k_slots)
    assert 1 in classes and 32 in classes
    from gaussiananything_amd import pointcloud
    d = pointcloud.knn_plan(4096, 4096, 8)
    assert set(d) == {"k_slots", "threads", "tile", "grid_x", "grid_y"} and d["k_slots"] >= 8 and d["grid_x"] * d["threads"] >= 4096
    with pytest.raises(RuntimeError):
        pointcloud.knn_plan(4096, 4096, 33)


def test_knn_ctypes_mirrors_have_the_layout_of_the_header(tmp_path):
    from gaussiananything_amd import _lib as _l
    mirrors = [_l.GaKnnArgs, _l.GaKnnPlan, _l.GaKnnBackwardArgs]
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "ga_pointcloud.h"', "int main(void) {",
             '  printf("GA_PC_KNN_MAX_K %d\\n", GA_PC_KNN_MAX_K);']
    for cls in mirrors:
        lines.append(f'  printf("{cls.__name__} %zu\\n", sizeof({cls.__name__}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cls.__name__}.{fname} %zu\\n", offsetof({cls.__name__}, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["GA_PC_KNN_MAX_K"]) == _l.GA_PC_KNN_MAX_K == 32
    for cls in mirrors:
        assert int(got[cls.__name__]) == ctypes.sizeof(cls), cls.__name__
        for fname, _ in cls._fields_:
            assert int(got[f"{cls.__name__}.{fname}"]) == getattr(cls, fname).offset, (cls.__name__, fname)


def test_knn_front_end_validates_on_the_host():
    import torch
    from gaussiananything_amd import pointcloud
    a, b = torch.zeros(1, 10, 3), torch.zeros(1, 12, 3)
    with pytest.raises(RuntimeError):   # GPU only, no fallback
        pointcloud.knn_points(a, b, K=2)
    with pytest.raises(ValueError, match="32"):
        pointcloud.knn_points(a, b, K=33)
    with pytest.raises(ValueError):
        pointcloud.knn_points(a, b, K=0)
    with pytest.raises(ValueError):
        pointcloud.knn_points(a, b, norm=3)
    with pytest.raises(NotImplementedError):
        pointcloud.knn_points(a, b, norm=1)
    with pytest.raises(ValueError):
        pointcloud.knn_points(torch.zeros(10, 3), b)
    with pytest.raises(RuntimeError):
        pointcloud.chamfer_distance(a, b, differentiable=True)   # CPU tensors
    with pytest.raises(RuntimeError):
        pointcloud.remove_statistical_outliers(torch.zeros(1, 100, 3))
    with pytest.raises(RuntimeError, match="forward only"):
        pointcloud.chamfer_distance(torch.zeros(1, 4, 3, requires_grad=True), torch.zeros(1, 4, 3), differentiable=False)
    with pytest.raises(ValueError):
        pointcloud.chamfer_distance(a, b, differentiable=True, point_reduction="max")


def test_knn_gather_is_pytorch3d_s_definition():
    """plain torch, so it runs anywhere: out[b,n,k] = x[b, idx[b,n,k]], zero where k >= lengths[b]; differentiable in x"""
    import torch
    from gaussiananything_amd.pointcloud import knn_gather
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 7, 5, generator=g, requires_grad=True)
    idx = torch.randint(0, 7, (2, 4, 3), generator=g)
    out = knn_gather(x, idx, lengths=torch.tensor([7, 2]))
    assert out.shape == (2, 4, 3, 5)
    for b in range(2):
        for n in range(4):
            for k in range(3):
                want = x[b, idx[b, n, k]] if k < (7, 2)[b] else torch.zeros(5)
                assert torch.equal(out[b, n, k], want.detach())
    out.sum().backward()
    counts = torch.zeros(2, 7)
    for b in range(2):
        for n in range(4):
            for k in range(min(3, (7, 2)[b])):
                counts[b, idx[b, n, k]] += 1
    assert torch.equal(x.grad, counts[:, :, None].expand(-1, -1, 5))
    assert torch.equal(knn_gather(x.detach(), idx), x.detach()[torch.arange(2)[:, None, None], idx])
