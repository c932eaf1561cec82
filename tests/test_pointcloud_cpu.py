"""CPU tests of the point-cloud operations (include/ga_pointcloud.h): the oracle's tie rule, the host validation of the C-ABI (no
launch happens for a rejected call, so no GPU is needed), the plan, the ctypes mirrors, and the host-side checks of the cascade."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import _pointcloud_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GA_ERR_NULL_ARG, GA_ERR_BAD_SHAPE, GA_ERR_WORKSPACE = -1, -2, -3


@pytest.mark.parametrize("n,distinct,K,start", [(1, None, 3, 0), (2, None, 2, 1), (300, None, 300, 7), (400, 150, 400, 0),
                                                 (100, 1, 10, 0), (2000, 900, 64, 1999)])
def test_fp32_fps_agrees_with_float64_brute_force_on_lattice_clouds(n, distinct, K, start):
    """Coordinates k/64, |k| <= 32: every square and sum is exact in fp32, so the fp32 restatement (``argmax``) and the float64 brute
    force (explicit lowest index among the farthest) must agree index for index, duplicates included."""
    p = ref.lattice_cloud(n, seed=n + K, distinct=distinct)
    if distinct is not None:
        assert len(np.unique(p, axis=0)) < n
    a, b = ref.fps_f32(p, K, start), ref.fps_f64(p, K, start)
    assert a.dtype == np.int64 and len(a) == min(K, n) and a[0] == start
    assert np.array_equal(a, b)
    if distinct == 1:
        assert np.array_equal(a[1:], np.zeros(len(a) - 1, np.int64))   # everything covered at distance 0: lowest index from then on


@pytest.mark.parametrize("nq,nt,distinct", [(1, 1, None), (65, 63, None), (500, 700, 200), (300, 40, 5)])
def test_fp32_nearest_agrees_with_float64_brute_force_on_lattice_clouds(nq, nt, distinct):
    q = ref.lattice_cloud(nq, seed=nq)
    t = ref.lattice_cloud(nt, seed=nt + 1, distinct=distinct)
    d32, i32 = ref.nearest_f32(q, t)
    d64, i64 = ref.nearest_f64(q, t)
    assert np.array_equal(i32, i64) and np.array_equal(d32.astype(np.float64), d64)


def _lib():
    from gaussiananything_amd import _lib
    return _lib, _lib.lib()


def _plan(N, K=1):
    _l, L = _lib()
    pl = _l.GaFpsPlan()
    assert L.ga_pc_fps_plan(N, K, ctypes.byref(pl)) == 0
    return pl.variant, pl.threads, pl.points_per_lane


def _first_streaming_n():
    lo, hi = 1, 1 << 24   # the plan is monotone (checked below), so bisect the boundary
    assert _plan(lo)[0] == 0 and _plan(hi)[0] == 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if _plan(mid)[0] == 0 else (lo, mid)
    return hi


def test_fps_host_validation_rejects_before_any_launch():
    """Fake, non-NULL device addresses: a call that got past validation would fault; every one here must be turned away."""
    _l, L = _lib()
    P = 0x1000   # never dereferenced
    big = _first_streaming_n()

    def call(B=2, N=100, K=10, points=P, out_idx=P, out_points=P, workspace=None, nbytes=0):
        a = _l.GaFpsArgs(B, N, K, points, None, None, out_idx, out_points, workspace, nbytes)
        return L.ga_pc_fps(ctypes.byref(a), None)

    assert L.ga_pc_fps(None, None) == GA_ERR_NULL_ARG
    assert call(points=None) == GA_ERR_NULL_ARG
    assert call(out_idx=None) == GA_ERR_NULL_ARG
    for kw in (dict(B=0), dict(B=-1), dict(N=0), dict(N=-5), dict(K=0), dict(K=-1), dict(B=65536), dict(N=(1 << 31) // 3 + 1)):
        assert call(**kw) == GA_ERR_BAD_SHAPE, kw
    need = L.ga_pc_fps_workspace_bytes(2, big, 10)
    assert need == 2 * big * 4
    assert call(N=big, workspace=P, nbytes=need - 1) == GA_ERR_WORKSPACE
    assert call(N=big, workspace=P, nbytes=0) == GA_ERR_WORKSPACE
    assert call(N=big, workspace=None, nbytes=need) == GA_ERR_NULL_ARG
    pl = _l.GaFpsPlan()
    assert L.ga_pc_fps_plan(100, 10, None) == GA_ERR_NULL_ARG
    assert L.ga_pc_fps_plan(0, 10, ctypes.byref(pl)) == GA_ERR_BAD_SHAPE
    assert L.ga_pc_fps_plan(10, 0, ctypes.byref(pl)) == GA_ERR_BAD_SHAPE


def test_nearest_host_validation_rejects_before_any_launch():
    _l, L = _lib()
    P = 0x1000

    def call(B=2, Nq=10, Nt=20, query=P, target=P, out_d=P, out_i=P):
        a = _l.GaNearestArgs(B, Nq, Nt, query, target, None, None, out_d, out_i)
        return L.ga_pc_nearest(ctypes.byref(a), None)

    assert L.ga_pc_nearest(None, None) == GA_ERR_NULL_ARG
    for kw in (dict(query=None), dict(target=None), dict(out_d=None), dict(out_i=None)):
        assert call(**kw) == GA_ERR_NULL_ARG, kw
    for kw in (dict(B=0), dict(Nq=0), dict(Nt=0), dict(Nq=-1), dict(Nt=-1), dict(B=65536), dict(Nt=(1 << 31) // 3 + 1)):
        assert call(**kw) == GA_ERR_BAD_SHAPE, kw


def test_fps_plan_is_monotone_and_consistent_with_the_workspace():
    _l, L = _lib()
    ns = sorted(set(list(range(1, 300)) + [2 ** e + d for e in range(8, 21) for d in (-1, 0, 1)] + [5000, 73728, 100000]))
    prev = None
    seen = set()
    for N in ns:
        variant, threads, ppl = _plan(N)
        seen.add(variant)
        assert threads in (64, 256, 1024) and threads * ppl >= N
        need = L.ga_pc_fps_workspace_bytes(3, N, 7)
        if variant == _l.GA_FPS_VARIANT_REGISTER:
            assert need == 0 and ppl <= 16
        else:
            assert need == 3 * N * 4 and ppl == -(-N // threads)
        if prev is not None:   # variant, workgroup and register slots never shrink as the cloud grows
            assert variant >= prev[0] and (variant != prev[0] or (threads >= prev[1] and threads * ppl >= prev[1] * prev[2]))
        prev = (variant, threads, ppl)
        assert _plan(N, 1) == _plan(N, 4096)   # K does not change the variant
    assert seen == {_l.GA_FPS_VARIANT_REGISTER, _l.GA_FPS_VARIANT_STREAMING}   # both reachable
    na = _first_streaming_n() - 1
    assert _plan(na)[0] == 0 and _plan(na + 1)[0] == 1 and L.ga_pc_fps_workspace_bytes(1, na, 1) == 0
    assert L.ga_pc_fps_workspace_bytes(0, 100, 1) == 0 and L.ga_pc_fps_workspace_bytes(1, 0, 1) == 0


def test_pointcloud_ctypes_mirrors_have_the_layout_of_the_header(tmp_path):
    from gaussiananything_amd import _lib as _l
    mirrors = [_l.GaFpsArgs, _l.GaFpsPlan, _l.GaNearestArgs]
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "ga_pointcloud.h"', "int main(void) {"]
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
    for cls in mirrors:
        assert int(got[cls.__name__]) == ctypes.sizeof(cls), cls.__name__
        for fname, _ in cls._fields_:
            assert int(got[f"{cls.__name__}.{fname}"]) == getattr(cls, fname).offset, (cls.__name__, fname)


def test_cloud_to_condition_rejects_a_cloud_that_is_too_small():
    import torch
    from gaussiananything_amd import cascade
    with pytest.raises(ValueError):
        cascade.cloud_to_condition(torch.zeros(1, 767, 3), 768)
    with pytest.raises(ValueError):
        cascade.cloud_to_condition(torch.zeros(2, 1000, 3), 768, lengths=[1000, 700])
    with pytest.raises(ValueError):
        cascade.cloud_to_condition(torch.zeros(1000, 3), 768)
    same = cascade.cloud_to_condition(torch.full((1, 768, 3), 0.7), 768)   # N == num_points: clipped, order kept, no kernel needed
    assert same.shape == (1, 768, 3) and float(same.max()) == pytest.approx(0.45)


def test_python_front_end_validates_on_the_host():
    import torch
    from gaussiananything_amd import pointcloud
    with pytest.raises(RuntimeError):   # GPU only, no fallback
        pointcloud.sample_farthest_points(torch.zeros(1, 10, 3), K=2)
    with pytest.raises(ValueError):
        pointcloud.sample_farthest_points(torch.zeros(10, 3), K=2)
    with pytest.raises(RuntimeError):
        pointcloud.chamfer_distance(torch.zeros(1, 4, 3, requires_grad=True), torch.zeros(1, 4, 3))
    with pytest.raises(ValueError):
        pointcloud.chamfer_distance(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3), point_reduction="max")
    assert pointcloud.fps_plan(100)["variant"] == "register" and pointcloud.fps_plan(1 << 20)["variant"] == "streaming"
