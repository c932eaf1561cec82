"""View mini-batches of the surfel fitter without a GPU: ``fitting.view_schedule`` against its numpy restatement, what the constructor
refuses before anything is enqueued, and the ctypes mirror of ``GaFitSelectArgs`` against the compiled header."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ((5, 1), (5, 2), (6, 2), (5, 5), (7, 3))


def _restated(max_steps, P, B, seed):
    """the definition in the docstring of fitting.view_schedule, once more"""
    rng = np.random.default_rng(seed)
    n = -(-P // B)
    rows = []
    while len(rows) < max_steps:
        perm = rng.permutation(P)
        for r in range(n):
            row = list(perm[r * B:(r + 1) * B])
            row += list(perm[:B - len(row)])               # a short last row: completed from the start of the same permutation
            rows.append(row)
    return np.array(rows[:max_steps], np.int32)


@pytest.mark.parametrize("P,B", CASES)
def test_view_schedule(P, B):
    from gaussiananything_amd import fitting
    per_epoch = -(-P // B)
    max_steps = 3 * per_epoch + 1                            # three whole epochs and the first row of a fourth
    tab = fitting.view_schedule(max_steps, P, B, seed=4)
    assert isinstance(tab, torch.Tensor) and tab.dtype == torch.int32 and tuple(tab.shape) == (max_steps, B)
    assert tab.device.type == "cpu" and tab.is_contiguous()
    t = tab.numpy()
    assert np.array_equal(t, _restated(max_steps, P, B, 4))
    assert t.min() >= 0 and t.max() < P
    for row in t:
        assert len(set(row.tolist())) == B                   # no row holds a view twice
    for e in range(3):
        epoch = t[e * per_epoch:(e + 1) * per_epoch]
        assert set(epoch.ravel().tolist()) == set(range(P))  # every epoch covers the pool
        assert sorted(epoch.ravel()[:P].tolist()) == list(range(P))   # ... its first P entries are the permutation itself
    assert torch.equal(tab, fitting.view_schedule(max_steps, P, B, seed=4))
    assert torch.equal(tab, fitting.view_schedule(max_steps, P, B, 4))
    if P > 1:
        other = [fitting.view_schedule(max_steps, P, B, seed=s) for s in (5, 6, 7)]
        assert any(not torch.equal(tab, o) for o in other)
    assert torch.equal(fitting.view_schedule(max_steps, P, B), fitting.view_schedule(max_steps, P, B, seed=0))
    assert torch.equal(tab[:2], fitting.view_schedule(2, P, B, seed=4))       # a shorter table is a prefix


def test_view_schedule_refusals():
    from gaussiananything_amd import fitting
    with pytest.raises(ValueError, match="exceeds the pool"):
        fitting.view_schedule(10, 3, 4)
    with pytest.raises(ValueError, match="batch_views"):
        fitting.view_schedule(10, 3, 0)
    with pytest.raises(ValueError, match="max_steps"):
        fitting.view_schedule(0, 3, 1)
    with pytest.raises(ValueError, match="pool_views"):
        fitting.view_schedule(4, 0, 1)
    with pytest.raises(ValueError, match="seed"):
        fitting.view_schedule(4, 3, 1, seed=-1)


def _views(P=4, size=16, dtype=torch.float32):
    from gaussiananything_amd import synthetic
    cams = synthetic.eval_cameras(P)
    targets = torch.zeros(P, 3, size, size, dtype=dtype)
    return synthetic.random_surfels(10, seed=1), cams["cam_view"], cams["cam_view_proj"], cams["tanfov"], targets


def test_the_constructor_refuses_before_anything_is_enqueued():
    """every tensor is on the CPU, so a constructor that got past its checks would end in "no CPU path": each refusal below comes first"""
    from gaussiananything_amd import fitting
    ok = _views()
    good = fitting.view_schedule(8, 4, 2)
    with pytest.raises(ValueError, match="exceeds the pool"):
        fitting.SurfelFitter(*ok, max_steps=8, batch_views=5)
    with pytest.raises(ValueError, match="batch_views must be"):
        fitting.SurfelFitter(*ok, max_steps=8, batch_views=0)
    with pytest.raises(ValueError, match="batch_views must be"):
        fitting.SurfelFitter(*ok, max_steps=8, batch_views=-2)
    with pytest.raises(ValueError, match="batch_views must be"):
        fitting.SurfelFitter(*ok, max_steps=8, batch_views=2.0)
    for bad in (4, -1):
        sched = good.clone()
        sched[3, 1] = bad
        with pytest.raises(ValueError, match=r"outside \[0, 4\)"):
            fitting.SurfelFitter(*ok, max_steps=8, batch_views=2, view_schedule=sched)
    for sched in (good[:7], good[:, :1], good.reshape(-1), good.t().contiguous()):
        with pytest.raises(ValueError, match=r"view_schedule must be \[max_steps, batch_views\]"):
            fitting.SurfelFitter(*ok, max_steps=8, batch_views=2, view_schedule=sched)
    for sched in (good.float(), good.double(), good.bool(), good.tolist()):
        with pytest.raises(TypeError, match="integer torch.Tensor"):
            fitting.SurfelFitter(*ok, max_steps=8, batch_views=2, view_schedule=sched)
    with pytest.raises(ValueError, match="without batch_views"):
        fitting.SurfelFitter(*ok, max_steps=8, view_schedule=good)
    u8 = _views(dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8 targets are taken only with batch_views"):
        fitting.SurfelFitter(*u8, max_steps=8)
    # nothing wrong but the device: float and uint8 pools, the project's schedule and the caller's (an int64 one is taken)
    for args, kw in ((ok, dict(batch_views=2)), (u8, dict(batch_views=2)), (ok, dict(batch_views=2, view_schedule=good.long())),
                     (ok, dict(batch_views=4, view_seed=3))):
        with pytest.raises(ValueError, match="no CPU path"):
            fitting.SurfelFitter(*args, max_steps=8, **kw)


def test_select_args_mirror_has_the_layout_of_the_header(tmp_path):
    from gaussiananything_amd import _lib as _l
    cls = _l.GaFitSelectArgs
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "ga_fit.h"', "int main(void) {",
             '  printf("GA_FIT_SELECT_U8_TARGETS %d\\n", GA_FIT_SELECT_U8_TARGETS);',
             f'  printf("{cls.__name__} %zu\\n", sizeof({cls.__name__}));']
    for fname, _ in cls._fields_:
        lines.append(f'  printf("{cls.__name__}.{fname} %zu\\n", offsetof({cls.__name__}, {fname}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["GA_FIT_SELECT_U8_TARGETS"]) == _l.GA_FIT_SELECT_U8_TARGETS
    assert int(got[cls.__name__]) == ctypes.sizeof(cls)
    for fname, _ in cls._fields_:
        assert int(got[f"{cls.__name__}.{fname}"]) == getattr(cls, fname).offset, fname
    assert "ga_fit_select_views" in _l.EXPORTS
