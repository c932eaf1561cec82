"""``GaFilterViewsArgs`` and ``GaVoxelThinArgs`` of include/ga_pointcloud.h against their ctypes mirrors in gaussiananything_amd/_lib.py:
one compiled check of the sizes, every field offset and the constants, as tests/test_unproject_layout_cpu.py does for ``GaUnprojectArgs``."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pc_filter_ctypes_mirrors_have_the_layout_of_the_header(tmp_path):
    from gaussiananything_amd import _lib as _l
    mirrors = [_l.GaFilterViewsArgs, _l.GaVoxelThinArgs]
    consts = ("GA_PC_FILTER_THREADS", "GA_PC_FILTER_BAND_ROWS", "GA_PC_FILTER_MAX_ROWS", "GA_PC_VOXEL_FIRST", "GA_PC_VOXEL_CENTER",
              "GA_PC_VOXEL_MAX_INDEX", "GA_PC_VOXEL_WAVE_MERGE", "GA_PC_DEPTH_Z", "GA_PC_DEPTH_RAY", "GA_PC_CAMERA_FLOATS")
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "ga_pointcloud.h"', "int main(void) {"]
    lines += [f'  printf("{c} %d\\n", {c});' for c in consts]
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
    for c in consts:
        assert int(got[c]) == getattr(_l, c), c
    for cls in mirrors:
        assert int(got[cls.__name__]) == ctypes.sizeof(cls), cls.__name__
        for fname, _ in cls._fields_:
            assert int(got[f"{cls.__name__}.{fname}"]) == getattr(cls, fname).offset, (cls.__name__, fname)
    from tests import _pc_filter_ref as ref
    assert (ref.THREADS, ref.BAND_ROWS, ref.MAX_INDEX) == (_l.GA_PC_FILTER_THREADS, _l.GA_PC_FILTER_BAND_ROWS, _l.GA_PC_VOXEL_MAX_INDEX)
    assert (ref.VOXEL_FIRST, ref.VOXEL_CENTER, ref.DEPTH_Z, ref.DEPTH_RAY) == (_l.GA_PC_VOXEL_FIRST, _l.GA_PC_VOXEL_CENTER, _l.GA_PC_DEPTH_Z,
                                                                               _l.GA_PC_DEPTH_RAY)
