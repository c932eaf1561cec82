"""``GaUnprojectArgs`` of include/ga_pointcloud.h against its ctypes mirror in gaussiananything_amd/_lib.py: one compiled check of
the size, every field offset and the constants, as tests/test_normals_cpu.py does for the structs before it."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_unproject_ctypes_mirror_has_the_layout_of_the_header(tmp_path):
    from gaussiananything_amd import _lib as _l
    mirrors = [_l.GaUnprojectArgs]
    consts = ("GA_PC_DEPTH_Z", "GA_PC_DEPTH_RAY", "GA_PC_COLOR_F32", "GA_PC_COLOR_U8", "GA_PC_UNPROJECT_THREADS",
              "GA_PC_UNPROJECT_TILE_PIXELS", "GA_PC_UNPROJECT_MAX_WIDTH", "GA_PC_UNPROJECT_MAX_ERODE", "GA_PC_CAMERA_FLOATS")
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
    from tests import _unproject_ref as ref
    assert (ref.THREADS, ref.TILE_PIXELS) == (_l.GA_PC_UNPROJECT_THREADS, _l.GA_PC_UNPROJECT_TILE_PIXELS)
