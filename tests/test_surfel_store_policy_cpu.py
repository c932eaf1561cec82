"""Host side of the store-policy field of GaSurfelForwardArgs.flags (include/ga_surfel.h, bits 4..11): it decodes to the documented
per-site policies, the undefined value 3 is refused by name and not ignored, and the Python mirror agrees with the header's macros."""
import ctypes
import itertools
import os
import subprocess

from gaussiananything_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GA_ERR_NULL_ARG, GA_ERR_BAD_FLAGS = -1, -5


def _decode(L, flags):
    out = (ctypes.c_int32 * 4)(-1, -1, -1, -1)
    return L.ga_surfel_store_policy(flags, ctypes.byref(out)), list(out)


def test_store_policy_field_decodes_per_site_and_rejects_the_undefined_value():
    L = _lib.lib()
    assert _lib._ERR[GA_ERR_BAD_FLAGS] == "GA_ERR_BAD_FLAGS"
    assert L.ga_surfel_store_policy(0, None) == GA_ERR_NULL_ARG
    other = (_lib.GA_SURFEL_FLAG_STATS | _lib.GA_SURFEL_FLAG_WORKSPACE_CLEAN | _lib.GA_SURFEL_FLAG_SPLIT_WALK |
             _lib.GA_SURFEL_FLAG_BG_IN_BLEND | (1 << 12))          # the neighbouring bits do not leak into the field
    for pol in itertools.product(range(4), repeat=4):              # (preprocess, fill, sort, blend)
        flags = _lib.store_flags(*pol)
        assert flags & ~(0xFF << 4) == 0
        assert flags == sum(p << (4 + 2 * site) for site, p in enumerate(pol))
        for extra in (0, other):
            rc, got = _decode(L, flags | extra)
            if 3 in pol:
                assert rc == GA_ERR_BAD_FLAGS and got == [-1] * 4, pol
            else:
                assert rc == 0 and got == list(pol), pol
    assert _decode(L, _lib.GA_SURFEL_STORE_DEFAULT)[0] == 0
    # the forward refuses the undefined value before it looks at anything else (no GPU needed), and only that value
    args = _lib.GaSurfelForwardArgs()
    args.num_points, args.num_views, args.image_height, args.image_width = 10, 1, 64, 64
    for site in range(4):
        args.flags = 3 << (4 + 2 * site)
        assert L.ga_surfel_forward(ctypes.byref(args), None) == GA_ERR_BAD_FLAGS
    args.flags = _lib.store_flags(1, 2, 1, 2)
    assert L.ga_surfel_forward(ctypes.byref(args), None) == GA_ERR_NULL_ARG        # (the pointers are missing: the next check)


def test_python_store_flags_mirror_the_header_macros(tmp_path):
    src = tmp_path / "policy.c"
    src.write_text('#include <stdio.h>\n#include "ga_surfel.h"\nint main(void) {\n'
                   '  printf("%d %d %d %d %d %d %d\\n", GA_SURFEL_STORE_FLAGS(1, 2, 0, 1), GA_SURFEL_STORE_FLAGS(2, 0, 1, 2), GA_SURFEL_STORE_DEFAULT,\n'
                   '         GA_SURFEL_STORE_MASK, GA_ERR_BAD_FLAGS, GA_SURFEL_STORE_WRITE_THROUGH, GA_SURFEL_STORE_NONTEMPORAL);\n  return 0;\n}\n')
    exe = tmp_path / "policy"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [_lib.store_flags(1, 2, 0, 1), _lib.store_flags(2, 0, 1, 2), _lib.GA_SURFEL_STORE_DEFAULT, 0xFF << 4, GA_ERR_BAD_FLAGS,
                   _lib.GA_SURFEL_STORE_WRITE_THROUGH, _lib.GA_SURFEL_STORE_NONTEMPORAL]
