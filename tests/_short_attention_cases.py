"""The case table of ga_attention_short_bf16 (short key lists, Lk <= 128, head dim 64), in the conventions of tests/_attention_cases.py
(whose case dicts, inputs, float64 reference and bound these cases use unchanged): every key length of {1, 37, 64, 77, 100, 128} with
every query length of {1, 5, 48, 768}; q given (with and without its per-head norm) and q projected inside the workgroup with
qp_k in {64, 1024}, the weight tiled and row-major, with and without the folded row scale, with and without the per-head norm; every
input family.  tests/test_t23d_cpu.py emulates the kernel's rounding model on every case against the bound; tests/test_t23d_short_gpu.py
runs every case on the GPU, every output element checked."""
from tests import _attention_cases as ac

KEY_LENGTHS = (1, 37, 64, 77, 100, 128)
QUERY_LENGTHS = (1, 5, 48, 768)
MODES = [(None, norm) for norm in ("", "q")] + [(dict(K=K, tiled=tiled, row_ss=rss), norm) for K in (64, 1024) for tiled in (False, True)
                                                for rss in (False, True) for norm in ("", "q")]


def _name(Lq, Lk, fam, qp, norm, B, H):
    mode = "q" if qp is None else f"qp{qp['K']}{'t' if qp['tiled'] else 'r'}{'s' if qp['row_ss'] else ''}"
    return f"short_{mode}_{B}x{H}x{Lq}x{Lk}_{fam}" + (f"_n{norm}" if norm else "")


def _case(Lq, Lk, fam, qp, norm, B, H):
    return ac.A(_name(Lq, Lk, fam, qp, norm, B, H), "fwd", B, H, Lq, Lk, fam, norm=norm, qp=qp)


CASES = []
_n = 0
for _Lk in KEY_LENGTHS:
    for _Lq in QUERY_LENGTHS:
        for _j in range(3):     # three (mode, family) pairs per geometry; the pairing shifts every round of the mode list
            _qp, _norm = MODES[_n % len(MODES)]
            _fam = ac.FAMILIES[(_n + _n // len(MODES)) % len(ac.FAMILIES)]
            CASES.append(_case(_Lq, _Lk, _fam, _qp, _norm, *((1, 2) if _Lq == 768 else (2, 3))))
            _n += 1
# the caption length with every family, q given and projected in turn
for _i, _fam in enumerate(ac.FAMILIES):
    _qp, _norm = (None, "q") if _i % 2 else (dict(K=1024, tiled=True, row_ss=True), "q")
    CASES.append(_case(48, 77, _fam, _qp, _norm, 2, 3))
# the release shapes: one sample's conditional half with the projection inside, a CFG pair with q given
CASES += [_case(768, 77, "planted8", dict(K=1024, tiled=True, row_ss=True), "q", 1, 16), _case(768, 77, "planted14", None, "", 2, 16)]

assert len({c["name"] for c in CASES}) == len(CASES)
assert {c["family"] for c in CASES} == set(ac.FAMILIES)
assert {(c["Lq"], c["Lk"]) for c in CASES} >= {(q, k) for q in QUERY_LENGTHS for k in KEY_LENGTHS}
for _qp, _norm in MODES:
    assert any(c["qp"] == _qp and c["norm"] == _norm for c in CASES)
