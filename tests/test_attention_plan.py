"""CPU test of the attention case table (tests/_attention_cases.py) through ga_attention_plan / ga_attention_hd_plan: the cases reach
every kernel instance the two dispatchers can launch -- listed by the library itself (ga_attention_instances,
ga_attention_hd_instances) -- at every key- and query-axis geometry that the instance's structure distinguishes, with every input
family.  A dispatcher change that makes another instance reachable fails here until a case reaches it."""
import ctypes

import pytest

from tests import _attention_cases as ac

# instance -> why no case reaches it without an environment override
UNREACHABLE = {("hdv", h, cfg): "configuration %d of the V^T variant is taken only when GA_ATTN_HD_QF forces it (dit_attention_hd.hip, "
                                "hdv_config); tests/test_dit_gpu.py runs it in child processes" % cfg
               for h in range(1, 9) for cfg in (1, 2)}


@pytest.fixture(scope="module")
def plans():
    return {c["name"]: ac.plan_of(c)[0] for c in ac.CASES}


def _instances():
    from gaussiananything_amd import dit_ops as ops
    fwd, hd = ops.attention_instances(), ops.attention_hd_instances()
    cells = [ac.cell(p) for p in fwd + hd]
    assert len(set(cells)) == len(cells), "an instance is listed twice"
    forced = {ac.cell(p) for p in hd if p.forced}
    return set(cells), forced


def test_every_reachable_attention_instance_has_a_case(plans):
    instances, forced = _instances()
    assert forced == set(UNREACHABLE), "the library's forced-only flags and the UNREACHABLE table disagree"
    hit = {}
    for c in ac.CASES:
        cell = ac.cell(plans[c["name"]])
        assert cell in instances, (c["name"], cell)
        hit.setdefault(cell, c["name"])
        if c["qp"]:
            assert plans[c["name"]].fuses_q == 1
            hit.setdefault(cell + ("qproj",), c["name"])
    print(f"{len(instances - forced)} reachable instances, {len(forced)} forced-only")
    for cell in sorted(instances, key=str):
        print(cell, "->", hit.get(cell, "UNREACHABLE: " + UNREACHABLE.get(cell, "?")))
    print(("fwd", 4, 3, 0, 1, "qproj"), "->", hit.get(("fwd", 4, 3, 0, 1, "qproj")))
    assert not set(hit) & set(UNREACHABLE), "an instance listed as unreachable is reached"
    missing = sorted((instances - forced) - set(hit), key=str)
    assert not missing, f"no case reaches {missing}"
    assert ("fwd", 4, 3, 0, 1, "qproj") in hit


def _groups(c, p):
    """how the case's tiles fall onto the plan's key groups / stages"""
    tiles = (c["Lk"] + 63) // 64
    tps = p.tps if hasattr(p, "tps") else 1
    return tiles, tps, p.ks


def test_every_instance_meets_every_geometry_and_family(plans):
    """per instance class (the fwd instances, fwd with the q projection, the two product configurations of hdv over all HD16, hd over
    all HDP): the key-axis geometries, the query-axis geometries and the input families that must each be met by some case"""
    seen = {}
    for c in ac.CASES:
        p = plans[c["name"]]
        cell = ac.cell(p)
        cls = cell if cell[0] == "fwd" else (("hdv", "config", cell[2]) if cell[0] == "hdv" else ("hd",))
        if c["qp"]:
            cls = cls + ("qproj",)
        tiles, tps, ks = _groups(c, p)
        Lq, Lk = c["Lq"], c["Lk"]
        tags = {"family " + c["family"], f"tiles {tiles}" if tiles <= 4 else "tiles > 4"}
        tags |= {t for t, ok in (("Lk 1", Lk == 1), ("Lk < 64", 1 < Lk < 64), ("Lk 64", Lk == 64), ("full + ragged tile", 64 < Lk < 128),
                                 ("ragged last tile", Lk % 64 != 0), ("tiles % (ks tps) != 0", tiles % (ks * tps) != 0),
                                 ("tiles < ks", tiles < ks), ("Lk 768", Lk == 768), ("Lk 1369", Lk == 1369), ("Lq 1", Lq == 1),
                                 ("Lq < 16", 1 < Lq < 16), ("Lq % rows != 0", Lq % p.queries_per_wg != 0),
                                 ("odd tiles", tiles % 2 == 1 and tiles > 1), ("even tiles", tiles % 2 == 0),
                                 ("norm inside: " + (c["norm"] or "none"), True)) if ok}
        if c["qp"]:
            q = c["qp"]
            tags |= {f"qp_k {q['K']}", "tiled" if q["tiled"] else "row-major", "row_ss" if q["row_ss"] else "no row_ss",
                     "slices < ks" if q["K"] // 64 < ks else "slices >= ks"}
        seen.setdefault(cls, {})
        for t in tags:
            seen[cls].setdefault(t, c["name"])
    key_axis = {"Lk 1", "Lk < 64", "Lk 64", "full + ragged tile", "ragged last tile", "tiles > 4"}
    query_axis = {"Lq 1", "Lq < 16", "Lq % rows != 0"}
    families = {"family " + f for f in ac.FAMILIES}
    want = {
        ("fwd", 4, 3, 0, 1): key_axis | query_axis | families | {"tiles 1", "tiles 2", "tiles 4", "tiles < ks", "tiles % (ks tps) != 0",
                                                                 "Lk 768", "Lk 1369"},
        ("fwd", 4, 3, 0, 1, "qproj"): families | {"Lk 1", "Lk < 64", "Lk 64", "ragged last tile", "tiles > 4", "Lq 1", "Lq < 16",
                                                  "Lq % rows != 0", "qp_k 64", "qp_k 192", "qp_k 1024", "tiled", "row-major", "row_ss",
                                                  "no row_ss", "slices < ks", "slices >= ks", "Lk 1369", "norm inside: none", "norm inside: q"},
        ("fwd", 8, 2, 0, 1): key_axis | query_axis | families | {"tiles 1", "tiles 3", "tiles < ks", "tiles % (ks tps) != 0", "Lk 768", "Lk 1369"},
        ("fwd", 8, 1, 0, 2): key_axis | query_axis | families | {"odd tiles", "even tiles", "tiles 1", "tiles % (ks tps) != 0", "Lk 768", "Lk 1369"},
        ("fwd", 8, 1, 1, 1): key_axis | query_axis | families | {"Lk 768", "norm inside: k", "norm inside: qk"},
        ("hdv", "config", 3): key_axis | query_axis | families | {"Lk 768", "norm inside: none", "norm inside: q", "norm inside: qk"},
        ("hdv", "config", 4): key_axis | query_axis | families | {"tiles 1", "odd tiles", "even tiles", "tiles < ks", "Lk 1369",
                                                                  "norm inside: none", "norm inside: q", "norm inside: qk"},
        ("hd",): {"Lk 1", "Lk < 64", "Lk 64", "ragged last tile", "tiles > 4", "Lq 1", "Lq % rows != 0", "Lk 768"} | families,
    }
    assert set(seen) == set(want), sorted(set(seen) ^ set(want), key=str)
    for cls, tags in want.items():
        missing = sorted(tags - set(seen[cls]))
        assert not missing, f"{cls}: no case with {missing}"
    # the V^T variant: every HD16 in both product configurations with each choice of norms inside
    combos = {(ac.cell(plans[c["name"]])[1:], c["norm"]) for c in ac.CASES if c["kind"] == "hdv"}
    assert combos >= {((h, cfg), n) for h in range(1, 9) for cfg in (3, 4) for n in ("", "q", "qk")}


def test_planted_maps_cover_the_key_axis():
    """across the pairs of a planted case every key index is some query's dominant key (where there are queries enough), and key
    Lk - 1 is dominant in every pair"""
    for c in ac.CASES:
        if c["family"].startswith("planted"):
            pi = ac.planted_map(c)
            assert bool((pi == c["Lk"] - 1).any(1).all()), c["name"]
            P = c["B"] if c["qp"] else c["B"] * c["H"]
            if (c["Lq"] - 1) * P >= c["Lk"]:
                assert len(set(pi.flatten().tolist())) == c["Lk"], c["name"]


def test_existing_op_level_tests_and_the_instances_they_reach():
    """Which instance each op-level parametrisation of tests/test_dit_gpu.py lands on: none reaches attention_fwd_kernel<8,1,false>
    and none the V^T variant with HD16 = 4 or 6 -- the gap the case table closes."""
    from gaussiananything_amd import dit_ops as ops
    F = ac.FAKE_PTR
    got = {}
    for B, H, Lq, Lk, norm in [(2, 2, 64, 64, "qk"), (1, 3, 100, 137, "qk"), (2, 16, 768, 768, "qk"), (2, 4, 96, 1369, "qk"),
                               (1, 2, 48, 80, ""), (2, 16, 768, 768, ""), (2, 16, 768, 768, "q"), (2, 16, 700, 1369, ""),
                               (1, 16, 768, 1369, "q"), (3, 16, 768, 100, ""), (3, 16, 520, 1, ""), (1, 1, 5, 63, ""), (1, 2, 130, 129, "q"),
                               (1, 1, 64, 256, "")]:
        p = ac.plan_of(ac.A("x", "fwd", B, H, Lq, Lk, "flat", norm=norm))[0]
        got.setdefault(ac.cell(p), []).append((B, H, Lq, Lk, norm))
    for B, H, Lq, Lk, K in [(1, 16, 768, 1369, 1024), (1, 12, 768, 1369, 768), (1, 3, 200, 137, 192), (2, 4, 100, 64, 256)]:
        p = ac.plan_of(ac.A("x", "fwd", B, H, Lq, Lk, "flat", norm="q", qp=dict(K=K, tiled=False, row_ss=False)))[0]
        got.setdefault(ac.cell(p) + ("qproj",), []).append((B, H, Lq, Lk, K))
    hd16 = set()
    for B, H, Lq, Lk, d in [(2, 16, 768, 768, 72), (1, 16, 768, 1369, 72), (2, 3, 100, 137, 40), (1, 2, 50, 64, 128), (1, 4, 33, 200, 8),
                            (1, 2, 3, 5, 24), (3, 5, 130, 65, 104)]:
        p = ac.plan_of(ac.A("x", "hdv", B, H, Lq, Lk, "flat", d=d))[0]
        got.setdefault(ac.cell(p), []).append((B, H, Lq, Lk, d))
        hd16.add(p.hd16)
    for cell, shapes in sorted(got.items(), key=str):
        print(cell, "<-", shapes)
    assert ("fwd", 8, 1, 0, 2) not in got and hd16 == {1, 2, 3, 5, 7, 8}
    assert ops.attention_plan(ac.make_args(ac.A("x", "fwd", 6, 16, 768, 768, "flat"))).tps == 2


def test_plan_queries_report_the_dispatch_rules_and_the_launch_errors():
    from gaussiananything_amd import dit_ops as ops
    L = ops.lib()
    p = ac.plan_of(ac.A("x", "fwd", 2, 16, 768, 768, "flat"))[0]
    assert (p.nw, p.ks, p.tps, p.queries_per_wg, p.grid_x * p.grid_y * p.grid_z, p.lds_bytes) == (8, 2, 1, 128, 192, 98304)
    p = ac.plan_of(ac.A("x", "fwd", 1, 16, 768, 1369, "flat"))[0]
    assert (p.nw, p.ks, p.queries_per_wg, p.grid_x * p.grid_y * p.grid_z) == (4, 3, 64, 192)
    p = ac.plan_of(ac.A("x", "hdv", 2, 16, 768, 768, "flat", d=72))[0]
    assert (p.hd16, p.config, p.qf, p.nw, p.ks, p.forced, p.grid_x * p.grid_y) == (5, 3, 1, 8, 1, 0, 192)
    p = ac.plan_of(ac.A("x", "hdv", 1, 16, 768, 1369, "flat", d=72))[0]
    assert (p.config, p.nw, p.ks, p.queries_per_wg, p.grid_x * p.grid_y, p.lds_bytes) == (4, 8, 2, 64, 192, 2 * 45568)
    plan, hplan = ops.GaAttentionPlan(), ops.GaAttentionHdPlan()
    bad = lambda a: L.ga_attention_plan(ctypes.byref(a), ctypes.byref(plan))          # noqa: E731
    a = ac.make_args(ac.A("x", "fwd", 1, 1, 5, 63, "flat"))
    a.k = None
    assert bad(a) == -1
    a = ac.make_args(ac.A("x", "fwd", 1, 1, 5, 65, "flat"), strides=dict(vt_ld=64))
    assert bad(a) == -2                                                                # V^T rows shorter than the padded key count
    a = ac.make_args(ac.A("x", "fwd", 1, 1, 5, 63, "flat"), strides=dict(out_stride=66))
    assert bad(a) == -2
    a = ac.make_args(ac.A("x", "fwd", 3, 16, 768, 64, "flat", norm="q", qp=dict(K=64, tiled=False, row_ss=False)))
    assert bad(a) == -2                                                                # only the 64-query configuration projects q
    a = ac.make_args(ac.A("x", "fwd", 1, 1, 5, 63, "flat", norm="qk", qp=dict(K=64, tiled=False, row_ss=False)))
    assert bad(a) == -1                                                                # ... and never with K normalised inside
    assert L.ga_attention_plan(ctypes.byref(a), None) == -1
    hbad = lambda a: L.ga_attention_hd_plan(ctypes.byref(a), ctypes.byref(hplan))      # noqa: E731
    a = ac.make_args(ac.A("x", "hdv", 1, 1, 5, 63, "flat", d=72))
    a.head_dim = 76
    assert hbad(a) == -2
    a = ac.make_args(ac.A("x", "hd", 1, 1, 5, 63, "flat", d=72))
    a.q_norm_weight = ac.FAKE_PTR
    assert hbad(a) == -2                                                               # the norms inside belong to the V^T variant
    a = ac.make_args(ac.A("x", "hdv", 1, 1, 5, 63, "flat", d=72), strides=dict(vt_ld=96))
    assert hbad(a) == -2
