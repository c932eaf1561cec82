"""CPU test of the GEMM case table (tests/_gemm_cases.py) through ga_gemm_plan: the cases reach every (kernel instance, epilogue) the
dispatcher of ga_gemm_bf16 can launch -- listed by the library itself (ga_gemm_instances, the table the launch is looked up in) --
and run every optional feature on every tile family that accepts it.  A dispatcher change that makes another instance reachable fails
here until a case reaches it."""
import pytest

from tests import _gemm_cases as gc

# (family, epilogue, tile_m, tile_n, waves, slots, rem, mt, splits) -> why the rules never pick it
UNREACHABLE = {
    (1, gc.EPI_F32, 96, 128, 4, 4, 0, 0, 1): "the 96 x 128 ring tile is chosen only for epilogues other than the fp32 store "
                                            "(dit_gemm.hip, gemm_plan: ring4_env && epilogue != GA_GEMM_EPI_STORE_F32)",
}
# (the general kernel with two slots and MT = 1 does serve EPI 2 / 3: rows <= 32 and more than 256 tile columns, N > 32768)

ALL7 = {"general", "192x128", "96x128", "96x64", "64x64", "splitk_192x128", "splitk_96x128"}
UNSPLIT = {"general", "192x128", "96x128", "96x64", "64x64"}
# feature -> the tile families that can run it (the split instances of the bf16-store epilogues exist for 192 x 128 only; no split
# with k_rows; more than 16 row partial sums never split, see the case splitk4_wide_row_ss_gelu)
FEATURES = {
    "gate": (lambda c: c["gate"], ALL7),
    "per-batch bias": (lambda c: c["bias"] == "batch", ALL7),
    "row_ss <= 16": (lambda c: 0 < c["row_ss"] <= 16, UNSPLIT | {"splitk_192x128"}),
    "row_ss > 16": (lambda c: c["row_ss"] > 16, UNSPLIT),
    "qk norm": (lambda c: c["qk"][1] > 0, UNSPLIT | {"splitk_192x128"}),
    "V^T store": (lambda c: c["vt"] > 0, UNSPLIT | {"splitk_192x128"}),
    "emit plain": (lambda c: c["emit"] == "plain", ALL7),
    "emit modulated": (lambda c: c["emit"] == "mod", ALL7),
    "k_rows": (lambda c: c["k_rows"] > 0, UNSPLIT),
    "w_tiled": (lambda c: c["N"] % 8 == 0, ALL7),      # (the GPU test runs every case with N % 8 == 0 on the tiled image too)
}


@pytest.fixture(scope="module")
def plans():
    return {c["name"]: gc.plan_of(c) for c in gc.CASES}


def test_every_reachable_gemm_instance_has_a_case(plans):
    from gaussiananything_amd import dit_ops as ops
    instances = {gc.cell(p) for p in ops.gemm_instances()}
    assert len(instances) == len(ops.gemm_instances()), "an instance is listed twice"
    assert set(UNREACHABLE) <= instances
    hit = {}
    for name, (p, cell) in plans.items():
        assert cell in instances, (name, cell)
        hit.setdefault(cell, name)
    reachable = instances - set(UNREACHABLE)
    print(f"{len(reachable)} reachable cells, {len(UNREACHABLE)} unreachable")
    for cell in sorted(instances):
        print(cell, "->", hit.get(cell, "UNREACHABLE: " + UNREACHABLE.get(cell, "?")))
    assert not set(hit) & set(UNREACHABLE), "a cell listed as unreachable is reached"
    missing = sorted(reachable - set(hit))
    assert not missing, f"no case reaches {missing}"


def test_every_feature_runs_on_every_tile_family_that_accepts_it(plans):
    for feature, (has, families) in FEATURES.items():
        got = {}
        for c in gc.CASES:
            if has(c):
                got.setdefault(gc.tile_family(plans[c["name"]][0]), c["name"])
        print(feature, got)
        assert set(got) == families, (feature, sorted(families - set(got)), sorted(set(got) - families))


def test_plan_query_reports_the_dispatch_rules():
    """What the dispatch comments name, and the argument errors ga_gemm_bf16 returns"""
    from gaussiananything_amd import dit_ops as ops
    xl_fc1, _ = gc.plan_of(gc.C("xl_fc1", 1536, 4608, 1152, gc.EPI_GELU))
    assert (xl_fc1.family, xl_fc1.mt, xl_fc1.slots, xl_fc1.grid_x * xl_fc1.grid_y) == (ops.GEMM_FAMILY_GENERAL, 4, 2, 432)
    l_qkv, _ = gc.plan_of(gc.C("l_qkv", 1536, 3072, 1024, gc.EPI_BF16))
    assert (l_qkv.family, l_qkv.tile_m, l_qkv.tile_n, l_qkv.waves, l_qkv.grid_x * l_qkv.grid_y) == (ops.GEMM_FAMILY_RING, 192, 128, 8, 192)
    b_proj, _ = gc.plan_of(gc.C("b_proj", 1536, 768, 768, gc.EPI_RES))
    assert (b_proj.tile_m, b_proj.tile_n, b_proj.xmap) == (96, 64, 1)
    a = gc.make_args(gc.C("bad", 100, 130, 64, gc.EPI_BF16))
    import ctypes
    plan = ops.GaGemmPlan()
    assert ops.lib().ga_gemm_plan(ctypes.byref(a), ctypes.byref(plan)) == -2          # N % 4 != 0
    a = gc.make_args(gc.C("bad", 100, 128, 64, 7))
    assert ops.lib().ga_gemm_plan(ctypes.byref(a), ctypes.byref(plan)) == -2          # no such epilogue
    a = gc.make_args(gc.C("ok", 100, 128, 64, gc.EPI_BF16))
    a.W = None
    assert ops.lib().ga_gemm_plan(ctypes.byref(a), ctypes.byref(plan)) == -1
