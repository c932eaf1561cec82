"""CPU tests of the geometry-loss restatements (tests/_geo_ref.py) that the GPU tests of csrc/geo_loss.hip are measured with: the fp32
reference-route restatement against the reference's own functions (tests/golden/geo_loss_ref.pt), the camera-space fp32 model of the
kernel against the GPU bars, the kernel's hand-written backward against autograd, and the zero-gradient rule."""
import pytest
import torch
import torch.nn.functional as F

from tests import _geo_ref as ref

T = 32   # the tile edge of csrc/geo_loss.hip (the GPU tests read it from ga_geo_loss_plan)
ROWS = {}   # case id -> line of profiles/geo_loss_bounds.txt


@pytest.fixture(scope="module", autouse=True)
def _bounds_file():
    """after the module: the per-case table of profiles/geo_loss_bounds.txt"""
    yield
    if len(ROWS) == len(ref.cases(T)):
        head = [f"tile {T}; per case the errors of the fp32 reference-route restatement against float64 (E_*: the bars are E_map + 1e-6 and",
                "E_grad + 2e-6, the means 1e-6 relative) and the errors of the fp32 camera-space model of the kernel against float64 (mod_*);",
                "gradient columns are relative L2; from-depth mode with a mask, weights tests/_geo_ref.py: grad_weights",
                f"{'family':<8} {'shape':<10} {'E_map':>9} {'mod_map':>9} {'mod_means':>9} {'E_g_rn':>9} {'mod_g_rn':>9} {'E_g_depth':>9} {'mod_g_dep':>9}"]
        ref.write_section("bars per GPU case (tests/test_geo_loss_cpu.py)", head + [ROWS[k] for k in sorted(ROWS)])


@pytest.fixture(scope="module")
def golden():
    return torch.load(ref.GOLDEN)


def test_fp32_reference_route_reproduces_the_reference(golden):
    """normals to 1e-6 (measured maximum: 0, every case bit-equal), the depth gradient of the golden loss to 2e-6 relative L2
    (measured maximum 0)"""
    assert len(golden["cases"]) >= 8 and {c["family"] for c in golden["cases"]} == set(ref.FAMILIES)
    worst_n = worst_g = 0.0
    for c in golden["cases"]:
        H, W = c["shape"]
        inp = ref.make_inputs(c["family"], (1, H, W), c["seed"])
        assert torch.equal(inp["w2c"][0], c["w2c"])
        d = inp["depth"][0].clone().requires_grad_(True)
        n = ref.normals_reference_route(c["w2c"], c["tanfov"], d, torch.float32)
        worst_n = max(worst_n, float((n.detach() - c["normal"]).abs().max()))
        assert bool((c["alpha"][(c["normal"] == 0).all(-1)] == 0).all())          # the condition the fixture was made under
        (1 - (inp["rend_normal"][0] * n.permute(2, 0, 1) * c["alpha"][None]).sum(0)).mean().backward()
        worst_g = max(worst_g, ref.rel_l2(d.grad[0], c["grad_depth"][0]))
    print("fp32 reference route against the golden: normals", worst_n, "gradient", worst_g)
    assert worst_n <= 1e-6 and worst_g <= 2e-6


@pytest.mark.parametrize("case", ref.cases(T), ids=lambda c: f"{c[0]}-{'x'.join(map(str, c[1]))}")
def test_camera_space_model_stays_within_the_gpu_bars(case):
    family, shape, seed = case
    inp = ref.make_inputs(family, shape, seed)
    w = ref.grad_weights(shape[0])
    r = ref.reference_errors(inp, w, use_mask=True)
    got = ref.measured(r, ref.evaluate(inp, w, "camera", torch.float32, use_mask=True))
    bar = ref.bars(r)
    ROWS[ref.cases(T).index(case)] = (f"{family:<8} {'x'.join(map(str, shape)):<10} {r['E_map']:9.2e} {got['map']:9.2e} {got['means']:9.2e} "
                                      f"{r['E_grad_rend_normal']:9.2e} {got['grad_rend_normal']:9.2e} {r['E_grad_depth']:9.2e} "
                                      f"{got['grad_depth']:9.2e}")
    for k in got:
        assert got[k] <= bar[k], (k, got[k], bar[k])
    # the kernel's backward, written out by hand, is the gradient of the model
    V, H, W = shape
    hand = torch.stack([ref.pullback_depth(inp["cam_view"][v], ref.TANFOV, inp["depth"][v, 0],
                                           (-(w[v, 0] / (H * W)) * inp["rend_normal"][v] * inp["alpha"][v]).permute(1, 2, 0))
                        for v in range(V)])[:, None]
    assert ref.rel_l2(hand, r["grad_depth"]) <= bar["grad_depth"]
    if H < 3 or W < 3:
        assert bool((hand == 0).all()) and bool((r["s"] == 0).all())


def test_model_and_reference_route_agree_with_the_golden_gradient(golden):
    """the camera-space model in float64 against the reference's own autograd gradient (fp32): within the reference's fp32 error"""
    for c in golden["cases"]:
        H, W = c["shape"]
        inp = ref.make_inputs(c["family"], (1, H, W), c["seed"])
        d = inp["depth"][0].double().requires_grad_(True)
        n = ref.normals_camera_model(inp["cam_view"][0].double(), c["tanfov"], d, torch.float64)
        assert float((n.detach() - c["normal"].double()).abs().max()) <= 2e-5
        (1 - (inp["rend_normal"][0].double() * n.permute(2, 0, 1) * c["alpha"][None].double()).sum(0)).mean().backward()
        assert ref.rel_l2(c["grad_depth"][0], d.grad[0]) <= 2e-5


def test_zero_gradient_rule_on_an_isolated_pixel():
    d0 = ref.island_depth()
    H, W = d0.shape[-2:]
    w2c = ref.look_at_w2c(5).double()
    g = torch.Generator().manual_seed(3)
    rn = torch.randn(3, H, W, generator=g, dtype=torch.float64)
    alpha = 0.5 + 0.5 * torch.rand(1, H, W, generator=g, dtype=torch.float64)       # alpha > 0 on the island and around it

    def grad(normalize):
        d = d0.clone().requires_grad_(True)
        n = ref.normals_reference_route(w2c, ref.TANFOV, d, torch.float64, normalize=normalize).permute(2, 0, 1)
        (1 - (rn * n * alpha).sum(0)).mean().backward()
        return n.detach(), d.grad[0]

    n_rule, g_rule = grad(ref.normalize_ruled)
    n_torch, g_torch = grad(lambda c: F.normalize(c, dim=-1))
    assert torch.equal(n_rule, n_torch)                                             # the forward value is unchanged
    degenerate = torch.zeros(H, W, dtype=torch.bool)
    degenerate[1:-1, 1:-1] = (n_torch[:, 1:-1, 1:-1] == 0).all(0)
    assert bool(degenerate[4, 5] and degenerate[6, 5] and degenerate[5, 4] and degenerate[5, 6])   # the island's four neighbours
    touched = torch.zeros(H, W, dtype=torch.bool)                                   # depth pixels a degenerate normal reads
    touched[:-1] |= degenerate[1:]
    touched[1:] |= degenerate[:-1]
    touched[:, :-1] |= degenerate[:, 1:]
    touched[:, 1:] |= degenerate[:, :-1]
    assert bool(torch.isfinite(g_rule).all()) and float(g_rule.abs().max()) < 1.0
    assert float(g_torch.abs().max()) > 1e6                                         # what the rule keeps out
    assert float((g_rule - g_torch)[~touched].abs().max()) <= 1e-12 * float(g_rule.abs().max())
    # the model agrees, and its hand-written backward
    d = d0.clone().requires_grad_(True)
    n = ref.normals_camera_model(w2c.T, ref.TANFOV, d, torch.float64).permute(2, 0, 1)
    (1 - (rn * n * alpha).sum(0)).mean().backward()
    assert ref.rel_l2(d.grad[0], g_rule) <= 2e-7     # the matrix is rigid to fp32 rounding (6e-8 per entry): transpose against inverse
    hand = ref.pullback_depth(w2c.T.float(), ref.TANFOV, d0[0].float(), (-(rn * alpha) / (H * W)).permute(1, 2, 0).float())
    assert ref.rel_l2(hand, g_rule) <= 2e-6 and bool(torch.isfinite(hand).all())
