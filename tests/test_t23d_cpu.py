"""CPU tests of the text-to-3D path: the caption-conditioned denoiser classes (state-dict keys of the reference, registry), the
host-only plan of the short-context attention kernel, the caption conditioning of the cascade, and the rounding model of the
short-context kernel against the bound its GPU test relies on."""
import ctypes
import math

import pytest
import torch

from tests import _attention_cases as ac
from tests import _bounds as bd
from tests import _short_attention_cases as sc
from tests.test_attention_bounds_cpu import operands_fp32


def _fixture(name):
    from gaussiananything_amd import synthetic
    return torch.load(synthetic.fixture_path(f"dit_t23d_ref_{name}.pt"))


# ------------------------------------------------------------------------------------------------------------------ the models
@pytest.mark.parametrize("name", ["stage1", "stage2", "L1", "L2"])
def test_text_models_have_the_reference_state_dict(name):
    """Both classes build on the CPU with the reference's constructor keywords; their state_dict keys and shapes are exactly the ones
    the reference's own classes had when the fixture was made, and the fixture's weights load with strict=True."""
    from gaussiananything_amd import synthetic
    from gaussiananything_amd.dit import DiT_PCD_PixelArt, DiT_PCD_PixelArt_tofeat
    z = _fixture(name)
    cls = DiT_PCD_PixelArt_tofeat if name.endswith("2") else DiT_PCD_PixelArt
    model = cls(**z["kwargs"])
    got = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    assert sorted(got) == sorted((k, tuple(s)) for k, s in z["keys"])
    model.load_state_dict(synthetic.recipe_state_dict(z["keys"], z["recipe_seed"]), strict=True)
    assert ("xyz_pos_embed.xyz_projection.weight" in dict(got)) == name.endswith("2")
    assert not any(k.startswith(("pooled_vec_embedder", "clip_spatial_proj")) or "cross_attn_dino" in k for k, _ in got)
    with pytest.raises(RuntimeError):        # no CPU path, no PyTorch fallback
        model(z["x"], z["t"], z["context"])


def test_text_registry_and_refusals():
    from gaussiananything_amd.dit import DiT_models, DiT_models_t23d, DiT_PCD_PixelArt, DiT_PCD_PixelArt_tofeat
    from gaussiananything_amd.dit import dit_trilatent
    assert DiT_models_t23d is dit_trilatent.DiT_models and "DiT-PCD-L" not in DiT_models       # the image registry is what it was
    want = {"DiT-PCD-B": (12, 768, 12, False), "DiT-PCD-L": (24, 1024, 16, False),
            "DiT-PCD-B-stage2-xyz2feat": (12, 768, 12, True), "DiT-PCD-L-stage2-xyz2feat": (24, 1024, 16, True)}
    assert set(DiT_models_t23d) == set(want)            # (the unreleased 16 x 72 XL entry is not built: heads of 64 only)
    for name, (depth, width, heads, stage2) in want.items():
        cfg = DiT_models_t23d[name].config
        assert (cfg["depth"], cfg["hidden_size"], cfg["num_heads"], cfg["stage2"]) == (depth, width, heads, stage2)
    m = DiT_models_t23d["DiT-PCD-B-stage2-xyz2feat"](input_size=8, num_classes=0, learn_sigma=False, in_channels=10, context_dim=768, roll_out=True)
    assert isinstance(m, DiT_PCD_PixelArt_tofeat) and (m.depth, m.embed_dim, m.num_heads) == (12, 768, 12) and m.use_pe_cond
    kw = dict(input_size=8, patch_size=1, in_channels=3, hidden_size=128, depth=1, num_heads=2, learn_sigma=False, context_dim=64)
    with pytest.raises(NotImplementedError):
        DiT_PCD_PixelArt(num_classes=1000, **kw)
    with pytest.raises(NotImplementedError):
        DiT_PCD_PixelArt_tofeat(num_classes=0, use_pe_cond=False, **kw)
    with pytest.raises(NotImplementedError):           # 16 heads of 72
        DiT_PCD_PixelArt(num_classes=0, **dict(kw, hidden_size=1152, num_heads=16))


# ------------------------------------------------------------------------------------------------------------------- the plans
def test_short_attention_plan():
    from gaussiananything_amd import dit_ops as ops
    base = ac.A("p", "fwd", 1, 16, 768, 77, "flat", norm="q", qp=dict(K=1024, tiled=True, row_ss=True))
    p = ops.attention_short_plan(ac.make_args(base))
    assert (p.queries_per_wg, p.key_tiles, p.fuses_q, p.grid_x, p.grid_y, p.grid_z) == (64, 2, 1, 16, 12, 1)
    assert p.lds_bytes == (2 * 2 + 3 * 2) * 64 * 64 * 2          # K + V^T of two key tiles, and the projection's three-slot ring
    p2 = ops.attention_short_plan(ac.make_args(dict(base, B=2, qp=None)))
    assert (p2.queries_per_wg, p2.key_tiles, p2.fuses_q, p2.grid_x, p2.grid_y, p2.grid_z) == (64, 2, 0, 32, 12, 1)
    assert p2.lds_bytes == 2 * 2 * 64 * 64 * 2                   # q given: no ring
    assert ops.attention_short_plan(ac.make_args(dict(base, Lk=64, Lq=5))).key_tiles == 1
    assert ops.attention_short_plan(ac.make_args(dict(base, Lk=128))).key_tiles == 2

    def rc(case, strides=None, ptr=None, **fields):
        a = ac.make_args(case, ptr, strides)
        for k, v in fields.items():
            setattr(a, k, v)
        rc_short = ops.lib().ga_attention_short_plan(ctypes.byref(a), ctypes.byref(ops.GaAttentionShortPlan()))
        return rc_short, ops.lib().ga_attention_plan(ctypes.byref(a), ctypes.byref(ops.GaAttentionPlan()))

    assert rc(dict(base, Lk=129))[0] == -2 and rc(dict(base, Lk=1369))[0] == -2 and rc(dict(base, Lk=129))[1] == 0
    assert rc(dict(base, norm="qk", qp=None))[0] == -2                     # K normalised inside: not this kernel
    # every misalignment ga_attention_plan refuses is refused with the same code
    plain = dict(base, qp=None)
    odd = lambda bad: (lambda n: ac.FAKE_PTR + (bad[n] if n in bad else 0))      # noqa: E731
    for case, kw in [(plain, dict(strides=dict(q_stride=1028))), (plain, dict(strides=dict(k_stride=1028))), (plain, dict(strides=dict(vt_ld=64))),
                     (plain, dict(strides=dict(vt_ld=132))), (plain, dict(strides=dict(out_stride=1026))), (plain, dict(ptr=odd({"q": 8}))),
                     (plain, dict(ptr=odd({"k": 8}))), (plain, dict(ptr=odd({"vt": 8}))), (plain, dict(ptr=odd({"out": 4}))),
                     (base, dict(ptr=odd({"A": 8}))), (base, dict(ptr=odd({"W": 8}))), (base, dict(ptr=odd({"row_ss": 8}))),
                     (base, dict(strides=dict(qp_lda=1020))), (base, dict(qp_k=1000)), (base, dict(qp_row_ss_tiles=18)),
                     (plain, dict(Lq=0)), (plain, dict(heads=0)), (plain, dict(k=None)), (plain, dict(q=None)), (base, dict(qp_w=None))]:
        r_short, r_fwd = rc(case, **kw)
        assert r_fwd != 0 and r_short == r_fwd, (kw, r_short, r_fwd)


def test_the_dispatcher_and_its_instance_table_are_what_they_were():
    """ga_attention_plan / ga_attention_instances answer for every case of tests/_attention_cases.CASES exactly as
    tests/test_attention_plan.py pins them; the short kernel is in neither."""
    from gaussiananything_amd import dit_ops as ops
    inst = {ac.cell(p) for p in ops.attention_instances()}
    assert inst == {("fwd", 4, 3, 0, 1), ("fwd", 8, 2, 0, 1), ("fwd", 8, 1, 0, 2), ("fwd", 8, 1, 1, 1)}
    for c in ac.CASES:
        if c["kind"] != "fwd":
            continue
        p, cell = ac.plan_of(c)
        w = (c["Lq"] + 127) // 128 * c["H"] * c["B"]
        want = (8, 1, 1) if "k" in c["norm"] else ((4, 3, 0) if w <= 128 else (8, 2, 0) if w <= 512 else (8, 1, 0))
        assert (p.nw, p.ks, p.knorm) == want and cell in inst, c["name"]
        assert p.queries_per_wg == 16 * p.nw and p.fuses_q == (1 if c["qp"] else 0)
    # the text cross-attention shapes still get the long-list configurations from the dispatcher
    for B, nw_ks in ((1, (4, 3)), (2, (8, 2))):
        p = ops.attention_plan(ac.make_args(ac.A("t", "fwd", B, 16, 768, 77, "flat")))
        assert (p.nw, p.ks) == nw_ks


# ----------------------------------------------------------------------------------------------------------------- the cascade
def test_caption_conditioning_of_the_cascade():
    from gaussiananything_amd import cascade
    g = torch.Generator().manual_seed(0)
    tok, vec = torch.randn(2, 77, 768, generator=g), torch.randn(2, 768, generator=g)
    cond, uc = cascade.condition_on_caption(tok, vec)
    assert set(cond) == set(uc) == {"caption_crossattn", "caption_vector"}
    assert torch.equal(cond["caption_crossattn"], tok) and torch.equal(cond["caption_vector"], vec)
    assert all(float(v.abs().max()) == 0.0 and v.shape == cond[k].shape and v.dtype == cond[k].dtype for k, v in uc.items())
    with pytest.raises(ValueError):
        cascade.condition_on_caption(tok, vec[:1])
    xyz = (torch.rand(2, 768, 3, generator=g) - 0.5) * 0.9
    c2, uc2 = cascade.stage2_caption_conditioning(cond, uc, xyz)
    assert set(c2) == set(uc2) == {"caption_crossattn", "caption_vector", "fps-xyz"}
    assert torch.equal(c2["fps-xyz"], xyz / 0.45) and c2["fps-xyz"] is uc2["fps-xyz"]          # the cloud is shared, scaled by PCD_Scaler
    assert float(uc2["caption_crossattn"].abs().max()) == 0.0 and float(uc2["caption_vector"].abs().max()) == 0.0      # CFG is real
    assert torch.equal(c2["caption_crossattn"], tok) and cascade.T23D_CFG_SCALE == 4.5
    # the image conditioning is what it was: uc == c unless asked otherwise
    ci = {"img_crossattn": tok, "img_vector": vec}
    i2, iu2 = cascade.stage2_conditioning(ci, {k: torch.zeros_like(v) for k, v in ci.items()}, xyz)
    assert iu2["img_crossattn"] is i2["img_crossattn"]


class _FakeDenoiser(torch.nn.Module):
    """records which surface cascade.sample calls (CPU, euler on a linear velocity)"""
    in_channels = 3

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.calls = []

    def forward_with_cfg(self, x, t, context=None, cfg_scale=None):
        self.calls.append(("cfg", x.shape[0], sorted(context)))
        return -x

    def forward_cond(self, x, t, context=None, cfg_scale=None):
        self.calls.append(("cond", x.shape[0], sorted(context)))
        return -x


def test_sample_takes_the_cfg_path_for_caption_conditioning():
    from gaussiananything_amd import cascade
    g = torch.Generator().manual_seed(1)
    cond, uc = cascade.condition_on_caption(torch.randn(1, 77, 64, generator=g), torch.randn(1, 64, generator=g))
    c2, uc2 = cascade.stage2_caption_conditioning(cond, uc, torch.zeros(1, 8, 3))
    for c, u in ((cond, uc), (c2, uc2)):
        m, stats = _FakeDenoiser(), {}
        out = cascade.sample(m, c, u, (8, 3), 1, cascade.T23D_CFG_SCALE, 0, 4, "euler", stats=stats)
        assert out.shape == (1, 8, 3) and "noop_cfg_dedup" not in stats
        assert m.calls and all(kind == "cfg" and n == 2 and keys == sorted(c) for kind, n, keys in m.calls)
    # the image stage 2 (uc is c) still dedups
    ci = {"img_crossattn": torch.randn(1, 5, 64, generator=g), "img_vector": torch.randn(1, 64, generator=g)}
    i2, iu2 = cascade.stage2_conditioning(ci, {k: torch.zeros_like(v) for k, v in ci.items()}, torch.zeros(1, 8, 3))
    m, stats = _FakeDenoiser(), {}
    cascade.sample(m, i2, iu2, (8, 3), 1, 4.0, 0, 4, "euler", stats=stats)
    assert stats.get("noop_cfg_dedup") and all(kind == "cond" for kind, _, _ in m.calls)


# ----------------------------------------------------------------------------------- the short kernel's rounding model and bound
def emulate_one_pass(qh, kh, v, mutate=None):
    """fp32 attention over [P, L, d] operands with the rounding points of attention_short_kernel: fp32 scores of the whole key list, the
    TRUE row maximum, exp2, the fp32 row sum of the unrounded P, bf16 P into the P V product, o (1 / l), bf16 store."""
    Lk = kh.shape[1]
    if mutate == "drop_last" and Lk > 1:          # the clamp of the ragged tile one key short
        kh = kh.clone()
        kh[:, Lk - 1] = kh[:, Lk - 2]
    if mutate == "swap_v" and Lk > 1:
        v = v.clone()
        v[:, [Lk - 2, Lk - 1]] = v[:, [Lk - 1, Lk - 2]]
    s = qh @ kh.transpose(1, 2)
    if mutate == "mask_extra":
        s[:, :, -1] = -1e30
    if mutate == "skip_tile" and Lk > 64:
        s[:, :, 64:] = -1e30
    p = torch.exp2(s - s.amax(-1, keepdim=True))
    o = p.to(torch.bfloat16).float() @ v
    return (o * (1.0 / p.sum(-1))[..., None]).to(torch.bfloat16).float()


@pytest.mark.parametrize("case", sc.CASES, ids=[c["name"] for c in sc.CASES])
def test_one_pass_softmax_stays_within_the_bound_of_the_attention_test(case):
    """The GPU test of the short kernel uses the bound of tests/_bounds.attention with groups = 1 (and the lazy-rescale allowance of the
    long-list kernel, which only loosens it).  Confirmed here, on EVERY case of the table, with the kernel's rounding model in fp32."""
    z = ac.inputs(case)
    o = ac.operands(case, z)
    qh, kh, v, cs = operands_fp32(case, z)
    assert cs == 1.0
    ref, bound, dom = bd.attention(o["qh"], o["dq"], o["kh"], o["dk"], o["v"], c=o["c"], n_acc=o["n_acc"], rel_c=o["rel_c"], lazy=o["lazy"], groups=1)
    r = (emulate_one_pass(qh, kh, v).double() - ref).abs() / bound
    assert bool(torch.isfinite(r).all()) and float(r.max()) <= 1.0, (case["name"], float(r.max()))


@pytest.mark.parametrize("family", ["planted8", "planted14", "fewhot"])
def test_seeded_bugs_of_a_short_kernel_exceed_the_bound(family):
    """what a subtly wrong short-context kernel would do -- the last key dropped, one key too many masked, two V rows swapped, the
    second tile skipped -- lands over the bound on the designed families, at the caption length"""
    for qp, norm in ((None, "q"), (dict(K=192, tiled=False, row_ss=True), "q")):
        case = ac.A(f"short_mut_{family}_{'qp' if qp else 'q'}", "fwd", 2, 3, 64, 77, family, norm=norm, qp=qp)
        z = ac.inputs(case)
        o = ac.operands(case, z)
        qh, kh, v, _ = operands_fp32(case, z)
        ref, bound, _ = bd.attention(o["qh"], o["dq"], o["kh"], o["dk"], o["v"], c=o["c"], n_acc=o["n_acc"], rel_c=o["rel_c"], lazy=o["lazy"], groups=1)
        for mutate in ("drop_last", "mask_extra", "swap_v", "skip_tile"):
            r = (emulate_one_pass(qh, kh, v, mutate).double() - ref).abs() / bound
            r = torch.where(torch.isfinite(r), r, torch.full_like(r, math.inf))
            assert float(r.max()) > 1.0, (family, mutate, float(r.max()))
