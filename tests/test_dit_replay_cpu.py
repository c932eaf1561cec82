"""The held-step bookkeeping behind the device-resident samplers (gaussiananything_amd/dit/device_samplers.py) with stand-in records
and no device: what is found again, what is not, and what a weight change (``drop()``) does to it."""
import torch

from gaussiananything_amd.dit import DiT_I23D_PCD_PixelArt_noclip, DiT_I23D_PCD_PixelArt_noclip_clay_stage2
from gaussiananything_amd.dit.device_samplers import KINDS, DeviceSamplers, HeldStep


def _record(samplers, *baked_in):
    return HeldStep({"y": torch.zeros(1)}, sig=samplers.stamp(baked_in), graph=object())


def test_every_model_starts_with_empty_records():
    kw = dict(input_size=8, in_channels=3, hidden_size=64, depth=1, num_heads=1, num_classes=0, learn_sigma=False, context_dim=64,
              patch_size=1)
    for model in (DiT_I23D_PCD_PixelArt_noclip(**kw), DiT_I23D_PCD_PixelArt_noclip_clay_stage2(use_pe_cond=True, **kw)):
        assert isinstance(model._samplers, DeviceSamplers) and model._samplers.model is model
        assert KINDS == ("euler", "dopri5", "sde") and all(model._samplers.held(kind) is None for kind in KINDS)
        assert model._pack is None and model._pooled_cache is None


def test_store_and_lookup_per_kind():
    s = DeviceSamplers(None)
    recs = {kind: _record(s, kind, 7) for kind in KINDS}
    for kind in KINDS:
        s.store(kind, recs[kind])
    for kind in KINDS:
        assert s.held(kind) is recs[kind]
        assert s.lookup(kind, s.stamp((kind, 7))) is recs[kind]


def test_a_signature_mismatch_returns_nothing():
    s = DeviceSamplers(None)
    s.store("euler", _record(s, "ws", 7))
    assert s.lookup("euler", s.stamp(("ws", 8))) is None
    assert s.lookup("euler", None) is None                      # nothing to replay against yet
    assert s.lookup("sde", s.stamp(("ws", 7))) is None          # another kind never captured
    s.store("dopri5", HeldStep({}, sig=None, graph=object()))   # a step captured without a signature is not found again
    assert s.lookup("dopri5", None) is None


def test_a_store_for_one_kind_leaves_the_others_in_place():
    s = DeviceSamplers(None)
    euler, sde = _record(s, "a"), _record(s, "a", ("Euler", 7, False, False))
    s.store("euler", euler)
    s.store("sde", sde)
    s.store("sde", _record(s, "a", ("Heun", 7, False, False)))
    assert s.held("euler") is euler and s.lookup("euler", s.stamp(("a",))) is euler
    assert s.held("sde") is not sde and s.held("dopri5") is None


def test_drop_empties_all_kinds():
    s = DeviceSamplers(None)
    for kind in KINDS:
        s.store(kind, _record(s, kind))
    s.drop()
    assert all(s.held(kind) is None for kind in KINDS)
    assert all(s.lookup(kind, s.stamp((kind,))) is None for kind in KINDS)


def test_a_signature_of_one_pack_generation_does_not_match_a_record_of_another():
    s = DeviceSamplers(None)
    old = _record(s, "ws", "kv")                # the same addresses: the allocator hands a new pack the blocks the old one freed
    s.drop()
    new = s.stamp(("ws", "kv"))
    assert new != old.sig
    s.store("euler", old)                       # (a step captured against the previous pack)
    assert s.lookup("euler", new) is None
