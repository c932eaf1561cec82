"""``DiT_PCD_PixelArt`` (stage 1) and ``DiT_PCD_PixelArt_tofeat`` (stage 2): the caption-conditioned denoisers of the reference's
text-to-3D mode (/root/reference/dit/dit_trilatent.py:262-419, registry :480-518, shell_scripts/release/inference/t23d/*.sh) on the
HIP kernels behind include/ga_dit.h.

They are the image models of ``dit_i23d`` with

* ``PixelArtTextCondDiTBlock`` blocks (dit_models_xformers.py:329-376): self-attention, cross-attention on the caption tokens --
  each block normalises them itself (``attention_y_norm``) before ``to_k`` / ``to_v`` --, MLP  (``GaDitModel.block_order = 1``);
* ``FinalLayer`` (:993-1016) in place of ``T2IFinalLayer``  (``GaDitModel.final_adaln_w``);
* ``cap_embedder(caption_vector)`` as the pooled branch;
* ``context = {'caption_crossattn' [S,77,768], 'caption_vector' [S,768] (, 'fps-xyz' [S,L,3])}``: the two outputs of the reference's
  ``FrozenOpenCLIPEmbedder2`` -- the caller supplies them, the CLIP text encoder is not part of this package.

Everything else -- weight packing, the K / V cache per conditioning tensor, the pooled vector once per conditioning, ``forward`` /
``forward_with_cfg`` / ``forward_cond``, ``sample_euler_fused``, ``sample_dopri5_device``, ``ca_skip`` -- is the host code of
``DiT_I23D_PCD_PixelArt_noclip``, inherited.  The parameters sit under exactly the reference's state-dict keys.  No PyTorch fallback.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .dit_i23d import DiT_I23D_PCD_PixelArt_noclip, _Attn, _CrossAttn, _FusedMLP, _Mlp, _RMSNormW, _TEmb, _XYZPosEmbed


class _TextBlock(nn.Module):  # PixelArtTextCondDiTBlock; creation order as in the reference
    def __init__(self, dim, heads, ctx, mlp_ratio):
        super().__init__()
        self.norm1 = _RMSNormW(dim)
        self.attn = _Attn(dim, heads)
        self.norm2 = _RMSNormW(dim)
        self.mlp = _FusedMLP(dim, int(mlp_ratio))
        self.cross_attn = _CrossAttn(dim, ctx, heads)
        self.scale_shift_table = nn.Parameter(torch.randn(6, dim) / dim ** 0.5)
        self.attention_y_norm = _RMSNormW(ctx)
        self.prenorm_ca_text = _RMSNormW(dim)


class _FinalLayer(nn.Module):  # FinalLayer: LayerNorm(no affine, 1e-6) * (1 + scale) + shift, Linear
    def __init__(self, dim, out_channels):
        super().__init__()
        self.linear = nn.Linear(dim, out_channels)
        self.adaLN_modulation = nn.Sequential(nn.SiLU(), nn.Linear(dim, 2 * dim, bias=True))


class DiT_PCD_PixelArt(DiT_I23D_PCD_PixelArt_noclip):
    """Stage-1 (point cloud) text denoiser.  The reference's constructor keywords; ``vit_blk`` / ``final_layer_blk`` are accepted and
    ignored (the reference passes its own two classes), ``num_classes`` must be 0 as in the release (script_util.py:398-407)."""

    _ctx_key, _vec_key = "caption_crossattn", "caption_vector"
    _ca_name, _ca_prenorm_name, _pooled_name = "cross_attn", "prenorm_ca_text", "cap_embedder"
    _block_order, _ctx_norm = 1, True

    def __init__(self, input_size=32, patch_size=2, in_channels=4, hidden_size=1152, depth=28, num_heads=16, mlp_ratio=4,
                 class_dropout_prob=0.1, num_classes=1000, learn_sigma=True, mixing_logit_init=-3, mixed_prediction=True,
                 context_dim=False, roll_out=False, vit_blk=None, final_layer_blk=None, _stage2=False):
        nn.Module.__init__(self)
        if num_classes != 0:
            raise NotImplementedError("the released t23d models are built with num_classes=0 (no label embedder)")
        if not context_dim or int(context_dim) % 64:
            raise ValueError("context_dim (the caption token width, 768 in the release) must be a multiple of 64")
        if hidden_size % num_heads or hidden_size % 64:
            raise ValueError("the width must be a multiple of 64 and of the head count")
        if hidden_size // num_heads != 64:
            raise NotImplementedError("the text block order is built for heads of 64 (every released t23d model); the registry's unreleased "
                                      "DiT-PCD-XL-stage2-xyz2feat (16 heads of 72) is not")
        assert patch_size == 1, "point-cloud latents are not patchified (patch_size=1 in every PCD registry entry)"
        self.in_channels = in_channels
        self.out_channels = in_channels * 2 if learn_sigma else in_channels
        self.embed_dim = hidden_size
        self.num_heads = num_heads
        self.depth = depth
        self.roll_out = roll_out
        self.context_dim = int(context_dim)
        self.has_caption = True
        D = hidden_size
        self.x_embedder = _Mlp(in_channels, D, D)
        self.t_embedder = _TEmb(D)
        self.blocks = nn.ModuleList([_TextBlock(D, num_heads, self.context_dim, mlp_ratio) for _ in range(depth)])
        self.final_layer = _FinalLayer(D, self.out_channels)
        self.adaLN_modulation = nn.Sequential(nn.SiLU(), nn.Linear(D, 6 * D, bias=True))
        self.cap_embedder = nn.Sequential(nn.LayerNorm(self.context_dim), nn.Linear(self.context_dim, D))
        self._stage2 = _stage2
        self.initialize_weights()
        self._init_runtime_state()

    def initialize_weights(self):   # dit_models_xformers.py:1119-1159, dit_trilatent.py:168-179
        def _basic_init(m):
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        self.apply(_basic_init)
        nn.init.normal_(self.t_embedder.mlp[0].weight, std=0.02)
        nn.init.normal_(self.t_embedder.mlp[2].weight, std=0.02)
        for lin in (self.final_layer.adaLN_modulation[-1], self.final_layer.linear, self.cap_embedder[-1]):
            nn.init.constant_(lin.weight, 0)
            nn.init.constant_(lin.bias, 0)


class DiT_PCD_PixelArt_tofeat(DiT_PCD_PixelArt):
    """Stage-2 (KL feature) text denoiser conditioned on the stage-1 point cloud (dit_trilatent.py:335-419)."""

    def __init__(self, *args, use_pe_cond=True, **kwargs):
        if not use_pe_cond:
            raise NotImplementedError("only the released use_pe_cond=True variant (xyz positional embedding) is built")
        super().__init__(*args, _stage2=True, **kwargs)
        self.use_pe_cond = use_pe_cond
        self.xyz_pos_embed = _XYZPosEmbed(self.embed_dim)
        nn.init.xavier_uniform_(self.xyz_pos_embed.xyz_projection.weight)
        nn.init.constant_(self.xyz_pos_embed.xyz_projection.bias, 0)
        self._init_runtime_state()


def _pcd(depth, hidden, heads, stage2=False):
    def make(**kw):
        cls = DiT_PCD_PixelArt_tofeat if stage2 else DiT_PCD_PixelArt
        return cls(depth=depth, hidden_size=hidden, patch_size=1, num_heads=heads, **kw)
    make.config = dict(depth=depth, hidden_size=hidden, num_heads=heads, stage2=stage2)
    return make


# the PCD entries of the reference registry (dit_trilatent.py:480-518, :523-).  DiT-PCD-XL-stage2-xyz2feat (28 x 1152, 16 heads of 72,
# unreleased) is left out: the text block order is not built for heads other than 64 (include/ga_dit.h: GaDitModel.block_order)
DiT_models = {
    "DiT-PCD-B": _pcd(12, 768, 12),
    "DiT-PCD-L": _pcd(24, 1024, 16),
    "DiT-PCD-B-stage2-xyz2feat": _pcd(12, 768, 12, stage2=True),
    "DiT-PCD-L-stage2-xyz2feat": _pcd(24, 1024, 16, stage2=True),
}
