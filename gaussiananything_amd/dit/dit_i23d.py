"""``DiT_I23D_PCD_PixelArt_noclip`` (stage 1) and ``DiT_I23D_PCD_PixelArt_noclip_clay_stage2`` (stage 2) with the
reference's operator surface -- /root/reference/dit/dit_i23d.py:437-567, 664-750, forward_with_cfg :159-172, registry
names :1665-1697 -- on top of the hand-written HIP kernels behind include/ga_dit.h.

* The modules own ordinary fp32 ``nn.Parameter`` s under exactly the reference's state-dict keys (including the leftovers
  the reference keeps but never uses: ``clip_spatial_proj.*``, ``cap_embedder.*``, ``attention_y_norm.weight``,
  ``blocks.i.attention_y_norm.weight``), so a released checkpoint loads with ``load_state_dict(strict=True)``.
  Only the parameters that survive the reference constructor chain are created (no 512x512 ``pos_embed``,
  SURVEY.md section 7 hard part 7).
* ``forward`` packs the weights once into the bf16 / fp32 buffers the kernels read (re-packed when a parameter changes),
  projects the step-invariant image tokens to K/V once per conditioning tensor, and then issues ONE C-ABI call per function
  evaluation.  There is no PyTorch fallback: CPU tensors or a missing HIP library raise.
"""
from __future__ import annotations

import ctypes
import contextlib
import os
import threading

import torch
import torch.nn as nn

from .. import dit_ops as ops
from .device_samplers import DeviceSamplers


class _RMSNormW(nn.Module):  # parameter holder: key "<name>.weight"
    def __init__(self, dim):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))


class _Bias(nn.Module):  # xformers FusedDropoutBias: key "<name>.bias"
    def __init__(self, dim):
        super().__init__()
        self.bias = nn.Parameter(torch.zeros(dim))


class _FusedMLP(nn.Module):  # keys mlp.0.weight, mlp.1.bias, mlp.2.weight, mlp.3.bias
    def __init__(self, dim, mult):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(dim, mult * dim, bias=False), _Bias(mult * dim),
                                 nn.Linear(mult * dim, dim, bias=False), _Bias(dim))


class _Mlp(nn.Module):  # timm Mlp keys fc1.*, fc2.*
    def __init__(self, i, h, o):
        super().__init__()
        self.fc1 = nn.Linear(i, h)
        self.fc2 = nn.Linear(h, o)


class _Attn(nn.Module):
    def __init__(self, dim, heads):
        super().__init__()
        self.qkv = nn.Linear(dim, 3 * dim, bias=True)
        self.proj = nn.Linear(dim, dim)
        self.q_norm = _RMSNormW(dim // heads)
        self.k_norm = _RMSNormW(dim // heads)


class _CrossAttn(nn.Module):
    def __init__(self, dim, ctx, heads):
        super().__init__()
        self.to_q = nn.Linear(dim, dim, bias=False)
        self.to_k = nn.Linear(ctx, dim, bias=False)
        self.q_norm = _RMSNormW(dim // heads)
        self.k_norm = _RMSNormW(dim // heads)
        self.to_v = nn.Linear(ctx, dim, bias=False)
        self.to_out = nn.Sequential(nn.Linear(dim, dim), nn.Dropout(0.0))


class _Block(nn.Module):  # ImageCondDiTBlockPixelArtRMSNormClayLRM (dit_models_xformers.py:717-787)
    def __init__(self, dim, heads, ctx, mlp_ratio):
        super().__init__()
        self.scale_shift_table = nn.Parameter(torch.randn(6, dim) / dim ** 0.5)
        self.norm1 = _RMSNormW(dim)
        self.norm2 = _RMSNormW(dim)
        self.attn = _Attn(dim, heads)
        self.mlp = _FusedMLP(dim, int(mlp_ratio))
        self.attention_y_norm = _RMSNormW(1024)  # unused leftover of the reference constructor chain
        self.cross_attn_dino = _CrossAttn(dim, ctx, heads)
        self.prenorm_ca_dino = _RMSNormW(dim)


class _TEmb(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.mlp = nn.Sequential(nn.Linear(256, dim), nn.SiLU(), nn.Linear(dim, dim))


class _Final(nn.Module):  # T2IFinalLayer (DiT_I23D.__init__ hard-codes it, dit_i23d.py:52-56)
    def __init__(self, dim, out_channels):
        super().__init__()
        self.linear = nn.Linear(dim, out_channels)
        self.scale_shift_table = nn.Parameter(torch.randn(2, dim) / dim ** 0.5)


class _CaptionEmbedder(nn.Module):
    def __init__(self, i, dim):
        super().__init__()
        self.y_proj = _Mlp(i, dim, dim)


class _XYZPosEmbed(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.xyz_projection = nn.Linear(63, dim)


class DiT_I23D_PCD_PixelArt_noclip(nn.Module):
    """Stage-1 (point cloud) denoiser.  Same constructor keywords as the reference; the ones that only steer the
    deleted / unused parts of the reference constructor chain are accepted and ignored."""

    def __init__(self, input_size=32, patch_size=2, in_channels=4, hidden_size=1152, depth=28, num_heads=16, mlp_ratio=4,
                 class_dropout_prob=0.1, num_classes=1000, learn_sigma=True, mixing_logit_init=-3, mixed_prediction=True,
                 context_dim=False, pooling_ctx_dim=768, roll_out=False, vit_blk=None, final_layer_blk=None,
                 create_cap_embedder=True, use_clay_ca=False, has_caption=False, rope_scaling_factor=1.0, ntk_factor=1.0,
                 enable_rope=False, _stage2=False):
        super().__init__()
        if enable_rope or has_caption:
            raise NotImplementedError("RoPE / caption conditioning are not used by the released i23d models")
        if hidden_size % num_heads or (hidden_size // num_heads) % 8 or hidden_size // num_heads > 128 or hidden_size % 64:
            raise ValueError("head_dim must be a multiple of 8 up to 128 and the width a multiple of 64 (64: the tuned kernels of the released "
                             "models; anything else, e.g. the 16 x 72 of DiT-PixArt-PCD-CLAY-XL, takes ga_attention_hd_bf16)")
        assert patch_size == 1, "point-cloud latents are not patchified (patch_size=1 in every CLAY registry entry)"
        self.in_channels = in_channels
        self.out_channels = in_channels * 2 if learn_sigma else in_channels
        self.embed_dim = hidden_size
        self.num_heads = num_heads
        self.depth = depth
        self.roll_out = roll_out
        self.context_dim = int(context_dim)
        self.has_caption = False
        D = hidden_size
        # creation order follows the reference so that seeded initialisation is comparable
        self.x_embedder = _Mlp(in_channels, D, D)
        self.t_embedder = _TEmb(D)
        self.blocks = nn.ModuleList([_Block(D, num_heads, self.context_dim, mlp_ratio) for _ in range(depth)])
        self.final_layer = _Final(D, self.out_channels)
        self.clip_spatial_proj = _CaptionEmbedder(1024, D)          # unused leftover
        self.adaLN_modulation = nn.Sequential(nn.SiLU(), nn.Linear(D, 6 * D, bias=True))
        if create_cap_embedder:
            self.cap_embedder = nn.Sequential(nn.LayerNorm(pooling_ctx_dim), nn.Linear(pooling_ctx_dim, D))  # unused
        self.attention_y_norm = _RMSNormW(1024)                      # unused leftover
        self.pooled_vec_embedder = nn.Sequential(nn.LayerNorm(self.context_dim), nn.Linear(self.context_dim, D))
        self._stage2 = _stage2
        self.initialize_weights()
        self._init_runtime_state()

    def _init_runtime_state(self):
        """what the host code below keeps per module besides the parameters (every constructor of the family ends with this)"""
        self._pack = None
        self._ctx_cache = None
        self._pooled_cache = None
        self._samplers = DeviceSamplers(self)  # resident conditioning and the captured sampler steps; _prepare() drops them with the pack
        self._busy = threading.RLock()        # see _exclusive()
        self._last_use = None                # (stream, event recorded behind the last call's work)

    # -- re-entrancy ----------------------------------------------------------------------------------------------------
    # The workspace, the cached K / V projections, the resident conditioning and the captured sampler steps with their state buffers
    # belong to the MODULE (one set per shape): that is what lets a captured step serve the next sample.  Two calls on one module
    # therefore must not overlap.  (i) Calls from different STREAMS of one thread are serialised on the device: a call first makes
    # its stream wait for the event recorded behind the previous call's work.  (ii) Calls from different host THREADS at the same
    # time are refused with an error -- use one module per concurrent sampling loop (the weights can be shared tensors).
    @contextlib.contextmanager
    def _exclusive(self, dev):
        if torch.cuda.is_current_stream_capturing():        # inside the caller's own capture: ordering is the caller's
            yield
            return
        if not self._busy.acquire(blocking=False):
            raise RuntimeError("this DiT module is already inside a forward / sampling call on another thread: its workspace, cached "
                               "context and captured sampler steps are per module -- use one module per concurrent sampling loop "
                               "(INTEGRATION.md section 3)")
        try:
            cur = torch.cuda.current_stream(dev)
            if self._last_use is not None and self._last_use[0] != cur:
                cur.wait_event(self._last_use[1])
            yield
            ev = self._last_use[1] if self._last_use is not None and self._last_use[0] == cur else torch.cuda.Event()
            ev.record(cur)
            self._last_use = (cur, ev)
        finally:
            self._busy.release()

    # -- initialisation (dit_models_xformers.py:1119-1159, dit_i23d.py:209-214,508-509) ---------------------------------
    def initialize_weights(self):
        def _basic_init(m):
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        self.apply(_basic_init)
        nn.init.normal_(self.t_embedder.mlp[0].weight, std=0.02)
        nn.init.normal_(self.t_embedder.mlp[2].weight, std=0.02)
        nn.init.constant_(self.final_layer.linear.weight, 0)
        nn.init.constant_(self.final_layer.linear.bias, 0)
        nn.init.constant_(self.adaLN_modulation[-1].weight, 0)
        nn.init.constant_(self.adaLN_modulation[-1].bias, 0)
        nn.init.constant_(self.pooled_vec_embedder[-1].weight, 0)
        nn.init.constant_(self.pooled_vec_embedder[-1].bias, 0)
        if hasattr(self, "cap_embedder"):
            nn.init.constant_(self.cap_embedder[-1].weight, 0)
            nn.init.constant_(self.cap_embedder[-1].bias, 0)

    # -- weight packing -------------------------------------------------------------------------------------------------
    def _signature(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters()) + (bool(self.fold_prenorm), bool(self.tile_weights))

    def _prepare(self, device):
        sig = self._signature()
        if self._pack is not None and self._pack["sig"] == sig and self._pack["device"] == device:
            return self._pack
        keep = []  # tensors the ctypes structs point into

        def bf(t):
            t = t.detach().to(device=device, dtype=torch.bfloat16).contiguous()
            keep.append(t)
            return t.data_ptr()

        def fp(t):
            t = t.detach().to(device=device, dtype=torch.float32).contiguous()
            keep.append(t)
            return t.data_ptr()

        tiled = bool(self.tile_weights)

        def gw(t):      # a weight the GEMM reads: stored as the LDS-DMA tile image (GaGemmArgs.w_tiled), packed once here
            t = t.detach().to(device=device, dtype=torch.bfloat16)
            t = ops.tile_weight(t) if tiled else t.contiguous()
            keep.append(t)
            return t.data_ptr()

        blocks = (ops.GaDitBlockWeights * self.depth)()
        for i, b in enumerate(self.blocks):
            ca, prenorm = getattr(b, self._ca_name), getattr(b, self._ca_prenorm_name)
            blocks[i] = ops.GaDitBlockWeights(
                fp(prenorm.weight), gw(ca.to_q.weight),
                gw(ca.to_q.weight.detach().float() * prenorm.weight.detach().float()[None, :]) if self.fold_prenorm else None,
                gw(torch.cat([ca.to_k.weight, ca.to_v.weight], 0)),
                fp(ca.q_norm.weight), fp(ca.k_norm.weight), gw(ca.to_out[0].weight), fp(ca.to_out[0].bias),
                fp(b.norm1.weight), gw(b.attn.qkv.weight), fp(b.attn.qkv.bias), fp(b.attn.q_norm.weight),
                fp(b.attn.k_norm.weight), gw(b.attn.proj.weight), fp(b.attn.proj.bias), fp(b.norm2.weight),
                gw(b.mlp.mlp[0].weight), fp(b.mlp.mlp[1].bias), gw(b.mlp.mlp[2].weight), fp(b.mlp.mlp[3].bias),
                fp(b.scale_shift_table), fp(b.attention_y_norm.weight) if self._ctx_norm else None)
        xyz_w = xyz_b = None
        if self._stage2:
            xyz_w, xyz_b = fp(self.xyz_pos_embed.xyz_projection.weight), fp(self.xyz_pos_embed.xyz_projection.bias)
        pooled = getattr(self, self._pooled_name)               # LayerNorm(affine) + Linear of the pooled conditioning vector
        final_adaln = self.final_layer.adaLN_modulation[1] if self._block_order == 1 else None   # FinalLayer of the text models
        model = ops.GaDitModel(
            self.embed_dim, self.depth, self.num_heads, self.in_channels, self.out_channels, self.context_dim,
            1 if self._stage2 else 0,
            bf(self.t_embedder.mlp[0].weight), fp(self.t_embedder.mlp[0].bias), bf(self.t_embedder.mlp[2].weight),
            fp(self.t_embedder.mlp[2].bias), fp(pooled[0].weight), fp(pooled[0].bias), bf(pooled[1].weight), fp(pooled[1].bias),
            bf(self.adaLN_modulation[1].weight), fp(self.adaLN_modulation[1].bias), fp(self.x_embedder.fc1.weight),
            fp(self.x_embedder.fc1.bias), gw(self.x_embedder.fc2.weight), fp(self.x_embedder.fc2.bias), xyz_w, xyz_b,
            fp(self.final_layer.scale_shift_table) if final_adaln is None else None,
            fp(self.final_layer.linear.weight), fp(self.final_layer.linear.bias), blocks, 1 if tiled else 0, self._block_order,
            bf(final_adaln.weight) if final_adaln is not None else None, fp(final_adaln.bias) if final_adaln is not None else None)
        self._pack = dict(sig=sig, device=device, model=model, blocks=blocks, keep=keep, ws=None, ws_key=None)
        self._ctx_cache = None
        self._pooled_cache = None
        self._samplers.drop()      # the captured sampler steps read the previous pack's weight copies by address
        return self._pack

    def invalidate_conditioning_cache(self):
        """Drop what the module derived from the conditioning tensors (K / V of ``img_crossattn``, the pooled-vector branch of
        ``img_vector``).  Both are keyed on (address, autograd version, shape): a write that does not move the version counter --
        ``.data.copy_``, a custom kernel, DLPack / another framework writing into the same storage -- must be followed by this call
        (INTEGRATION.md section 3).  The sampling entry points copy their conditioning into module-owned buffers with ``copy_``
        every call, so they never serve a stale projection."""
        self._ctx_cache = None
        self._pooled_cache = None

    # What tells the caption-conditioned twins (dit/dit_trilatent.py) from these models, for the shared host code: the context keys,
    # the names of the cross-attention modules, the block order / final layer (GaDitModel.block_order) and the per-block context norm
    _ctx_key, _vec_key = "img_crossattn", "img_vector"
    _ca_name, _ca_prenorm_name, _pooled_name = "cross_attn_dino", "prenorm_ca_dino", "pooled_vec_embedder"
    _block_order, _ctx_norm = 0, False

    ca_skip = True  # skip the cross-attention of batch items whose image tokens are all zero (exact; tests switch it off)
    # fold the (un-modulated) cross-attention pre-norm into the neighbouring GEMMs (include/ga_dit.h); GA_DIT_FOLD=0: A/B aid
    fold_prenorm = os.environ.get("GA_DIT_FOLD", "1") != "0"
    # GEMM weights stored as 1-KiB LDS-DMA tiles (GaGemmArgs.w_tiled); GA_DIT_TILED=0: row-major, A/B aid
    tile_weights = os.environ.get("GA_DIT_TILED", "1") != "0"

    def _context_kv(self, pack, ctx_tokens: torch.Tensor):
        key = (ctx_tokens.data_ptr(), ctx_tokens._version, tuple(ctx_tokens.shape), ctx_tokens.dtype)
        if self._ctx_cache is not None and self._ctx_cache[0] == key:
            return self._ctx_cache[1]
        B, M, C = ctx_tokens.shape
        ctx = ctx_tokens.detach().to(torch.bfloat16).contiguous()
        Mp = (M + 63) // 64 * 64
        old = self._ctx_cache[1] if self._ctx_cache is not None else None
        kcols = self.embed_dim      # (round 6: K row-major + V^T for every head dim)
        if old is not None and old[0].shape == (self.depth, B * M, kcols) and old[0].device == ctx.device:
            ck, cvt = old[0], old[1]   # same shapes: projected in place (the pad columns of cvt stay zero), so a captured sampler step
                                       # that has these addresses baked in serves the next sample's conditioning as well
        else:
            ck = torch.empty((self.depth, B * M, kcols), dtype=torch.bfloat16, device=ctx.device)
            cvt = torch.zeros((self.depth, B * self.embed_dim, Mp), dtype=torch.bfloat16, device=ctx.device)
        stream = ctypes.c_void_p(torch.cuda.current_stream(ctx.device).cuda_stream)
        if self._ctx_norm:     # every block normalises the tokens itself before its to_k / to_v: a scratch for the normalised copy
            nscr = ops.lib().ga_dit_context_scratch_bytes(ctypes.byref(pack["model"]), B, M)
            scr = torch.empty(nscr + 256, dtype=torch.uint8, device=ctx.device)
            ops.check(ops.lib().ga_dit_cache_context_ws(ctypes.byref(pack["model"]), B, M, ctx.data_ptr(), ck.data_ptr(), cvt.data_ptr(),
                                                        scr.data_ptr() + ((-scr.data_ptr()) % 256), nscr, stream), "ga_dit_cache_context_ws")
            scr.record_stream(torch.cuda.current_stream(ctx.device))
        else:
            ops.check(ops.lib().ga_dit_cache_context(ctypes.byref(pack["model"]), B, M, ctx.data_ptr(), ck.data_ptr(),
                                                     cvt.data_ptr(), stream), "ga_dit_cache_context")
        # leading batch items with a non-zero context; the all-zero ones (unconditional half of a CFG batch) skip the
        # cross-attention exactly (include/ga_dit.h: ca_batch).  One host read per conditioning tensor.
        nz = (ctx_tokens.detach().reshape(B, -1) != 0).any(dim=1).tolist()
        ca_batch = sum(nz) if (self.ca_skip and nz == sorted(nz, reverse=True)) else B
        self._ctx_cache = (key, (ck, cvt, max(ca_batch, 1)), ctx_tokens)  # keeps the key tensor alive (address not reused)
        return ck, cvt, max(ca_batch, 1)

    # pooled_vec_embedder(img_vector) does not depend on the time: once per conditioning vector (GaDitForwardArgs.pooled_vec), kept in a
    # buffer of its own that is rewritten in place for the next vector of the same shape (a captured sampler step has its address baked in)
    pooled_once = os.environ.get("GA_DIT_POOLED_ONCE", "1") != "0"     # GA_DIT_POOLED_ONCE=0: inside every evaluation, A/B aid

    def _pooled(self, pack, vec: torch.Tensor):
        if not self.pooled_once:
            return None
        key = (vec.data_ptr(), vec._version, tuple(vec.shape))
        held = self._pooled_cache
        if held is not None and held[0] == key:
            return held[1]
        B = vec.shape[0]
        out = held[1] if held is not None and held[1].shape == (B, self.embed_dim) and held[1].device == vec.device else \
            torch.empty((B, self.embed_dim), dtype=torch.float32, device=vec.device)
        scratch = torch.empty((B, self.context_dim), dtype=torch.float32, device=vec.device)
        stream = ctypes.c_void_p(torch.cuda.current_stream(vec.device).cuda_stream)
        ops.check(ops.lib().ga_dit_pooled_vector(ctypes.byref(pack["model"]), B, vec.data_ptr(), scratch.data_ptr(), out.data_ptr(), stream),
                  "ga_dit_pooled_vector")
        self._pooled_cache = (key, out, vec)     # keeps the key tensor alive (its address is not reused)
        return out

    # -- the reference surface ------------------------------------------------------------------------------------------
    def forward(self, x, timesteps=None, context=None, y=None, get_attr="", _step=None, **kwargs):
        assert isinstance(context, dict)
        if x.device.type != "cuda":
            raise RuntimeError("gaussiananything_amd DiT only runs on an MI355X (HIP) device; there is no CPU path")
        with self._exclusive(x.device):
            return self._forward(x, timesteps, context, _step)

    def _forward(self, x, timesteps, context, _step):
        dev = x.device
        pack = self._prepare(dev)
        B, L, C = x.shape
        assert C == self.in_channels
        ck, cvt, ca_batch = self._context_kv(pack, context[self._ctx_key])
        Mctx = context[self._ctx_key].shape[1]
        xin = x if _step is not None else x.detach().float().contiguous()
        t = timesteps.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        if t.numel() == 1 and B > 1:
            t = t.expand(B).contiguous()
        vec = context[self._vec_key].detach().float().contiguous()
        pooled = self._pooled(pack, vec) if vec is context[self._vec_key] or vec.data_ptr() == context[self._vec_key].data_ptr() else None
        xyz = context["fps-xyz"].detach().float().contiguous() if self._stage2 else None
        out = torch.empty((B, L, self.out_channels), dtype=torch.float32, device=dev) if _step is None else None
        Lib = ops.lib()
        ws_key = (B, L, Mctx)
        if pack["ws_key"] != ws_key:
            nbytes = Lib.ga_dit_workspace_bytes(ctypes.byref(pack["model"]), B, L, Mctx)
            if nbytes == 0:
                raise RuntimeError("ga_dit_workspace_bytes rejected the model / batch shape")
            buf = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
            pack["ws"], pack["ws_key"], pack["ws_bytes"] = buf, ws_key, nbytes
        buf = pack["ws"]
        base = buf.data_ptr() + ((-buf.data_ptr()) % 256)
        args = ops.GaDitForwardArgs(B, L, Mctx, xin.data_ptr(), t.data_ptr(), vec.data_ptr(),
                                    xyz.data_ptr() if xyz is not None else None, ck.data_ptr(), cvt.data_ptr(),
                                    out.data_ptr() if out is not None else None, base, pack["ws_bytes"], ca_batch,
                                    ctypes.pointer(_step) if _step is not None else None,
                                    pooled.data_ptr() if pooled is not None else None)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        ops.check(Lib.ga_dit_forward(ctypes.byref(pack["model"]), ctypes.byref(args), stream), "ga_dit_forward")
        return out

    def forward_with_cfg(self, x, t, context, cfg_scale):
        eps = self.forward(x, t, context)
        cond_eps, uncond_eps = torch.split(eps, len(eps) // 2, dim=0)
        half_eps = uncond_eps + cfg_scale * (cond_eps - uncond_eps)
        return torch.cat([half_eps, half_eps], dim=0)

    def forward_cond(self, x, t, context, cfg_scale=None):
        """The conditional evaluation alone, with the call signature of ``forward_with_cfg``: what the sampling loop uses when
        guidance is a no-op (unconditional conditioning == conditional one, the release's stage 2; cascade.sample)."""
        return self.forward(x, t, context)

    # The device-resident samplers: residency of the conditioning, the captured steps held between calls, the rule for replaying one
    # and the three step bodies live in dit/device_samplers.py (self._samplers); here, the guard around a call on this module
    def sample_euler_fused(self, y0, t_grid, context, cfg_scale=1.0, cfg=True):
        with self._exclusive(y0.device):
            return self._samplers.euler(y0, t_grid, context, cfg_scale, cfg)

    def sample_dopri5_device(self, y0, t_grid, context, cfg_scale=1.0, cfg=True, atol=1e-6, rtol=1e-3, stats=None, max_steps=1 << 16):
        with self._exclusive(y0.device):
            return self._samplers.dopri5(y0, t_grid, context, cfg_scale, cfg, atol, rtol, stats, max_steps)

    def sample_sde_device(self, x0, coef, context, method="Euler", last_step="Mean", cfg_scale=1.0, cfg=True, seed=0, noise=None,
                          noise_out=None):
        with self._exclusive(x0.device):
            return self._samplers.sde(x0, coef, context, method, last_step, cfg_scale, cfg, seed, noise, noise_out)


class DiT_I23D_PCD_PixelArt_noclip_clay_stage2(DiT_I23D_PCD_PixelArt_noclip):
    """Stage-2 (KL feature) denoiser conditioned on the stage-1 point cloud (dit_i23d.py:664-750)."""

    def __init__(self, *args, use_pe_cond=False, **kwargs):
        if not use_pe_cond:
            raise NotImplementedError("only the released use_pe_cond=True variant (xyz positional embedding) is built")
        super().__init__(*args, _stage2=True, **kwargs)
        self.use_pe_cond = use_pe_cond
        self.xyz_pos_embed = _XYZPosEmbed(self.embed_dim)
        self._init_runtime_state()


def _clay(depth, hidden, heads, stage2=False):
    def make(**kw):
        kw.pop("vit_blk", None)
        if stage2:
            return DiT_I23D_PCD_PixelArt_noclip_clay_stage2(depth=depth, hidden_size=hidden, patch_size=1, num_heads=heads,
                                                            use_clay_ca=True, use_pe_cond=True, **kw)
        return DiT_I23D_PCD_PixelArt_noclip(depth=depth, hidden_size=hidden, patch_size=1, num_heads=heads,
                                            use_clay_ca=True, **kw)
    return make


# the CLAY entries of the reference registry (dit_i23d.py:1665-1697)
DiT_models = {
    "DiT-PixArt-PCD-CLAY-XL": _clay(28, 1152, 16),  # 16 heads of 72 (dit_i23d.py:1526-1535): ga_attention_hd_bf16, nothing folded
    "DiT-PixArt-PCD-CLAY-L": _clay(24, 1024, 16),
    "DiT-PixArt-PCD-CLAY-B": _clay(12, 768, 12),
    "DiT-PixArt-PCD-CLAY-stage2-B": _clay(12, 768, 12, stage2=True),
    "DiT-PixArt-PCD-CLAY-stage2-L": _clay(24, 1024, 16, stage2=True),
}
