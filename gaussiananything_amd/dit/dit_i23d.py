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
        held = getattr(self, "_pooled_cache", None)
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

    def _resident_context(self, context):
        """The conditioning of a sampling call copied into buffers the model owns (one set per shape): every evaluation of the call --
        and the captured sampler step, which has their addresses baked in -- reads these, so the step captured for one sample is
        replayed for the next one (capturing ~1 750 launches costs ~10 ms per call)."""
        held = getattr(self, "_ctx_bufs", None) or {}
        out = {}
        for name, t in context.items():
            want = torch.float32 if name in (self._vec_key, "fps-xyz") else t.dtype
            buf = held.get(name)
            if buf is None or buf.shape != t.shape or buf.dtype != want or buf.device != t.device:
                buf = torch.empty(t.shape, dtype=want, device=t.device)
            buf.copy_(t.detach())
            out[name] = buf
        self._ctx_bufs = out
        return out

    def _replay_signature(self, context, shape, n, cfg, cfg_scale):
        """What a captured sampler step has baked in besides its own buffers: the model's workspace, the K / V projections of the
        conditioning tokens (refreshed here, in place when the shapes are those of the previous call), the number of batch items
        that skip the cross-attention, the resident conditioning vectors -- all by address.  None: nothing to replay against yet."""
        B, L, _ = shape
        tok = context[self._ctx_key]
        pack = self._prepare(tok.device)
        ck, cvt, ca_batch = self._context_kv(pack, tok)
        if pack.get("ws") is None or pack["ws_key"] != (B, L, tok.shape[1]):
            return None
        sig = [tuple(shape), n, bool(cfg), float(cfg_scale), pack["ws"].data_ptr(), ck.data_ptr(), cvt.data_ptr(), ca_batch]
        vec = context[self._vec_key]
        if self.pooled_once and vec.dtype == torch.float32 and vec.is_contiguous():
            sig.append(self._pooled(pack, vec).data_ptr())     # (refreshed in place for this call's vector)
        for name in (self._vec_key,) + (("fps-xyz",) if self._stage2 else ()):
            t = context[name]
            if t.dtype != torch.float32 or not t.is_contiguous():
                return None   # (forward() would hand the kernels a temporary copy)
            sig.append((t.data_ptr(), tuple(t.shape)))
        return tuple(sig)

    def sample_euler_fused(self, y0, t_grid, context, cfg_scale=1.0, cfg=True):
        with self._exclusive(y0.device):
            return self._sample_euler_fused(y0, t_grid, context, cfg_scale, cfg)

    @torch.no_grad()
    def _sample_euler_fused(self, y0, t_grid, context, cfg_scale=1.0, cfg=True):
        """The reference's fixed-grid Euler sampling loop (transport/integrators.py:100-119 with method "euler":
        y_{k+1} = y_k + (t_{k+1} - t_k) f(t_k, y_k), all grid states returned) with the whole step on the device: the
        function evaluation, the CFG combine of ``forward_with_cfg`` and the state update leave through the final-layer
        kernel (GaDitSamplerStep), a one-thread kernel moves the step counter / time / step size on, and one step is
        captured into a HIP graph and replayed -- nothing but this library's kernels between two steps, no host
        synchronisation.  Bit-identical to the eager loop over ``forward_with_cfg`` / ``forward_cond``."""
        if self.out_channels != self.in_channels:
            raise ValueError("the fused sampler step needs a velocity of the state's shape (learn_sigma=False)")
        dev = y0.device
        tt = [float(v) for v in t_grid]
        n = len(tt)
        context = self._resident_context(context)
        sig = self._replay_signature(context, y0.shape, n, cfg, cfg_scale) if n >= 2 else None
        held = getattr(self, "_euler_replay", None)
        if sig is not None and held is not None and held[0] == sig:     # the step captured by an earlier call, on its buffers
            _, y, out, t_arr, dt_arr, counter, tvec, dt, step, graph, keep = held
            out[0].copy_(y0.detach().float())
            t_arr.copy_(torch.tensor(tt[:-1], dtype=torch.float32))
            dt_arr.copy_(torch.tensor([b - a for a, b in zip(tt[:-1], tt[1:])], dtype=torch.float32))
            y.copy_(out[0]); counter.zero_(); tvec.fill_(tt[0]); dt.copy_(dt_arr[0:1])
            for _ in range(n - 1):
                graph.replay()
            return out.clone()
        y = y0.detach().float().contiguous().clone()
        out = torch.empty((n,) + tuple(y.shape), dtype=torch.float32, device=dev)
        out[0].copy_(y)
        if n < 2:
            return out
        B = y.shape[0]
        t_arr = torch.tensor(tt[:-1], dtype=torch.float32, device=dev)
        dt_arr = torch.tensor([b - a for a, b in zip(tt[:-1], tt[1:])], dtype=torch.float32, device=dev)
        counter = torch.zeros(1, dtype=torch.int32, device=dev)
        tvec = torch.empty(B, dtype=torch.float32, device=dev)
        dt = torch.empty(1, dtype=torch.float32, device=dev)
        step = ops.GaDitSamplerStep(float(cfg_scale), 1 if cfg else 0, dt.data_ptr(), y.data_ptr(), out.data_ptr(),
                                    y.numel(), counter.data_ptr(), None)
        Lib = ops.lib()

        def one_step():
            self.forward(y, tvec, context, _step=step)
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            ops.check(Lib.ga_dit_sampler_advance(counter.data_ptr(), t_arr.data_ptr(), dt_arr.data_ptr(), n - 1,
                                                 tvec.data_ptr(), B, dt.data_ptr(), stream), "ga_dit_sampler_advance")

        def reset():
            y.copy_(out[0])
            counter.zero_()
            tvec.fill_(tt[0])
            dt.copy_(dt_arr[0:1])

        reset()
        cur = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(dev)
        side.wait_stream(cur)
        with torch.cuda.stream(side):   # warm-up outside the capture: lazy initialisation, workspace sizing, K/V caches
            one_step()
        cur.wait_stream(side)
        reset()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            one_step()
        reset()   # (capture does not execute; the state is as before)
        for _ in range(n - 1):
            graph.replay()
        # kept for the replays in flight -- and for later calls on the same conditioning tensors (see _replay_signature)
        sig = self._replay_signature(context, y.shape, n, cfg, cfg_scale)
        self._euler_replay = (sig, y, out, t_arr, dt_arr, counter, tvec, dt, step, graph, tuple(context.values()))
        return out.clone() if sig is not None else out


    def sample_dopri5_device(self, y0, t_grid, context, cfg_scale=1.0, cfg=True, atol=1e-6, rtol=1e-3, stats=None, max_steps=1 << 16):
        with self._exclusive(y0.device):
            return self._sample_dopri5_device(y0, t_grid, context, cfg_scale, cfg, atol, rtol, stats, max_steps)

    @torch.no_grad()
    def _sample_dopri5_device(self, y0, t_grid, context, cfg_scale=1.0, cfg=True, atol=1e-6, rtol=1e-3, stats=None, max_steps=1 << 16):
        """The reference's DEFAULT sampler -- torchdiffeq's dopri5 behind ``ode.sample`` (transport/integrators.py:100-119,
        flow_matching_trainer.py:715) -- with the adaptive loop on the device (csrc/ode_dopri5.hip): one attempted step = six
        (stage input, function evaluation with the guided velocity leaving through the final-layer kernel) pairs, the error norm, a
        one-thread controller and a predicated accept kernel with the dense output, captured into ONE HIP graph and replayed; time,
        step size, decisions and counters live in a device block and the host only reads the ``done`` word after a replay.  Same
        decisions as ``transport/odeint.py`` / ``oracle/ode.py`` (the initial step size is chosen on the host as there: two
        evaluations).  Returns the states at every requested time."""
        from ..transport.odeint import _initial_step
        if self.out_channels != self.in_channels:
            raise ValueError("the device-resident dopri5 needs a velocity of the state's shape (learn_sigma=False)")
        dev = y0.device
        tt = [float(v) for v in t_grid]
        ng = len(tt)
        Lib = ops.lib()
        B, n = y0.shape[0], y0.numel()
        context = self._resident_context(context)
        sig = self._replay_signature(context, y0.shape, ng, cfg, cfg_scale)
        held = getattr(self, "_dopri5_replay", None)
        if sig is not None and held is not None and held["sig"] == sig:     # buffers and captured step of an earlier call
            st = held
        else:
            y = torch.empty(tuple(y0.shape), dtype=torch.float32, device=dev)
            st = {"sig": None, "y": y, "out": torch.empty((ng,) + tuple(y.shape), dtype=torch.float32, device=dev),
                  "k": [torch.empty_like(y) for _ in range(7)], "ystage": torch.empty_like(y),
                  "tvec": torch.empty(B, dtype=torch.float32, device=dev),
                  "ctl": torch.zeros(ops.GA_ODE_CTL_ALLOC, dtype=torch.float64, device=dev),
                  "tg": torch.empty(ng, dtype=torch.float64, device=dev), "graph": None,
                  "host": torch.empty(ops.GA_ODE_CTL_WORDS, dtype=torch.float64).pin_memory(), "keep": tuple(context.values())}
        y, out, k, ystage, tvec, ctl, tg, host = (st[q] for q in ("y", "out", "k", "ystage", "tvec", "ctl", "tg", "host"))
        y.copy_(y0.detach().float())
        out[0].copy_(y)
        tg.copy_(torch.tensor(tt, dtype=torch.float64))
        nfe = [0]

        def velocity_into(dst, x, tv):
            nfe[0] += 1
            self.forward(x, tv, context, _step=ops.GaDitSamplerStep(float(cfg_scale), 1 if cfg else 0, None, None, None, 0, None, dst.data_ptr()))

        def rhs(ts, yy):      # (the two host-side evaluations of the initial step size)
            r = torch.empty_like(y)
            velocity_into(r, yy.contiguous(), torch.full((B,), float(ts), dtype=torch.float32, device=dev))
            return r

        tvec.fill_(tt[0])
        velocity_into(k[0], y, tvec)
        dt0 = _initial_step(rhs, tt[0], y, k[0], rtol, atol)
        head = torch.zeros(ops.GA_ODE_CTL_WORDS, dtype=torch.float64)
        head[ops.GA_ODE_T], head[ops.GA_ODE_DT], head[ops.GA_ODE_ATOL], head[ops.GA_ODE_RTOL], head[ops.GA_ODE_JNEXT] = tt[0], dt0, atol, rtol, 1
        ctl[:ops.GA_ODE_CTL_WORDS].copy_(head)
        evals_before = nfe[0]
        if ng > 1:
            if st["graph"] is None:
                ode = ops.GaOdeDopri5(n, B, ng, y.data_ptr(), (ops.c_p * 7)(*[t.data_ptr() for t in k]), ystage.data_ptr(), tvec.data_ptr(),
                                      ctl.data_ptr(), tg.data_ptr(), out.data_ptr(), ctl.numel())

                def attempt():
                    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                    for i in range(6):
                        ops.check(Lib.ga_ode_dopri5_stage(ctypes.byref(ode), i, stream), "ga_ode_dopri5_stage")
                        velocity_into(k[i + 1], ystage, tvec)
                    ops.check(Lib.ga_ode_dopri5_finish(ctypes.byref(ode), stream), "ga_ode_dopri5_finish")

                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):     # (capture executes nothing; the evaluations above were the warm-up)
                    attempt()
                st["graph"], st["ode"] = graph, ode
                nfe[0] = evals_before
                # (the signature exists once the first evaluations have sized the workspace and cached the K / V)
                st["sig"] = self._replay_signature(context, y.shape, ng, cfg, cfg_scale)
                self._dopri5_replay = st
            graph = st["graph"]
            done_evt = torch.cuda.Event()
            while True:
                graph.replay()
                host.copy_(ctl[:ops.GA_ODE_CTL_WORDS], non_blocking=True)
                done_evt.record()
                done_evt.synchronize()
                if host[ops.GA_ODE_DONE] != 0 or host[ops.GA_ODE_STEPS] >= max_steps:
                    break
            err, steps = int(host[ops.GA_ODE_ERROR]), int(host[ops.GA_ODE_STEPS])
            if err == 1:
                raise FloatingPointError(f"dopri5: non-finite error ratio at t = {float(host[ops.GA_ODE_T])}: the model returned NaN/inf")
            if err == 2:
                raise FloatingPointError(f"dopri5: step size underflow at t = {float(host[ops.GA_ODE_T])}")
            if host[ops.GA_ODE_DONE] == 0:
                raise RuntimeError(f"dopri5: more than {max_steps} attempted steps")
            if stats is not None:
                stats.update(nfe=evals_before + 6 * steps, steps=steps, rejected=int(host[ops.GA_ODE_REJECTED]), graph=True, device_loop=True,
                             ctl=[float(v) for v in host])     # the controller's scalar block after the last step (tests: bit-reproducible)
        elif stats is not None:
            stats.update(nfe=evals_before, steps=0, rejected=0, graph=True, device_loop=True)
        return out.clone()

    def sample_sde_device(self, x0, coef, context, method="Euler", last_step="Mean", cfg_scale=1.0, cfg=True, seed=0, noise=None,
                          noise_out=None):
        with self._exclusive(x0.device):
            return self._sample_sde_device(x0, coef, context, method, last_step, cfg_scale, cfg, seed, noise, noise_out)

    @torch.no_grad()
    def _sample_sde_device(self, x0, coef, context, method, last_step, cfg_scale, cfg, seed, noise, noise_out):
        """The reference's SDE sampling loop (``Sampler.sample_sde``, transport/transport.py:322-382: the stepper of
        transport/integrators.py:8-75 and one last step) with every step on the device (csrc/ode_sde.hip, GaSdeStep in
        include/ga_dit.h): a step is the function evaluation with the guided velocity leaving through the final-layer kernel, the
        Euler-Maruyama update (``method="Euler"``) or Heun's three phases around two evaluations (``"Heun"``) with the noise drawn
        inside the kernel, and the one-thread advance -- captured into ONE HIP graph and replayed for every interval, then the last
        step eagerly.  The step index, the coefficient table ``coef`` ([intervals + 1, GA_SDE_COEF_STRIDE] fp32, built by
        ``transport.sampler.sde_coefficients``), the seed and the initial state are device data rewritten per call: the captured step
        serves any seed, diffusion form and norm, and every replay draws fresh noise.  ``cfg``: the state is a doubled CFG batch whose
        halves take the same noise.  ``noise`` [intervals, n_draw]: normals to use instead; ``noise_out`` [intervals, n_draw]: receives
        the normals every step used.  Returns [intervals + 1, *x0.shape] fp32: slot k is the state after step k, the last slot the
        last step's output.  Bit-identical to the eager loop of ``transport/sampler.py`` on the same normals."""
        if self.out_channels != self.in_channels:
            raise ValueError("the device-resident SDE sampler needs a velocity of the state's shape (learn_sigma=False)")
        phases = {"Euler": (ops.GA_SDE_EM,), "Heun": (ops.GA_SDE_HEUN_PERTURB, ops.GA_SDE_HEUN_PREDICT, ops.GA_SDE_HEUN_CORRECT)}
        lasts = {"Mean": ops.GA_SDE_LAST_MEAN, "Tweedie": ops.GA_SDE_LAST_TWEEDIE, "Euler": ops.GA_SDE_LAST_EULER, None: ops.GA_SDE_LAST_NONE}
        if method not in phases or last_step not in lasts:
            raise ValueError(f"SDE sampler: method {method!r} / last step {last_step!r} (have {tuple(phases)} / {tuple(lasts)})")
        dev = x0.device
        ni = coef.shape[0] - 1
        if coef.dim() != 2 or coef.shape[1] != ops.GA_SDE_COEF_STRIDE or ni < 1:
            raise ValueError("coef is the [intervals + 1, GA_SDE_COEF_STRIDE] table of sde_coefficients")
        B, n = x0.shape[0], x0.numel()
        nd = n // 2 if cfg else n
        if cfg and B % 2:
            raise ValueError("a CFG state holds the conditional and the unconditional half")
        for name, t in (("noise", noise), ("noise_out", noise_out)):
            if t is not None and (t.numel() != ni * nd or t.shape[0] != ni):
                raise ValueError(f"{name} is [intervals = {ni}, n_draw = {nd}]")
        Lib = ops.lib()
        context = self._resident_context(context)
        key = (method, ni + 1, noise is not None, noise_out is not None)
        sig = self._replay_signature(context, x0.shape, ni + 1, cfg, cfg_scale)
        held = getattr(self, "_sde_replay", None)
        if sig is not None and held is not None and held["sig"] == (sig, key):     # buffers and captured step of an earlier call
            st = held
        else:
            y = torch.empty(tuple(x0.shape), dtype=torch.float32, device=dev)
            st = {"sig": None, "y": y, "vel": torch.empty_like(y), "k1": torch.empty_like(y), "xhat": torch.empty_like(y),
                  "out": torch.empty((ni + 1,) + tuple(y.shape), dtype=torch.float32, device=dev),
                  "counter": torch.zeros(1, dtype=torch.int32, device=dev), "tvec": torch.empty(B, dtype=torch.float32, device=dev),
                  "coef": torch.empty((ni + 1, ops.GA_SDE_COEF_STRIDE), dtype=torch.float32, device=dev),
                  "seed": torch.zeros(1, dtype=torch.int64, device=dev),
                  "noise": torch.empty((ni, nd), dtype=torch.float32, device=dev) if noise is not None else None,
                  "nout": torch.empty(nd, dtype=torch.float32, device=dev) if noise_out is not None else None,
                  "graph": None, "keep": tuple(context.values())}
        y, vel, out, counter, tvec, cf = (st[q] for q in ("y", "vel", "out", "counter", "tvec", "coef"))
        cf.copy_(coef.detach().to(torch.float32))
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        st["seed"].copy_(torch.tensor([seed - (1 << 64) if seed >> 63 else seed], dtype=torch.int64))
        if noise is not None:
            st["noise"].copy_(noise.detach().reshape(ni, nd))
        sde = ops.GaSdeStep(n, B, ni, 1 if cfg else 0, y.data_ptr(), vel.data_ptr(), st["k1"].data_ptr(), st["xhat"].data_ptr(),
                            out.data_ptr(), counter.data_ptr(), tvec.data_ptr(), cf.data_ptr(), st["seed"].data_ptr(),
                            st["noise"].data_ptr() if noise is not None else None, st["nout"].data_ptr() if noise_out is not None else None)
        vstep = ops.GaDitSamplerStep(float(cfg_scale), 1 if cfg else 0, None, None, None, 0, None, vel.data_ptr())

        def phase(p):
            stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            ops.check(Lib.ga_sde_step(ctypes.byref(sde), p, stream), "ga_sde_step")

        def one_step():     # a single chain of launches
            if method == "Euler":
                self.forward(y, tvec, context, _step=vstep)
                phase(ops.GA_SDE_EM)
            else:
                phase(ops.GA_SDE_HEUN_PERTURB)
                self.forward(st["xhat"], tvec, context, _step=vstep)
                phase(ops.GA_SDE_HEUN_PREDICT)
                self.forward(y, tvec, context, _step=vstep)
                phase(ops.GA_SDE_HEUN_CORRECT)
            phase(ops.GA_SDE_ADVANCE)

        def reset():
            y.copy_(x0.detach().float())
            counter.zero_()
            tvec.copy_(cf[0, ops.GA_SDE_C_T].expand(B))

        reset()
        if st["graph"] is None:
            cur = torch.cuda.current_stream(dev)
            side = torch.cuda.Stream(dev)
            side.wait_stream(cur)
            with torch.cuda.stream(side):   # warm-up outside the capture: lazy initialisation, workspace sizing, K/V caches
                one_step()
            cur.wait_stream(side)
            reset()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                one_step()
            reset()   # (capture does not execute; the state is as before)
            st["graph"] = graph
            # (the signature exists once the first evaluation has sized the workspace and cached the K / V)
            sig = self._replay_signature(context, y.shape, ni + 1, cfg, cfg_scale)
            st["sig"] = (sig, key) if sig is not None else None
            self._sde_replay = st
        for k in range(ni):
            st["graph"].replay()
            if noise_out is not None:
                noise_out[k].reshape(-1).copy_(st["nout"])
        if last_step is not None:
            self.forward(y, tvec, context, _step=vstep)      # (ADVANCE left t1 in tvec)
        phase(lasts[last_step])
        return out.clone()


class DiT_I23D_PCD_PixelArt_noclip_clay_stage2(DiT_I23D_PCD_PixelArt_noclip):
    """Stage-2 (KL feature) denoiser conditioned on the stage-1 point cloud (dit_i23d.py:664-750)."""

    def __init__(self, *args, use_pe_cond=False, **kwargs):
        if not use_pe_cond:
            raise NotImplementedError("only the released use_pe_cond=True variant (xyz positional embedding) is built")
        super().__init__(*args, _stage2=True, **kwargs)
        self.use_pe_cond = use_pe_cond
        self.xyz_pos_embed = _XYZPosEmbed(self.embed_dim)
        self._pack = None


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
