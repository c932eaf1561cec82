"""The cascaded image-to-3D / text-to-3D sampling loop around the hot path: what ``FlowMatchingEngine.sample`` and the two sampling
scripts do between the conditioner and the renderer (/root/reference/nsr/lsgm/flow_matching_trainer.py:700-744 ``sample``;
:1206-1225 stage hand-off; :1400-1424 ``render_gs_video_given_latent``; shell_scripts/release/inference/i23d/*.sh).

    stage 1  z ~ N(0, I) [S, 768, 3]  --250-step ODE, CFG-->  normalised point cloud;  x 0.164 (``xyz_std``, :987-1000), clipped to
             +-0.45 when it is read back as the stage-2 condition (:1079)
    stage 2  z ~ N(0, I) [S, 768, 10], context + {'fps-xyz'}  --250-step ODE, CFG-->  KL latent
    decode   {latent_normalized, query_pcd_xyz} -> surfels (SurfelDecoder)  ->  triplane_decode -> renders per level

The reference writes the stage-1 cloud to a PLY file and a second script loads it; here the tensor stays on the device.
Host orchestration only -- every kernel launch is behind the three C-ABI headers.
"""
from __future__ import annotations

import torch

from .transport import Sampler, create_transport

XYZ_STD = 0.164  # flow_matching_trainer.py:987
PCD_SCALING_FACTOR = 0.45  # sgm/configs/stage2-i23d.yaml:55-57 -> PCD_Scaler (sgm/modules/encoders/modules.py:1746-1768)


@torch.no_grad()
def sample(model, cond, uc, shape, batch_size=1, cfg_scale=4.0, seed=42, num_steps=250, sampling_method="dopri5",
           transport_sampler=None, noise_dtype=torch.bfloat16, stats=None, dedup_noop_cfg=True, sde=None, **ode_kwargs):
    """``FlowMatchingEngine.sample`` (flow_matching_trainer.py:700-744): CPU-seeded noise, CFG batch = [cond | uncond],
    ``sample_ode(num_steps=250, cfg=True)`` (dopri5 by default, as upstream), last state, conditional half.

    ``noise_dtype``: the reference draws fp32 noise on the CPU and rounds it to the engine dtype before sampling
    (``.to(self.dtype)``, :720; the release runs bf16 AMP), so the initial state is a bf16-representable tensor; the ODE
    state is fp32 from the first update on.  ``None`` keeps the un-rounded fp32 draw.

    ``dedup_noop_cfg``: when the unconditional conditioning IS the conditional one (``uc[k] is cond[k]`` for every key -- the
    release's stage 2, ``stage2_conditioning``), both halves of the CFG batch are the same sequence, ``forward_with_cfg``
    returns ``uncond + s * (cond - uncond) = cond`` and the two halves of the ODE state stay equal (dopri5's RMS norm over
    the doubled state equals that over one half): the denoiser is evaluated on the conditional half alone -- the same
    numbers up to the GEMM tile shapes chosen for the smaller batch, half the work.

    ``sde``: a dict of ``Sampler.sample_sde`` keywords (may be empty) samples this stage with the SDE sampler instead of
    ``sample_ode`` -- ``num_steps`` and ``seed`` default to this call's, ``sampling_method`` / ``ode_kwargs`` are then not used;
    ``stats`` receives nfe / steps / sde=True."""
    if transport_sampler is None:
        transport_sampler = Sampler(create_transport("GVP", "velocity", None, None, None, snr_type="uniform"))
    if sde is not None:
        sample_fn = transport_sampler.sample_sde(**dict({"num_steps": num_steps, "seed": seed}, **sde))
        last = "last_sde"
    else:
        sample_fn = transport_sampler.sample_ode(sampling_method=sampling_method, num_steps=num_steps, cfg=True, **ode_kwargs)
        last = "last_ode"
    dev = next(model.parameters()).device
    torch.manual_seed(seed)
    zs = torch.randn(batch_size, *shape).to(dev)
    if noise_dtype is not None:
        zs = zs.to(noise_dtype).float()
    if dedup_noop_cfg and all(uc[k] is cond[k] for k in cond):
        def cond_only(x, t, context=None, cfg_scale=None):
            return model.forward(x, t, context)
        samples = sample_fn(zs, getattr(model, "forward_cond", cond_only), context=dict(cond), cfg_scale=cfg_scale)[-1]
        if stats is not None:
            stats.update(getattr(getattr(transport_sampler, last, None), "last_stats", {}) or {}, noop_cfg_dedup=True)
        return samples
    c_out = {k: torch.cat((cond[k], uc[k]), 0) for k in cond}
    zs = torch.cat([zs, zs], 0)
    samples = sample_fn(zs, model.forward_with_cfg, context=c_out, cfg_scale=cfg_scale)[-1]
    if stats is not None:   # function evaluations / accepted / rejected steps of this stage's ODE solve
        stats.update(getattr(getattr(transport_sampler, last, None), "last_stats", {}) or {})
    samples, _ = samples.chunk(2, dim=0)
    return samples


@torch.no_grad()
def condition_on_image(embedder, image):
    """The conditioning dicts of the i23d release from an image batch in [-1, 1] (``FrozenDinov2ImageEmbedder`` with
    ``output_cls=True``, configs: sgm/modules/encoders/modules.py:791-931): cond = {'img_crossattn': patch tokens
    [S,1369,1024], 'img_vector': cls token [S,1024]}; the unconditional half of CFG is all zeros
    (flow_matching_trainer.py:1148-1153 ``get_unconditional_conditioning`` with ucg force-zero)."""
    tokens, cls = embedder(image, no_dropout=True)  # get_unconditional_conditioning forces ucg_rate = 0 (modules.py:185-194)
    cond = {"img_crossattn": tokens.contiguous(), "img_vector": cls.contiguous()}
    return cond, {k: torch.zeros_like(v) for k, v in cond.items()}


T23D_CFG_SCALE = 4.5  # the guidance scale of both text stages (shell_scripts/release/inference/t23d/stage{1,2}-t23d.sh)


@torch.no_grad()
def condition_on_caption(crossattn, vector):
    """The conditioning dicts of the t23d release from the two outputs of its caption embedder (``FrozenOpenCLIPEmbedder2``:
    the token states behind the text tower's last block, ``z["last"]`` [S,77,768], and the pooled, projected vector [S,768] -- computed by the caller, the CLIP text
    encoder is not part of this package): cond = {'caption_crossattn', 'caption_vector'}; the unconditional half of CFG is all
    zeros, as ``sgm`` builds it (``GeneralConditioner.forward`` with ``force_zero_embeddings``)."""
    if crossattn.dim() != 3 or vector.dim() != 2 or crossattn.shape[0] != vector.shape[0]:
        raise ValueError("caption_crossattn is [S, tokens, width] and caption_vector [S, width]")
    cond = {"caption_crossattn": crossattn.contiguous(), "caption_vector": vector.contiguous()}
    return cond, {k: torch.zeros_like(v) for k, v in cond.items()}


@torch.no_grad()
def stage2_caption_conditioning(cond, uc, fps_xyz):
    """Stage-2 conditioning dicts of the text cascade (stage2-t23d.sh: ``cond_key = caption``): the unconditional caption stays the
    zero one -- classifier-free guidance is REAL in the text stage 2, unlike the image one -- and both halves share the stage-1 cloud,
    which the denoiser's XYZPosEmbed sees as ``xyz / 0.45`` (``PCD_Scaler``, as in ``stage2_conditioning``)."""
    return stage2_conditioning(cond, uc, fps_xyz, zero_image_uc=True)


def _is_caption(cond):
    return "caption_crossattn" in cond


@torch.no_grad()
def stage2_conditioning(cond, uc, fps_xyz, zero_image_uc=False):
    """Stage-2 conditioning dicts from the stage-1 cloud, as the release's conditioner builds them
    (sgm/configs/stage2-i23d.yaml): the ``fps-xyz`` embedder is ``PCD_Scaler`` -- the denoiser's XYZPosEmbed sees
    ``xyz / 0.45`` (only the decoder gets the raw cloud).  Stage 2 runs with ``cond_key = 'img-xyz'``, so
    ``ucg_keys = ['img-xyz']`` matches no embedder input key ('img', 'fps-xyz') and ``get_unconditional_conditioning``
    returns uc == c (flow_matching_trainer.py:1039,1148-1155): classifier-free guidance is a no-op there.
    ``zero_image_uc=True`` is the non-reference variant that guides against the zero-image branch."""
    scaled = fps_xyz / PCD_SCALING_FACTOR
    cond2 = dict(cond)
    cond2["fps-xyz"] = scaled
    uc2 = dict(uc) if zero_image_uc else dict(cond)
    uc2["fps-xyz"] = scaled
    return cond2, uc2


def _stage2_and_decode(stage2, decoder, cond, uc, fps_xyz, cameras, cfg_scale, seed, num_steps, sampling_method, render_all_scale,
                       stage2_zero_image_uc, st2, ode_kwargs):
    """What follows stage 1 -- shared by ``cascade`` and ``from_point_cloud``, so the two cannot drift apart."""
    S, L = fps_xyz.shape[0], fps_xyz.shape[1]
    if _is_caption(cond):
        cond2, uc2 = stage2_caption_conditioning(cond, uc, fps_xyz)
    else:
        cond2, uc2 = stage2_conditioning(cond, uc, fps_xyz, zero_image_uc=stage2_zero_image_uc)
    latent = sample(stage2, cond2, uc2, (L, stage2.in_channels), S, cfg_scale, seed, num_steps, sampling_method,
                    stats=st2, **ode_kwargs)
    ret = decoder.decode(latent, fps_xyz)
    if cameras is not None:
        ret["renders"] = decoder.triplane_decode(ret, cameras, render_all_scale=render_all_scale)
    return ret


@torch.no_grad()
def cascade(stage1, stage2, decoder, cond, uc, cameras=None, cfg_scale=4.0, seed=42, num_steps=250,
            sampling_method="dopri5", render_all_scale=True, stage2_zero_image_uc=False, stats=None, **ode_kwargs):
    """Stage 1 -> stage 2 -> surfel decode (-> renders when ``cameras`` = {cam_view, cam_view_proj [B,V,4,4], cam_pos
    [B,V,3], tanfov} is given).  ``cond`` / ``uc``: {'img_crossattn' [S,1369,1024], 'img_vector' [S,1024]} (``condition_on_image``)
    or, with the text denoisers, {'caption_crossattn' [S,77,768], 'caption_vector' [S,768]} (``condition_on_caption``; the release
    runs both text stages at ``cfg_scale = T23D_CFG_SCALE``, and its stage 2 is guided against the zero caption)."""
    S = cond["caption_crossattn" if _is_caption(cond) else "img_crossattn"].shape[0]
    L = decoder.vit_decoder.pos_embed.shape[1]  # 768 latent tokens in the release (z_shape, flow_matching_trainer.py:1158)
    st1, st2 = ({}, {}) if stats is not None else (None, None)
    xyz = sample(stage1, cond, uc, (L, stage1.in_channels), S, cfg_scale, seed, num_steps, sampling_method, stats=st1,
                 **ode_kwargs)
    fps_xyz = (xyz * XYZ_STD).clip(-0.45, 0.45)
    ret = _stage2_and_decode(stage2, decoder, cond, uc, fps_xyz, cameras, cfg_scale, seed, num_steps, sampling_method,
                             render_all_scale, stage2_zero_image_uc, st2, ode_kwargs)
    if stats is not None:
        stats.update(stage1=st1, stage2=st2)
    return ret


@torch.no_grad()
def cloud_to_condition(points, num_points, lengths=None, outlier_neighbors=None, outlier_std_ratio=2.0):
    """Any cloud [S,N,3] -- a scan, mesh samples, a stage-1 output with points added or removed -- as the ``fps-xyz`` stage 2 and the
    decoder are built for: ``num_points`` farthest points from index 0 when N > num_points (``pytorch3d.ops.sample_farthest_points``
    in the reference, whence the key's name; the HIP kernel of ``pointcloud`` here), the cloud itself in its own order when
    N == num_points, clipped to +-0.45 either way (flow_matching_trainer.py:1079).  ``lengths`` [S]: the valid points of each padded
    cloud, every one at least ``num_points``.  ``outlier_neighbors`` = k: ``pointcloud.remove_statistical_outliers(points, lengths,
    k, outlier_std_ratio)`` runs first -- farthest point sampling picks stray points of a scan FIRST by construction -- and the
    length requirement applies to what the filter leaves; None (default) runs no filter."""
    if points.dim() != 3 or points.shape[-1] != 3:
        raise ValueError("points is an [S, N, 3] cloud")
    N = points.shape[1]
    if outlier_neighbors is not None and N >= num_points:
        from .pointcloud import remove_statistical_outliers
        points, lengths, _ = remove_statistical_outliers(points, lengths, outlier_neighbors, outlier_std_ratio)
    lens = [N] * points.shape[0] if lengths is None else [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
    if N < num_points or min(lens) < num_points:
        raise ValueError(f"a cloud of {min(N, min(lens))} points cannot condition a model of {num_points}: add points, the sampler only removes them")
    if N == num_points:
        return points.float().clip(-0.45, 0.45)
    from .pointcloud import sample_farthest_points
    return sample_farthest_points(points, lengths=lengths, K=num_points)[0].clip(-0.45, 0.45)


@torch.no_grad()
def from_point_cloud(stage2, decoder, cond, uc, points, cameras=None, cfg_scale=4.0, seed=42, num_steps=250,
                     sampling_method="dopri5", render_all_scale=True, stage2_zero_image_uc=False, stats=None, lengths=None,
                     outlier_neighbors=None, outlier_std_ratio=2.0, **ode_kwargs):
    """Stage 2 -> surfel decode (-> renders) on a cloud of the USER's: the reference's stage-2 entry, which reads the cloud from a PLY
    file (flow_matching_trainer.py:1079 text mode, :1110-1134 image mode, with its ``# ! edit`` lines stretching the cloud by hand) --
    the paper's 3D editing: keep the image or caption, change the shape.  ``points`` [S,N,3] with N >= the decoder's token count goes
    through ``cloud_to_condition`` (with its outlier filter when ``outlier_neighbors`` is given); everything after is exactly what
    ``cascade`` does behind its stage 1, for both conditionings.
    ``stats`` receives {'stage2': ...}."""
    S = cond["caption_crossattn" if _is_caption(cond) else "img_crossattn"].shape[0]
    L = decoder.vit_decoder.pos_embed.shape[1]
    if points.shape[0] != S:
        raise ValueError(f"{points.shape[0]} clouds for {S} conditionings")
    dev = next(stage2.parameters()).device
    fps_xyz = cloud_to_condition(points.to(dev), L, lengths, outlier_neighbors, outlier_std_ratio)
    st2 = {} if stats is not None else None
    ret = _stage2_and_decode(stage2, decoder, cond, uc, fps_xyz, cameras, cfg_scale, seed, num_steps, sampling_method,
                             render_all_scale, stage2_zero_image_uc, st2, ode_kwargs)
    if stats is not None:
        stats.update(stage2=st2)
    return ret


@torch.no_grad()
def from_mesh(stage2, decoder, cond, uc, vertices, faces, num_surface_samples=16384, mesh_seed=0, **kw):
    """``from_point_cloud`` for a user whose asset is a MESH: ``num_surface_samples`` area-weighted samples of its surface
    (``mesh.sample_points_from_mesh`` with ``mesh_seed``) are the [S,N,3] cloud, every other keyword is ``from_point_cloud``'s.
    ``vertices`` [V,3] and ``faces`` [F,3] for one conditioning; lists of S of each for S > 1 (one sampling call per mesh: batches of
    meshes are not built).  The default of 16 384 samples keeps the farthest point sampling behind it on its register-resident path."""
    from .mesh import sample_points_from_mesh
    dev = next(stage2.parameters()).device
    if isinstance(vertices, torch.Tensor):
        vertices, faces = [vertices], [faces]
    if len(vertices) != len(faces):
        raise ValueError(f"{len(vertices)} vertex arrays for {len(faces)} face arrays")
    cloud = torch.stack([sample_points_from_mesh(v.to(dev), f.to(dev), num_surface_samples, seed=mesh_seed) for v, f in zip(vertices, faces)])
    return from_point_cloud(stage2, decoder, cond, uc, cloud, **kw)
