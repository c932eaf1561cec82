"""GPU tests of the hand-offs built on the mesh sampler: ``cascade.from_mesh`` and ``io_formats.export_fps_points_from_mesh``."""
import numpy as np
import pytest
import torch

from tests import _mesh_ops_ref as ref

pytestmark = pytest.mark.gpu


def test_from_mesh_equals_from_point_cloud_on_its_samples(gpu_device):
    """stage 2 -> decode from a mesh on the small golden models: exactly ``from_point_cloud`` on ``sample_points_from_mesh`` with the same
    seeds, for one mesh and for a list of two"""
    from gaussiananything_amd import cascade, mesh, synthetic
    from gaussiananything_amd.decode import SurfelDecoder
    from gaussiananything_amd.dit import DiT_I23D_PCD_PixelArt_noclip_clay_stage2
    z2 = torch.load(synthetic.fixture_path("dit_ref_stage2.pt"))
    m2 = DiT_I23D_PCD_PixelArt_noclip_clay_stage2(**dict(z2["kwargs"], use_pe_cond=True))
    m2.load_state_dict(z2["state_dict"])
    zd = torch.load(synthetic.fixture_path("decode_ref.pt"))
    cfg = zd["config"]
    dec = SurfelDecoder(embed_dim=cfg["D"], depth=cfg["depth"], num_heads=cfg["heads"], tokens=cfg["tokens"],
                        ldm_z_channels=cfg["z_channels"])
    dec.load_state_dict(zd["state_dict"])
    m2.to(gpu_device)
    dec.to(gpu_device)
    ctx = torch.load(synthetic.fixture_path("dit_ref_stage1.pt"))["context"]
    cond = {k: v[:1].to(gpu_device) for k, v in ctx.items()}
    uc = {k: torch.zeros_like(v) for k, v in cond.items()}
    v, f = ref.icosphere(2)
    tv, tf = torch.from_numpy(v * np.float32(0.5)).to(gpu_device), torch.from_numpy(f).to(gpu_device)   # past the +-0.45 box: the clip acts
    kw = dict(num_steps=4, sampling_method="euler", seed=3)
    out = cascade.from_mesh(m2, dec, cond, uc, tv, tf, num_surface_samples=3000, mesh_seed=21, **kw)
    cloud = mesh.sample_points_from_mesh(tv, tf, 3000, seed=21)
    want = cascade.from_point_cloud(m2, dec, cond, uc, cloud[None], **kw)
    assert torch.equal(out["query_pcd_xyz"], want["query_pcd_xyz"])
    assert torch.equal(out["gaussians_upsampled_3"], want["gaussians_upsampled_3"])
    assert float(out["query_pcd_xyz"].abs().max()) == pytest.approx(0.45)
    other = cascade.from_mesh(m2, dec, cond, uc, tv, tf, num_surface_samples=3000, mesh_seed=22, **kw)
    assert not torch.equal(other["query_pcd_xyz"], out["query_pcd_xyz"])
    # S = 2: a list of meshes, one sampling call each
    cond2 = {k: torch.cat([t, t]) for k, t in cond.items()}
    uc2 = {k: torch.zeros_like(t) for k, t in cond2.items()}
    v1, f1 = ref.icosphere(1)
    tv1, tf1 = torch.from_numpy(v1 * np.float32(0.3)).to(gpu_device), torch.from_numpy(f1).to(gpu_device)
    out2 = cascade.from_mesh(m2, dec, cond2, uc2, [tv, tv1], [tf, tf1], num_surface_samples=3000, mesh_seed=21, **kw)
    clouds = torch.stack([cloud, mesh.sample_points_from_mesh(tv1, tf1, 3000, seed=21)])
    want2 = cascade.from_point_cloud(m2, dec, cond2, uc2, clouds, **kw)
    assert torch.equal(out2["gaussians_upsampled_3"], want2["gaussians_upsampled_3"])
    with pytest.raises(ValueError):
        cascade.from_mesh(m2, dec, cond2, uc2, tv, tf, num_surface_samples=3000, **kw)          # one mesh for two conditionings


def test_export_fps_points_from_mesh(gpu_device, tmp_path):
    from gaussiananything_amd import io_formats, mesh
    from gaussiananything_amd.pointcloud import sample_farthest_points
    v, f = ref.icosphere(2)
    path = str(tmp_path / "fps-512.ply")
    pts = io_formats.export_fps_points_from_mesh(v, f, path, K=512, num_samples=5000, seed=6)
    back = io_formats.load_points_ply(path)
    assert pts.shape == (512, 3) and pts.dtype == np.float32 and np.array_equal(np.asarray(back, np.float32), pts)
    samples = mesh.sample_points_from_mesh(torch.from_numpy(v).to(gpu_device), torch.from_numpy(f).to(gpu_device), 5000, seed=6)
    assert np.array_equal(sample_farthest_points(samples[None], K=512)[0][0].cpu().numpy(), pts)
    assert np.array_equal(samples.cpu().numpy(), ref.sample(v, f, 5000, 6)["points"])
    assert np.abs(np.linalg.norm(pts, axis=1) - 1).max() < 0.02        # on the icosphere's surface, just inside the unit sphere
