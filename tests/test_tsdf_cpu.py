"""CPU tests of the TSDF / mesh-export oracle and host code: the derived marching-cubes table,
the restatement of Open3D's integration on analytic frames, the post-processing and the OBJ writer; the device copy of the table,
the vertex set stated a second way, the comparisons of the GPU tests on planted defects, and what the C-ABI turns away.  Open3D is absent:
parity with the reference's mesh is UNPINNED (oracle/tsdf.py header); what is checked here are the properties any correct
fusion + extraction has."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import tsdf as otsdf
from tests import _tsdf_util as tu
from tests._tsdf_util import sphere_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _edge_counts(tris):
    e = np.concatenate([tris[:, [0, 1]], tris[:, [1, 2]], tris[:, [2, 0]]])
    und = np.sort(e, axis=1)
    _, cnt = np.unique(und, axis=0, return_counts=True)
    _, dcnt = np.unique(e, axis=0, return_counts=True)
    return cnt, dcnt


def _sphere_volume(res_units=4, radius=0.31, voxel=0.02, seed=0):
    vol = otsdf.Volume((res_units,) * 3, (-(res_units // 2),) * 3, voxel, 0.1)
    R = res_units * 16
    idx = (np.arange(R) + 0.5) * voxel + vol.unit0[0] * vol.unit_length
    x, y, z = np.meshgrid(idx, idx, idx, indexing="ij")
    rng = np.random.default_rng(seed)
    sdf = np.sqrt((x - 0.013) ** 2 + (y + 0.021) ** 2 + (z - 0.007) ** 2) - radius
    vol.tsdf[:] = np.clip(sdf / 0.1, -1, 1).astype(np.float32)
    vol.weight[:] = 1
    vol.color[:] = rng.uniform(0, 255, vol.color.shape).astype(np.float32)
    vol.allocated[:] = True
    return vol


def test_every_case_of_the_table_is_a_closed_cut_of_the_cube():
    t = otsdf.mc_table()
    assert t["max_triangles"] == 5 and len(t["triangles"]) == 256
    corners = t["edge_corners"]
    for case, row in enumerate(t["triangles"]):
        edges = [e for e in row if e >= 0]
        cut = {e for e in range(12) if ((case >> corners[e][0]) ^ (case >> corners[e][1])) & 1}
        assert set(edges) == cut, case            # every intersected edge is used, no other
        assert len(edges) % 3 == 0


def test_mesh_of_a_sphere_is_closed_oriented_and_has_the_sphere_s_volume():
    vol = _sphere_volume()
    v, c, t = otsdf.extract_mesh(vol)
    assert len(v) > 500 and len(t) > 1000 and t.min() == 0 and t.max() == len(v) - 1
    cnt, dcnt = _edge_counts(t)
    assert (cnt == 2).all() and (dcnt == 1).all()          # closed, consistently oriented
    E = len(cnt)
    assert len(v) - E + len(t) == 2                          # one sphere
    p = v.astype(np.float64)
    vol6 = np.einsum("ij,ij->i", p[t[:, 0]], np.cross(p[t[:, 1]], p[t[:, 2]])).sum() / 6.0
    assert abs(vol6 - 4 / 3 * np.pi * 0.31 ** 3) / (4 / 3 * np.pi * 0.31 ** 3) < 0.01     # outward normals: positive volume
    r = np.linalg.norm(p - np.array([0.013, -0.021, 0.007]), axis=1)
    assert np.abs(r - 0.31).max() < 0.02 * 0.25               # vertices on the zero level set (a quarter voxel)
    assert c.min() >= 0 and c.max() <= 1


def test_cubes_with_an_unobserved_corner_give_no_triangles():
    vol = _sphere_volume()
    vol.weight[:32] = 0                                        # half the volume never observed
    v, c, t = otsdf.extract_mesh(vol)
    assert len(t) > 0 and v[:, 0].min() > (32 + 0.5) * 0.02 + vol.unit0[0] * vol.unit_length - 1e-6
    cnt, _ = _edge_counts(t)
    assert (cnt <= 2).all() and (cnt == 1).any()               # an open boundary where the observed part ends


def test_integration_of_analytic_sphere_frames():
    fr = sphere_frames(3, 64)
    vol = otsdf.Volume((4, 4, 4), (-2, -2, -2), 0.0125, 0.075)
    for f in fr:
        touched = otsdf.integrate(vol, f["rgb"], f["depth"], f["alpha"], 0.08, f["depth_trunc"], f["intr"], f["ext"])
        assert touched.any()
    assert vol.weight.max() == 3 and vol.allocated.any()
    R = 64
    idx = (np.arange(R) + 0.5) * 0.0125 - 2 * vol.unit_length
    x, y, z = np.meshgrid(idx, idx, idx, indexing="ij")
    true = np.sqrt((x - 0.02) ** 2 + (y + 0.01) ** 2 + (z - 0.03) ** 2) - 0.3
    seen3 = (vol.weight == 3) & (np.abs(true) < 0.03)
    assert seen3.sum() > 1000
    # (the projective distance along the ray exceeds the true distance by the cosine of the incidence angle, and the three
    # cameras see the band around the silhouettes at grazing angles: loose bars on the volume, tight ones on the mesh)
    err = vol.tsdf[seen3] * 0.075 - true[seen3]
    assert np.abs(err).mean() < 0.015 and (np.sign(vol.tsdf[seen3]) == np.sign(true[seen3])).mean() > 0.93
    v, c, t = otsdf.extract_mesh(vol)
    r = np.linalg.norm(v.astype(np.float64) - np.array([0.02, -0.01, 0.03]), axis=1)
    assert len(t) > 1000 and np.abs(r - 0.3).mean() < 0.004 and np.abs(r - 0.3).max() < 0.02


def test_post_process_keeps_large_clusters_only_and_obj_writer(tmp_path):
    from gaussiananything_amd import mesh
    vol = _sphere_volume()
    v, c, t = otsdf.extract_mesh(vol)
    # a floater of four triangles far away
    fv = np.array([[2, 2, 2], [2.1, 2, 2], [2, 2.1, 2], [2, 2, 2.1]], np.float32)
    ft = np.array([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]], np.int32) + len(v)
    v2, c2, t2 = np.concatenate([v, fv]), np.concatenate([c, np.zeros((4, 3), np.float32)]), np.concatenate([t, ft])
    for fn in (mesh.post_process_mesh, otsdf.post_process_mesh):
        pv, pc, pt = fn(v2, c2, t2)
        assert len(pv) == len(v) and len(pt) == len(t) and np.array_equal(pt, t) and np.array_equal(pv, v)
    path = os.path.join(tmp_path, "a", "0-mesh_raw.obj")
    mesh.write_obj(path, v, c, t)
    lines = open(path).read().splitlines()
    assert sum(l.startswith("v ") for l in lines) == len(v) and sum(l.startswith("f ") for l in lines) == len(t)
    assert np.allclose(mesh.rotation_matrix_x(-90) @ np.array([0, 1, 0]), [0, 0, -1]) and np.allclose(
        mesh.rotation_matrix_y(np.pi) @ np.array([1, 0, 0]), [-1, 0, 0], atol=1e-12)


def test_camera_conversion_and_post_processing_against_the_reference_s_own_functions():
    """tests/golden/mesh_cam_ref.npz: produced by running /root/reference/utils/mesh_util.py (to_cam_open3d_compat,
    post_process_mesh) itself, see tests/golden/make_mesh_golden.py."""
    import torch
    from gaussiananything_amd import cameras, mesh, synthetic
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "mesh_cam_ref.npz"))
    cams = synthetic.eval_cameras(8)
    for i in range(8):
        c = {"cam_view": cams["cam_view"][i], "cam_pos": cams["cam_pos"][i], "tanfov": cams["tanfov"]}
        intr, ext = mesh.to_cam_open3d_compat(c, 512)
        assert intr == tuple(z["intrinsics"][i][:4]), (intr, z["intrinsics"][i])
        assert np.array_equal(ext, z["extrinsics"][i])
    # ... and the branch that takes the reference's projection matrix
    fov = cameras.focal2fov(float(cams["poses"][0][16]), 1)
    pm = cameras.getProjectionMatrix(0.01, 100.0, fov, fov).transpose(0, 1)
    intr2, ext2 = mesh.to_cam_open3d_compat({"cam_view": cams["cam_view"][0], "projection_matrix": pm}, 512)
    assert intr2 == tuple(z["intrinsics"][0][:4]) and np.array_equal(ext2, z["extrinsics"][0])
    pv, pc, pt = mesh.post_process_mesh(torch.from_numpy(z["pp_vertices"]), torch.zeros(len(z["pp_vertices"]), 3),
                                        torch.from_numpy(z["pp_triangles"]))
    assert np.array_equal(pt.numpy(), z["pp_out_triangles"]) and np.array_equal(pv.numpy(), z["pp_out_vertices"])
    ov, oc, ot = otsdf.post_process_mesh(z["pp_vertices"], np.zeros((len(z["pp_vertices"]), 3), np.float32), z["pp_triangles"])
    assert np.array_equal(ot, z["pp_out_triangles"]) and np.array_equal(ov, z["pp_out_vertices"])


def test_random_fields_give_closed_meshes_through_every_ambiguous_case():
    """White-noise signs put every one of the 256 cube cases, including all ambiguous faces, next to every other: the derived
    table must still give a surface without cracks -- every mesh edge that is not on the volume's outer faces is shared by
    exactly two triangles, with opposite directions."""
    rng = np.random.default_rng(7)
    vol = otsdf.Volume((2, 2, 2), (0, 0, 0), 1.0, 1.0)
    vol.tsdf[:] = rng.uniform(-1, 1, vol.tsdf.shape).astype(np.float32)
    vol.weight[:] = 1
    vol.allocated[:] = True
    v, c, t = otsdf.extract_mesh(vol)
    cases = set()
    ins = vol.tsdf < 0
    R = 32
    cs = np.zeros((R - 1,) * 3, np.int32)
    for i in range(8):
        o = (i & 1, (i >> 1) & 1, (i >> 2) & 1)
        cs |= ins[o[0]:R - 1 + o[0], o[1]:R - 1 + o[1], o[2]:R - 1 + o[2]].astype(np.int32) << i
    assert len(np.unique(cs)) >= 250                                  # (practically all of the 256 cases occur)
    assert len(t) > 50000
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    und = np.sort(e, axis=1)
    uniq, inv, cnt = np.unique(und, axis=0, return_inverse=True, return_counts=True)
    lo, hi = 0.5, R - 0.5                                             # voxel centres span [0.5, 31.5]
    on_face = lambda p: (np.isclose(p, lo) | np.isclose(p, hi)).any(axis=1)
    boundary_edge = on_face(v[uniq[:, 0]]) & on_face(v[uniq[:, 1]])
    assert (cnt[~boundary_edge] == 2).all() and (cnt <= 2).all()
    # orientation: an interior edge is traversed once in each direction
    direction = np.where(e[:, 0] < e[:, 1], 1, -1)
    balance = np.bincount(inv.reshape(-1), weights=direction, minlength=len(uniq))
    assert (balance[~boundary_edge] == 0).all()


# ---- the table, the vertex set, the mesh invariants, the comparisons and the host validation (tests/_tsdf_util.py) -----------------


def _braced_ints(text, name):
    body = text[text.index(name):]
    body = body[body.index("=") + 1:body.index(";")]
    return [int(x) for x in re.findall(r"-?\d+", body)]


def test_device_table_json_table_and_generator_agree_row_by_row():
    """csrc/mc_table.h is a second, generated copy of oracle/mc_table.json: both equal what tools/gen_mc_table.py derives"""
    import importlib.util
    text = open(os.path.join(ROOT, "gaussiananything_amd", "csrc", "mc_table.h")).read()
    js = otsdf.mc_table()
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(ROOT, "tools", "gen_mc_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)                                    # (main() runs under __main__ only: nothing is written)
    width = 3 * js["max_triangles"]
    assert f"kMcMaxTriangles = {js['max_triangles']};" in text and f"kMcTriangles[256][{width}]" in text
    tri = _braced_ints(text, "kMcTriangles[256]")
    cnt = _braced_ints(text, "kMcTriangleCount[256]")
    ec = _braced_ints(text, "kMcEdgeCorners[12][2]")
    assert len(tri) == 256 * width and len(cnt) == 256 and len(ec) == 24
    assert [ec[2 * e:2 * e + 2] for e in range(12)] == js["edge_corners"] == [list(gen.EDGE_CORNERS[e]) for e in range(12)]
    for c in range(256):
        row = tri[c * width:(c + 1) * width]
        want = [e for t in gen.case_triangles(c) for e in t]
        assert row == js["triangles"][c], c
        assert row == want + [-1] * (width - len(want)), c
        assert cnt[c] == len(want) // 3, c


def test_block_is_the_storage_address_of_the_header_voxel_by_voxel():
    units = (2, 3, 2)
    X, Y, Z = (16 * u for u in units)
    arr = np.arange(X * Y * Z, dtype=np.int64).reshape(X, Y, Z)
    got = tu.block(arr, units)
    want = np.full(X * Y * Z, -1, np.int64)
    for x in range(X):
        for y in range(Y):
            for z in range(Z):
                a = (((x >> 4) * units[1] + (y >> 4)) * units[2] + (z >> 4)) * 4096 + (z & 15) * 256 + (x & 15) * 16 + (y & 15)
                want[a] = arr[x, y, z]
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", tu.MC_NAMES)
def test_oracle_vertices_are_the_independently_stated_vertex_set(name):
    vol = tu.mc_volume(name)
    v, c, t = tu.mc_oracle_mesh(name)
    mine = tu.independent_vertices(vol)
    assert mine.shape == v.shape, (mine.shape, v.shape)
    assert np.array_equal(tu.sort_rows(v), mine)                    # bit for bit


@pytest.mark.parametrize("name", tu.MC_NAMES)
def test_oracle_meshes_of_the_named_volumes_keep_the_mesh_invariants(name):
    vol = tu.mc_volume(name)
    v, c, t = tu.mc_oracle_mesh(name)
    tu.check_mesh_invariants(t, len(v))
    cases = tu.cube_cases(vol)
    n_cases = len(np.unique(cases[cases >= 0]))
    print(f"{name}: units {int(np.prod(vol.units))}, vertices {len(v)}, triangles {len(t)}, distinct cube cases {n_cases}")
    assert len(t) == int(np.array([len([e for e in r if e >= 0]) // 3 for r in otsdf.mc_table()["triangles"]])[cases[(cases > 0) & (cases < 255)]].sum())
    if name == "M1":
        assert n_cases >= 250
    if name == "M5a":
        assert (len(v), len(t)) == (6, 8)
    if name == "M5d":
        assert (len(v), len(t)) == (0, 0)
    if name in ("M5b", "M5c"):                                        # the first and the last voxel of the box: one cube cuts the corner off
        assert (len(v), len(t)) == (3, 1)
    if name == "M3":                                                  # cubes cross from unit 1023 into unit 1024
        z0 = (64 - 60) * vol.unit_length
        assert ((v[:, 2] > z0 - vol.voxel_length) & (v[:, 2] < z0)).any()


def _expect_failure(fn, *args):
    with pytest.raises(AssertionError):
        fn(*args)


def test_the_comparisons_fail_on_each_planted_defect(monkeypatch):
    """The oracle's own output with one defect at a time, as a subtly wrong kernel would give it (never a broken kernel on the
    device: a wrong base index writes out of bounds)."""
    # intact: everything passes
    vol2, mesh2 = tu.mc_volume("M2"), tu.mc_oracle_mesh("M2")
    tu.check_mesh(tuple(a.copy() for a in mesh2), mesh2)
    # (a) one table row's diagonal flipped, for a case that occurs: same vertices, same counts, other index list
    cases = tu.cube_cases(vol2)
    assert (cases == 3).any()
    tab = otsdf.mc_table()
    flipped = dict(tab, triangles=[list(r) for r in tab["triangles"]])
    assert flipped["triangles"][3][:6] == [4, 8, 9, 4, 9, 5]
    flipped["triangles"][3][:6] = [4, 8, 5, 8, 9, 5]
    monkeypatch.setattr(otsdf, "_TABLE", flipped)
    bad = otsdf.extract_mesh(vol2)
    monkeypatch.setattr(otsdf, "_TABLE", tab)
    assert bad[2].shape == mesh2[2].shape and np.array_equal(bad[0], mesh2[0])
    _expect_failure(tu.check_mesh, bad, mesh2)
    # (b) a lost carry of the unit scan: the triangles of the units past linear index 1023 shifted by a constant
    vol3, (v3, c3, t3) = tu.mc_volume("M3"), tu.mc_oracle_mesh("M3")
    count = np.array([len([e for e in r if e >= 0]) // 3 for r in tab["triangles"]])
    cs = tu.cube_cases(vol3)
    below = cs[:, :, :64 * 16]                                          # cubes anchored in the units up to linear index 1023
    first = int(count[below[below > 0]].sum())
    # (only units (2,2,64) and (2,2,119) lie past 1023, and they come last: `first` triangles are anchored at z < 64 * 16)
    assert 0 < first < len(t3) and t3[first:].min() > t3[:first].min()
    shifted = t3.copy()
    shifted[first:] -= 7
    _expect_failure(tu.check_mesh, (v3, c3, shifted), (v3, c3, t3))
    _expect_failure(tu.check_mesh_invariants, shifted, len(v3))        # (what the end-to-end test looks at: the last vertices lose their triangles)
    # (c) one vertex moved by 2e-6, one colour likewise
    v, c, t = (a.copy() for a in mesh2)
    v[len(v) // 2, 1] += np.float32(2e-6)
    assert abs(float(v[len(v) // 2, 1]) - float(mesh2[0][len(v) // 2, 1])) > 1e-6
    _expect_failure(tu.check_mesh, (v, c, t), mesh2)
    v, c, t = (a.copy() for a in mesh2)
    c[3, 0] += np.float32(2e-6)
    _expect_failure(tu.check_mesh, (v, c, t), mesh2)
    # ... a slot left unwritten, a count off by one
    v, c, t = (a.copy() for a in mesh2)
    t[-1] = -1
    _expect_failure(tu.check_mesh, (v, c, t), mesh2)
    v[0, 0] = np.nan
    _expect_failure(tu.check_mesh, (v, c, mesh2[2]), mesh2)
    _expect_failure(tu.check_mesh, (mesh2[0][:-1], mesh2[1][:-1], mesh2[2]), mesh2)
    # (d) one opened unit missing, (e) one voxel's weight off by one, a tsdf or a colour beyond its bar: a fused volume
    fr = sphere_frames(2, 48)
    vol = otsdf.Volume((3, 4, 5), (-1, -2, -3), 0.0125, 0.075)
    for f in fr:
        touched = otsdf.integrate(vol, f["rgb"], f["depth"], f["alpha"], 0.08, f["depth_trunc"], f["intr"], f["ext"])
    want = (vol.tsdf, vol.weight, vol.color, vol.allocated)
    tu.check_volume(tuple(a.copy() for a in want), want)
    tu.check_units(touched.copy(), touched)
    missing = touched.copy()
    missing[tuple(np.argwhere(touched)[0])] = False
    _expect_failure(tu.check_units, missing, touched)
    alloc = vol.allocated.copy()
    alloc[tuple(np.argwhere(alloc)[-1])] = False
    _expect_failure(tu.check_volume, (vol.tsdf, vol.weight, vol.color, alloc), want)
    at = tuple(np.argwhere(vol.weight == 2)[0])
    w = vol.weight.copy()
    w[at] += 1
    _expect_failure(tu.check_volume, (vol.tsdf, w, vol.color, vol.allocated), want)
    t_ = vol.tsdf.copy()
    t_[at] += np.float32(2e-6)
    _expect_failure(tu.check_volume, (t_, vol.weight, vol.color, vol.allocated), want)
    c_ = vol.color.copy()
    c_[(1,) + at] += np.float32(3e-4)
    _expect_failure(tu.check_volume, (vol.tsdf, vol.weight, c_, vol.allocated), want)
    t_ = vol.tsdf.copy()
    t_[at] = np.nan
    _expect_failure(tu.check_volume, (t_, vol.weight, vol.color, vol.allocated), want)


def test_analytic_frames_hit_the_sphere_and_the_plane_where_they_are():
    fr = tu.analytic_frames([(0.9, 0.3, 0.8)], (0.1, 0.0, -0.1), 48, 80, 70.0, 62.0, 43.0, 20.25, sphere=((0.1, 0.0, -0.1), 0.15),
                            plane=((0.0, 0.0, -0.3), (0.0, 0.0, 1.0)))[0]
    pose = np.linalg.inv(fr["ext"])
    v, u = np.meshgrid(np.arange(48.0), np.arange(80.0), indexing="ij")
    z = fr["depth"].astype(np.float64)
    pc = np.stack([(u - 43.0) / 70.0 * z, (v - 20.25) / 62.0 * z, z, np.ones_like(z)], -1)
    pw = (pc @ pose.T)[..., :3]
    hit = z > 0
    on_sphere = np.abs(np.linalg.norm(pw - np.array([0.1, 0.0, -0.1]), axis=-1) - 0.15) < 1e-6
    on_plane = np.abs(pw[..., 2] + 0.3) < 1e-6
    assert hit.sum() > 1000 and (on_sphere & hit).sum() > 100 and (on_plane & hit).sum() > 100 and (on_sphere | on_plane)[hit].all()
    assert np.array_equal(fr["alpha"] > 0, hit) and fr["rgb"].shape == (3, 48, 80) and fr["rgb"].min() >= 0 and fr["rgb"].max() <= 1
    assert np.abs(pose[:3, 3] - np.array([0.9, 0.3, 0.8])).max() < 1e-12 and np.abs(fr["ext"][:3, :3] @ fr["ext"][:3, :3].T - np.eye(3)).max() < 1e-12


def test_tsdf_c_abi_rejects_before_any_launch():
    """Fake, non-NULL device addresses: a call that got past validation would fault; every one here must be turned away."""
    from gaussiananything_amd import _lib as _l
    L = _l.lib()
    P = 0x1000
    NULL_ARG, BAD_SHAPE, WORKSPACE = -1, -2, -3
    nan = float("nan")

    def volume(**kw):
        v = dict(units=(2, 3, 2), unit0=(-1, 0, 0), voxel_length=0.0125, sdf_trunc=0.075, tsdf=P, weight=P, color=P, touched=P, allocated=P)
        v.update(kw)
        return _l.GaTsdfVolume((ctypes.c_int32 * 3)(*v["units"]), (ctypes.c_int32 * 3)(*v["unit0"]), v["voxel_length"], v["sdf_trunc"],
                               v["tsdf"], v["weight"], v["color"], v["touched"], v["allocated"])

    def frame(**kw):
        f = dict(height=8, width=8, rgb=P, depth=P, alpha=None, alpha_thres=0.08, depth_trunc=3.0, fx=10.0, fy=10.0, cx=3.5, cy=3.5, stride=4)
        f.update(kw)
        eye = (ctypes.c_double * 16)(*np.eye(4).reshape(-1).tolist())
        return _l.GaTsdfFrame(f["height"], f["width"], f["rgb"], f["depth"], f["alpha"], f["alpha_thres"], f["depth_trunc"], f["fx"], f["fy"],
                              f["cx"], f["cy"], eye, eye, f["stride"])

    bad_volumes = [dict(units=(0, 3, 2)), dict(units=(2, -1, 2)), dict(units=(2, 3, 0)), dict(units=(257, 256, 256)),
                   dict(voxel_length=0.0), dict(voxel_length=-0.0125), dict(voxel_length=nan), dict(sdf_trunc=0.0), dict(sdf_trunc=-1.0),
                   dict(sdf_trunc=nan)]
    need = L.ga_tsdf_mesh_scratch_bytes(ctypes.byref(volume()))
    # 6 bytes per voxel and 16 per unit, each of the five arrays padded to 256 bytes
    nvox, pad = 12 * 4096, lambda n: -(-n // 256) * 256
    assert need == 2 * pad(nvox) + pad(4 * nvox) + 2 * pad(8 * 12)
    assert L.ga_tsdf_mesh_scratch_bytes(None) == 0
    # ga_tsdf_integrate
    assert L.ga_tsdf_integrate(None, ctypes.byref(frame()), None) == NULL_ARG
    assert L.ga_tsdf_integrate(ctypes.byref(volume()), None, None) == NULL_ARG
    for kw in bad_volumes:
        assert L.ga_tsdf_integrate(ctypes.byref(volume(**kw)), ctypes.byref(frame()), None) == BAD_SHAPE, kw
        assert L.ga_tsdf_mesh_scratch_bytes(ctypes.byref(volume(**kw))) == 0, kw
        assert L.ga_tsdf_mesh_count(ctypes.byref(volume(**kw)), P, need, P, None) == BAD_SHAPE, kw
        assert L.ga_tsdf_mesh_emit(ctypes.byref(volume(**kw)), P, need, 3, 1, P, P, P, None) == BAD_SHAPE, kw
    for name in ("tsdf", "weight", "color", "touched", "allocated"):
        assert L.ga_tsdf_integrate(ctypes.byref(volume(**{name: None})), ctypes.byref(frame()), None) == NULL_ARG, name
    for name in ("rgb", "depth"):
        assert L.ga_tsdf_integrate(ctypes.byref(volume()), ctypes.byref(frame(**{name: None})), None) == NULL_ARG, name
    for kw in (dict(height=0), dict(height=-8), dict(width=0), dict(width=-1), dict(stride=0), dict(stride=-4), dict(fx=0.0), dict(fx=-10.0),
               dict(fx=nan), dict(fy=0.0), dict(fy=-10.0), dict(fy=nan)):
        assert L.ga_tsdf_integrate(ctypes.byref(volume()), ctypes.byref(frame(**kw)), None) == BAD_SHAPE, kw
    # ga_tsdf_mesh_count
    assert L.ga_tsdf_mesh_count(None, P, need, P, None) == NULL_ARG
    assert L.ga_tsdf_mesh_count(ctypes.byref(volume()), None, need, P, None) == NULL_ARG
    assert L.ga_tsdf_mesh_count(ctypes.byref(volume()), P, need, None, None) == NULL_ARG
    for name in ("tsdf", "weight", "color", "allocated"):
        assert L.ga_tsdf_mesh_count(ctypes.byref(volume(**{name: None})), P, need, P, None) == NULL_ARG, name
    assert L.ga_tsdf_mesh_count(ctypes.byref(volume()), P, need - 1, P, None) == WORKSPACE
    # ga_tsdf_mesh_emit
    emit = lambda vol, scratch=P, nbytes=need, nv=3, nt=1, v=P, c=P, t=P: L.ga_tsdf_mesh_emit(vol, scratch, nbytes, nv, nt, v, c, t, None)  # noqa: E731
    assert emit(None) == NULL_ARG
    assert emit(ctypes.byref(volume()), scratch=None) == NULL_ARG
    for name in ("tsdf", "weight", "color", "allocated"):               # (the volume ga_tsdf_mesh_count was given: its kernels read tsdf and colour)
        assert emit(ctypes.byref(volume(**{name: None}))) == NULL_ARG, name
        assert emit(ctypes.byref(volume(**{name: None})), nv=0, v=None, c=None) == NULL_ARG, name
    third = 0x7FFFFFFF // 3
    for kw in (dict(nv=-1), dict(nt=-1), dict(nv=third + 1), dict(nt=third + 1), dict(nv=1 << 40)):
        assert emit(ctypes.byref(volume()), **kw) == BAD_SHAPE, kw
    for kw in (dict(v=None), dict(c=None), dict(t=None), dict(nt=0, v=None), dict(nv=0, t=None)):
        assert emit(ctypes.byref(volume()), **kw) == NULL_ARG, kw
    assert emit(ctypes.byref(volume()), nbytes=need - 1) == WORKSPACE
    assert emit(ctypes.byref(volume()), nv=third, nt=third, nbytes=need - 1) == WORKSPACE     # (the largest counts are accepted as counts)
    # ga_mesh_cluster_labels
    C = L.ga_mesh_cluster_labels
    assert C(P, P, 4, None, 10, None) == NULL_ARG
    assert C(None, P, 4, P, 10, None) == NULL_ARG and C(P, None, 4, P, 10, None) == NULL_ARG and C(None, None, 1, P, 10, None) == NULL_ARG
    assert C(P, P, 4, P, 0, None) == BAD_SHAPE and C(P, P, 4, P, -3, None) == BAD_SHAPE and C(P, P, 4, P, 0x80000000, None) == BAD_SHAPE
    assert C(P, P, -1, P, 10, None) == BAD_SHAPE and C(None, None, -1, P, 10, None) == BAD_SHAPE
