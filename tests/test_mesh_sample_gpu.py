"""GPU tests of ``ga_mesh_sample`` (include/ga_mesh.h, csrc/mesh_ops.hip).

The raw C-ABI call is compared with the numpy restatement (tests/_mesh_ops_ref.py) for EQUALITY, bit for bit: faces, barycentric
weights, points, normals and colours.  Every raw call poisons its outputs first and checks guard words behind each of them and behind
the workspace.  The face counts of the edge cases come from ``ga_mesh_sample_plan``, so the tests follow the kernel's constants."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _mesh_ops_ref as ref

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 64            # int32 words behind every buffer
GUARD_WORD = 0x5A5A5A5A
POISON = -77          # as a float: a NaN pattern no arithmetic here produces


def _guarded(n_words, device):
    t = torch.full((n_words + GUARD,), GUARD_WORD, dtype=torch.int32, device=device)
    t[:n_words] = POISON
    return t


def _take(buf, n, shape, dtype=torch.float32):
    """the first n words of a guarded buffer as numpy; the guards intact, every word written"""
    assert bool((buf[n:] == GUARD_WORD).all()), "guard words overwritten"
    assert not bool((buf[:n] == POISON).any()), "an output element was not written"
    return buf[:n].view(dtype).reshape(shape).cpu().numpy()


def _same(got, want, what):
    a, b = np.ascontiguousarray(got, F32).view(np.uint32), np.ascontiguousarray(want, F32).view(np.uint32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = a != b
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ in bits, first at {np.argwhere(bad)[0].tolist()}: " \
                          f"got {np.asarray(got, F32)[bad][0]!r}, want {np.asarray(want, F32)[bad][0]!r}"


def _seed_words(seed):
    """the two 32-bit words (low, high) of a 64-bit seed as an int32 tensor"""
    return torch.from_numpy(np.asarray([seed & 0xFFFFFFFF, seed >> 32], np.uint32).view(np.int32).copy())


def plan(num_faces, num_samples=1):
    from gaussiananything_amd import mesh
    return mesh.mesh_sample_plan(num_faces, num_samples)


class Raw:
    """one bound ``ga_mesh_sample`` call: device copies of the mesh, guarded outputs and workspace"""

    def __init__(self, device, vertices, faces, S, seed=0, colors=None, normals=True, device_seed=False):
        from gaussiananything_amd import _lib
        self._lib, self.L, self.S = _lib, _lib.lib(), S
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)   # noqa: E731
        self.v, self.f = dev(np.asarray(vertices, F32)), dev(np.asarray(faces, np.int32))
        self.c = dev(np.asarray(colors, F32)) if colors is not None else None
        self.words = _seed_words(seed).to(device) if device_seed else None
        self.points, self.bary, self.face = _guarded(3 * S, device), _guarded(3 * S, device), _guarded(S, device)
        self.normals = _guarded(3 * S, device) if normals else None
        self.colors = _guarded(3 * S, device) if colors is not None else None
        self.ws_bytes = plan(self.f.shape[0], S)["workspace_bytes"]
        assert self.ws_bytes % 16 == 0
        self.ws = _guarded(self.ws_bytes // 4, device)
        p = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
        self.args = _lib.GaMeshSampleArgs(self.v.shape[0], self.f.shape[0], S, 0, 0 if device_seed else seed, p(self.words),
                                          self.v.data_ptr(), self.f.data_ptr(), p(self.c), self.points.data_ptr(), self.face.data_ptr(),
                                          self.bary.data_ptr(), p(self.normals), p(self.colors), self.ws.data_ptr(), self.ws_bytes)

    def enqueue(self, stream):
        self._lib.check(self.L.ga_mesh_sample(ctypes.byref(self.args), ctypes.c_void_p(stream.cuda_stream)), "ga_mesh_sample")

    def poison(self):
        for b in (self.points, self.bary, self.face, self.normals, self.colors):
            if b is not None:
                b[:-GUARD] = POISON

    def outputs(self):
        S = self.S
        assert bool((self.ws[self.ws_bytes // 4:] == GUARD_WORD).all()), "guard words behind the workspace overwritten"
        out = dict(points=_take(self.points, 3 * S, (S, 3)), bary=_take(self.bary, 3 * S, (S, 3)),
                   face=_take(self.face, S, (S,), torch.int32))
        if self.normals is not None:
            out["normals"] = _take(self.normals, 3 * S, (S, 3))
        if self.colors is not None:
            out["colors"] = _take(self.colors, 3 * S, (S, 3))
        return out


def _check(got, want):
    assert np.array_equal(got["face"], want["face"]), "faces differ"
    for k in ("bary", "points", "normals", "colors"):
        if k in got:
            _same(got[k], want[k], k)


def _mesh(name):
    fpg, per_trip = plan(1)["faces_per_group"], plan(1)["sums_per_trip"]
    if name == "one":
        v, f = ref.unit_square()
        return v, f[:1]
    if name == "two":
        return ref.unit_square()
    if name == "spliced":
        return ref.spliced_soup()[:2]
    return ref.strip({"group-1": fpg - 1, "group": fpg, "group+1": fpg + 1, "trip+1": fpg * per_trip + 1}[name])


@pytest.mark.parametrize("name,S,colors,normals", [
    ("one", 257, True, True), ("two", 255, False, True), ("group-1", 257, True, False), ("group", 255, False, False),
    ("group+1", 257, True, True), ("trip+1", 257, True, True), ("spliced", 1, False, True), ("spliced", 255, True, True),
    ("spliced", 2000, False, False)])
def test_sample_bits(gpu_device, name, S, colors, normals):
    v, f = _mesh(name)
    c = np.random.default_rng(1).uniform(0, 1, v.shape).astype(F32) if colors else None
    seed = 0x9E3779B97F4A7C15 ^ S
    with torch.cuda.device(gpu_device):
        raw = Raw(gpu_device, v, f, S, seed=seed, colors=c, normals=normals)
        raw.enqueue(torch.cuda.current_stream(gpu_device))
        torch.cuda.synchronize()
        got = raw.outputs()
    want = ref.sample(v, f, S, seed, colors=c)
    assert (want["face"] >= 0).all()
    _check(got, want)


def test_all_degenerate_mesh(gpu_device):
    v, f = ref.strip(300)
    f = np.zeros_like(f)
    f[7] = (-1, 2, 3)
    with torch.cuda.device(gpu_device):
        raw = Raw(gpu_device, v, f, 300, seed=1, colors=np.ones_like(v))
        raw.enqueue(torch.cuda.current_stream(gpu_device))
        torch.cuda.synchronize()
        got = raw.outputs()
    assert (got["face"] == -1).all()
    for k in ("points", "bary", "normals", "colors"):
        assert not got[k].view(np.uint32).any(), k


def test_front_end_and_argument_checks(gpu_device):
    from gaussiananything_amd import _lib, mesh
    v, f = ref.icosphere(2)
    c = np.random.default_rng(2).uniform(0, 1, v.shape).astype(F32)
    tv, tf, tc = (torch.from_numpy(a).to(gpu_device) for a in (v, f, c))
    pts, nrm, col, (face, bary) = mesh.sample_points_from_mesh(tv, tf.long(), 1000, colors=tc, seed=12, return_normals=True,
                                                               return_faces=True)
    want = ref.sample(v, f, 1000, 12, colors=c)
    assert face.dtype == torch.int64 and pts.device == tv.device
    _check(dict(points=pts.cpu().numpy(), normals=nrm.cpu().numpy(), colors=col.cpu().numpy(), face=face.cpu().numpy().astype(np.int32),
                bary=bary.cpu().numpy()), want)
    only = mesh.sample_points_from_mesh(tv, tf, 1000, seed=12)
    assert isinstance(only, torch.Tensor) and torch.equal(only, pts)
    with pytest.raises(RuntimeError):
        mesh.sample_points_from_mesh(tv.cpu(), tf.cpu(), 10)
    with pytest.raises(ValueError):
        mesh.sample_points_from_mesh(tv[None], tf[None], 10)          # a batch of meshes is not built
    L = _lib.lib()
    raw = Raw(gpu_device, v, f, 16)
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu_device).cuda_stream)
    for field, value, code in (("num_faces", 0, -2), ("num_samples", 0, -2), ("reserved", 1, -5), ("vertices", None, -1),
                               ("workspace_bytes", raw.ws_bytes - 16, -3), ("colors", raw.points.data_ptr(), -1)):
        args = _lib.GaMeshSampleArgs.from_buffer_copy(raw.args)
        setattr(args, field, value)
        assert L.ga_mesh_sample(ctypes.byref(args), stream) == code, field


def test_graph_replay_with_a_device_seed(gpu_device):
    """captured once with the seed on the device, replayed after the two words were overwritten: the samples of the new seed"""
    v, f = ref.icosphere(2)
    first_seed, second_seed = 0x0123456789ABCDEF, 0xFEDCBA9876543210
    with torch.cuda.device(gpu_device):
        raw = Raw(gpu_device, v, f, 513, seed=first_seed, device_seed=True)
        side = torch.cuda.Stream(device=gpu_device)
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            raw.enqueue(side)          # warm-up on the capture stream
            side.synchronize()
            with torch.cuda.graph(graph, stream=side):
                raw.enqueue(side)
        torch.cuda.synchronize()
        _check(raw.outputs(), ref.sample(v, f, 513, first_seed))
        raw.words.copy_(_seed_words(second_seed))
        raw.poison()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        got = raw.outputs()
    want = ref.sample(v, f, 513, second_seed)
    assert not np.array_equal(want["face"], ref.sample(v, f, 513, first_seed)["face"])
    _check(got, want)
