"""The colouring along the vertex normals without a GPU: the float64 restatement of the vertex normals
(tests/mesh_normals_ref.py) on hand-made meshes, PLY files with normals, the new C-ABI entry points, and fixture G21
(tests/golden/make_golden_mesh_normals.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import mesh_normals_ref as NR
from tests import mesh_ref as MR
from tests.golden import fixtures as FX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("mnrf_vertex_normals_scratch_bytes", "mnrf_vertex_normals", "mnrf_normal_rays", "mnrf_rgb_to_uint8")


@pytest.fixture(scope="module")
def L():
    from mirror_nerf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


# ----------------------------------------------------------------------------------------------- the restatement
TETRA_V = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float32)
TETRA_T = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int32)      # wound outwards
OCTA_V = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float32)
OCTA_T = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], dtype=np.int32)


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def test_single_triangle():
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 3, 0]], dtype=np.float32)
    n = NR.vertex_normals(v, [[0, 1, 2]])
    assert n.dtype == np.float32 and np.array_equal(n, np.tile([0, 0, 1], (3, 1)))
    assert np.array_equal(NR.vertex_normals(v, [[0, 2, 1]]), np.tile([0, 0, -1], (3, 1)))
    # weighted by area: the big triangle in the z = 0 plane outweighs the small one in the y = 0 plane at the shared vertices
    v = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 1]], dtype=np.float32)
    n = NR.vertex_normals(v, [[0, 1, 2], [0, 3, 1]], dtype=np.float64)
    np.testing.assert_allclose(n[0], _unit([0, 4, 16]), atol=1e-15)
    np.testing.assert_allclose(n[2], [0, 0, 1], atol=1e-15)
    np.testing.assert_allclose(n[3], [0, 1, 0], atol=1e-15)


@pytest.mark.parametrize("name", ["tetrahedron", "octahedron"])
def test_regular_solids(name):
    v, t = (TETRA_V, TETRA_T) if name == "tetrahedron" else (OCTA_V, OCTA_T)
    assert MR.is_closed_oriented(t) and MR.signed_volume(v, t) > 0
    n = NR.vertex_normals(v, t, dtype=np.float64)
    np.testing.assert_allclose(n, _unit(v), atol=1e-15)
    np.testing.assert_allclose(NR.vertex_normals(v, t[:, ::-1], dtype=np.float64), -_unit(v), atol=1e-15)


def test_degenerate_cases():
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [5, 5, 5], [0, 1, 0]], dtype=np.float32)
    n = NR.vertex_normals(v, [[0, 1, 2]])                  # a zero-area triangle and two isolated vertices
    assert np.array_equal(n, np.tile([0, 0, 1], (5, 1)))
    n = NR.vertex_normals(v, [[0, 1, 2], [0, 4, 1]])       # vertex 2 has only the degenerate one
    assert np.array_equal(n[[2, 3]], np.tile([0, 0, 1], (2, 1))) and np.array_equal(n[[0, 1, 4]], np.tile([0, 0, -1], (3, 1)))
    assert NR.vertex_normals(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)).shape == (0, 3)
    v[4] = [np.nan, 1, 0]
    assert np.array_equal(NR.vertex_normals(v, [[0, 4, 1]])[[0, 1, 4]], np.tile([0, 0, 1], (3, 1)))


def test_order_of_the_triangles_is_immaterial():
    rs = np.random.RandomState(2)
    v = rs.normal(size=(200, 3)).astype(np.float32)
    t = rs.randint(0, 200, (900, 3)).astype(np.int32)
    want = NR.vertex_normals(v, t, dtype=np.float64)
    assert np.abs(np.linalg.norm(want, axis=1) - 1).max() < 1e-15
    assert np.abs(NR.vertex_normals(v, t[rs.permutation(len(t))], dtype=np.float64) - want).max() <= 1e-15
    rot = np.stack([np.roll(row, -s) for row, s in zip(t, rs.randint(0, 3, len(t)))])
    assert np.abs(NR.vertex_normals(v, rot, dtype=np.float64) - want).max() <= 1e-15


def test_large_mesh_builders():
    """The meshes tests/test_hip_mesh_normals.py takes past one sweep of the maximum kernel (262 144 triangles): what their
    doc strings promise, at full size, and the restatement's normals on them."""
    n = 400
    v, t = NR.height_field_mesh(n)
    T = 2 * (n - 1) ** 2
    assert v.shape == (n * n, 3) and t.shape == (T, 3) and T == 318402 and T > 262144
    c = NR.cross_products(v, t)
    assert (c[:, 2] == 1.0).all() and np.abs(c[:, :2]).max() < 0.3
    corner = n * n - 1
    assert np.array_equal(np.nonzero((t == corner).any(1))[0], [T - 2, T - 1])
    assert t[T - 2].tolist() == [corner - n - 1, corner, corner - n] and t[T - 1].tolist() == [corner - n - 1, corner - 1, corner]
    nrm = NR.vertex_normals(v, t, dtype=np.float64)
    assert nrm[:, 2].min() > 0.9 and np.abs(np.linalg.norm(nrm, axis=1) - 1).max() < 1e-15
    fv, ft = NR.fan_mesh(100000)
    fc = NR.cross_products(fv, ft)
    big = np.abs(fc).max(1)
    assert (ft[:, 0] == 0).all() and np.bincount(ft.reshape(-1))[1:].tolist() == [2] * 100000
    assert big.min() > 0.99 * big.max() and (fc[:, 2] == big).all()      # congruent triangles, the largest component is z
    fn = NR.vertex_normals(fv, ft, dtype=np.float64)
    np.testing.assert_allclose(fn[0], [0, 0, 1], atol=1e-9)
    rim = fv[1:, :2].astype(np.float64)
    assert ((fn[1:, :2] * rim).sum(1) > 0).all() and fn[1:, 2].min() > 0.9      # tilted outwards, as a cone's are


# ----------------------------------------------------------------------------------------------- PLY
def _expected_ply(v, t, c=None):
    """Today's layout without normals, byte for byte."""
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}", "property float x", "property float y",
            "property float z"]
    if c is not None:
        head += ["property uchar red", "property uchar green", "property uchar blue"]
    head += [f"element face {len(t)}", "property list uchar int vertex_indices", "end_header"]
    body = b"".join(v[i].astype("<f4").tobytes() + (b"" if c is None else c[i].astype("u1").tobytes()) for i in range(len(v)))
    body += b"".join(b"\x03" + t[i].astype("<i4").tobytes() for i in range(len(t)))
    return ("\n".join(head) + "\n").encode("ascii") + body


@pytest.mark.parametrize("with_colors", [False, True])
def test_ply_round_trip_with_normals(tmp_path, with_colors):
    from mirror_nerf_amd import mesh
    rs = np.random.RandomState(4)
    v = rs.normal(size=(37, 3)).astype(np.float32)
    n = _unit(rs.normal(size=(37, 3))).astype(np.float32)
    n[0] = [np.float32(1e-42), -0.0, 1.0]      # a denormal and a signed zero: bit for bit
    t = rs.randint(0, 37, (55, 3)).astype(np.int32)
    c = rs.randint(0, 256, (37, 3)).astype(np.uint8) if with_colors else None
    path = str(tmp_path / "m.ply")
    mesh.write_ply(path, v, t, c, normals=n)
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    want = ["ply", "format binary_little_endian 1.0", "element vertex 37", "property float x", "property float y",
            "property float z", "property float nx", "property float ny", "property float nz"]
    if with_colors:
        want += ["property uchar red", "property uchar green", "property uchar blue"]
    want += ["element face 55", "property list uchar int vertex_indices"]
    assert head.decode("ascii").split("\n") == want + [""]
    assert len(body) == 37 * (27 if with_colors else 24) + 55 * 13
    assert body[:24] == v[0].astype("<f4").tobytes() + n[0].astype("<f4").tobytes()
    if with_colors:
        assert body[24:27] == c[0].tobytes()
    v2, t2, c2, n2 = mesh.read_ply(path, return_normals=True)
    assert v2.dtype == np.float32 and v2.tobytes() == v.tobytes() and t2.dtype == np.int32 and np.array_equal(t2, t)
    assert n2.dtype == np.float32 and n2.tobytes() == n.tobytes()
    assert (c2 is None) if not with_colors else (c2.dtype == np.uint8 and np.array_equal(c2, c))
    # present callers see the 3-tuple they always saw
    three = mesh.read_ply(path)
    assert len(three) == 3 and three[0].tobytes() == v.tobytes() and np.array_equal(three[1], t)
    import torch
    mesh.write_ply(path, torch.from_numpy(v), torch.from_numpy(t), None if c is None else torch.from_numpy(c), torch.from_numpy(n))
    assert open(path, "rb").read() == raw
    with pytest.raises(ValueError):
        mesh.write_ply(path, v, t, c, normals=n[:5])
    # without normals: today's bytes, and a fourth value of None when asked
    mesh.write_ply(path, v, t, c)
    assert open(path, "rb").read() == _expected_ply(v, t, c)
    assert mesh.read_ply(path, return_normals=True)[3] is None and len(mesh.read_ply(path)) == 3
    mesh.write_ply(path, v, t, colors=c, normals=None)
    assert open(path, "rb").read() == _expected_ply(v, t, c)


# ----------------------------------------------------------------------------------------------- C ABI
def test_new_symbols_are_declared_and_exported(L):
    from mirror_nerf_amd import _lib
    declared = set(re.findall(r"\b(mnrf_[a-z0-9_]+)\s*\(", open(os.path.join(ROOT, "include", "mnrf.h")).read()))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.SIGNATURES and hasattr(L, name), name


def test_argument_validation_without_gpu(L):
    null = None
    one = ctypes.c_void_p(16)      # a non-null pointer that is never dereferenced: every call below is refused first
    err = lambda: L.mnrf_last_error()  # noqa: E731
    assert L.mnrf_vertex_normals_scratch_bytes(0) == 8 and L.mnrf_vertex_normals_scratch_bytes(3) == 96
    assert L.mnrf_vertex_normals_scratch_bytes(1000) >= 1000 * 3 * 8 and L.mnrf_vertex_normals_scratch_bytes(1000) % 8 == 0
    assert L.mnrf_vertex_normals_scratch_bytes(-1) < 0 and b"mnrf_vertex_normals_scratch_bytes" in err()
    assert L.mnrf_vertex_normals_scratch_bytes((1 << 29) + 1) < 0
    assert L.mnrf_vertex_normals(null, 4, one, 2, one, one, null) < 0 and b"mnrf_vertex_normals: null" in err()
    assert L.mnrf_vertex_normals(one, 4, null, 2, one, one, null) < 0
    assert L.mnrf_vertex_normals(one, 4, one, 2, null, one, null) < 0
    assert L.mnrf_vertex_normals(one, 4, one, 2, one, null, null) < 0
    assert L.mnrf_vertex_normals(one, -4, one, 2, one, one, null) < 0 and b"bad size" in err()
    assert L.mnrf_vertex_normals(one, 4, one, -2, one, one, null) < 0
    assert L.mnrf_vertex_normals(one, 4, one, (1 << 31) // 3 + 1, one, one, null) < 0
    assert L.mnrf_vertex_normals(one, 4, one, 2, ctypes.c_void_p(20), one, null) < 0 and b"aligned" in err()
    assert L.mnrf_vertex_normals(null, 0, null, 0, null, null, null) == 0            # no vertices: nothing to do
    assert L.mnrf_normal_rays(null, one, 4, 0.05, 8.0, 1.0, one, null) < 0 and b"mnrf_normal_rays" in err()
    assert L.mnrf_normal_rays(one, null, 4, 0.05, 8.0, 1.0, one, null) < 0
    assert L.mnrf_normal_rays(one, one, 4, 0.05, 8.0, 1.0, null, null) < 0
    assert L.mnrf_normal_rays(one, one, -1, 0.05, 8.0, 1.0, one, null) < 0
    assert L.mnrf_normal_rays(null, null, 0, 0.05, 8.0, 1.0, null, null) == 0
    assert L.mnrf_rgb_to_uint8(null, 4, one, null) < 0 and b"mnrf_rgb_to_uint8" in err()
    assert L.mnrf_rgb_to_uint8(one, 4, null, null) < 0 and L.mnrf_rgb_to_uint8(one, -4, one, null) < 0
    assert L.mnrf_rgb_to_uint8(null, 0, null, null) == 0


def test_python_interface_exists():
    import inspect
    from mirror_nerf_amd import mesh
    sig = inspect.signature(mesh.normal_vertex_colors)
    assert list(sig.parameters) == ["vertices", "triangles", "models", "embeddings", "near", "far", "near_t", "N_samples",
                                    "N_importance", "white_back", "chunk", "normals", "return_rgb"]
    d = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert d == dict(near_t=1.0, N_samples=64, N_importance=128, white_back=False, chunk=32 * 1024, normals=None, return_rgb=False)
    assert list(inspect.signature(mesh.normal_rays).parameters) == ["vertices", "normals", "near", "far", "near_t"]
    assert list(inspect.signature(mesh.vertex_normals).parameters) == ["vertices", "triangles"]


# ----------------------------------------------------------------------------------------------- fixture G21
def test_g21_loads_and_is_well_conditioned():
    from mirror_nerf_amd import mesh
    g21, g20 = FX.Fixture("g21_mesh_normal_colors"), FX.Fixture("g20_mesh_trained")
    m, s = g21.meta, g21.meta["stats"]
    g21.state_dicts()      # the checksums of the G11 pair
    V = m["n_vertices"]
    assert V == 4096 and (m["N_samples"], m["N_importance"], m["near"], m["far"], m["near_t"]) == (64, 128, 0.05, 8.0, 1.0)
    assert g21.inputs["vertices"].shape == (V, 3) and g21.inputs["normals"].shape == (V, 3) and g21.inputs["rays"].shape == (V, 8)
    assert g21.outputs["rgb_fine"].shape == (V, 3) and g21.outputs["rgb_fine"].dtype == np.float32
    assert g21.outputs["rgb_fine_fp64_minus_fp32"].dtype == np.float32
    # the generator's assertions, on the stored arrays
    ref64 = g21.outputs["rgb_fine"].astype(np.float64) + g21.outputs["rgb_fine_fp64_minus_fp32"].astype(np.float64)
    med, p95, share, d = NR.ray_error_stats(g21.outputs["rgb_fine"], ref64)
    print(f"G21: reference fp32 vs fp64 per ray: median {med:.2e}, p95 {p95:.2e}, share > 1e-4 {share:.4f} "
          f"({int((d > 1e-4).sum())} rays), max {d.max():.3f}; normals towards higher density {s['normals_towards_higher_density']:.3f}")
    assert med <= 1e-6 and p95 <= 4e-5 and share <= 0.02
    assert abs(share - s["ref_share_1e4"]) <= 1.5 / V and s["ref_median"] <= 1e-6 and s["ref_p95"] <= 4e-5
    assert s["normals_towards_higher_density"] > 2.0 / 3.0      # (the generator's "clear majority")
    # its normals are the restatement's on the mesh it names, its rays the reference's three lines
    vol = np.maximum(g20.outputs["sigma"], 0)
    v, t = MR.marching_cubes(vol, g20.meta["threshold"], mesh.mc_table())
    lv, lt, _, _ = MR.largest_component(v, t)
    world = MR.index_to_world(lv, g20.meta["x_range"], g20.meta["y_range"], g20.meta["z_range"], g20.meta["N"])
    assert (len(world), len(lt)) == (m["largest_vertices"], m["largest_triangles"])
    pick = g21.inputs["pick"]
    assert np.array_equal(world[pick], g21.inputs["vertices"])
    assert np.array_equal(NR.vertex_normals(world, lt)[pick], g21.inputs["normals"])
    assert np.array_equal(NR.normal_rays_torch(g21.inputs["vertices"], g21.inputs["normals"], m["near"], m["far"], m["near_t"]),
                          g21.inputs["rays"])
