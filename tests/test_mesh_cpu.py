"""Mesh extraction without a GPU: the new C-ABI entry points validate their arguments, the 256-case marching-cubes table
read through mnrf_mc_table is exhaustively consistent (crossed edges, 2-manifold patches, matching faces = no cracks,
outward winding), PLY files round-trip, and extract_mesh's index-to-world mapping restates the reference's three lines."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from tests import mesh_ref as MR


@pytest.fixture(scope="module")
def L():
    from mirror_nerf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def table(L):
    from mirror_nerf_amd import mesh
    t = mesh.mc_table()
    assert t.shape == (256, 16) and t.dtype == np.int8
    return t


NEW_SYMBOLS = ("mnrf_grid_points", "mnrf_clamp_zero", "mnrf_mc_blocks", "mnrf_mc_count", "mnrf_mc_emit", "mnrf_mc_table",
               "mnrf_cc_init", "mnrf_cc_step", "mnrf_cc_count", "mnrf_project_colors", "mnrf_accumulate_colors")


def test_symbols_exist(L):
    from mirror_nerf_amd import _lib
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(L, name), name


def test_argument_validation_without_gpu(L):
    null = None
    one = ctypes.c_void_p(16)      # a non-null pointer that is never dereferenced: every call below is refused first
    err = lambda: L.mnrf_last_error()  # noqa: E731
    # grid points: N < 2, negative count, a range beyond N^3, a null output
    assert L.mnrf_grid_points(0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 1, 0, 1, one, null) < 0 and b"N must be at least 2" in err()
    assert L.mnrf_grid_points(0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 4, 0, -1, one, null) < 0 and b"mnrf_grid_points" in err()
    assert L.mnrf_grid_points(0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 4, 60, 5, one, null) < 0
    assert L.mnrf_grid_points(0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 4, 0, 64, null, null) < 0 and b"null" in err()
    assert L.mnrf_grid_points(0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 4, 64, 0, null, null) == 0      # nothing to do is not an error
    assert L.mnrf_clamp_zero(null, 4, null) < 0 and L.mnrf_clamp_zero(null, -1, null) < 0 and L.mnrf_clamp_zero(null, 0, null) == 0
    # marching cubes: a null volume, a side below 2, too many points, a NaN threshold, negative counts
    assert L.mnrf_mc_count(null, 4, 4, 4, 0.5, one, null) < 0 and b"null volume" in err()
    assert L.mnrf_mc_count(one, 1, 4, 4, 0.5, one, null) < 0 and b"at least 2" in err()
    assert L.mnrf_mc_count(one, 4, 4, 4, 0.5, null, null) < 0
    assert L.mnrf_mc_count(one, 2048, 2048, 2048, 0.5, one, null) < 0 and b"2^30" in err()
    assert L.mnrf_mc_count(one, 4, 4, 4, float("nan"), one, null) < 0 and b"NaN" in err()
    assert L.mnrf_mc_blocks(4, 4, 1) < 0 and L.mnrf_mc_blocks(4, 4, 4) == 1 and L.mnrf_mc_blocks(16, 16, 17) == 17
    assert L.mnrf_mc_emit(null, 4, 4, 4, 0.5, one, one, 1, 1, one, one, null) < 0 and b"null volume" in err()
    assert L.mnrf_mc_emit(one, 4, 4, 4, 0.5, one, one, -1, 1, one, one, null) < 0 and b"mnrf_mc_emit" in err()
    assert L.mnrf_mc_emit(one, 4, 4, 4, 0.5, one, one, 1, -1, one, one, null) < 0
    assert L.mnrf_mc_emit(one, 4, 4, 4, 0.5, one, one, 3, 1, null, one, null) < 0
    assert L.mnrf_mc_emit(one, 4, 4, 4, 0.5, null, one, 3, 1, one, one, null) < 0
    assert L.mnrf_mc_emit(one, 4, 4, 4, 0.5, one, one, 0, 0, null, null, null) == 0         # an empty mesh
    row = (ctypes.c_int8 * 16)()
    assert L.mnrf_mc_table(-1, ctypes.cast(row, ctypes.c_void_p)) < 0 and b"0 to 255" in err()
    assert L.mnrf_mc_table(256, ctypes.cast(row, ctypes.c_void_p)) < 0
    assert L.mnrf_mc_table(3, null) < 0
    # components
    assert L.mnrf_cc_init(null, 4, null) < 0 and L.mnrf_cc_init(one, -1, null) < 0 and L.mnrf_cc_init(null, 0, null) == 0
    assert L.mnrf_cc_step(null, 4, one, 4, one, null) < 0 and b"mnrf_cc_step" in err()
    assert L.mnrf_cc_step(one, -4, one, 4, one, null) < 0
    assert L.mnrf_cc_step(one, 4, one, 4, null, null) < 0
    assert L.mnrf_cc_count(one, 4, one, 4, null, null) < 0 and L.mnrf_cc_count(one, 4, one, -4, one, null) < 0
    # colours
    cam = (ctypes.c_double * 12)()
    org = (ctypes.c_float * 3)()
    assert L.mnrf_project_colors(null, 4, one, 8, 8, cam, org, 10.0, 0.1, one, one, one, null) < 0 and b"mnrf_project_colors" in err()
    assert L.mnrf_project_colors(one, 4, one, 0, 8, cam, org, 10.0, 0.1, one, one, one, null) < 0
    assert L.mnrf_project_colors(one, -4, one, 8, 8, cam, org, 10.0, 0.1, one, one, one, null) < 0
    assert L.mnrf_project_colors(one, 4, one, 8, 8, None, org, 10.0, 0.1, one, one, one, null) < 0
    assert L.mnrf_accumulate_colors(one, one, null, 0.2, 4, one, one, null) < 0 and b"mnrf_accumulate_colors" in err()
    assert L.mnrf_accumulate_colors(one, one, one, 0.2, -1, one, one, null) < 0


# ----------------------------------------------------------------------------------------------- the table, exhaustively
EDGE = [MR.edge_ends(e) for e in range(12)]                                  # (lower corner offset, axis)
EDGE_CORNERS = []
for lo, a in EDGE:
    hi = list(lo)
    hi[a] = 1
    EDGE_CORNERS.append((lo[0] | lo[1] << 1 | lo[2] << 2, hi[0] | hi[1] << 1 | hi[2] << 2))
EDGE_MID = [np.array(lo, dtype=float) + 0.5 * np.eye(3)[a] for lo, a in EDGE]
FACES = list(itertools.product(range(3), (0, 1)))                            # (axis, side)


def _inside(case, c):
    return (case >> c) & 1


def _triangles(row):
    n = int((row >= 0).sum())
    assert n % 3 == 0 and (row[n:] == -1).all() and (row[:n] < 12).all(), row
    return [tuple(int(e) for e in row[t:t + 3]) for t in range(0, n, 3)]


def _in_face(e, face):
    axis, side = face
    lo, a = EDGE[e]
    return a != axis and lo[axis] == side


def _boundary(tris):
    """Directed triangle edges that have no opposite partner; asserts that no directed edge is used twice."""
    seen = set()
    for t in tris:
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            assert (a, b) not in seen, "a directed edge is used twice: the patch is not an oriented manifold"
            seen.add((a, b))
    return {(a, b) for (a, b) in seen if (b, a) not in seen}


def test_table_edges_are_crossed_and_all_used(table):
    # (a) every triangle corner lies on an edge whose two cube corners have opposite inside bits; (b) every such edge is used
    for case in range(256):
        tris = _triangles(table[case])
        crossed = {e for e in range(12) if _inside(case, EDGE_CORNERS[e][0]) != _inside(case, EDGE_CORNERS[e][1])}
        used = {e for t in tris for e in t}
        assert used <= crossed, (case, used - crossed)
        assert used == crossed, (case, crossed - used)
        for t in tris:
            assert len(set(t)) == 3, (case, t)


def test_table_patches_are_manifolds_with_boundary_in_the_faces(table):
    # (c) each case's patch is a 2-manifold whose boundary lies entirely in the cube's faces
    for case in range(256):
        tris = _triangles(table[case])
        boundary = _boundary(tris)
        for a, b in boundary:
            assert any(_in_face(a, f) and _in_face(b, f) for f in FACES), (case, a, b)
        for e in {e for t in tris for e in t}:
            # every vertex sits on the cube's surface: it has one incoming and one outgoing boundary segment, and the
            # triangles around it form one fan from the one to the other
            assert sum(1 for s in boundary if s[0] == e) == 1 and sum(1 for s in boundary if s[1] == e) == 1, (case, e)
            link = []
            for t in tris:
                if e in t:
                    i = t.index(e)
                    link.append((t[(i + 1) % 3], t[(i + 2) % 3]))
            nxt = dict(link)
            assert len(nxt) == len(link), (case, e)
            starts = [a for a, _ in link if a not in {b for _, b in link}]
            assert len(starts) == 1, (case, e)
            n, cur = 0, starts[0]
            while cur in nxt:
                cur, n = nxt[cur], n + 1
            assert n == len(link), (case, e)


def _face_local(e, face):
    axis, _ = face
    lo, a = EDGE[e]
    return (a,) + tuple(lo[i] for i in range(3) if i != axis)


def _face_bits(case, face):
    axis, side = face
    corners = [c for c in range(8) if ((c >> axis) & 1) == side]      # increasing c = increasing (other axes) order
    return tuple(_inside(case, c) for c in corners)


def test_table_faces_match_their_neighbours(table):
    # (d) 256 x 6 checks: the oriented boundary segments on a face depend only on that face's four corner bits, and are the
    # exact reverse of what the cell on the other side of the face (same four bits on its opposite face) produces
    seen = {}
    n = 0
    for case in range(256):
        boundary = _boundary(_triangles(table[case]))
        for face in FACES:
            segs = frozenset((_face_local(a, face), _face_local(b, face)) for a, b in boundary
                             if _in_face(a, face) and _in_face(b, face))
            key = (face, _face_bits(case, face))
            assert seen.setdefault(key, segs) == segs, (case, face)
            n += 1
    assert n == 256 * 6 and len(seen) == 6 * 16
    for axis in range(3):
        for bits in itertools.product((0, 1), repeat=4):
            low, high = seen[((axis, 0), bits)], seen[((axis, 1), bits)]
            assert low == frozenset((b, a) for a, b in high), (axis, bits)
            # and the segments on a face use each of its crossed edges exactly once
            crossed = sum(bits[i] != bits[j] for i, j in ((0, 1), (2, 3), (0, 2), (1, 3)))
            assert len(low) * 2 == crossed and len({e for s in low for e in s}) == crossed, (axis, bits)


def test_table_winding_points_outwards(table):
    # (e) each triangle's normal has a positive component towards an outside corner (and a negative one towards an inside one)
    corners = [np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=float) for c in range(8)]
    for case in range(1, 255):
        for t in _triangles(table[case]):
            p = [EDGE_MID[e] for e in t]
            normal = np.cross(p[1] - p[0], p[2] - p[0])
            assert np.linalg.norm(normal) > 1e-9, (case, t)
            centre = sum(p) / 3.0
            out = [np.dot(normal, corners[c] - centre) for c in range(8) if not _inside(case, c)]
            ins = [np.dot(normal, corners[c] - centre) for c in range(8) if _inside(case, c)]
            assert max(out) > 1e-9 and min(ins) < -1e-9, (case, t)


def test_table_is_what_the_generator_derives(table):
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gen_mc_table", os.path.join(root, "scripts", "gen_mc_table.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert np.array_equal(np.array(gen.table(), dtype=np.int8), table)


# ----------------------------------------------------------------------------------------------- PLY
@pytest.mark.parametrize("with_colors", [False, True])
def test_ply_round_trip(tmp_path, with_colors):
    from mirror_nerf_amd import mesh
    rs = np.random.RandomState(3)
    v = rs.normal(size=(37, 3)).astype(np.float32)
    v[0] = [np.float32(1e-42), -0.0, np.float32(3.4e38)]      # a denormal, a signed zero, a huge value: bit for bit
    t = rs.randint(0, 37, (55, 3)).astype(np.int32)
    c = rs.randint(0, 256, (37, 3)).astype(np.uint8) if with_colors else None
    path = str(tmp_path / "m.ply")
    mesh.write_ply(path, v, t, c)
    v2, t2, c2 = mesh.read_ply(path)
    assert v2.dtype == np.float32 and v2.tobytes() == v.tobytes()
    assert t2.dtype == np.int32 and np.array_equal(t2, t)
    assert (c2 is None) if not with_colors else (c2.dtype == np.uint8 and np.array_equal(c2, c))
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    want = ["ply", "format binary_little_endian 1.0", "element vertex 37", "property float x", "property float y",
            "property float z"]
    if with_colors:
        want += ["property uchar red", "property uchar green", "property uchar blue"]
    want += ["element face 55", "property list uchar int vertex_indices"]
    assert head.decode("ascii").split("\n") == want + [""]
    assert len(body) == 37 * (15 if with_colors else 12) + 55 * 13
    assert body[:4] == v[0, :1].astype("<f4").tobytes()
    # torch tensors are accepted too, and an empty mesh is a valid file
    import torch
    mesh.write_ply(path, torch.from_numpy(v), torch.from_numpy(t), None if c is None else torch.from_numpy(c))
    assert open(path, "rb").read() == raw
    mesh.write_ply(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    v3, t3, c3 = mesh.read_ply(path)
    assert v3.shape == (0, 3) and t3.shape == (0, 3) and c3 is None


# ----------------------------------------------------------------------------------------------- index -> world
@pytest.mark.parametrize("exact_spacing", [False, True])
def test_index_to_world_restates_the_reference(exact_spacing):
    import torch
    from mirror_nerf_amd import mesh
    rs = np.random.RandomState(5)
    for N, xr, yr, zr in ((48, (-1.5, 1.5), (-1.5, 1.5), (-0.3, 1.7)), (256, (-1.0, 1.0), (-1.0, 1.0), (-1.0, 1.0)),
                          (7, (-0.37, 2.2), (0.11, 0.93), (-3.0, -1.1))):
        v = rs.uniform(0, N - 1, (500, 3)).astype(np.float32)
        v[:3] = [[0, 0, 0], [N - 1, N - 1, N - 1], [N - 1, 0, 2]]
        got = mesh.index_to_world(torch.from_numpy(v), xr, yr, zr, N, exact_spacing=exact_spacing).numpy()
        # the three lines of extract_color_mesh.py:193-199 (float32 arrays times Python floats)
        s = (v.astype(np.float64) / (N - 1 if exact_spacing else N)).astype(np.float32)
        (xmin, xmax), (ymin, ymax), (zmin, zmax) = xr, yr, zr
        if exact_spacing:
            x_, y_ = (xmax - xmin) * s[:, 1] + xmin, (ymax - ymin) * s[:, 0] + ymin
        else:
            x_, y_ = (ymax - ymin) * s[:, 1] + ymin, (xmax - xmin) * s[:, 0] + xmin
        z_ = (zmax - zmin) * s[:, 2] + zmin
        want = np.stack([x_, y_, z_], 1)
        assert want.dtype == np.float32 and got.dtype == np.float32
        assert np.array_equal(got, want)
        assert np.array_equal(MR.index_to_world(v, xr, yr, zr, N, exact_spacing), want)
        if exact_spacing:      # grid corners land on the box corners
            np.testing.assert_allclose(got[0], [xmin, ymin, zmin], atol=1e-6)
            np.testing.assert_allclose(got[1], [xmax, ymax, zmax], atol=1e-6)
            np.testing.assert_allclose(got[2], [xmin, ymax, zmin + 2 * (zmax - zmin) / (N - 1)], atol=1e-6)
