"""Mesh extraction without a GPU: the new C-ABI entry points validate their arguments, the 256-case marching-cubes table
read through mnrf_mc_table is exhaustively consistent (crossed edges, 2-manifold patches, matching faces = no cracks,
outward winding), PLY files round-trip, and extract_mesh's index-to-world mapping restates the reference's three lines.
The restatements the GPU tests lean on are held to plainer ones here: the cropped marching cubes to the uncropped, the
per-block counts to a loop over points, the union-find under renumbering and on long strips, the projection on one pixel."""
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


# ----------------------------------------------------------------------------------------------- the restatements themselves
def _smooth(shape, seed):
    rs = np.random.RandomState(seed)
    X, Y, Z = np.meshgrid(*[np.linspace(-1, 1, n) for n in shape], indexing="ij")
    f = np.zeros(shape)
    for _ in range(5):
        k = rs.uniform(2, 7, 3)
        f += rs.uniform(0.5, 1) * np.sin(k[0] * X + k[1] * Y + k[2] * Z + rs.uniform(0, 6.28))
    return f.astype(np.float32)


def _blob(shape, centre, r):
    I, J, K = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    return (r - np.sqrt((I - centre[0]) ** 2 + (J - centre[1]) ** 2 + (K - centre[2]) ** 2)).astype(np.float32)


@pytest.mark.parametrize("name", ["blob_inside", "cut_by_boundary"])
def test_cropped_marching_cubes_is_the_uncropped_one(name, table):
    """marching_cubes_cropped against marching_cubes where both can run: the same vertex bits, the same triangles, in the
    same order (so also the same canonical mesh); the crop is a strict part of the volume in one case and touches three of
    its faces in the other."""
    if name == "blob_inside":
        vol, thr = _blob((21, 19, 23), (13.3, 11.6, 15.2), 3.7), 0.0
    else:
        vol, thr = _blob((14, 15, 13), (11.5, 12.8, 1.2), 4.4), 0.0      # cut by the faces i = 13, j = 14 and k = 0
    box = MR.crop_box(vol, thr)
    v, t = MR.marching_cubes(vol, thr, table)
    cv, ct = MR.marching_cubes_cropped(vol, thr, table)
    assert len(t) > 100 and v.tobytes() == cv.tobytes() and np.array_equal(t, ct)
    a, b = MR.canonical(v, t), MR.canonical(cv, ct)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    size = [hi - lo for lo, hi in box]
    if name == "blob_inside":
        assert all(lo > 0 and hi < n for (lo, hi), n in zip(box, vol.shape)) and np.prod(size) < vol.size / 3
        assert MR.is_closed_oriented(ct) and MR.euler_characteristic(len(cv), ct) == 2
    else:
        assert box[0][1] == 14 and box[1][1] == 15 and box[2][0] == 0 and box[0][0] > 0 and not MR.is_closed_oriented(ct)
    assert MR.marching_cubes_cropped(np.full((5, 6, 7), -1.0, np.float32), 0.0, table)[1].shape == (0, 3)


def test_block_counts_restatement(table):
    """block_counts against the cell loop: the per-block numbers add up to the restatement's mesh, block by block they are
    what a plain loop over the points of the block gives, and a checkerboard fills a block inside one z-row to the 768
    vertices csrc/mnrf_mesh.hip names as the most a block can hold."""
    one = np.array([[[1, 0], [0, 0]], [[0, 0], [0, 0]]], np.float32)
    assert MR.block_counts(one, 0.5, table).tolist() == [[3, 1]]
    vol = _smooth((7, 9, 11), 3)
    bc = MR.block_counts(vol, 0.1, table, block=64)
    v, t = MR.marching_cubes(vol, 0.1, table)
    assert bc.shape == ((7 * 9 * 11 + 63) // 64, 2) and bc[:, 0].sum() == len(v) == MR.crossed_edges(vol, 0.1) and bc[:, 1].sum() == len(t)
    ins = vol >= np.float32(0.1)
    cases = MR.cell_cases(vol, 0.1)
    want = np.zeros_like(bc)
    for p in range(vol.size):
        i, j, k = np.unravel_index(p, vol.shape)
        for a, (di, dj, dk) in enumerate(((1, 0, 0), (0, 1, 0), (0, 0, 1))):
            if i + di < 7 and j + dj < 9 and k + dk < 11 and ins[i + di, j + dj, k + dk] != ins[i, j, k]:
                want[p // 64, 0] += 1
        if i < 6 and j < 8 and k < 10:
            want[p // 64, 1] += int((table[cases[i, j, k]] >= 0).sum()) // 3
    assert np.array_equal(bc, want)
    I, J, K = np.meshgrid(np.arange(3), np.arange(3), np.arange(600), indexing="ij")
    checker = ((I + J + K) % 2).astype(np.float32)
    bc = MR.block_counts(checker, 0.5, table)
    assert bc[:, 0].max() == 768 and bc[:, 0].sum() == MR.crossed_edges(checker, 0.5) and bc[:, 1].max() <= 5 * 256


def test_union_find_on_renumbered_and_chain_meshes():
    """union_find_labels is independent of the numbering: a renumbered mesh has the renumbered partition, each part labelled
    with its smallest new number; strips are one component under any numbering; and 3 * 10^5 triangles stay cheap (measured
    0.6 s for the shuffled strip here, printed)."""
    import time
    rs = np.random.RandomState(0)
    # three components: two strips and a single triangle, glued by nothing; vertex 72 is unreferenced
    t = np.concatenate([MR.triangle_strip(40), MR.triangle_strip(25, first=42), [[70, 69, 71]]]).astype(np.int32)
    V = 73
    base = MR.union_find_labels(V, t)
    assert sorted(set(base.tolist())) == [0, 42, 69, 72]
    for seed in range(3):
        perm, rt = MR.renumber(V, t, seed)
        got = MR.union_find_labels(V, rt)
        for lab in set(base.tolist()):
            members = perm[base == lab]
            assert (got[members] == members.min()).all()
        assert sorted(map(sorted, rt.tolist())) == sorted(map(sorted, perm[t].tolist()))      # the same triangles
        w = np.arange(V * 3).reshape(V, 3)
        nv = np.empty_like(w)
        nv[perm] = w
        lv, lt, n_comp, largest = MR.largest_component(nv, rt)
        assert (n_comp, largest) == (3, 40) and sorted(lv[:, 0].tolist()) == list(range(0, 42 * 3, 3))
    T = 300000
    strip = MR.triangle_strip(T)
    for name, tri in (("ascending", strip), ("descending", T + 1 - strip), ("shuffled", MR.renumber(T + 2, strip, 1)[1])):
        t0 = time.perf_counter()
        lab = MR.union_find_labels(T + 2, tri)
        print(f"union_find_labels, strip of {T} triangles, {name}: {time.perf_counter() - t0:.2f} s")
        assert not lab.any()
    two = np.concatenate([MR.triangle_strip(500, 0, 2), MR.triangle_strip(500, 1, 2)])
    lab = MR.union_find_labels(1004, two[rs.permutation(1000)])
    assert np.array_equal(lab, np.arange(1004) % 2)
    lv, lt, n_comp, largest = MR.largest_component(np.arange(1004)[:, None].repeat(3, 1), two)
    assert (n_comp, largest) == (2, 500) and np.array_equal(lv[:, 0], np.arange(0, 1004, 2))      # the tie goes to label 0


def test_project_view_restatement_on_one_pixel_axes():
    """MR.project_view needs no special case for a one-pixel axis: np.clip(., 0, 0), floor and min(x0 + 1, W - 1) all land on
    pixel 0, the weights multiply one pixel with itself.  A 1 x 1 image colours every vertex with its pixel; with H == 1 the
    colour is the linear interpolation along the row alone."""
    rs = np.random.RandomState(1)
    verts = rs.uniform(-1, 1, (50, 3)).astype(np.float32)
    verts[:, 2] -= 3.0
    pose = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(np.float32)
    img = rs.randint(0, 256, (1, 1, 3)).astype(np.uint8)
    colors, depth, pix, _ = MR.project_view(verts, img, pose, 20.0, 0.05)
    assert (pix == 0).all() and np.array_equal(colors, np.tile(img[0, 0].astype(np.float64), (50, 1))) and (depth > 0).all()
    row = rs.randint(0, 256, (1, 9, 3)).astype(np.uint8)
    colors, _, pix, _ = MR.project_view(verts, row, pose, 20.0, 0.05)
    assert (pix[:, 1] == 0).all() and len(np.unique(pix[:, 0])) > 10
    x0 = np.floor(pix[:, 0]).astype(int)
    fx = (pix[:, 0].astype(np.float64) - x0)[:, None]
    want = (1 - fx) * row[0, x0] + fx * row[0, np.minimum(x0 + 1, 8)]
    np.testing.assert_allclose(colors, want, rtol=0, atol=1e-12)
    col = np.ascontiguousarray(row.transpose(1, 0, 2))
    colors_t, _, pix_t, _ = MR.project_view(verts[:, [1, 0, 2]] * np.float32([-1, 1, 1]), col, pose, 20.0, 0.05)
    assert (pix_t[:, 0] == 0).all() and len(np.unique(pix_t[:, 1])) > 10


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
