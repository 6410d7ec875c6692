"""Plain numpy / Python restatements for the mesh tests: marching cubes as a loop over cells, a union-find, the
canonical form two meshes are compared in, mesh invariants, and the float64 colour fusion.

`marching_cubes` shares one thing with the kernels of csrc/mnrf_mesh.hip: the 256-case table, which it is handed (read
through mnrf_mc_table and checked exhaustively in tests/test_mesh_cpu.py).  Everything else -- how vertices are welded
(a dictionary keyed by the grid edge, filled in cell order), how indices are assigned, how cells are visited -- is
independent of the kernels' ownership and scan scheme.  `marching_cubes_cropped` runs the same loop on the bounding box
of the surface (for volumes too large to loop over), `block_counts` restates what the count kernel leaves per block,
`renumber` and `triangle_strip` make the numberings and chains the component kernels are held to.
"""
import numpy as np

CORNER = np.array([[c & 1, (c >> 1) & 1, (c >> 2) & 1] for c in range(8)])


def edge_ends(e):
    """(lower corner offset, axis) of edge e in the table's numbering (include/mnrf.h, mnrf_mc_table)."""
    a, k = divmod(int(e), 4)
    others = [i for i in range(3) if i != a]
    lo = [0, 0, 0]
    lo[others[0]], lo[others[1]] = k & 1, k >> 1
    return tuple(lo), a


def cell_cases(volume, threshold):
    """(nx - 1, ny - 1, nz - 1) int32: the case index of every cell (bit c <=> corner c >= threshold; a NaN is outside)."""
    vol = np.asarray(volume, dtype=np.float32)
    nx, ny, nz = vol.shape
    inside = vol >= np.float32(threshold)
    cases = np.zeros((nx - 1, ny - 1, nz - 1), dtype=np.int32)
    for c in range(8):
        ox, oy, oz = CORNER[c]
        cases |= inside[ox:nx - 1 + ox, oy:ny - 1 + oy, oz:nz - 1 + oz].astype(np.int32) << c
    return cases


def marching_cubes(volume, threshold, table, origin=(0, 0, 0), return_edges=False):
    """(vertices (V, 3) float32 in index coordinates, triangles (T, 3) int32); float32 arithmetic, the vertex evaluated from
    the lower-index end of its edge.  `origin`: the index of volume[0, 0, 0] in a larger volume this one was cut from; it is
    added to the integer grid point before the vertex is formed, so the float32 position is that of the larger volume.
    return_edges: also the (V, 4) int64 grid edge [i, j, k, axis] of every vertex (lower end and direction, in the volume given)."""
    vol = np.asarray(volume, dtype=np.float32)
    thr = np.float32(threshold)
    index, verts, tris = {}, [], []
    active = cell_cases(vol, thr)
    for i, j, k in zip(*np.nonzero((active != 0) & (active != 255))):
        row = table[active[i, j, k]]
        for t in range(0, 15, 3):
            if row[t] < 0:
                break
            tri = []
            for e in row[t:t + 3]:
                lo, a = edge_ends(e)
                p0 = (i + lo[0], j + lo[1], k + lo[2])
                key = (p0, a)
                if key not in index:
                    p1 = list(p0)
                    p1[a] += 1
                    s0, s1 = vol[p0], vol[tuple(p1)]
                    pos = np.array([p0[0] + origin[0], p0[1] + origin[1], p0[2] + origin[2]], dtype=np.float32)
                    with np.errstate(all="ignore"):      # (a NaN or inf end gives a NaN position; the topology stands)
                        pos[a] = pos[a] + (thr - s0) / (s1 - s0)
                    index[key] = len(verts)
                    verts.append(pos)
                tri.append(index[key])
            tris.append(tri)
    v = np.array(verts, dtype=np.float32).reshape(-1, 3)
    t = np.array(tris, dtype=np.int32).reshape(-1, 3)
    if return_edges:
        edges = np.array([p0 + (a,) for (p0, a), _ in sorted(index.items(), key=lambda kv: kv[1])], dtype=np.int64).reshape(-1, 4)
        return v, t, edges
    return v, t


def flat_edge_rank(edges, shape):
    """The number a vertex has when the crossed edges are counted in the flat (z fastest) order of their lower end, +x, +y,
    +z within a point: the order csrc/mnrf_mesh.hip documents for its output.  edges: (V, 4) [i, j, k, axis]."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 4)
    key = ((e[:, 0] * shape[1] + e[:, 1]) * shape[2] + e[:, 2]) * 3 + e[:, 3]
    rank = np.empty(len(e), dtype=np.int64)
    rank[np.argsort(key)] = np.arange(len(e))
    return rank


def crop_box(volume, threshold):
    """((i0, i1), (j0, j1), (k0, k1)) half-open POINT ranges: the bounding box of the cells that straddle the threshold, padded
    by one point on every side and clipped to the volume; None where no cell straddles it."""
    cases = cell_cases(volume, threshold)
    act = (cases != 0) & (cases != 255)
    if not act.any():
        return None
    box = []
    for axis in range(3):
        hit = np.nonzero(act.any(axis=tuple(a for a in range(3) if a != axis)))[0]
        # cells hit[0] .. hit[-1] span points hit[0] .. hit[-1] + 1
        box.append((max(int(hit[0]) - 1, 0), min(int(hit[-1]) + 3, cases.shape[axis] + 1)))
    return tuple(box)


def marching_cubes_cropped(volume, threshold, table):
    """marching_cubes of a volume too large to loop over: marching cubes is local, so the cell loop runs on `crop_box` alone
    and the crop's offset goes back into the integer part of every vertex (exact: the same float32 values as uncropped)."""
    vol = np.asarray(volume, dtype=np.float32)
    box = crop_box(vol, threshold)
    if box is None:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
    (i0, i1), (j0, j1), (k0, k1) = box
    return marching_cubes(vol[i0:i1, j0:j1, k0:k1], threshold, table, origin=(i0, j0, k0))


def crossed_edges(volume, threshold):
    """Number of grid edges whose ends differ (= the number of welded vertices); a NaN end is outside, as under `>=`."""
    ins = np.asarray(volume, dtype=np.float32) >= np.float32(threshold)
    return int((ins[1:] != ins[:-1]).sum() + (ins[:, 1:] != ins[:, :-1]).sum() + (ins[:, :, 1:] != ins[:, :, :-1]).sum())


def block_counts(volume, threshold, table, block=256):
    """(ceil(points / block), 2) int64: per run of `block` points in flat (z fastest) order the [crossed edges, triangles] of
    the points in it.  A point owns the edges towards its +x, +y and +z neighbours and the cell it is the lowest corner of."""
    vol = np.asarray(volume, dtype=np.float32)
    ins = vol >= np.float32(threshold)
    edges = np.zeros(vol.shape, dtype=np.int64)
    edges[:-1] += ins[1:] != ins[:-1]
    edges[:, :-1] += ins[:, 1:] != ins[:, :-1]
    edges[:, :, :-1] += ins[:, :, 1:] != ins[:, :, :-1]
    per_case = (np.asarray(table)[:, 0:15:3] >= 0).sum(1)
    tris = np.zeros(vol.shape, dtype=np.int64)
    tris[:-1, :-1, :-1] = per_case[cell_cases(vol, threshold)]
    n = vol.size
    blocks = (n + block - 1) // block
    out = np.zeros((blocks * block, 2), dtype=np.int64)
    out[:n, 0], out[:n, 1] = edges.reshape(-1), tris.reshape(-1)
    return out.reshape(blocks, block, 2).sum(1)


def canonical_triangles(triangles):
    """Topology alone: each triangle rotated to its smallest index first (winding kept), the rows sorted.  For two meshes whose
    vertex numbering is known to agree but whose positions cannot be compared (NaN)."""
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    if len(t) == 0:
        return t
    t = np.stack([np.roll(t, -s, 1) for s in range(3)], 0)[np.argmin(t, 1), np.arange(len(t))]
    return t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]


def canonical(vertices, triangles):
    """Sort the vertices lexicographically, remap, rotate each triangle to its smallest index first (the winding is
    kept), sort the triangles.  Vertices at the same position (a corner value equal to the threshold puts the vertices of
    all crossed edges at that corner on the corner) cannot be told apart by position: they are merged into one, on both
    sides of a comparison alike; the number of welded vertices is compared separately."""
    v = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    if len(v) == 0:
        return v, t
    uniq, rank = np.unique(v, axis=0, return_inverse=True)
    t = rank.reshape(-1)[t]
    if len(t):
        rots = np.stack([np.roll(t, -s, 1) for s in range(3)], 0)      # the smallest rotation (a merged vertex may repeat)
        key = (rots[..., 0] * (len(uniq) + 1) + rots[..., 1]) * (len(uniq) + 1) + rots[..., 2]
        t = rots[np.argmin(key, 0), np.arange(len(t))]
        t = t[np.lexsort((t[:, 2], t[:, 1], t[:, 0]))]
    return uniq, t


def on_grid_edges(vertices):
    """For welded marching-cubes vertices: every vertex has at most one non-integer coordinate."""
    v = np.asarray(vertices, dtype=np.float64)
    return bool(((v != np.floor(v)).sum(1) <= 1).all())


def union_find_labels(n_vertices, triangles):
    """labels[v] = the smallest vertex index of v's component."""
    parent = list(range(n_vertices))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in np.asarray(triangles).tolist():
        for u, w in ((a, b), (b, c)):
            ru, rw = find(u), find(w)
            if ru != rw:
                parent[max(ru, rw)] = min(ru, rw)
    return np.array([find(x) for x in range(n_vertices)], dtype=np.int64)


def largest_component(vertices, triangles):
    """(vertices, triangles, n_components, largest size): the component with the most triangles (ties: smallest label),
    unreferenced vertices dropped, order kept."""
    v, t = np.asarray(vertices), np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    if len(t) == 0:
        return v[:0], t.astype(np.int32), 0, 0
    labels = union_find_labels(len(v), t)
    tl = labels[t[:, 0]]
    counts = np.bincount(tl, minlength=len(v))
    best = int(np.argmax(counts))
    keep_t = tl == best
    keep_v = labels == best
    new = np.cumsum(keep_v) - 1
    return v[keep_v], new[t[keep_t]].astype(np.int32), int((counts > 0).sum()), int(counts[best])


def renumber(n_vertices, triangles, seed):
    """A seeded random renumbering of one mesh: (perm, triangles') with vertex v renamed perm[v], the triangle order
    shuffled and every triangle's corners rotated by a random amount (the winding is kept).  Vertex data moves with
    `new[perm] = old`."""
    rs = np.random.RandomState(seed)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    perm = rs.permutation(n_vertices)
    t = perm[t][rs.permutation(len(t))]
    rot = rs.randint(0, 3, len(t))
    t = np.stack([np.roll(t, -s, 1) for s in range(3)], 0)[rot, np.arange(len(t))]
    return perm, t.astype(np.int32)


def triangle_strip(n_triangles, first=0, step=1):
    """(n_triangles, 3) int32: the strip (v, v + step, v + 2 step) from v = first on: n_triangles + 2 vertices, one component,
    and a chain of that length for a union-find."""
    v = first + step * np.arange(n_triangles, dtype=np.int64)
    return np.stack([v, v + step, v + 2 * step], 1).astype(np.int32)


def directed_edges(triangles):
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]], 0)


def is_closed_oriented(triangles):
    """Every edge is used by exactly two triangles, once in each direction."""
    e = directed_edges(triangles)
    if len(e) == 0:
        return True
    fwd = {}
    for a, b in e.tolist():
        if (a, b) in fwd:
            return False
        fwd[(a, b)] = 1
    return all((b, a) in fwd for (a, b) in fwd)


def euler_characteristic(n_vertices, triangles):
    e = np.sort(directed_edges(triangles), 1)
    return n_vertices - len(np.unique(e, axis=0)) + len(np.asarray(triangles).reshape(-1, 3))


def signed_volume(vertices, triangles):
    v = np.asarray(vertices, dtype=np.float64)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    return float(np.einsum("ij,ij->i", v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6.0)


def index_to_world(vertices, x_range, y_range, z_range, N, exact_spacing=False):
    """The three lines of the reference's mapping (float32 arrays times Python floats), or the exact one."""
    (xmin, xmax), (ymin, ymax), (zmin, zmax) = x_range, y_range, z_range
    v = (np.asarray(vertices, dtype=np.float64) / (N - 1 if exact_spacing else N)).astype(np.float32)
    f = np.float32
    if exact_spacing:
        x = f(xmax - xmin) * v[:, 1] + f(xmin)
        y = f(ymax - ymin) * v[:, 0] + f(ymin)
    else:
        x = f(ymax - ymin) * v[:, 1] + f(ymin)
        y = f(xmax - xmin) * v[:, 0] + f(xmin)
    z = f(zmax - zmin) * v[:, 2] + f(zmin)
    return np.stack([x, y, z], 1).astype(np.float32)


def project_view(vertices, image, pose, focal, near):
    """Float64 restatement of one view: (colors (V, 3) float64 bilinear samples, depth (V,) float64, pixel (V, 2) float32,
    rays (V, 8) float64)."""
    v = np.asarray(vertices, dtype=np.float32)
    H, W = image.shape[:2]
    pose = np.asarray(pose, dtype=np.float32).reshape(3, 4)
    K = np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]]).astype(np.float32)
    c2w = np.concatenate([pose, np.array([0, 0, 0, 1]).reshape(1, 4)], 0)
    w2c = np.linalg.inv(c2w)[:3]
    cam = w2c @ np.concatenate([v, np.ones((len(v), 1))], 1).T
    cam[1:] *= -1
    img = (K @ cam).T
    depth = img[:, 2] + 1e-5
    with np.errstate(all="ignore"):
        pix = (img[:, :2] / depth[:, None]).astype(np.float32)
    pix[:, 0] = np.clip(pix[:, 0], 0, W - 1)
    pix[:, 1] = np.clip(pix[:, 1], 0, H - 1)
    px, py = pix[:, 0].astype(np.float64), pix[:, 1].astype(np.float64)
    x0, y0 = np.floor(px).astype(int), np.floor(py).astype(int)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    fx, fy = (px - x0)[:, None], (py - y0)[:, None]
    im = image.astype(np.float64)
    colors = (1 - fy) * ((1 - fx) * im[y0, x0] + fx * im[y0, x1]) + fy * ((1 - fx) * im[y1, x0] + fx * im[y1, x1])
    o = pose[:, 3].astype(np.float64)
    d = v.astype(np.float64) - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([np.broadcast_to(o, d.shape), d, np.full((len(v), 1), near), depth[:, None]], 1)
    return colors, depth, pix, rays


def fuse(colors_per_view, depth_per_view, opacity_per_view, occ_threshold):
    """Float64 sums of the reference's weighting; returns (uint8 colours, color_sum, weight_sum)."""
    csum, wsum = 0.0, 0.0
    for c, d, op in zip(colors_per_view, depth_per_view, opacity_per_view):
        op = np.nan_to_num(np.asarray(op, dtype=np.float32), 1)      # (as the reference calls it: copy=1, a NaN becomes 0)
        w = 0.1 / d + (op < np.float32(occ_threshold))
        csum = csum + c * w[:, None]
        wsum = wsum + w
    return (csum / wsum[:, None]).astype(np.uint8), csum, wsum
