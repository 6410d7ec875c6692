"""numpy float64 restatement of the object-bounds rule (include/mnrf.h: mnrf_occupancy_bits, mnrf_object_cull) and the ray
families the tests of it share.

The rule is stated on the OBJECT-FRAME ray q as written in fp32 (a row of mnrf_object_rays): the segment is
{o + d z : z in [q[6], q[7]]}, cell (i, j, k) the closed box lo + (i..i+1, j..j+1, k..k+1) * (hi - lo) / R.
  must keep: the segment intersects a set cell, or q has a non-finite component;
  must cull: the segment does not intersect the set cells grown by one cell extent per axis.
Runs of set cells along x are merged into one box each (the union of closed cells of a run is a closed box, and so is the
union of their grown versions), so a 64^3 grid costs a few thousand boxes, not a quarter of a million."""
import numpy as np

F32, F64 = np.float32, np.float64


# ----------------------------------------------------------------------------------------------- occupancy bits
def occupancy_cells(volume, sigma_min, dilate):
    """(Rz+1, Ry+1, Rx+1) corner samples -> (Rz, Ry, Rx) bool: a cell is set when one of its 8 corners has !(sigma < sigma_min)
    (NaN sets it); dilate = 1 grows the set by one cell over the 26-neighbourhood."""
    with np.errstate(invalid="ignore"):
        flag = ~(np.asarray(volume, F32) < F32(sigma_min))
    cells = np.zeros(tuple(s - 1 for s in flag.shape), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                cells |= flag[dz:dz + cells.shape[0], dy:dy + cells.shape[1], dx:dx + cells.shape[2]]
    if dilate:
        pad = np.pad(cells, 1)
        grown = np.zeros_like(cells)
        for dz in range(3):
            for dy in range(3):
                for dx in range(3):
                    grown |= pad[dz:dz + cells.shape[0], dy:dy + cells.shape[1], dx:dx + cells.shape[2]]
        cells = grown
    return cells


def pack_bits(cells):
    """(Rz, Ry, Rx) bool -> (Rz, Ry, ceil(Rx / 32)) uint32: cell i is bit i % 32 of word i / 32, padding bits zero."""
    rz, ry, rx = cells.shape
    words = (rx + 31) // 32
    padded = np.zeros((rz, ry, words * 32), np.uint64)
    padded[:, :, :rx] = cells
    return (padded.reshape(rz, ry, words, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


# ----------------------------------------------------------------------------------------------- the rule
def run_boxes(cells, lo, hi, grow=0.0):
    """The set cells as closed boxes (M, 2, 3), one per run of set cells along x, each grown by `grow` cell extents per axis."""
    cells = np.asarray(cells, bool)
    rz, ry, rx = cells.shape
    lo, hi = np.asarray(lo, F64), np.asarray(hi, F64)
    size = (hi - lo) / np.array([rx, ry, rz], F64)
    edge = np.diff(np.pad(cells, ((0, 0), (0, 0), (1, 1))).astype(np.int8), axis=2)       # +1 where a run starts, -1 behind its end
    k0, j0, i0 = np.nonzero(edge == 1)
    k1, j1, i1 = np.nonzero(edge == -1)
    assert (k0 == k1).all() and (j0 == j1).all() and (i1 > i0).all()
    first = np.stack([i0, j0, k0], 1).astype(F64)
    last = np.stack([i1, j0 + 1, k0 + 1], 1).astype(F64)
    return np.stack([lo + (first - grow) * size, lo + (last + grow) * size], 1)


def segment_meets_any(q, boxes, chunk=256):
    """Does the segment of each ray q (n, 8; float64 arithmetic on the given values) intersect one of the closed boxes?"""
    q = np.asarray(q, F64)
    out = np.zeros(q.shape[0], bool)
    if boxes.shape[0] == 0:
        return out
    a0, a1 = boxes[None, :, 0, :], boxes[None, :, 1, :]
    for s in range(0, q.shape[0], chunk):
        o, d = q[s:s + chunk, None, 0:3], q[s:s + chunk, None, 3:6]
        zn, zf = q[s:s + chunk, None, 6], q[s:s + chunk, None, 7]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            ta, tb = (a0 - o) / d, (a1 - o) / d
            par = d == 0
            t_in = np.where(par, -np.inf, np.minimum(ta, tb))
            t_out = np.where(par, np.inf, np.maximum(ta, tb))
            inside = (~par | ((o >= a0) & (o <= a1))).all(-1)
            t0 = np.maximum(zn, t_in.max(-1))
            t1 = np.minimum(zf, t_out.min(-1))
            out[s:s + chunk] = (inside & (t0 <= t1)).any(-1)
    return out


def classify(q, cells, lo, hi):
    """-> (must_keep, must_cull) of the object-frame rays q (n, 8) against the set cells of the box [lo, hi]."""
    q = np.asarray(q)
    bad = ~np.isfinite(q.astype(F64)).all(1)
    safe = np.where(bad[:, None], 0.0, q.astype(F64))
    must_keep = segment_meets_any(safe, run_boxes(cells, lo, hi)) | bad
    must_cull = ~segment_meets_any(safe, run_boxes(cells, lo, hi, grow=1.0)) & ~bad
    return must_keep, must_cull


# ----------------------------------------------------------------------------------------------- grids of the tests
BOX_LO, BOX_HI = (-0.6, -0.4, -0.5), (0.7, 0.5, 0.3)


def grid_cells(name):
    """The set cells (Rz, Ry, Rx) of the test grids: 1x1x1; 4x4x4 with a 2x2x1 block and a lone cell; 33x5x7 (a row of 33
    cells is two words with one padding-free bit in the second) with a diagonal, a short run into x = 32 and a block;
    64^3 with an off-centre ball."""
    if name == "1x1x1":
        return np.ones((1, 1, 1), bool)
    if name == "4x4x4":
        c = np.zeros((4, 4, 4), bool)
        c[1, 1:3, 0:2] = True
        c[3, 3, 3] = True
        return c
    if name == "33x5x7":
        c = np.zeros((7, 5, 33), bool)
        for t in range(5):
            c[t + 1, t, 6 * t + 1] = True
        c[0, 4, 30:33] = True
        c[5:7, 0:2, 14:18] = True
        return c
    if name == "64x64x64":
        z, y, x = np.meshgrid(*(np.arange(64) + 0.5,) * 3, indexing="ij")
        return (x - 40) ** 2 + (y - 28) ** 2 + (z - 24) ** 2 <= 11.0 ** 2
    raise KeyError(name)


GRIDS = ("1x1x1", "4x4x4", "33x5x7", "64x64x64")
SIMILARITY = np.array([[0.0, -1.25, 0.0, 0.1], [1.25 * 0.8, 0.0, -1.25 * 0.6, -0.2], [1.25 * 0.6, 0.0, 1.25 * 0.8, 0.05]])
POSES = {"no_pose": None, "identity": np.eye(3, 4), "similarity": SIMILARITY}
MOVE = dict(scale=2.0, translation=(0.1, -0.3, 0.2))


def to_scene(q, pose, scale, translation):
    """Object-frame rays (float64) -> the scene rays that mnrf_object_rays moves onto them (up to fp32 rounding): the inverse
    of o' = (A o + p) * scale + t, d' = normalize(A d)."""
    q = np.asarray(q, F64).copy()
    o = (q[:, :3] - np.asarray(translation, F64)) / scale
    d = q[:, 3:6]
    if pose is not None:
        A, p = np.asarray(pose, F64)[:3, :3], np.asarray(pose, F64)[:3, 3]
        Ai = np.linalg.inv(A)
        with np.errstate(invalid="ignore"):          # (the NaN and inf rows)
            o = (o - p) @ Ai.T
            d = d @ Ai.T
        n = np.linalg.norm(d, axis=1, keepdims=True)
        d = np.where(n > 0, d / np.where(n > 0, n, 1.0), d)
    q[:, :3], q[:, 3:6] = o, d
    return q


def object_rays64(rays, pose, scale, translation):
    """mnrf_object_rays in float64 on fp32 scene rays, rounded to fp32: what the CPU check of the construction classifies."""
    r = np.asarray(rays, F32).astype(F64)
    o, d = r[:, :3], r[:, 3:6]
    if pose is not None:
        A, p = np.asarray(pose, F32).astype(F64)[:3, :3], np.asarray(pose, F32).astype(F64)[:3, 3]
        o = o @ A.T + p
        d = d @ A.T
        d = d / np.sqrt(np.maximum((d * d).sum(1, keepdims=True), 1.1920928955078125e-07))
    with np.errstate(invalid="ignore", over="ignore"):
        return np.concatenate([o * scale + np.asarray(translation, F64), d, r[:, 6:]], 1).astype(F32)


def _unit(rs, n):
    d = rs.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def ray_families(cells, lo, hi, n_random, seed):
    """Object-frame rays (float64) by family -> dict name -> (m, 8).  "through" and "missing" are the random families whose
    share in the band between the two rules the tests bound."""
    rs = np.random.RandomState(seed)
    lo, hi = np.asarray(lo, F64), np.asarray(hi, F64)
    rz, ry, rx = cells.shape
    size = (hi - lo) / np.array([rx, ry, rz], F64)
    diag = float(np.linalg.norm(hi - lo))
    k, j, i = np.nonzero(cells)
    set_idx = np.stack([i, j, k], 1).astype(F64)

    def in_set_cell(m):
        pick = set_idx[rs.randint(0, len(set_idx), m)]
        return lo + (pick + rs.uniform(0.15, 0.85, (m, 3))) * size

    def through(m, p=None):
        p = in_set_cell(m) if p is None else p
        d = _unit(rs, m)
        s = rs.uniform(0.5, 3.0, (m, 1)) * diag
        near = rs.uniform(0.0, 0.3, (m, 1)) * s
        return np.concatenate([p - d * s, d, near, s + rs.uniform(0.1, 2.0, (m, 1)) * diag], 1)

    fam = {}
    m = n_random // 2
    # random through the object (half aimed at a set cell, half at any point of the box) and random missing it (from far away,
    # in any direction: a few of those hit after all)
    any_point = lo + rs.uniform(0, 1, (m - m // 2, 3)) * (hi - lo)
    fam["through"] = np.concatenate([through(m // 2), through(m - m // 2, any_point)], 0)
    o = (lo + hi) / 2 + _unit(rs, n_random - m) * rs.uniform(3.0, 5.0, (n_random - m, 1)) * diag
    fam["missing"] = np.concatenate([o, _unit(rs, n_random - m), rs.uniform(0.0, 0.5, (n_random - m, 1)),
                                     rs.uniform(6.0, 12.0, (n_random - m, 1)) * diag], 1)
    # axis-parallel: two zero components; through the footprint of a set cell, and well beside the box
    rows = []
    for a in range(3):
        for sign in (1.0, -1.0):
            for beside in (False, True):
                p = in_set_cell(1)[0]
                if beside:
                    p[(a + 1) % 3] = hi[(a + 1) % 3] + 2.3 * size[(a + 1) % 3]
                d = np.zeros(3)
                d[a] = sign
                o = p - d * 2.0 * diag
                rows.append(np.concatenate([o, d, [0.05, 5.0 * diag]]))
    fam["axis_parallel"] = np.array(rows)
    # the origin inside a set cell: a short segment that never leaves it, from z = 0 and from z > 0; and a zero direction
    p = in_set_cell(8)
    d = _unit(rs, 8)
    short = 0.1 * size.min()
    fam["origin_inside"] = np.concatenate([p, d, np.repeat([[0.0], [0.25 * short]], 4, 0), np.full((8, 1), short)], 1)
    fam["zero_direction"] = np.concatenate([np.concatenate([in_set_cell(2), hi + 3.0 * size * np.ones((2, 3))], 0), np.zeros((4, 3)),
                                            np.full((4, 1), 0.5), np.full((4, 1), 2.0)], 1)
    # the segment ends before the box / starts behind it / is empty (far < near)
    t = through(12)
    before, behind, empty = t[:4].copy(), t[4:8].copy(), t[8:].copy()
    before[:, 7] = before[:, 6] + 0.02 * diag                            # far: a little beyond near, short of the aimed-at cell
    behind[:, 6] = behind[:, 7] + 4.0 * diag                             # near: beyond the box for certain
    behind[:, 7] = behind[:, 6] + 1.0
    empty[:, 6], empty[:, 7] = empty[:, 7].copy(), empty[:, 6].copy()    # far < near
    fam["ends_before"], fam["starts_behind"], fam["far_below_near"] = before, behind, empty
    # a row of NaN / inf per column
    for name, val in (("nan", np.nan), ("inf", np.inf)):
        t = through(8)
        t[np.arange(8), np.arange(8)] = val
        fam[name] = t
    return fam
