"""A numpy float32 restatement of mnrf_place_mirrors_from and mnrf_mirror_sources (csrc/mnrf_mirrors.hip), written from THE RULE
in include/mnrf.h: mnrf_place_mirrors' rule over tests/mirrors_ref.py `intersect`, with the one change
`hit_k = inside && s > 0 && !blocked && k != source`.  Every step is one IEEE float32 operation in the documented order, so this
is what the kernel must return bit for bit (tests/test_hip_mirrors_from.py)."""
import numpy as np

from tests import mirrors_ref as MR

F = np.float32


def place_mirrors(rays, depth, mask, normal, x_surface, mirrors, near, any_in=0, source=None):
    """mirrors_ref.place_mirrors with `source`: (n,) integers, the mirror each ray left at the level above -- no hit for that
    ray; a value outside 0 .. K-1 excludes nothing -- or None (no ray has one).  The same keys; per[k] gains `excluded`."""
    assert 1 <= len(mirrors) <= 8
    rays = np.asarray(rays, F)
    depth, mask = np.array(depth, F), np.array(mask, F)
    normal, x_surface = np.array(normal, F), np.array(x_surface, F)
    n = rays.shape[0]
    source = np.full(n, -1, np.int64) if source is None else np.asarray(source).astype(np.int64)
    assert source.shape == (n,)
    depth0, near = depth.copy(), F(near)
    best = np.full(n, -1, np.int32)
    best_dist = np.zeros(n, F)
    best_x = np.zeros((n, 3), F)
    per = []
    for k, m in enumerate(mirrors):
        p = MR.intersect(rays, m)
        with np.errstate(all="ignore"):
            p["blocked"] = (p["dist"] > depth0) & (depth0 > near)
            p["excluded"] = source == k
            p["hit"] = p["inside"] & (p["s"] > 0) & ~p["blocked"] & ~p["excluded"]
            take = p["hit"] & ((best < 0) | (p["dist"] <= best_dist))
        best[take] = k
        best_dist[take] = p["dist"][take]
        best_x[take] = p["x"][take]
        per.append(p)
    won = best >= 0
    x_surface[won] = best_x[won]
    depth[won] = best_dist[won]
    for k, m in enumerate(mirrors):
        normal[best == k] = np.array(m["normal"], F)
    merged = (mask != 0) | won
    return dict(depth=depth, mask=merged.astype(F), normal=normal, x_surface=x_surface, mask_bool=merged.astype(np.uint8), index=best,
                any=int(any_in) | int(merged.any()), per=per)


def mirror_sources(level_index, compaction_index, m, n_rep):
    """out[j * m + p] = level_index[compaction_index[p]] for j < n_rep; a None compaction_index means p itself, a None
    level_index -1 everywhere: (n_rep * m,) int32."""
    if level_index is None:
        row = np.full(m, -1, np.int32)
    elif compaction_index is None:
        row = np.asarray(level_index, np.int32)[:m]
    else:
        row = np.asarray(level_index, np.int32)[np.asarray(compaction_index, np.int64)[:m]]
    assert row.shape == (m,)
    return np.tile(row, n_rep).astype(np.int32)
