"""A numpy restatement of mnrf_objects_merge (csrc/mnrf_objects.hip): the K-object rule of placed_objects=.

Per ray, for k = 0 .. K-1 in list order, merge_ray (csrc/mnrf_object.h, eval.py:261-291) of object k on the ray's current
(rgb, depth, mask): float32 operations in merge_ray's order -- two divisions, the comparisons as written -- as a loop over k on
whole arrays (rays are independent, so a vector step per object is the per-ray loop).  It takes what the kernel takes: per
object the maps of its kept rows (or None: not rendered), slot (K, N), counts (K), capacity, scale and pose_scale0 per object,
near, the level's maps, and nothing else.
"""
import numpy as np

F32 = np.float32


def merge_objects(obj_rgb, obj_depth, obj_opacity, slot, counts, capacity, scales, pose_scale0, near, rgb, depth, mask):
    """-> (rgb, depth, mask, n_used): copies of the level's maps after the K merges (mask None stays None) and, per object,
    the number of rays that took it when its turn came."""
    K, N = slot.shape
    rgb, depth = np.array(rgb, F32), np.array(depth, F32)
    mask = None if mask is None else np.array(mask, F32)
    n_used = np.zeros(K, np.int32)
    rows = np.arange(N)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in range(K):
            if obj_rgb[k] is None:
                continue
            s = slot[k].astype(np.int64)
            listed = (s >= 0) & (s < min(max(int(counts[k]), 0), int(capacity)))
            dst, src = rows[listed], s[listed]
            d = (np.asarray(obj_depth[k], F32)[src] / F32(scales[k])) / F32(pose_scale0[k])        # eval.py:261-265
            cur = depth[dst]
            obj = (d > F32(0)) & (np.asarray(obj_opacity[k], F32)[src] > F32(0.8))                 # eval.py:268-272
            blocked = (d > cur) & (cur > F32(near))                                                # eval.py:275-281
            use = obj & ~blocked
            rgb[dst[use]] = np.asarray(obj_rgb[k], F32)[src[use]]
            depth[dst[use]] = d[use]
            if mask is not None:
                mask[dst[use]] = F32(0)
            n_used[k] = int(use.sum())
    return rgb, depth, mask, n_used


def identity_slots(K, N):
    """slot and counts of K objects that list every ray in order (no bounds)."""
    return np.tile(np.arange(N, dtype=np.int32), (K, 1)), np.full(K, N, np.int32)


def slots_of(kept):
    """(slot (K, N), index (K, N) with -1 behind the counts, counts (K)) of boolean keep masks (K, N): the compaction in source
    order that mnrf_objects_cull writes."""
    kept = np.asarray(kept, bool)
    K, N = kept.shape
    slot = np.full((K, N), -1, np.int32)
    index = np.full((K, N), -1, np.int32)
    counts = kept.sum(1).astype(np.int32)
    for k in range(K):
        rows = np.nonzero(kept[k])[0]
        slot[k, rows] = np.arange(len(rows))
        index[k, :len(rows)] = rows
    return slot, index, counts
