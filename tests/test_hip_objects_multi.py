"""GPU tests of several placed objects (csrc/mnrf_objects.hip, mirror_nerf_amd/placed_objects.py).

mnrf_objects_cull is held, object by object and bit for bit, to what the single-object kernels write for that object alone on
the same rays (mnrf_object_cull; mnrf_object_rays for an object without bounds): the same device functions decide, so there is
no band of undecided rays and no case is left out.  mnrf_objects_merge is held bit for bit to K successive
mnrf_object_merge_indexed calls AND to the numpy restatement (tests/objects_multi_ref.py).  batched_inference(placed_objects=)
is held to the single-object keywords (K = 1: this inherits fixtures G26 and G27) and to the chain of K single-object passes
(`_object_chain=True`) on the 37 x 53 rays of g12_rays_37x53, chunk 96, two recursion levels.  scripts/eval_scene.py
--objects_json renders two frames with a nerf_pl and a D-NeRF object and is held to the direct call."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import object_cull_ref as CR
from tests import objects_multi_ref as R
from tests.golden import fixtures as FX

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
NEAR = 0.05
SIZES = [0, 1, 65, 1024, 1025, 2500]      # nothing; one ray; a wave and a tail; the compaction block's edge; past it; a partial tail
COUNTS = [1, 2, 3, 8]
SENTINEL = -7.0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


# ----------------------------------------------------------------------------------------------- the cull
SIMILARITY = np.asarray(CR.POSES["similarity"], F32).reshape(3, 4)
TURN = np.array([[0.0, -1.5, 0.0, 0.2], [1.5, 0.0, 0.0, -0.1], [0.0, 0.0, 1.5, 0.3]], F32)


def _grid_bits(res, seed, share):
    rx, ry, rz = res
    cells = np.random.RandomState(seed).uniform(size=(rz, ry, rx)) < share
    return CR.pack_bits(cells).view(np.int32)


# posed and unposed; bits, a box only, no bounds; overlapping boxes (0, 1, 4, 6); one box no ray meets and one grid with no set
# cell (3, 7): their count is 0 unless a non-finite ray is among the rays
OBJECTS = [
    dict(pose=SIMILARITY, scale=1.0, t=(0.0, 0.0, 0.0), lo=(-0.6, -0.6, -0.6), hi=(0.6, 0.6, 0.6), res=(4, 4, 4), bits=("grid", 1, 0.4)),
    dict(pose=None, scale=1.0, t=(0.1, 0.0, 0.0), lo=(-0.3, -0.3, -0.3), hi=(0.9, 0.9, 0.9), res=(1, 1, 1), bits=None),
    dict(pose=TURN, scale=2.0, t=(0.0, 1.0, 0.5), unbounded=True),
    dict(pose=None, scale=1.0, t=(0.0, 0.0, 0.0), lo=(1e5, 1e5, 1e5), hi=(1e5 + 1, 1e5 + 1, 1e5 + 1), res=(1, 1, 1), bits=None),
    dict(pose=None, scale=0.5, t=(0.0, 0.1, 0.0), lo=(-0.5, -0.4, -0.6), hi=(0.7, 0.5, 0.4), res=(33, 5, 7), bits=("grid", 2, 0.3)),
    dict(pose=None, scale=1.0, t=(0.0, 0.0, 0.0), unbounded=True),
    dict(pose=TURN, scale=1.0, t=(0.0, 0.0, 0.0), lo=(-0.8, -0.2, -0.5), hi=(0.2, 0.8, 0.5), res=(1, 1, 1), bits=None),
    dict(pose=SIMILARITY, scale=1.0, t=(0.0, 0.0, 0.0), lo=(-0.6, -0.6, -0.6), hi=(0.6, 0.6, 0.6), res=(4, 4, 4), bits=("zero",)),
]
NAN_ROW, EMPTY_ROW = 1100, 3


def _cull_rays():
    """Rays from a shell around the origin, aimed near it with a spread that lets a good share miss every box; one empty
    segment (far < near) and one NaN ray."""
    rs = np.random.RandomState(11)
    n = SIZES[-1]
    o = rs.normal(size=(n, 3))
    o = o / np.linalg.norm(o, axis=1, keepdims=True) * rs.uniform(2.0, 3.0, (n, 1))
    target = rs.uniform(-1.2, 1.2, (n, 3))
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d, np.full((n, 1), 0.05), rs.uniform(2.0, 8.0, (n, 1))], 1).astype(F32)
    rays[EMPTY_ROW, 6], rays[EMPTY_ROW, 7] = 4.0, 1.0
    rays[NAN_ROW, 4] = np.nan
    return rays


_CULL = {}


def _cull_setup():
    if not _CULL:
        _CULL["rays"] = _cull_rays()
        dev_bits = []
        for o in OBJECTS:
            b = o.get("bits")
            if b is None:
                dev_bits.append(None)
            elif b[0] == "zero":
                dev_bits.append(torch.zeros(o["res"][2], o["res"][1], (o["res"][0] + 31) // 32, dtype=torch.int32, device=DEV))
            else:
                dev_bits.append(_dev(_grid_bits(o["res"], b[1], b[2])))
        _CULL["bits"] = dev_bits
    return _CULL["rays"], _CULL["bits"]


def _pose_c(o):
    return (ctypes.c_float * 12)(*o["pose"].reshape(-1).tolist()) if o["pose"] is not None else None


def _single(o, bits, src, n):
    """What the single-object kernels write for this object alone: (out (n, 8), index (n,), count)."""
    from mirror_nerf_amd import _lib
    p = _lib.ptr
    out = torch.full((n, 8), SENTINEL, dtype=torch.float32, device=DEV)
    if o.get("unbounded"):
        _lib.check(_lib.lib().mnrf_object_rays(p(src), n, _pose_c(o), o["scale"], *o["t"], p(out), _lib.stream()), "mnrf_object_rays")
        return out.cpu().numpy(), np.arange(n, dtype=np.int32), n
    index = torch.full((n,), -3, dtype=torch.int32, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().mnrf_object_cull(p(src), n, _pose_c(o), o["scale"], *o["t"], (ctypes.c_float * 3)(*o["lo"]), (ctypes.c_float * 3)(*o["hi"]),
                                           *o["res"], p(bits), p(out), p(index), p(count), _lib.stream()), "mnrf_object_cull")
    return out.cpu().numpy(), index.cpu().numpy(), int(count.item())


def _fused(objs, bits, src, n):
    from mirror_nerf_amd import _lib
    K = len(objs)
    posed, poses, scales, trans = (ctypes.c_int * K)(), (ctypes.c_float * (12 * K))(), (ctypes.c_float * K)(), (ctypes.c_float * (3 * K))()
    unb, lo, hi, res = (ctypes.c_int * K)(), (ctypes.c_float * (3 * K))(), (ctypes.c_float * (3 * K))(), (ctypes.c_int * (3 * K))()
    tab = (ctypes.c_void_p * K)()
    for k, o in enumerate(objs):
        posed[k] = o["pose"] is not None
        if o["pose"] is not None:
            poses[12 * k:12 * k + 12] = o["pose"].reshape(-1).tolist()
        scales[k] = o["scale"]
        trans[3 * k:3 * k + 3] = o["t"]
        unb[k] = bool(o.get("unbounded"))
        if not o.get("unbounded"):
            lo[3 * k:3 * k + 3], hi[3 * k:3 * k + 3], res[3 * k:3 * k + 3] = o["lo"], o["hi"], o["res"]
            tab[k] = bits[k].data_ptr() if bits[k] is not None else None
    pad = 16                                                       # sentinel elements behind every buffer
    out = torch.full((K * n * 8 + pad,), SENTINEL, dtype=torch.float32, device=DEV)
    index = torch.full((K * n + pad,), -3, dtype=torch.int32, device=DEV)
    slot = torch.full((K * n + pad,), -5, dtype=torch.int32, device=DEV)
    counts = torch.full((K + pad,), 0, dtype=torch.int32, device=DEV)
    counts[K:] = -9
    p = _lib.ptr
    _lib.check(_lib.lib().mnrf_objects_cull(p(src), n, K, posed, poses, scales, trans, unb, lo, hi, res, tab, p(out), p(index), p(slot),
                                            p(counts), _lib.stream()), "mnrf_objects_cull")
    torch.cuda.synchronize()
    out, index, slot, counts = (t.cpu().numpy() for t in (out, index, slot, counts))
    assert (out[K * n * 8:] == SENTINEL).all() and (index[K * n:] == -3).all() and (slot[K * n:] == -5).all() and (counts[K:] == -9).all(), \
        "a sentinel behind a buffer was written"
    return out[:K * n * 8].reshape(K, n, 8), index[:K * n].reshape(K, n), slot[:K * n].reshape(K, n), counts[:K]


@pytest.mark.parametrize("K", COUNTS)
@pytest.mark.parametrize("n", SIZES)
def test_cull_equals_the_single_object_kernels(n, K):
    rays, all_bits = _cull_setup()
    src = _dev(rays[:n])
    picks = [list(range(K))] if K == 8 else [list(range(K)), list(range(8 - K, 8)), [3, 2, 7][:K]]
    for pick in picks:
        objs, bits = [OBJECTS[i] for i in pick], [all_bits[i] for i in pick]
        out, index, slot, counts = _fused(objs, bits, src, n)
        for k, (o, b) in enumerate(zip(objs, bits)):
            w_out, w_index, w_count = _single(o, b, src, n)
            c = int(counts[k])
            assert c == w_count, (pick, k, c, w_count)
            assert np.array_equal(index[k, :c], w_index[:c]), (pick, k)
            assert _same_bits(out[k, :c], w_out[:c]), (pick, k)
            want_slot = np.full(n, -1, np.int32)
            want_slot[w_index[:c]] = np.arange(c, dtype=np.int32)
            assert np.array_equal(slot[k], want_slot), (pick, k)
            # what the case is there for
            finite = np.isfinite(rays[:n]).all(1)
            if o.get("unbounded"):
                assert c == n
            elif pick[k] in (3, 7):
                assert c == int((~finite).sum())                      # nothing but the NaN ray, once it is among the rays
            elif n >= 1024:
                assert 0.03 * n < c < 0.95 * n, (pick, k, c)
                assert not np.isin(EMPTY_ROW, index[k, :c]) and (n <= NAN_ROW or np.isin(NAN_ROW, index[k, :c]))
        assert _same_bits(src.cpu().numpy(), rays[:n]), "the source rays were written"
    if n == SIZES[-1] and K == 8:
        kept = [set(index[k, :counts[k]].tolist()) for k in (0, 1)]
        assert kept[0] & kept[1] and kept[1] - kept[0]                                # the boxes overlap, and differ


# ----------------------------------------------------------------------------------------------- the merge
SCALES = [2.0, 1.0, 3.0, 4.0, 0.5, 3.0, 1.0, 2.0]
POSE_SCALES = [1.0, 0.5, 0.7, 2.0, 1.0, 1.3, 1.0, 0.25]
EXACT = [0, 1, 3, 4, 6, 7]               # powers of two: obj_depth = d * scale * pose_scale0 divides back to d exactly


def _merge_inputs(n, K, seed):
    """Ray-space maps of every object (rows 0..47 by hand, the rest random), then gathered into each object's kept rows."""
    rs = np.random.RandomState(seed)
    depth = rs.uniform(-0.2, 3.0, n).astype(F32)
    rgb = rs.uniform(0, 1, (n, 3)).astype(F32)
    mask = rs.uniform(0, 1, n).astype(F32)
    kept = rs.uniform(size=(K, n)) < rs.uniform(0.3, 0.9, (K, 1))
    full = []
    for k in range(K):
        sp = F32(SCALES[k]) * F32(POSE_SCALES[k])
        full.append(dict(rgb=rs.uniform(0, 1, (n, 3)).astype(F32), depth=(rs.uniform(-0.5, 4.0, n).astype(F32) * sp).astype(F32),
                         op=rs.choice(np.array([0.5, 0.8, 0.85, 0.95, 1.0], F32), n), sp=sp))
    if n >= 65:
        kept[:, :48] = True
        kept[:, 60:65] = False                                      # rows no object lists
        depth[0:48] = 3.0
        for k in range(K):
            f = full[k]
            f["op"][0:48] = 1.0
            f["depth"][0:8] = F32(1.5 if k in EXACT else 2.5) * f["sp"]      # a tie of every exact object at d = 1.5, the others behind
            f["depth"][8:16] = F32(2.0 + 0.125 * k) * f["sp"]        # d == the scene's depth for object 0 (below)
            f["depth"][16:24] = F32(3.5 - 0.25 * k) * f["sp"]        # behind a scene depth == near: nothing hides
            f["depth"][24:28] = (F32(0.03) if k == 0 else F32(2.0 + k)) * f["sp"]        # object 0 below near, the others farther
            f["depth"][28:32] = F32(1.0 + k) * f["sp"]
            f["op"][28:32] = F32(0.8) if k % 2 == 0 else np.nextafter(F32(0.8), F32(1))  # exactly the threshold / one ulp above
            f["depth"][32:36] = F32(1.0 + 0.5 * k) * f["sp"]
        depth[8:16] = 2.0
        depth[16:24] = F32(NEAR)
        full[0]["depth"][32] = np.nan
        full[K - 1]["op"][33] = np.nan
        depth[34] = np.nan
        full[0]["rgb"][35, 1] = np.nan
        rgb[36, 0] = np.nan
        mask[37] = np.nan
        depth[38] = F32(NEAR)                                        # depth at near against the random rows of the objects
        depth[39] = np.nextafter(F32(NEAR), F32(1))
    elif n == 1:
        kept[:, 0] = True
        depth[0] = 3.0
        for k in range(K):
            full[k]["depth"][0], full[k]["op"][0] = F32(1.5) * full[k]["sp"], 1.0
    slot, index, counts = R.slots_of(kept)
    maps = []
    for k in range(K):
        rows = index[k, :counts[k]]
        tail = 3                                                     # rows behind the count, never to be read as rows to merge
        maps.append(tuple(np.concatenate([full[k][key][rows], np.full((tail,) + full[k][key].shape[1:], 0.9, F32)])
                          for key in ("rgb", "depth", "op")))
    return maps, slot, index, counts, rgb, depth, mask


def _merge_fused(maps, given, slot, counts, cap, lvl, with_mask, K):
    from mirror_nerf_amd import _lib
    n = slot.shape[1]
    tabs = [(ctypes.c_void_p * K)() for _ in range(3)]
    hold = []
    for k in range(K):
        if given[k]:
            for tab, a in zip(tabs, maps[k]):
                hold.append(_dev(a))
                tab[k] = hold[-1].data_ptr()
    t = [_dev(a) for a in lvl]
    used = torch.zeros(K + 4, dtype=torch.int32, device=DEV)
    used[K:] = -9
    p = _lib.ptr
    d_slot, d_counts = _dev(slot), _dev(counts)
    _lib.check(_lib.lib().mnrf_objects_merge(*tabs, K, p(d_slot), p(d_counts), n, cap, (ctypes.c_float * K)(*SCALES[:K]),
                                             (ctypes.c_float * K)(*POSE_SCALES[:K]), NEAR, p(t[0]), p(t[1]), p(t[2]) if with_mask else None,
                                             p(used), _lib.stream()), "mnrf_objects_merge")
    torch.cuda.synchronize()
    used = used.cpu().numpy()
    assert (used[K:] == -9).all()
    return [a.cpu().numpy() for a in t], used[:K]


def _merge_chain(maps, given, index, counts, cap, lvl, with_mask, K):
    from mirror_nerf_amd import _lib
    t = [_dev(a) for a in lvl]
    used = torch.zeros(K, dtype=torch.int32, device=DEV)
    p = _lib.ptr
    for k in range(K):
        if not given[k] or cap == 0:
            continue
        m = [_dev(a) for a in maps[k]]
        d_index, d_count = _dev(np.maximum(index[k], 0)), _dev(counts[k:k + 1])
        _lib.check(_lib.lib().mnrf_object_merge_indexed(p(m[0]), p(m[1]), p(m[2]), p(d_index), p(d_count), cap,
                                                        SCALES[k], POSE_SCALES[k], NEAR, p(t[0]), p(t[1]), p(t[2]) if with_mask else None,
                                                        p(used[k:k + 1]), _lib.stream()), "mnrf_object_merge_indexed")
    torch.cuda.synchronize()
    return [a.cpu().numpy() for a in t], used.cpu().numpy()


@pytest.mark.parametrize("K", COUNTS)
@pytest.mark.parametrize("n", SIZES)
def test_merge_equals_the_chain_and_the_restatement(n, K):
    maps, slot, index, counts, rgb, depth, mask = _merge_inputs(n, K, seed=100 + n + K)
    lvl = (rgb, depth, mask)
    variants = [(True, [True] * K, n)]
    if n == 1025:
        variants += [(False, [True] * K, n), (True, [k != 1 for k in range(K)], n), (True, [True] * K, 100)]      # null mask; a null entry; a clipping capacity
        variants += [(True, [False] * K, n)]
    for with_mask, given, cap in variants:
        (g_rgb, g_depth, g_mask), g_used = _merge_fused(maps, given, slot, counts, cap, lvl, with_mask, K)
        (c_rgb, c_depth, c_mask), c_used = _merge_chain(maps, given, index, counts, cap, lvl, with_mask, K)
        obj = [[m[i] if given[k] else None for k, m in enumerate(maps)] for i in range(3)]
        r_rgb, r_depth, r_mask, r_used = R.merge_objects(*obj, slot, counts, cap, SCALES[:K], POSE_SCALES[:K], NEAR, rgb, depth,
                                                         mask if with_mask else None)
        what = (n, K, with_mask, given, cap)
        assert _same_bits(g_rgb, c_rgb) and _same_bits(g_depth, c_depth) and _same_bits(g_mask, c_mask), what
        assert np.array_equal(g_used, c_used), (what, g_used, c_used)
        assert _same_bits(g_rgb, r_rgb) and _same_bits(g_depth, r_depth) and _same_bits(g_mask, r_mask if with_mask else mask), what
        assert np.array_equal(g_used, r_used), (what, g_used, r_used)
        unlisted = (slot < 0).all(0) if n else np.zeros(0, bool)
        assert _same_bits(g_rgb[unlisted], rgb[unlisted]) and _same_bits(g_depth[unlisted], depth[unlisted]) and _same_bits(g_mask[unlisted], mask[unlisted])
        if n >= 65 and all(given) and cap == n:
            assert unlisted[60:65].all() and 0 < g_used.sum()
            taken = lambda r: (_bits(g_rgb[r]) != _bits(rgb[r])).any()  # noqa: E731
            last_exact = max(k for k in EXACT if k < K)
            assert _same_bits(g_rgb[0:8], maps[last_exact][0][slot[last_exact, 0:8]])           # the tie: the later object
            assert (g_depth[0:8] == F32(1.5)).all()
            assert (g_depth[8:16] == F32(2.0)).all() and _same_bits(g_rgb[8:16], maps[0][0][slot[0, 8:16]])      # d == depth: taken; the farther ones hidden
            assert all(taken(r) for r in range(16, 24))                                           # scene at near: nothing hides
            if K > 1:
                assert (g_depth[24:28] > 1.0).all() and g_used[0] >= 4                           # object 0 below near was taken, then replaced
            else:
                assert (g_depth[24:28] < NEAR).all()
            if K == 1:
                assert not any(taken(r) for r in range(28, 32))                                   # opacity exactly 0.8: no object
            else:
                assert (g_depth[28:32] == F32(2.0)).all()                                         # ... one ulp above: object 1
            assert g_depth[32] != F32(1.0) and (K > 1 or not taken(32))                          # a NaN depth never counts
            assert np.isnan(g_rgb[35, 1])                                                         # a NaN colour of the nearest object is copied as it is
        if not any(given) or n == 0:
            assert _same_bits(g_rgb, rgb) and _same_bits(g_depth, depth) and g_used.sum() == 0


# ----------------------------------------------------------------------------------------------- batched_inference
CHUNK = 96
_PIPE = {}


def _pipe():
    """Scene models (the random-init weights of fixture G26's office case), the nerf_pl object of G26 and the D-NeRF object of
    G27 with their placements, and the 37 x 53 rays; two boxes of 0.6 scene units, each around a point three scene units down a ray
    near the centre of the image, ten pixels apart: each is met by about a fifth of the primary rays, and they overlap."""
    if _PIPE:
        return SimpleNamespace(**_PIPE)
    import mirror_nerf_amd as M
    from mirror_nerf_amd import recursion
    from tests import test_hip_dnerf as TD
    from tests import test_hip_objects as TO
    g26, g27 = FX.Fixture("g26_object_office_l2"), FX.Fixture("g27_dnerf_office_l2")
    sds = g26.state_dicts()
    _PIPE["models"] = {"coarse": TO._module(sds[0]), "fine": TO._module(sds[1])}
    _PIPE["emb"] = TO._emb()
    _PIPE["args"] = dict(g26.meta["args"], max_recursive_level=2)
    _PIPE["rays"] = _dev(FX.Fixture("g12_rays_37x53").outputs["rays"])
    assert _PIPE["rays"].shape == (37 * 53, 8)
    _PIPE["field_a"], _PIPE["place_a"] = TO._object_system(g26.meta), g26.meta["new_object"]
    _PIPE["field_b"], _PIPE["place_b"], _PIPE["time_b"] = TD._object_kwargs(g27.meta), g27.meta["new_object"], g27.meta["frame_time"]
    rays = _PIPE["rays"].cpu().numpy().astype(np.float64)
    for name, place, row, half in (("a", _PIPE["place_a"], 18 * 53 + 20, 0.3), ("b", _PIPE["place_b"], 18 * 53 + 30, 0.3)):
        x = recursion.resolve_new_object(None, place)
        q = CR.object_rays64(rays[row:row + 1], np.asarray(x["pose"]).reshape(3, 4) if x["pose"] is not None else None, x["scale"],
                             x["translation"])[0].astype(np.float64)
        centre = q[:3] + q[3:6] * 3.0 * x["scale"] * x["pose_scale0"]
        _PIPE["box_" + name] = M.ObjectBounds(centre - half * x["scale"], centre + half * x["scale"])
    return SimpleNamespace(**_PIPE)


def _run(key, **kw):
    """batched_inference on the shared scene -> (maps as numpy, object_used as a list or None); cached under `key`."""
    if key in _PIPE.get("runs", {}):
        return _PIPE["runs"][key]
    import mirror_nerf_amd as M
    P = _pipe()
    n_used = kw.pop("n_used", None)
    used = torch.full((n_used,), 77, dtype=torch.int32, device=DEV) if n_used else None
    args = dict(P.args, **kw.pop("args", {}))
    out = M.batched_inference(P.models, P.emb, P.rays, 64, 64, False, CHUNK, args=args, trace_secondary_rays=True, to_cpu=False, maps_only=True,
                              object_used=used, **kw)
    got = {k: v.detach().cpu().numpy() for k, v in out.items()}, (used.cpu().tolist() if used is not None else None)
    _PIPE.setdefault("runs", {})[key] = got
    return got


def _same(a, b):
    assert set(a) == set(b), set(a) ^ set(b)
    assert {"rgb_fine", "depth_fine", "mirror_mask_fine", "rgb_fine_reflect", "depth_fine_reflect", "x_surface_fine"} <= set(a)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def _objects(P, bounded):
    import mirror_nerf_amd as M
    a = M.PlacedObject(P.field_a, P.place_a, bounds=P.box_a if bounded else None)
    b = M.PlacedObject(P.field_b, P.place_b, bounds=P.box_b if bounded else None, time=0.8)      # its own phase, not the call's
    return a, b


def test_the_boxes_cut_the_primary_rays():
    from mirror_nerf_amd import recursion
    P = _pipe()
    for box, place in ((P.box_a, P.place_a), (P.box_b, P.place_b)):
        count = int(box.cull(P.rays, recursion.resolve_new_object(None, place))[2].item())
        print("kept primary rays:", count, "of", P.rays.shape[0])
        assert 0.05 * P.rays.shape[0] < count < 0.5 * P.rays.shape[0]


@pytest.mark.parametrize("bounded", [True, False], ids=["bounds", "no_bounds"])
def test_one_nerf_pl_object_equals_the_single_object_keywords(bounded):
    import mirror_nerf_amd as M
    P = _pipe()
    legacy, n_legacy = _run(("legacy_a", bounded), args=dict(obj_model_type="nerf_pl"), system_obj=P.field_a, new_object=P.place_a,
                            object_bounds=P.box_a if bounded else None, n_used=1)
    got, n_got = _run(("a", bounded), placed_objects=[M.PlacedObject(P.field_a, P.place_a, bounds=P.box_a if bounded else None)], n_used=1)
    print("rays that took the object:", n_got)
    assert n_got == n_legacy and n_got[0] > 0
    _same(legacy, got)
    if bounded:                                                      # the scene, its mirrors and the object are all in the frame
        off, _ = _run("off", args=dict(app_reflect_newly_placed_objects=False))
        changed = (got["depth_fine"] != off["depth_fine"])
        assert 0 < changed.sum() < changed.size and (got["rgb_fine_reflect"] != 0).any()


def test_one_dnerf_object_equals_the_single_object_keywords():
    import mirror_nerf_amd as M
    P = _pipe()
    legacy, n_legacy = _run("legacy_b", args=dict(obj_model_type="d_nerf"), render_kwargs_test_d_nerf=P.field_b, new_object=P.place_b,
                            frame_time=P.time_b, object_bounds=P.box_b, n_used=1)
    got, n_got = _run("b", placed_objects=[M.PlacedObject(P.field_b, P.place_b, bounds=P.box_b)], frame_time=P.time_b, n_used=1)
    own, n_own = _run("b_own_time", placed_objects=[M.PlacedObject(P.field_b, P.place_b, bounds=P.box_b, time=P.time_b)], n_used=1)
    print("rays that took the object:", n_got)
    assert n_got == n_legacy == n_own and n_got[0] > 0
    _same(legacy, got)
    _same(legacy, own)


@pytest.mark.parametrize("bounded", [True, False], ids=["bounds", "no_bounds"])
def test_two_objects_equal_the_chain(bounded):
    P = _pipe()
    fused, n_fused = _run(("ab", bounded), placed_objects=list(_objects(P, bounded)), n_used=2)
    chain, n_chain = _run(("ab_chain", bounded), placed_objects=list(_objects(P, bounded)), _object_chain=True, n_used=2)
    print("rays that took the objects:", n_fused)
    assert n_fused == n_chain and min(n_fused) > 0
    _same(chain, fused)
    if bounded:
        one, _ = _run(("a", True), placed_objects=[_objects(P, True)[0]], n_used=1)
        assert (fused["depth_fine"] != one["depth_fine"]).any()      # the second object is in the frame


def test_an_object_with_no_set_cell_changes_nothing():
    import mirror_nerf_amd as M
    P = _pipe()
    a = _objects(P, True)[0]
    empty = M.PlacedObject(P.field_b, P.place_b, bounds=M.ObjectBounds(P.box_b.lo, P.box_b.hi, (4, 4, 4), torch.zeros(16, dtype=torch.int32)),
                           time=0.8)
    one, n_one = _run(("a", True), placed_objects=[a], n_used=1)
    got, n_got = _run("a_empty", placed_objects=[a, empty], n_used=2)
    assert n_got == [n_one[0], 0]
    _same(one, got)


def test_the_same_object_twice_is_the_object_once():
    P = _pipe()
    a = _objects(P, True)[0]
    one, n_one = _run(("a", True), placed_objects=[a], n_used=1)
    got, n_got = _run("aa", placed_objects=[a, a], n_used=2)
    assert n_got == [n_one[0], n_one[0]] and n_one[0] > 0
    _same(one, got)


def test_object_used_of_one_element_is_the_total():
    P = _pipe()
    per_object = _run(("ab", True), placed_objects=list(_objects(P, True)), n_used=2)[1]
    total = _run("ab_total", placed_objects=list(_objects(P, True)), n_used=1)[1]
    assert total == [sum(per_object)] and total[0] > 0


# ----------------------------------------------------------------------------------------------- scripts/eval_scene.py
def test_eval_scene_with_two_objects(tmp_path):
    """scripts/eval_scene.py --objects_json end to end on a Blender-layout directory of 2 frames of 8 x 8 with a nerf_pl object
    in a box and a D-NeRF object at time 0.25 + 0.5 * i / 2: the frames are those of the direct
    batched_inference(placed_objects=) call, and both objects are in them."""
    import json
    from PIL import Image
    import mirror_nerf_amd as M
    from mirror_nerf_amd import checkpoint
    from mirror_nerf_amd import synthetic as SY
    from mirror_nerf_amd.data import RayBank
    from mirror_nerf_amd.dnerf import load_dnerf_object
    from mirror_nerf_amd.recursion import load_object_system
    from tests import test_hip_dnerf as TD
    from tests import test_hip_objects as TO
    root = tmp_path / "office"
    (root / "test").mkdir(parents=True)
    rng = np.random.default_rng(0)
    frames_meta = []
    for i, eye in enumerate(((0.0, -4.0, 1.5), (1.0, -3.5, 2.0))):
        Image.fromarray(rng.integers(0, 256, size=(8, 8, 3), dtype=np.uint8)).save(root / "test" / f"r_{i}.png")
        pose = np.eye(4)
        pose[:3, :4] = SY.look_at_pose(eye=eye)
        frames_meta.append({"file_path": f"./test/r_{i}", "transform_matrix": pose.tolist()})
    with open(root / "transforms_test.json", "w") as f:
        json.dump({"camera_angle_x": SY.CAMERA_ANGLE_X, "frames": frames_meta}, f)
    models = SY.build_models(DEV, SY.STRADDLE, seed=0)[0]
    ckpt = tmp_path / "last.ckpt"
    checkpoint.save_ckpt(str(ckpt), SimpleNamespace(nerf_coarse=models["coarse"], nerf_fine=models["fine"]))
    g26, g27 = FX.Fixture("g26_object_office_l2").meta, FX.Fixture("g27_dnerf_office_l2").meta
    torch.save({"state_dict": {f"nerf_{n}.{k}": torch.from_numpy(v) for n, sd in zip(("coarse", "fine"), TO._object_sds(g26))
                               for k, v in sd.items()}}, str(tmp_path / "object.ckpt"))
    okw = TD._object_kwargs(g27)
    obj_dir = tmp_path / "logs" / "object"
    obj_dir.mkdir(parents=True)
    torch.save({"global_step": 1, "network_fn_state_dict": {k: v.cpu() for k, v in okw["network_fn"].state_dict().items()},
                "network_fine_state_dict": {k: v.cpu() for k, v in okw["network_fine"].state_dict().items()}}, str(obj_dir / "000001.tar"))
    (obj_dir / "config.txt").write_text("expname = object\nnerf_type = direct_temporal\nuse_viewdirs = True\nN_samples = 64\n"
                                        "N_importance = 64\nuse_two_models_for_fine = True\n")
    box = [-1e3, -1e3, -1e3, 1e3, 1e3, 1e3]
    entries = [dict(ckpt_path="object.ckpt", model_type="nerf_pl", bounds=box, **{k: g26["new_object"][k] for k in ("pose_align", "scale", "translation")}),
               dict(ckpt_path=str(obj_dir / "000001.tar"), model_type="d_nerf", time_offset=0.25, time_scale=0.5,
                    **{k: g27["new_object"][k] for k in ("pose_align", "scale", "translation")})]
    spec = tmp_path / "objects.json"
    spec.write_text(json.dumps(entries))
    out = tmp_path / "results"
    argv = ["--root_dir", str(root), "--split", "test", "--img_wh", "8", "8", "--ckpt_path", str(ckpt), "--N_samples", "64",
            "--N_importance", "64", "--chunk", "32768", "--trace_secondary_rays", "--near", str(SY.NEAR), "--far", str(SY.FAR),
            "--out_dir", str(out)]
    app = ["--app_reflect_newly_placed_objects", "--objects_json", str(spec)]
    ES = TO._load_script("eval_scene")
    assert ES.main(argv + app) == 0
    args = ES.get_opts(argv + app)
    system = ES.load_system(args, torch.device(DEV))
    a = load_object_system(str(tmp_path / "object.ckpt"), torch.device(DEV), 64)
    b = load_dnerf_object(str(obj_dir / "000001.tar"), torch.device(DEV))
    bank = RayBank.from_blender(str(root), "test", (8, 8), SY.NEAR, SY.FAR, device=torch.device(DEV))
    total = np.zeros(2, np.int64)
    for i in range(2):
        rays = bank.frame(i)["rays"]
        used = torch.zeros(2, dtype=torch.int32, device=DEV)
        placed = [M.PlacedObject(a, g26["new_object"], bounds=M.ObjectBounds(box[:3], box[3:])),
                  M.PlacedObject(b, g27["new_object"], time=0.25 + 0.5 * i / 2)]
        res = M.batched_inference(system.models, system.embeddings, rays, 64, 64, False, 32768, args=args, trace_secondary_rays=True,
                                  white_back=False, to_cpu=False, maps_only=True, placed_objects=placed, object_used=used)
        images = M.finish_frame(res, "fine")
        png = np.asarray(Image.open(out / f"rgb_fine_{i:03d}.png"))
        assert png.shape == (8, 8, 3) and (png.reshape(64, 3) == images["rgb_fine"].cpu().numpy()).all()
        png = np.asarray(Image.open(out / "depth" / f"depth_fine_{i:03d}.png"))
        assert (png.reshape(64, 3) == images["depth_fine"].cpu().numpy()).all()
        total += used.cpu().numpy()
    assert (total > 0).all(), f"rays that took the objects over the two frames: {total}"
    # a time that leaves [0, 1] is refused before anything is rendered
    entries[1]["time_scale"] = 2.0
    spec.write_text(json.dumps(entries))
    late = tmp_path / "late"
    with pytest.raises(SystemExit, match="outside \\[0, 1\\]"):
        ES.main(argv[:-1] + [str(late)] + app)
    assert not late.exists()
