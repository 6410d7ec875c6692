"""CPU-side checks of several placed objects (mirror_nerf_amd/placed_objects.py, csrc/mnrf_objects.hip): the numpy restatement
of the K-object merge (tests/objects_multi_ref.py) against the property it must have and against hand-worked opposite cases,
the argument validation of the two C entry points (it happens before any launch), every refusal of `placed_objects=`, and the
single-object refusals of batched_inference as they were."""
import ctypes
import itertools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import objects_multi_ref as R

F32 = np.float32
NEAR = 0.05


# ----------------------------------------------------------------------------------------------- the restatement: a property
def _property_inputs(N, K, seed):
    """Every depth, scene and objects, in [0.5, 4] and no two equal on a ray; scales and pose scales are powers of two, so the
    two divisions are exact and the drawn depth IS d.  Part of the objects are not opaque, part of the rays not listed."""
    rs = np.random.RandomState(seed)
    scales = [F32(2.0 ** rs.randint(-1, 3)) for _ in range(K)]
    ps0 = [F32(2.0 ** rs.randint(-1, 2)) for _ in range(K)]
    while True:
        depths = rs.uniform(0.5, 4.0, (K + 1, N)).astype(F32)            # row 0: the scene
        srt = np.sort(depths, 0)
        if (np.diff(srt, axis=0) > 0).all():
            break
    kept = rs.uniform(size=(K, N)) < 0.7
    slot, index, counts = R.slots_of(kept)
    obj_rgb, obj_depth, obj_op, d_of = [], [], [], np.full((K, N), np.nan, F32)
    for k in range(K):
        rows = index[k, :counts[k]]
        m = len(rows) + 3                                                # (rows behind the count: never read as rows to merge)
        rgb = rs.uniform(0, 1, (m, 3)).astype(F32)
        dep = np.full(m, 0.75, F32)
        dep[:len(rows)] = depths[k + 1, rows] * scales[k] * ps0[k]
        op = rs.choice(np.array([0.5, 0.8, 0.81, 0.95, 1.0], F32), m)
        obj_rgb.append(rgb), obj_depth.append(dep), obj_op.append(op)
        d_of[k, rows] = (dep[:len(rows)] / scales[k]) / ps0[k]
    scene = dict(rgb=rs.uniform(0, 1, (N, 3)).astype(F32), depth=depths[0].copy(), mask=rs.uniform(0, 1, N).astype(F32))
    return dict(obj_rgb=obj_rgb, obj_depth=obj_depth, obj_op=obj_op, slot=slot, index=index, counts=counts, scales=scales, ps0=ps0,
                scene=scene, d_of=d_of, depths=depths)


def _run_ref(inp, order):
    o = list(order)
    return R.merge_objects([inp["obj_rgb"][k] for k in o], [inp["obj_depth"][k] for k in o], [inp["obj_op"][k] for k in o],
                           inp["slot"][o], inp["counts"][o], inp["slot"].shape[1], [inp["scales"][k] for k in o],
                           [inp["ps0"][k] for k in o], NEAR, inp["scene"]["rgb"], inp["scene"]["depth"], inp["scene"]["mask"])


@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_nearest_counted_object_wins_whatever_the_order(K):
    N = 400
    inp = _property_inputs(N, K, seed=K)
    # the conditions of the test, for every ray: all depths in [0.5, 4] (so every depth is valid: > near) and distinct
    d_all = np.concatenate([inp["scene"]["depth"][None], inp["d_of"]])
    listed = ~np.isnan(d_all)
    assert np.array_equal(inp["d_of"][listed[1:]], inp["depths"][1:][listed[1:]])          # the divisions were exact
    assert ((d_all[listed] >= F32(0.5)) & (d_all[listed] <= F32(4.0))).all() and NEAR < 0.5
    for r in range(N):
        col = d_all[:, r][listed[:, r]]
        assert len(np.unique(col)) == len(col), r
    # what the rule must give: the nearest counted object, where it is not behind the (valid) scene depth
    want_rgb, want_depth, want_mask = (inp["scene"][k].copy() for k in ("rgb", "depth", "mask"))
    took = 0
    for r in range(N):
        best = None
        for k in range(K):
            s = inp["slot"][k, r]
            if s < 0 or not inp["obj_op"][k][s] > F32(0.8):
                continue
            if best is None or inp["d_of"][k, r] < inp["d_of"][best, r]:
                best = k
        if best is not None and not inp["d_of"][best, r] > inp["scene"]["depth"][r]:
            want_rgb[r], want_depth[r], want_mask[r] = inp["obj_rgb"][best][inp["slot"][best, r]], inp["d_of"][best, r], 0.0
            took += 1
    assert N // 10 < took < N - N // 10 or K == 8                                          # both outcomes occur
    orders = [tuple(range(K)), tuple(reversed(range(K)))] + [tuple(np.random.RandomState(s).permutation(K)) for s in range(3)]
    if K <= 3:
        orders = list(itertools.permutations(range(K)))
    for order in orders:
        rgb, depth, mask, n_used = _run_ref(inp, order)
        assert np.array_equal(rgb, want_rgb) and np.array_equal(depth, want_depth) and np.array_equal(mask, want_mask), order
        assert n_used.sum() >= took
    # the scene's maps were not written
    assert inp["scene"]["depth"].tobytes() == inp["depths"][0].tobytes()


# ----------------------------------------------------------------------------------------------- the opposite cases, by hand
def _hand(obj, scene_depth, scales=None, ps0=None, slot=None):
    """obj: per object (rgb value, depth, opacity) on ONE ray -> (rgb[0, 0], depth[0], mask[0], n_used)."""
    K = len(obj)
    rgb = [np.full((1, 3), o[0], F32) for o in obj]
    dep = [np.array([o[1]], F32) for o in obj]
    op = [np.array([o[2]], F32) for o in obj]
    slot_, counts = R.identity_slots(K, 1)
    out = R.merge_objects(rgb, dep, op, slot_ if slot is None else slot, counts, 1, scales or [1.0] * K, ps0 or [1.0] * K, NEAR,
                          np.full((1, 3), 0.25, F32), np.array([scene_depth], F32), np.array([0.7], F32))
    return float(out[0][0, 0]), float(out[1][0]), float(out[2][0]), out[3].tolist()


def test_a_tie_goes_to_the_later_object():
    assert _hand([(0.5, 2.0, 1.0), (0.75, 2.0, 1.0)], 3.0) == (0.75, 2.0, 0.0, [1, 1])
    assert _hand([(0.75, 2.0, 1.0), (0.5, 2.0, 1.0)], 3.0) == (0.5, 2.0, 0.0, [1, 1])
    # ... a tie with the scene too: d == depth is not "behind"
    assert _hand([(0.5, 3.0, 1.0)], 3.0) == (0.5, 3.0, 0.0, [1])
    # the tie is one of d, after the divisions: 4 / 2 / 1 == 1 / 1 / 0.5
    assert _hand([(0.5, 4.0, 1.0), (0.75, 1.0, 1.0)], 3.0, scales=[2.0, 1.0], ps0=[1.0, 0.5]) == (0.75, 2.0, 0.0, [1, 1])


def test_an_object_at_or_below_near_hides_nothing():
    # object 0 at d = 0.03 <= near is opaque and taken; the depth it leaves is not valid, so the farther object 1 replaces it
    assert _hand([(0.5, 0.03, 1.0), (0.75, 2.0, 1.0)], 3.0) == (0.75, 2.0, 0.0, [1, 1])
    assert _hand([(0.5, NEAR, 1.0), (0.75, 2.0, 1.0)], 3.0) == (0.75, 2.0, 0.0, [1, 1])
    # the other order: the near object comes last and stays
    got = _hand([(0.75, 2.0, 1.0), (0.5, 0.03, 1.0)], 3.0)
    assert got[0] == 0.5 and got[1] == float(F32(0.03)) and got[3] == [1, 1]
    # just above near it hides as any depth does
    above = float(np.nextafter(F32(NEAR), F32(1)))
    got = _hand([(0.5, above, 1.0), (0.75, 2.0, 1.0)], 3.0)
    assert got[0] == 0.5 and got[3] == [1, 0]


def test_a_nan_never_counts():
    nan = float("nan")
    assert _hand([(0.5, nan, 1.0), (0.75, 2.0, 1.0)], 3.0) == (0.75, 2.0, 0.0, [0, 1])
    assert _hand([(0.5, 1.0, nan), (0.75, 2.0, 1.0)], 3.0) == (0.75, 2.0, 0.0, [0, 1])
    assert _hand([(0.5, nan, 1.0), (0.75, 1.0, nan)], 3.0) == (0.25, 3.0, float(F32(0.7)), [0, 0])
    # not opaque (exactly 0.8), no depth, a negative depth: no object either
    assert _hand([(0.5, 1.0, 0.8), (0.5, 0.0, 1.0), (0.5, -1.0, 1.0)], 3.0) == (0.25, 3.0, float(F32(0.7)), [0, 0, 0])
    # a ray that an object's list does not hold, and an object that was not rendered
    assert _hand([(0.5, 1.0, 1.0), (0.75, 2.0, 1.0)], 3.0, slot=np.array([[-1], [0]], np.int32)) == (0.75, 2.0, 0.0, [0, 1])
    slot, counts = R.identity_slots(2, 1)
    out = R.merge_objects([None, np.full((1, 3), 0.75, F32)], [None, np.array([2.0], F32)], [None, np.array([1.0], F32)], slot, counts, 1,
                          [1.0, 1.0], [1.0, 1.0], NEAR, np.full((1, 3), 0.25, F32), np.array([3.0], F32), None)
    assert out[1][0] == 2.0 and out[2] is None and out[3].tolist() == [0, 1]


def test_a_scene_depth_at_or_below_near_hides_nothing():
    for scene in (0.01, NEAR, 0.0, -1.0):
        assert _hand([(0.5, 3.0, 1.0)], scene) == (0.5, 3.0, 0.0, [1]), scene
    assert _hand([(0.5, 3.0, 1.0)], 1.0) == (0.25, 1.0, float(F32(0.7)), [0])              # a valid, nearer scene depth does
    # ... and then the nearest object still wins among those that follow
    assert _hand([(0.5, 3.0, 1.0), (0.75, 2.0, 1.0), (0.6, 2.5, 1.0)], 0.01) == (0.75, 2.0, 0.0, [1, 1, 0])


def test_a_count_or_capacity_clips_the_list():
    rgb = [np.arange(12, dtype=F32).reshape(4, 3) / 16]
    dep, op = [np.full(4, 1.0, F32)], [np.ones(4, F32)]
    slot = np.array([[0, 1, 2, 3]], np.int32)
    lvl = (np.zeros((4, 3), F32), np.full(4, 3.0, F32), None)
    assert R.merge_objects(rgb, dep, op, slot, [2], 4, [1.0], [1.0], NEAR, *lvl)[1].tolist() == [1.0, 1.0, 3.0, 3.0]
    assert R.merge_objects(rgb, dep, op, slot, [4], 3, [1.0], [1.0], NEAR, *lvl)[1].tolist() == [1.0, 1.0, 1.0, 3.0]
    assert R.merge_objects(rgb, dep, op, slot, [-2], 4, [1.0], [1.0], NEAR, *lvl)[3].tolist() == [0]


# ----------------------------------------------------------------------------------------------- the C ABI
@pytest.fixture(scope="module")
def L():
    from mirror_nerf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _cull_args(K=1, **over):
    a = dict(rays=None, n=0, K=K, posed=(ctypes.c_int * 8)(), poses=(ctypes.c_float * 96)(), scales=(ctypes.c_float * 8)(*[1.0] * 8),
             trans=(ctypes.c_float * 24)(), unbounded=(ctypes.c_int * 8)(), lo=(ctypes.c_float * 24)(), hi=(ctypes.c_float * 24)(*[1.0] * 24),
             res=(ctypes.c_int * 24)(*[1] * 24), bits=(ctypes.c_void_p * 8)(), out=None, index=None, slot=None, counts=None, stream=None)
    a.update(over)
    return list(a.values())


def test_objects_cull_validates_its_arguments(L):
    from mirror_nerf_amd import _lib
    assert _lib.MNRF_OBJECTS_MAX == 8
    assert L.mnrf_objects_cull(*_cull_args()) == 0                                      # zero rays: a no-op
    for K in (0, 9, -1):
        assert L.mnrf_objects_cull(*_cull_args(K=K)) < 0 and b"1..8" in L.mnrf_last_error()
    for n in (-1, 2 ** 31):
        assert L.mnrf_objects_cull(*_cull_args(n=n)) < 0 and b"bad size" in L.mnrf_last_error()
    for name in ("posed", "poses", "scales", "trans", "unbounded", "lo", "hi", "res", "bits"):
        assert L.mnrf_objects_cull(*_cull_args(**{name: None})) < 0 and b"host array is null" in L.mnrf_last_error(), name
    bad_lo = (ctypes.c_float * 24)()
    bad_lo[3 + 1] = 1.0                                                                 # object 1: lo == hi on y
    assert L.mnrf_objects_cull(*_cull_args(K=2, lo=bad_lo)) < 0 and b"lo < hi" in L.mnrf_last_error()
    assert L.mnrf_objects_cull(*_cull_args(K=1, lo=bad_lo)) == 0                        # (object 1 is not read at K = 1)
    unb = (ctypes.c_int * 8)(0, 1)
    assert L.mnrf_objects_cull(*_cull_args(K=2, lo=bad_lo, unbounded=unb)) == 0         # an object without bounds: its box is not read
    bad_res = (ctypes.c_int * 24)(*[1] * 24)
    bad_res[2] = 1025
    some_bits = (ctypes.c_void_p * 8)(64)
    assert L.mnrf_objects_cull(*_cull_args(res=bad_res, bits=some_bits)) < 0 and b"1..1024" in L.mnrf_last_error()
    assert L.mnrf_objects_cull(*_cull_args(res=bad_res)) == 0                           # without bits the grid is not read
    good = dict(rays=64, out=128, index=64, slot=64, counts=64)
    for miss in good:
        assert L.mnrf_objects_cull(*_cull_args(n=4, **dict(good, **{miss: None}))) < 0 and b"null pointer" in L.mnrf_last_error(), miss
    assert L.mnrf_objects_cull(*_cull_args(n=4, **dict(good, out=64))) < 0 and b"out of place" in L.mnrf_last_error()
    assert L.mnrf_objects_cull(*_cull_args(n=4, **dict(good, rays=68))) < 0 and b"16 bytes" in L.mnrf_last_error()
    assert L.mnrf_objects_cull(*_cull_args(n=4, **dict(good, out=136))) < 0 and b"16 bytes" in L.mnrf_last_error()


def test_objects_merge_validates_its_arguments(L):
    tab = lambda *v: (ctypes.c_void_p * 8)(*v)  # noqa: E731
    one = (ctypes.c_float * 8)(*[1.0] * 8)

    def call(rgb=tab(64), dep=tab(64), op=tab(64), K=1, slot=64, counts=64, n=4, cap=4, scales=one, ps0=one, lvl=(64, 64)):
        return L.mnrf_objects_merge(rgb, dep, op, K, slot, counts, n, cap, scales, ps0, 0.05, lvl[0], lvl[1], None, None, None)
    for K in (0, 9):
        assert call(K=K) < 0 and b"1..8" in L.mnrf_last_error()
    assert call(n=-1) < 0 and b"bad size" in L.mnrf_last_error()
    assert call(cap=-1) < 0 and b"bad size" in L.mnrf_last_error()
    for name in ("rgb", "dep", "op", "scales", "ps0"):
        assert call(**{name: None}) < 0 and b"host array is null" in L.mnrf_last_error(), name
    assert call(dep=tab()) < 0 and b"together or not at all" in L.mnrf_last_error()
    assert call(K=2, op=tab(64, 64)) < 0 and b"together or not at all" in L.mnrf_last_error()
    assert call(n=0) == 0 and call(cap=0) == 0                                          # nothing to do
    assert call(rgb=tab(), dep=tab(), op=tab(), slot=None, counts=None, lvl=(None, None)) == 0      # no object was rendered
    for miss in (dict(slot=None), dict(counts=None), dict(lvl=(None, 64)), dict(lvl=(64, None))):
        assert call(**miss) < 0 and b"null pointer" in L.mnrf_last_error(), miss


# ----------------------------------------------------------------------------------------------- PlacedObject and the refusals
def _models(mask_head=True):
    import mirror_nerf_amd as M
    make = lambda: M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=mask_head)  # noqa: E731
    return {"coarse": make(), "fine": make()}


def _args(**over):
    a = dict(predict_normal=True, only_one_field=False, only_one_field_fine_epoch=2, max_recursive_level=1, near=0.05,
             root_dir="office", app_reflect_newly_placed_objects=True)
    a.update(over)
    return a


PLACE = dict(pose_align=None, scale=2.0, translation=(0.0, 3.0, 0.5))
NERF_PL = SimpleNamespace(models=[], embeddings=[])
DNERF = dict(network_fn=object(), network_fine=None)


def _call(args, models=None, n_importance=64, **kw):
    import mirror_nerf_amd as M
    return M.batched_inference(models or _models(), {}, torch.zeros(4, 8), 64, n_importance, False, 32, args=args, trace_secondary_rays=True, **kw)


def test_placed_object_validation():
    import mirror_nerf_amd as M
    from mirror_nerf_amd import placed_objects as PO
    assert PO.MAX_OBJECTS == 8 and M.PlacedObject is PO.PlacedObject and "PlacedObject" in M.__all__
    a = M.PlacedObject(NERF_PL, PLACE)
    assert (a.kind, a.bounds, a.time) == ("nerf_pl", None, None)
    d = M.PlacedObject(DNERF, None, time=0.25)
    assert (d.kind, d.time, d.placement) == ("d_nerf", 0.25, None)
    with pytest.raises(TypeError, match="nerf_pl system_obj"):
        M.PlacedObject(object(), PLACE)
    with pytest.raises(TypeError, match="network_fn"):
        M.PlacedObject({}, PLACE)
    # the placement: resolve_new_object's own refusals
    with pytest.raises(ValueError, match="missing: \\['scale'\\]"):
        M.PlacedObject(NERF_PL, dict(pose_align=None, translation=(0, 0, 0)))
    with pytest.raises(ValueError, match="scale must be positive"):
        M.PlacedObject(NERF_PL, dict(PLACE, scale=0.0))
    with pytest.raises(ValueError, match="translation has 3 entries"):
        M.PlacedObject(NERF_PL, dict(PLACE, translation=(0, 0)))
    with pytest.raises(ValueError, match="None, 3x4 or 4x4"):
        M.PlacedObject(NERF_PL, dict(PLACE, pose_align=np.eye(3)))
    with pytest.raises(ValueError, match="first column"):
        M.PlacedObject(NERF_PL, dict(PLACE, pose_align=np.zeros((3, 4))))
    # the bounds
    box = M.ObjectBounds((-1, -1, -1), (1, 1, 1))
    assert M.PlacedObject(NERF_PL, PLACE, bounds=box).bounds is box
    assert M.PlacedObject(NERF_PL, PLACE, bounds="auto", region=((-1,) * 3, (1,) * 3), bounds_res=32).bounds_res == 32
    with pytest.raises(ValueError, match="None, an ObjectBounds or 'auto'"):
        M.PlacedObject(NERF_PL, PLACE, bounds="tight")
    with pytest.raises(ValueError, match="needs region="):
        M.PlacedObject(NERF_PL, PLACE, bounds="auto")
    with pytest.raises(ValueError, match="pass bounds='auto'"):
        M.PlacedObject(NERF_PL, PLACE, region=((-1,) * 3, (1,) * 3))
    with pytest.raises(ValueError, match="does not move"):
        M.PlacedObject(NERF_PL, PLACE, time=0.5)
    # resolved for a call: the preset of args.root_dir where the placement is None, the call's time where the object has none
    r = d.resolve(SimpleNamespace(root_dir="data/office"), 0.75, "cpu")
    assert r["xform"]["scale"] == 2.0 and r["xform"]["translation"] == (0.0, 3.0, 0.5) and r["time"] == 0.25 and r["bounds"] is None
    assert M.PlacedObject(DNERF, PLACE).resolve(None, 0.75, "cpu")["time"] == 0.75
    assert M.PlacedObject(NERF_PL, PLACE, bounds=box).resolve(None, None, "cpu")["bounds"] is box
    with pytest.raises(ValueError, match="needs frame_time="):
        M.PlacedObject(DNERF, PLACE).resolve(None, None, "cpu")


def test_every_refusal_of_placed_objects():
    import mirror_nerf_amd as M
    a, d = M.PlacedObject(NERF_PL, PLACE), M.PlacedObject(DNERF, PLACE)
    box = M.ObjectBounds((-1, -1, -1), (1, 1, 1))
    # beside a single-object keyword
    for name, value in (("system_obj", NERF_PL), ("render_kwargs_test_d_nerf", DNERF), ("new_object", PLACE), ("object_bounds", box),
                        ("object_region", ((-1,) * 3, (1,) * 3))):
        with pytest.raises(ValueError, match=f"cannot be combined with {name}= \\(the single-object keywords\\)"):
            _call(_args(), placed_objects=[a], **{name: value})
    # without the application
    off = {k: v for k, v in _args().items() if k != "app_reflect_newly_placed_objects"}
    with pytest.raises(ValueError, match="placed_objects= lists the objects of app_reflect_newly_placed_objects: the application is not on"):
        _call(off, placed_objects=[a])
    with pytest.raises(ValueError, match="application is not on"):
        _call(dict(off, app_place_new_mirror=True), placed_objects=[a])
    # K = 0, K > 8, and what is not a list of PlacedObject
    with pytest.raises(ValueError, match="holds 1..8 objects \\(MNRF_OBJECTS_MAX\\), not 0"):
        _call(_args(), placed_objects=[])
    with pytest.raises(ValueError, match="holds 1..8 objects \\(MNRF_OBJECTS_MAX\\), not 9"):
        _call(_args(), placed_objects=[a] * 9)
    with pytest.raises(TypeError, match="must be a list of PlacedObject, not PlacedObject"):
        _call(_args(), placed_objects=a)
    with pytest.raises(TypeError, match="placed_objects\\[1\\] must be a PlacedObject, not SimpleNamespace"):
        _call(_args(), placed_objects=[a, NERF_PL])
    # a D-NeRF object with no time of its own and none from the call
    with pytest.raises(ValueError, match="placed_objects\\[1\\] is a D-NeRF object without time=: it needs frame_time="):
        _call(_args(), placed_objects=[a, d])
    # another application
    for other in ("app_place_new_mirror", "app_reflection_substitution", "app_control_mirror_roughness"):
        with pytest.raises(ValueError, match=f"cannot be combined with {other} \\(one application at a time\\)"):
            _call(_args(**{other: True}), placed_objects=[a])
    # no fine mirror mask, no near
    with pytest.raises(ValueError, match="needs a fine mirror mask"):
        _call(_args(), models=_models(mask_head=False), placed_objects=[a])
    with pytest.raises(ValueError, match="needs a fine mirror mask"):
        _call(_args(only_one_field=True), placed_objects=[a])
    with pytest.raises(ValueError, match="needs a fine mirror mask"):
        _call(_args(), n_importance=0, placed_objects=[a])
    with pytest.raises(ValueError, match="needs args.near"):
        _call(_args(near=None), placed_objects=[a])
    # args.obj_model_type is not consulted: neither its value nor what it would ask for
    with pytest.raises(ValueError, match="needs args.near"):
        _call(_args(near=None, obj_model_type="mesh"), placed_objects=[a])
    # object_used of a wrong size
    with pytest.raises(ValueError, match="object_used holds 2 elements \\(one per placed object\\) or 1 \\(their total\\), not 3"):
        _call(_args(), placed_objects=[a, a], object_used=torch.zeros(3, dtype=torch.int32))


def test_without_the_keyword_the_refusals_are_the_old_ones():
    box_kw = dict(object_bounds="auto", object_region=((-1,) * 3, (1,) * 3))
    off = {k: v for k, v in _args().items() if k != "app_reflect_newly_placed_objects"}
    with pytest.raises(NotImplementedError, match="needs the D-NeRF object itself"):        # obj_model_type defaults to d_nerf
        _call(_args())
    with pytest.raises(NotImplementedError, match="needs the D-NeRF object itself"):
        _call(_args(), placed_objects=None)
    with pytest.raises(ValueError, match="needs frame_time="):
        _call(_args(obj_model_type="d_nerf"), render_kwargs_test_d_nerf=DNERF)
    with pytest.raises(ValueError, match="must be 'nerf_pl' or 'd_nerf', not 'mesh'"):
        _call(_args(obj_model_type="mesh"), system_obj=NERF_PL)
    with pytest.raises(ValueError, match="needs system_obj="):
        _call(_args(obj_model_type="nerf_pl"))
    for other in ("app_place_new_mirror", "app_reflection_substitution", "app_control_mirror_roughness"):
        with pytest.raises(ValueError, match=f"cannot be combined with {other}"):
            _call(_args(obj_model_type="nerf_pl", **{other: True}), system_obj=NERF_PL)
    with pytest.raises(ValueError, match="needs a fine mirror mask"):
        _call(_args(obj_model_type="nerf_pl"), models=_models(mask_head=False), system_obj=NERF_PL)
    with pytest.raises(ValueError, match="needs args.near"):
        _call(_args(obj_model_type="nerf_pl", near=None), system_obj=NERF_PL)
    with pytest.raises(ValueError, match="new_object needs the keys"):
        _call(_args(obj_model_type="nerf_pl"), system_obj=NERF_PL, new_object=dict(scale=1.0))
    with pytest.raises(ValueError, match="application is not on"):
        _call(off, **box_kw)
    with pytest.raises(ValueError, match="needs object_region"):
        _call(_args(obj_model_type="nerf_pl"), system_obj=NERF_PL, object_bounds="auto")
    with pytest.raises(ValueError, match="needs system_substitution="):
        _call(dict(off, app_reflection_substitution=True))


# ----------------------------------------------------------------------------------------------- scripts/eval_scene.py --objects_json
def _eval_scene():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("eval_scene", os.path.join(root, "scripts", "eval_scene.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_objects_json_of_the_eval_driver(tmp_path, capsys):
    import json
    ES = _eval_scene()
    base = ["--root_dir", "r", "--ckpt_path", "c", "--out_dir", "o"]
    spec = tmp_path / "objects.json"
    spec.write_text(json.dumps([{"ckpt_path": "a.ckpt", "model_type": "nerf_pl", "bounds": [0, 0, 0, 1, 1, 1]},
                                {"ckpt_path": "/abs/b.tar", "model_type": "d_nerf", "time_offset": 0.5, "time_scale": 0.5, "scale": 2.0}]))
    args = ES.get_opts(base + ["--app_reflect_newly_placed_objects", "--objects_json", str(spec)])
    assert args.objects_json == str(spec)
    # exclusive with the single-object flags, and only with the application
    for extra in (["--obj_ckpt_path", "x"], ["--obj_model_type", "nerf_pl"], ["--obj_bounds", "auto"], ["--obj_bounds_res=32"]):
        with pytest.raises(SystemExit):
            ES.get_opts(base + ["--app_reflect_newly_placed_objects", "--objects_json", str(spec)] + extra)
        assert "cannot be combined with " + extra[0].split("=")[0] in capsys.readouterr().err
    with pytest.raises(SystemExit):
        ES.get_opts(base + ["--objects_json", str(spec)])
    assert "--app_reflect_newly_placed_objects" in capsys.readouterr().err
    assert ES.get_opts(base + ["--app_reflect_newly_placed_objects", "--obj_ckpt_path", "x"]).objects_json is None      # as before
    # the entries: defaults filled in, a relative checkpoint path taken from the file's directory
    a, b = ES.read_objects_json(str(spec))
    assert a["ckpt_path"] == str(tmp_path / "a.ckpt") and b["ckpt_path"] == "/abs/b.tar"
    assert (a["scale"], a["pose_align"], a["bounds_res"], a["time_scale"]) == (1.0, None, 64, 1.0) and b["scale"] == 2.0
    assert [ES.object_time(b, i, 4) for i in range(4)] == [0.5, 0.625, 0.75, 0.875]
    ES.check_object_times([a, b], 4)
    ES.check_object_times([dict(a, time_offset=7.0)], 4)                         # a nerf_pl object has no time
    with pytest.raises(SystemExit, match="object 1 would be rendered at time 1.1250 in frame 1 of 4"):
        ES.check_object_times([a, dict(b, time_offset=0.875, time_scale=1.0)], 4)
    with pytest.raises(SystemExit, match="outside \\[0, 1\\]"):
        ES.check_object_times([dict(b, time_offset=-0.1)], 4)
    for bad, why in (({"a": 1}, "list of 1..8"), ([], "list of 1..8"), ([{"ckpt_path": "x", "model_type": "nerf_pl"}] * 9, "list of 1..8"),
                     ([3], "not a JSON object"), ([{"ckpt_path": "x"}], "missing keys \\['model_type'\\]"),
                     ([{"ckpt_path": "x", "model_type": "nerf_pl", "pose": 1}], "unknown keys \\['pose'\\]"),
                     ([{"ckpt_path": "x", "model_type": "mesh"}], "model_type must be"),
                     ([{"ckpt_path": "x", "model_type": "nerf_pl", "bounds": [0, 1]}], "bounds must be"),
                     ([{"ckpt_path": "x", "model_type": "nerf_pl", "bounds": "tight"}], "bounds must be"),
                     ([{"ckpt_path": "x", "model_type": "nerf_pl", "region": [0, 1]}], "region holds six")):
        spec.write_text(json.dumps(bad))
        with pytest.raises(SystemExit, match=why):
            ES.read_objects_json(str(spec))
    # the frame's list: a box, "auto" with its region, a D-NeRF object at its time
    import mirror_nerf_amd as M
    fields = [(dict(a, bounds=[0, 0, 0, 1, 2, 3]), NERF_PL), (dict(a, bounds="auto", region=[-1, -1, -1, 1, 1, 1], bounds_res=32), NERF_PL), (b, DNERF)]
    p = ES.placed_objects(fields, 1, 4)
    assert all(isinstance(o, M.PlacedObject) for o in p) and [o.kind for o in p] == ["nerf_pl", "nerf_pl", "d_nerf"]
    assert p[0].bounds.hi == (1.0, 2.0, 3.0) and p[1].bounds == "auto" and p[1].region == ((-1, -1, -1), (1, 1, 1)) and p[1].bounds_res == 32
    assert (p[0].time, p[2].time, p[2].placement["scale"]) == (None, 0.625, 2.0)
