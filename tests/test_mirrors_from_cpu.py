"""CPU-side checks of `exclude_source_mirror=` (mnrf_place_mirrors_from, mnrf_mirror_sources): the numpy restatement
(tests/mirrors_from_ref.py) against mirrors_ref.place_mirrors where no ray has a source, the chain of reflections between two
facing tilted mirrors with and without the exclusion, an excluded winner giving way, the refusals of batched_inference, the
binding read from the header and the argument validation of the C entry points without a GPU."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import mirrors_from_ref as MF
from tests import mirrors_ref as MR
from tests import rough_ref as RR

F = np.float32
NEAR2 = 0.1          # the absolute near of a reflected ray (recursion.RAY_FORWARD_OFFSET)
KEYS = ("depth", "mask", "normal", "x_surface", "mask_bool", "index")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32}[a.dtype.itemsize])


def facing_pair():
    """Two parallel frame mirrors tilted by 0.3 rad about z, facing each other across the camera of camera()."""
    from mirror_nerf_amd import PlacedMirror
    s, c = np.sin(0.3), np.cos(0.3)
    return [PlacedMirror((0, 1, 0.6), (s, -c, 0), (0, 0, 1), (3, 3)), PlacedMirror((0, -1, 0.6), (-s, c, 0), (0, 0, 1), (8, 8))]


def camera(near=1e9):
    from tests import test_hip_mirrors as TM
    return TM.camera_rays((0.0, 0.0, 0.6), (0.1, 1.0, 0.65), near=near)


def _case(rays, seed=0):
    n = len(rays)
    rs = np.random.RandomState(seed)
    return dict(rays=rays, depth=np.full(n, 10.0, F), mask=np.zeros(n, F), normal=rs.normal(size=(n, 3)).astype(F),
                x_surface=rs.normal(size=(n, 3)).astype(F))


# ------------------------------------------------------------------------------------------------ identity with the old rule
@pytest.mark.parametrize("K", [1, 2, 3, 8])
def test_without_a_source_the_rule_is_the_old_one(K):
    from tests import test_hip_mirrors as TM
    mirrors = TM.mirrors_for(K)
    c = TM.seeded_case(321, mirrors, 100 + K)
    want = MR.place_mirrors(mirrors=mirrors, near=0.05, any_in=2, **c)
    for source in (None, np.full(321, -1, np.int32)):
        got = MF.place_mirrors(mirrors=mirrors, near=0.05, any_in=2, source=source, **c)
        for k in KEYS:
            assert got[k].dtype == want[k].dtype and np.array_equal(_bits(got[k]), _bits(want[k])), k
        assert got["any"] == want["any"]
        for p, q in zip(got["per"], want["per"]):
            assert not p["excluded"].any() and np.array_equal(p["hit"], q["hit"])
    assert (want["index"] >= 0).sum() >= 32


def test_a_source_outside_the_list_excludes_nothing():
    from tests import test_hip_mirrors as TM
    mirrors = TM.mirrors_for(3)
    c = TM.seeded_case(257, mirrors, 5)
    want = MR.place_mirrors(mirrors=mirrors, near=0.05, **c)
    got = MF.place_mirrors(mirrors=mirrors, near=0.05, source=np.resize(np.array([-2, 3, 127, -1], np.int32), 257), **c)
    for k in KEYS:
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k


# ------------------------------------------------------------------------------------------------ the chain on the facing pair
def chain(exclude, levels=3):
    """Levels 0 .. `levels` of the recursion on the facing pair, restated: place, reflect the rays that took a mirror about the
    written normal (rough_ref.reflect_direction_ref), origin at x_surface, near 0.1.  -> per level dict(index, left, depth):
    the mirror taken, the mirror the ray left at the level above (tracked either way) and the depth written, on the level's rays."""
    mirrors = [m.as_dict() for m in facing_pair()]
    rays, left, out = camera(), None, []
    for _ in range(levels + 1):
        res = MF.place_mirrors(mirrors=mirrors, near=1e9, source=left if exclude else None, **_case(rays))
        took = np.nonzero(res["index"] >= 0)[0].astype(np.int32)
        out.append(dict(index=res["index"], left=left, depth=res["depth"], took=took))
        d = RR.reflect_direction_ref(res["normal"][took], None, 0.0, rays[took, 3:6])
        rays = np.concatenate([res["x_surface"][took], d, np.full((len(took), 1), NEAR2, F), rays[took, 7:8]], 1).astype(F)
        left = MF.mirror_sources(res["index"], took, len(took), 1)
    return out


def test_the_chain_on_the_facing_pair():
    off, on = chain(False), chain(True)
    assert (off[0]["index"] == 0).all() and np.array_equal(on[0]["index"], off[0]["index"]), "every camera ray takes the first mirror"
    # a condition on the inputs: without the exclusion the set-up shows what the keyword is for
    lvl = off[1]
    again = (lvl["index"] == lvl["left"]) & (lvl["index"] >= 0)
    print("without source, level 1:", int(again.sum()), "of", len(again), "rays re-hit the mirror they left; smallest depth taken",
          float(lvl["depth"][lvl["took"]].min()))
    assert len(again) == 256 and again.sum() >= 32 and (lvl["depth"][again] < 1e-6).all()
    for level in (1, 2, 3):
        lvl = on[level]
        taken = lvl["index"] >= 0
        print(f"with source, level {level}: {len(taken)} rays, {int(taken.sum())} take a mirror, smallest depth taken",
              float(lvl["depth"][taken].min()))
        assert taken.sum() >= 32, (level, int(taken.sum()))
        assert not (lvl["index"] == lvl["left"])[taken].any(), level
        assert (lvl["depth"][taken] > 1.9).all(), level


# ------------------------------------------------------------------------------------------------ an excluded winner gives way
def test_an_excluded_winner_gives_way():
    """The facing pair and a third mirror, parallel to the first and half a unit behind it.  With source = 0 on every ray the third
    wins exactly where the first would have won -- inside it, facing it, nothing nearer -- and nothing else changes."""
    from mirror_nerf_amd import PlacedMirror
    s, c = np.sin(0.3), np.cos(0.3)
    third = PlacedMirror((-0.5 * s, 1 + 0.5 * c, 0.6), (s, -c, 0), (0, 0, 1), (6, 6))
    mirrors = [m.as_dict() for m in facing_pair() + [third]]
    rs = np.random.RandomState(3)
    rays = camera()
    rays[:, 3:6] = np.where(rs.uniform(size=(256, 1)) < 0.25, -1, 1) * rays[:, 3:6]        # a quarter looks the other way
    rays[:, 0:3] += rs.normal(0, 0.15, (256, 3)).astype(F)                                # (the origins stay between the pair)
    case = _case(rays, 1)
    old = MR.place_mirrors(mirrors=mirrors, near=1e9, **case)
    new = MF.place_mirrors(mirrors=mirrors, near=1e9, source=np.zeros(256, np.int32), **case)
    first, third_hit = old["index"] == 0, old["per"][2]["hit"]
    assert first.sum() >= 64 and (old["index"] == 1).sum() >= 16 and third_hit[first].all(), "the third mirror is behind all of the first"
    assert np.array_equal(new["index"], np.where(first, 2, old["index"]))
    assert np.array_equal(_bits(new["depth"][first]), _bits(old["per"][2]["dist"][first]))
    assert np.array_equal(_bits(new["x_surface"][first]), _bits(old["per"][2]["x"][first]))
    for k in KEYS:
        assert np.array_equal(_bits(new[k][~first]), _bits(old[k][~first])), k
    # the only hit is the excluded one: no flag, no mask, nothing written
    alone = MF.place_mirrors(mirrors=mirrors[:1], near=1e9, source=np.zeros(256, np.int32), **case)
    assert MR.place_mirrors(mirrors=mirrors[:1], near=1e9, **case)["any"] == 1
    assert alone["any"] == 0 and (alone["index"] == -1).all() and not alone["mask_bool"].any()
    for k in ("depth", "mask", "normal", "x_surface"):
        assert np.array_equal(_bits(alone[k]), _bits(case[k])), k


def test_mirror_sources_restatement():
    idx = np.array([3, -1, 0, 7, -1], np.int32)
    assert MF.mirror_sources(idx, np.array([4, 0, 3], np.int32), 3, 2).tolist() == [-1, 3, 7, -1, 3, 7]
    assert MF.mirror_sources(idx, None, 5, 1).tolist() == idx.tolist()
    assert MF.mirror_sources(None, np.array([1, 2], np.int32), 2, 3).tolist() == [-1] * 6
    out = MF.mirror_sources(None, None, 0, 3)
    assert out.dtype == np.int32 and out.shape == (0,)


# ------------------------------------------------------------------------------------------------ batched_inference
def _models():
    import mirror_nerf_amd as M
    return {name: M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=True)
            for name in ("coarse", "fine")}


ARGS = dict(predict_normal=True, only_one_field=False, only_one_field_fine_epoch=2, max_recursive_level=2, near=0.05, root_dir="office")


def _call(**kw):
    import mirror_nerf_amd as M
    return M.batched_inference(_models(), {}, torch.zeros(4, 8), 64, 64, False, 32, args=dict(ARGS), **kw)


@pytest.mark.parametrize("kw,msg", [
    (dict(exclude_source_mirror=True), "needs new_mirrors="),
    (dict(exclude_source_mirror=True, source_mirror=torch.zeros(4, dtype=torch.int32)), "needs new_mirrors="),
    (dict(new_mirrors=True, exclude_source_mirror=1), "exclude_source_mirror is a bool"),
    (dict(new_mirrors=True, exclude_source_mirror="yes"), "exclude_source_mirror is a bool"),
    (dict(new_mirrors=True, exclude_source_mirror=None), "exclude_source_mirror is a bool"),
    (dict(new_mirrors=True, source_mirror=torch.zeros(4, dtype=torch.int32)), "exclude_source_mirror=True alone"),
    (dict(new_mirrors=True, exclude_source_mirror=False, source_mirror=torch.zeros(4, dtype=torch.int32)), "exclude_source_mirror=True alone"),
    (dict(new_mirrors=True, exclude_source_mirror=True, source_mirror=torch.zeros(4, dtype=torch.int64)), "must be an int32 tensor"),
    (dict(new_mirrors=True, exclude_source_mirror=True, source_mirror=torch.zeros(4)), "must be an int32 tensor"),
    (dict(new_mirrors=True, exclude_source_mirror=True, source_mirror=[0, 0, 0, 0]), "must be an int32 tensor"),
    (dict(new_mirrors=True, exclude_source_mirror=True, source_mirror=torch.zeros(5, dtype=torch.int32)), "one index per ray"),
    (dict(new_mirrors=True, exclude_source_mirror=True, source_mirror=torch.zeros(4, 1, dtype=torch.int32)), "one index per ray"),
    (dict(new_mirrors=True, exclude_source_mirror=True, source_mirror=torch.zeros(4, dtype=torch.int32, device="meta")), "is on meta"),
], ids=["no_list", "no_list_with_source", "int", "str", "none", "source_alone", "source_with_false", "int64", "float32", "list", "length", "shape",
        "device"])
def test_refusals(kw, msg):
    if kw.get("new_mirrors") is True:
        kw = dict(kw, new_mirrors=facing_pair())
    with pytest.raises(ValueError, match=msg):
        _call(**kw)


def test_the_keyword_is_allowed_wherever_the_list_is():
    from mirror_nerf_amd import PlacedObject
    from mirror_nerf_amd.recursion import _refuse_apps
    obj = PlacedObject(SimpleNamespace(models={}, embeddings={}), dict(pose_align=None, scale=1.0, translation=(0, 0, 0)))
    on = dict(new_mirrors=facing_pair(), exclude_source_mirror=True, _N_importance=64)
    _refuse_apps(SimpleNamespace(**ARGS), _models(), on)
    _refuse_apps(SimpleNamespace(**ARGS), _models(), dict(on, source_mirror=torch.zeros(4, dtype=torch.int32)))
    _refuse_apps(SimpleNamespace(**ARGS), _models(), dict(on, rough_times=2, scene_roughness=0.01))
    _refuse_apps(SimpleNamespace(app_reflect_newly_placed_objects=True, **ARGS), _models(), dict(on, placed_objects=[obj]))
    _refuse_apps(SimpleNamespace(app_reflection_substitution=True, **ARGS), _models(), dict(on, system_substitution=object()))
    _refuse_apps(SimpleNamespace(**ARGS), _models(), dict(new_mirrors=facing_pair(), exclude_source_mirror=False, _N_importance=64))
    # the list's own refusals stay in front
    with pytest.raises(ValueError, match="app_control_mirror_roughness cannot"):
        _refuse_apps(SimpleNamespace(app_control_mirror_roughness=True, **ARGS), _models(), on)


# ------------------------------------------------------------------------------------------------ the binding
def test_the_binding_is_read_from_the_header():
    from mirror_nerf_amd import _lib
    V, I, Fp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_float)
    old = _lib.SIGNATURES["mnrf_place_mirrors"]
    assert old == (ctypes.c_int, [V, ctypes.c_int64, ctypes.c_int, I, I, I, Fp, Fp, Fp, Fp, ctypes.c_float] + [V] * 8)
    res, args = _lib.SIGNATURES["mnrf_place_mirrors_from"]
    assert res is ctypes.c_int and list(args) == list(old[1][:11]) + [V] + list(old[1][11:]), "mnrf_place_mirrors' arguments, source before depth"
    assert _lib.SIGNATURES["mnrf_mirror_sources"] == (ctypes.c_int, [V, V, ctypes.c_int64, ctypes.c_int, V, V])
    classes = [c and c[0] for c in _lib.POINTEES["mnrf_place_mirrors_from"]]
    assert classes[11] == "int32" and classes[12] == "float" and classes[-2] == "int32"
    assert [c and c[0] for c in _lib.POINTEES["mnrf_mirror_sources"]][:5] == ["int32", "int32", None, None, "int32"]


# ------------------------------------------------------------------------------------------------ the C entry points
@pytest.fixture(scope="module")
def L():
    from mirror_nerf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_place_mirrors_from_argument_validation(L):
    null = None

    def call(n, K=1, kinds=(0,), shapes=(0,), axes=(0,), host=True):
        K_arr = max(K, 1)
        i = lambda v: (ctypes.c_int * max(len(v), K_arr, 8))(*v)  # noqa: E731
        f = lambda m: (ctypes.c_float * (m * 8))()  # noqa: E731
        h = (i(kinds), i(shapes), i(axes), f(1), f(9), f(3), f(4)) if host else (null,) * 7
        return L.mnrf_place_mirrors_from(null, n, K, *h, 0.05, null, null, null, null, null, null, null, null, null)

    assert call(0) == 0                                        # zero rays: a no-op
    assert call(0, K=8, kinds=(0, 1) * 4, shapes=(1, 0) * 4, axes=(1, 0) * 4) == 0
    assert call(-1) < 0 and b"mnrf_place_mirrors_from: bad size" in L.mnrf_last_error()
    for K in (0, 9, -1):
        assert call(4, K=K) < 0 and b"n_mirrors" in L.mnrf_last_error()
        assert call(0, K=K) < 0 and b"n_mirrors" in L.mnrf_last_error()
    assert call(4, kinds=(2,)) < 0 and b"kind" in L.mnrf_last_error()
    assert call(4, shapes=(2,)) < 0 and b"shape" in L.mnrf_last_error()
    assert call(4, axes=(2,)) < 0 and b"axis" in L.mnrf_last_error()
    assert call(0, kinds=(1,), axes=(7,)) == 0                 # a frame mirror has no axis
    assert call(4, host=False) < 0 and b"host array" in L.mnrf_last_error()
    assert call(4) < 0 and b"mnrf_place_mirrors_from: null pointer" in L.mnrf_last_error()


def test_mirror_sources_argument_validation(L):
    null = None
    assert L.mnrf_mirror_sources(null, null, 0, 1, null, null) == 0          # nothing to write: a no-op
    assert L.mnrf_mirror_sources(null, null, 0, 3, null, null) == 0
    assert L.mnrf_mirror_sources(null, null, -1, 1, null, null) < 0 and b"mnrf_mirror_sources: bad size" in L.mnrf_last_error()
    assert L.mnrf_mirror_sources(null, null, 1 << 31, 1, null, null) < 0 and b"bad size" in L.mnrf_last_error()
    for n_rep in (0, -1):
        assert L.mnrf_mirror_sources(null, null, 4, n_rep, null, null) < 0 and b"n_rep" in L.mnrf_last_error()
        assert L.mnrf_mirror_sources(null, null, 0, n_rep, null, null) < 0 and b"n_rep" in L.mnrf_last_error()
    assert L.mnrf_mirror_sources(null, null, 4, 1, null, null) < 0 and b"null pointer" in L.mnrf_last_error()
