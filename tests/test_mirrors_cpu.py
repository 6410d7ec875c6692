"""CPU-side checks of `new_mirrors=` (mirror_nerf_amd/placed_mirrors.py, mnrf_place_mirrors): the numpy restatement of the
K-mirror rule (tests/mirrors_ref.py) against the single-mirror restatement for K = 1, the frames PlacedMirror builds and its
refusals, the refusals and allowed combinations of batched_inference, the parsing of scripts/eval_scene.py --mirrors_json, and
the argument validation of the C entry point without a GPU."""
import ctypes
import importlib.util
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import apps_ref as AR
from tests import mirrors_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEAR = 0.05


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32}[a.dtype.itemsize])


# ------------------------------------------------------------------------------------------------ the restatement, K = 1
@pytest.mark.parametrize("n", [64, 257, 1000])
@pytest.mark.parametrize("name", list(AR.PLANES))
def test_one_axis_mirror_equals_the_single_mirror_restatement(name, n):
    """K = 1, kind axis, shape rect on apps_ref's seeded cases: depth, x_surface, both masks and the flag are those of
    apps_ref.place_mirror bit for bit; the normal is equal on every ray outside S = inside and not hit (where the single mirror
    writes the plane's normal and the K-mirror rule keeps the ray's own)."""
    kw, c = AR.plane_case(name, n, NEAR)
    want = AR.place_mirror(dtype=np.float32, **kw, **c)
    got = MR.place_mirrors(mirrors=[MR.axis(kw["axis"], kw["position"], kw["plane_normal"], kw["rect"])], near=kw["near"], **c)
    for k in ("depth", "x_surface", "mask", "mask_bool"):
        assert np.array_equal(_bits(got[k]), _bits(want[k])), k
    assert got["any"] == want["any"]
    p = got["per"][0]
    for k, j in (("u", "u"), ("w", "w"), ("dist", "dist"), ("s", "s")):
        assert np.array_equal(_bits(p[k]), _bits(want[j])), k
    assert np.array_equal(p["inside"], want["in_rect"]) and np.array_equal(p["hit"], want["hit"]) and np.array_equal(p["blocked"], want["blocked"])
    assert np.array_equal(got["index"], np.where(want["hit"], 0, -1))
    S = want["in_rect"] & ~want["hit"]
    assert S.any() and want["hit"].any(), "the seeded case holds rays of both kinds"
    assert np.array_equal(_bits(got["normal"][~S]), _bits(want["normal"][~S]))
    assert np.array_equal(_bits(got["normal"][S]), _bits(c["normal"][S])), "inside and not taken: the ray's own normal is kept"
    assert not np.array_equal(got["normal"][S], want["normal"][S])


def test_the_winner_is_the_nearest_and_a_tie_goes_to_the_later_mirror():
    rays = np.array([[0, 0, 0, 1, 0, 0, 0.05, 6]], np.float32)
    c = dict(rays=rays, depth=np.array([10.0], np.float32), mask=np.zeros(1, np.float32), normal=np.zeros((1, 3), np.float32),
             x_surface=np.zeros((1, 3), np.float32))
    rect = (-1, 1, -1, 1)
    a, b = MR.axis("x", 2.0, (-1, 0, 0), rect), MR.axis("x", 1.0, (0, 0, -1), rect)
    twin = MR.axis("x", 2.0, (0, 1, 0), rect)
    assert MR.place_mirrors(mirrors=[a, b], near=NEAR, **c)["index"][0] == 1
    assert MR.place_mirrors(mirrors=[b, a], near=NEAR, **c)["index"][0] == 0
    got = MR.place_mirrors(mirrors=[a, twin], near=NEAR, **c)
    assert got["index"][0] == 1 and got["normal"][0].tolist() == [0, 1, 0] and got["depth"][0] == 2.0


# ------------------------------------------------------------------------------------------------ PlacedMirror
FRAMES = [dict(center=(0.3, -1.2, 0.8), normal=(0.2, -1.0, 0.17), up=(0, 0, 1), size=(1.5, 0.7)),
          dict(center=(1, 2, 3), normal=(0, 0, 5), up=(1, 1, 0.3), size=(0.2, 4.0)),
          dict(center=(0, 0, 0), normal=(1e-3, 2e-3, -1e-3), up=(0.5, 0.1, 7.0), size=(1, 1)),
          dict(center=(-4, 0.5, 0.1), normal=(-3, 0.1, 0.2), up=(0, 1, 1e-3), size=(3, 2))]


@pytest.mark.parametrize("kw", FRAMES, ids=[str(i) for i in range(len(FRAMES))])
def test_frames_are_orthonormal(kw):
    from mirror_nerf_amd import PlacedMirror
    m = PlacedMirror(shape="ellipse", **kw)
    fr = m.frame64
    assert fr.dtype == np.float64 and np.abs(fr @ fr.T - np.eye(3)).max() <= 1e-7
    n = np.asarray(kw["normal"], np.float64)
    assert np.abs(fr[0] - n / np.linalg.norm(n)).max() <= 1e-15
    assert np.dot(fr[2], kw["up"]) > 0 and np.abs(np.cross(fr[2], fr[0]) - fr[1]).max() <= 1e-15       # e_u = cross(e_w, n)
    # rounded once to float32
    for row, got in zip(fr, (m.normal, m.e_u, m.e_w)):
        assert got == tuple(float(np.float32(v)) for v in row)
    w, h = kw["size"]
    assert m.rect == tuple(float(np.float32(v)) for v in (-w / 2, w / 2, -h / 2, h / 2)) and m.shape == "ellipse" and m.kind == "frame"


@pytest.mark.parametrize("name", ["x_default", "y_livingroom"])
def test_world_axes_reproduce_the_axis_preset(name):
    """center / normal / up along world axes: the frame is the preset's plane -- e_u and e_w are the world axes of the preset's
    rectangle, exactly -- and on the seeded rays (u, w), the inside set and the hits are those of the axis kind."""
    from mirror_nerf_amd import PlacedMirror
    axis, pos, normal, rect = AR.PLANES[name]
    a = 1 if axis == AR.PLANE_Y else 0
    cu, cw = 0.5 * (rect[0] + rect[1]), 0.5 * (rect[2] + rect[3])
    center = [0.0, 0.0, cw]
    center[a], center[1 - a] = pos, cu
    # e_u = cross(z, n): +y for n = +x, +x for n = -y -- the first rectangle coordinate of plane_x resp. plane_y
    m = PlacedMirror(center, normal, (0, 0, 1), (rect[1] - rect[0], rect[3] - rect[2]))
    e_u = [0.0, 0.0, 0.0]
    e_u[1 - a] = 1.0
    assert m.normal == tuple(float(v) for v in normal) and m.e_u == tuple(e_u) and m.e_w == (0.0, 0.0, 1.0)
    assert m.center == tuple(float(np.float32(v)) for v in center)
    kw, c = AR.plane_case(name, 500, NEAR)
    want = MR.intersect(c["rays"], MR.axis(axis, pos, normal, rect))
    got = MR.intersect(c["rays"], m.as_dict())
    f = np.float32
    # the frame's coordinates are relative to the centre: u_axis - cu up to the roundings of the two subtractions
    assert np.abs((got["u"] + f(cu)) - want["u"]).max() <= 1e-5 and np.abs((got["w"] + f(cw)) - want["w"]).max() <= 1e-5
    assert np.abs(got["x"] - want["x"]).max() <= 1e-5
    clear = (np.abs(np.abs(want["u"] - f(cu)) - f(0.5 * (rect[1] - rect[0]))) > 1e-4) & (np.abs(np.abs(want["w"] - f(cw)) - f(0.5 * (rect[3] - rect[2]))) > 1e-4)
    assert clear.mean() > 0.9 and np.array_equal(got["inside"][clear], want["inside"][clear])


def test_axis_aligned_takes_the_keys_of_new_mirror():
    from mirror_nerf_amd import PlacedMirror
    from mirror_nerf_amd.recursion import resolve_new_mirror
    preset = resolve_new_mirror(SimpleNamespace(plane_pos="plane_y", root_dir="livingroom"))
    m = PlacedMirror.axis_aligned(**preset)
    assert (m.kind, m.shape, m.axis, m.position, m.normal, m.rect) == ("axis", "rect", "y", float(np.float32(1.65)), (0.0, -1.0, 0.0),
                                                                       tuple(float(np.float32(v)) for v in (-0.3, 1.5, -0.5, 1.0)))
    assert PlacedMirror.axis_aligned("x", 0, (1, 0, 0), (0, 1, 0, 1), shape="ellipse").shape == "ellipse"


@pytest.mark.parametrize("kw,msg", [
    (dict(normal=(0, 0, 0)), "normal is zero"),
    (dict(up=(0.4, -2.0, 0.34)), "parallel"),
    (dict(up=(-0.2, 1.0, -0.17)), "parallel"),
    (dict(up=(0, 0, 0)), "parallel"),
    (dict(size=(0, 1)), "positive"),
    (dict(size=(1, -2)), "positive"),
    (dict(center=(0, np.nan, 0)), "finite"),
    (dict(normal=(np.inf, 0, 0)), "finite"),
    (dict(up=(0, 0, np.nan)), "finite"),
    (dict(size=(np.inf, 1)), "finite"),
    (dict(size=(1, 2, 3)), "holds 2"),
    (dict(shape="disc"), "shape"),
], ids=["zero_normal", "up_parallel", "up_antiparallel", "zero_up", "zero_size", "negative_size", "nan_center", "inf_normal", "nan_up",
        "inf_size", "three_sizes", "shape"])
def test_placed_mirror_refusals(kw, msg):
    from mirror_nerf_amd import PlacedMirror
    with pytest.raises(ValueError, match=msg):
        PlacedMirror(**dict(FRAMES[0], **kw))


def test_axis_aligned_refusals():
    from mirror_nerf_amd import PlacedMirror
    ok = dict(axis="x", position=0.0, normal=(1, 0, 0), rect=(0, 1, 0, 1))
    for kw, msg in ((dict(axis="z"), "axis"), (dict(position=np.nan), "finite"), (dict(rect=(0, 1, 0)), "holds 4"), (dict(normal=(1, 0)), "holds 3"),
                    (dict(shape="round"), "shape")):
        with pytest.raises(ValueError, match=msg):
            PlacedMirror.axis_aligned(**dict(ok, **kw))


# ------------------------------------------------------------------------------------------------ batched_inference
def _models(mask_head=True):
    import mirror_nerf_amd as M
    return {name: M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=mask_head)
            for name in ("coarse", "fine")}


def _args(**over):
    a = dict(predict_normal=True, only_one_field=False, only_one_field_fine_epoch=2, max_recursive_level=1, near=0.05, root_dir="office")
    a.update(over)
    return SimpleNamespace(**a)


def _mirror():
    from mirror_nerf_amd import PlacedMirror
    return PlacedMirror(**FRAMES[0])


def _object():
    from mirror_nerf_amd import PlacedObject
    return PlacedObject(SimpleNamespace(models={}, embeddings={}), dict(pose_align=None, scale=1.0, translation=(0, 0, 0)))


def _refuse(args, **kw):
    from mirror_nerf_amd.recursion import _refuse_apps
    return _refuse_apps(args, kw.pop("models", None) or _models(), dict(kw, _N_importance=64))


def test_allowed_combinations():
    _refuse(_args(), new_mirrors=[_mirror()])
    _refuse(_args(), new_mirrors=[_mirror()] * 8)
    _refuse(_args(), new_mirrors=(_mirror(), _mirror()))
    _refuse(_args(app_reflect_newly_placed_objects=True), new_mirrors=[_mirror()], placed_objects=[_object()])
    _refuse(_args(app_reflection_substitution=True), new_mirrors=[_mirror()], system_substitution=object())


@pytest.mark.parametrize("args,kw,exc,msg", [
    (dict(app_place_new_mirror=True), {}, ValueError, "cannot be combined with app_place_new_mirror"),
    (dict(), dict(new_mirror=dict(axis="x", position=0.0, normal=(1, 0, 0), rect=(0, 1, 0, 1))), ValueError, "cannot be combined with app_place_new_mirror or new_mirror="),
    (dict(app_reflect_newly_placed_objects=True, obj_model_type="nerf_pl"), dict(system_obj=object()), ValueError, "single-object keywords"),
    (dict(app_reflect_newly_placed_objects=True), dict(render_kwargs_test_d_nerf={}, frame_time=0.5), ValueError, "single-object keywords"),
    (dict(app_reflect_newly_placed_objects=True), {}, ValueError, "single-object keywords"),
    (dict(), dict(object_bounds="auto"), ValueError, "single-object keywords"),
    (dict(app_control_mirror_roughness=True), {}, ValueError, "app_control_mirror_roughness cannot"),
    (dict(near=None), {}, ValueError, "needs args.near"),
    (dict(app_reflection_substitution=True), {}, ValueError, "needs system_substitution"),
], ids=["place", "new_mirror", "system_obj", "dnerf_keyword", "objects_without_list", "object_bounds", "roughness", "no_near", "subst_without_system"])
def test_refusals(args, kw, exc, msg):
    with pytest.raises(exc, match=msg):
        _refuse(_args(**args), new_mirrors=[_mirror()], **kw)


def test_refusals_of_the_list_itself():
    from mirror_nerf_amd import PlacedMirror
    with pytest.raises(ValueError, match="1..8 mirrors"):
        _refuse(_args(), new_mirrors=[])
    with pytest.raises(ValueError, match="1..8 mirrors"):
        _refuse(_args(), new_mirrors=[_mirror()] * 9)
    with pytest.raises(TypeError, match="list of PlacedMirror"):
        _refuse(_args(), new_mirrors=_mirror())
    with pytest.raises(TypeError, match=r"new_mirrors\[1\]"):
        _refuse(_args(), new_mirrors=[_mirror(), dict(axis="x")])
    with pytest.raises(ValueError, match="needs a mirror-mask head"):
        _refuse(_args(), new_mirrors=[_mirror()], models=_models(mask_head=False))
    assert isinstance(_mirror(), PlacedMirror)


def test_refusal_through_batched_inference_and_nothing_changes_without_the_keyword():
    import mirror_nerf_amd as M
    with pytest.raises(ValueError, match="1..8 mirrors"):
        M.batched_inference(_models(), {}, torch.zeros(4, 8), 64, 64, False, 32, args=vars(_args()), new_mirrors=[])
    # without the keyword the refusals are the ones of before
    with pytest.raises(ValueError, match="app_place_new_mirror needs args.near"):
        M.batched_inference(_models(), {}, torch.zeros(4, 8), 64, 64, False, 32, args=vars(_args(app_place_new_mirror=True, near=None)))
    _refuse(_args(app_place_new_mirror=True), new_mirror=dict(axis="x", position=0.0, normal=(1, 0, 0), rect=(0, 1, 0, 1)))


# ------------------------------------------------------------------------------------------------ --mirrors_json
def _eval_scene():
    spec = importlib.util.spec_from_file_location("eval_scene", os.path.join(ROOT, "scripts", "eval_scene.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ENTRIES = [dict(center=[0.3, -1.2, 0.8], normal=[0.2, -1.0, 0.17], up=[0, 0, 1], size=[1.5, 0.7], shape="ellipse"),
           dict(axis="x", position=-1.0, normal=[1, 0, 0], rect=[-1, 1, -0.5, 0.5]),
           dict(center=[0, 0, 0], normal=[0, 0, 1], up=[0, 1, 0], size=[1, 1])]


def test_mirrors_json_parsing(tmp_path):
    ES = _eval_scene()
    path = tmp_path / "mirrors.json"
    path.write_text(json.dumps(ENTRIES))
    got = ES.read_mirrors_json(str(path))
    assert [m.kind for m in got] == ["frame", "axis", "frame"] and [m.shape for m in got] == ["ellipse", "rect", "rect"]
    from mirror_nerf_amd import PlacedMirror
    assert got[0].as_dict() == PlacedMirror(**ENTRIES[0]).as_dict() and got[1].as_dict() == PlacedMirror.axis_aligned(**ENTRIES[1]).as_dict()

    def refused(entries, match):
        path.write_text(json.dumps(entries))
        with pytest.raises(SystemExit, match=match) as e:
            ES.read_mirrors_json(str(path))
        assert str(path) in str(e.value)
    refused([], "list of 1..8 mirrors")
    refused([ENTRIES[0]] * 9, "list of 1..8 mirrors")
    refused({"center": 1}, "list of 1..8 mirrors")
    refused([ENTRIES[0], 3], "mirror 1 is not a JSON object")
    refused([ENTRIES[0], dict(ENTRIES[0], colour="red")], r"mirror 1: unknown keys \['colour'\]")
    refused([dict(center=[0, 0, 0], normal=[0, 0, 1], size=[1, 1])], r"mirror 0: .*missing keys \['up'\]")
    refused([ENTRIES[1], dict(axis="y", position=1.0, rect=[0, 1, 0, 1])], r"mirror 1: .*missing keys \['normal'\]")
    refused([dict(ENTRIES[1], center=[0, 0, 0])], r"mirror 0: unknown keys \['center'\]")
    refused([dict(ENTRIES[0], normal=[0, 0, 0])], "mirror 0: .*normal is zero")
    refused([dict(shape="rect")], "mirror 0: .*missing keys")


def test_mirrors_json_flag(tmp_path, capsys):
    ES = _eval_scene()
    path = tmp_path / "mirrors.json"
    path.write_text(json.dumps(ENTRIES))
    base = ["--root_dir", "r", "--ckpt_path", "c", "--out_dir", "o"]
    a = ES.get_opts(base + ["--mirrors_json", str(path)])
    assert a.mirrors_json == str(path) and not a.app_place_new_mirror
    with pytest.raises(SystemExit):
        ES.get_opts(base + ["--mirrors_json", str(path), "--app_place_new_mirror"])
    assert "--app_place_new_mirror" in capsys.readouterr().err
    assert ES.get_opts(base).mirrors_json is None


# ------------------------------------------------------------------------------------------------ the C entry point
@pytest.fixture(scope="module")
def L():
    from mirror_nerf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_place_mirrors_argument_validation(L):
    from mirror_nerf_amd import _lib
    assert (_lib.MNRF_MIRRORS_MAX, _lib.MNRF_MIRROR_AXIS, _lib.MNRF_MIRROR_FRAME, _lib.MNRF_MIRROR_RECT, _lib.MNRF_MIRROR_ELLIPSE) == (8, 0, 1, 0, 1)
    null = None

    def call(n, K=1, kinds=(0,), shapes=(0,), axes=(0,), ptrs=(null,) * 5, host=True):
        K_arr = max(K, 1)
        i = lambda v: (ctypes.c_int * max(len(v), K_arr, 8))(*v)  # noqa: E731
        f = lambda m: (ctypes.c_float * (m * 8))()  # noqa: E731
        h = (i(kinds), i(shapes), i(axes), f(1), f(9), f(3), f(4)) if host else (null,) * 7
        return L.mnrf_place_mirrors(ptrs[0], n, K, *h, 0.05, ptrs[1], ptrs[2], ptrs[3], ptrs[4], null, null, null, null)

    assert call(0) == 0                                        # zero rays: a no-op
    assert call(0, K=8, kinds=(0, 1) * 4, shapes=(1, 0) * 4, axes=(1, 0) * 4) == 0
    assert call(-1) < 0 and b"bad size" in L.mnrf_last_error()
    for K in (0, 9, -1):
        assert call(4, K=K) < 0 and b"n_mirrors" in L.mnrf_last_error()
        assert call(0, K=K) < 0 and b"n_mirrors" in L.mnrf_last_error()
    assert call(4, kinds=(2,)) < 0 and b"kind" in L.mnrf_last_error()
    assert call(4, K=2, kinds=(0, -1)) < 0 and b"kind" in L.mnrf_last_error()
    assert call(4, shapes=(2,)) < 0 and b"shape" in L.mnrf_last_error()
    assert call(4, axes=(2,)) < 0 and b"axis" in L.mnrf_last_error()
    assert call(0, kinds=(1,), axes=(7,)) == 0                 # a frame mirror has no axis
    assert call(4, host=False) < 0 and b"host array" in L.mnrf_last_error()
    assert call(4) < 0 and b"null pointer" in L.mnrf_last_error()
