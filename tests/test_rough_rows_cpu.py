"""CPU-side checks of a roughness per placed mirror: PlacedMirror's `roughness`, the refusals and the allowed
combinations of batched_inference(rough_times=, scene_roughness=), the parsing of scripts/eval_scene.py (--mirrors_json entries
with "roughness", --rough_times, --scene_roughness), the argument validation of the three C entry points without a GPU, and the
numpy restatements (tests/rough_rows_ref.py) against the uniform route's (tests/rough_ref.py) where every std is the same."""
import ctypes
import importlib.util
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import rough_ref as RR
from tests import rough_rows_ref as RW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FRAME = dict(center=[0.3, -1.2, 0.8], normal=[0.2, -1.0, 0.17], up=[0, 0, 1], size=[1.5, 0.7])
AXIS = dict(axis="x", position=-1.0, normal=[1, 0, 0], rect=[-1, 1, -0.5, 0.5])


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ------------------------------------------------------------------------------------------------ PlacedMirror
def test_placed_mirror_roughness():
    from mirror_nerf_amd import PlacedMirror
    for make, kw in ((PlacedMirror, FRAME), (PlacedMirror.axis_aligned, AXIS)):
        plain = make(**kw)
        assert plain.roughness == 0.0 and isinstance(plain.roughness, float) and "roughness" not in repr(plain)
        m = make(**kw, roughness=0.1)
        assert m.roughness == float(F(0.1)) and m.roughness != 0.1, "rounded once to float32"
        assert f"roughness={m.roughness}" in repr(m)
        assert m.as_dict() == plain.as_dict() and "roughness" not in m.as_dict()
        assert make(**kw, roughness=np.float64(0.25)).roughness == 0.25 and make(**kw, roughness=0).roughness == 0.0
        for bad in (-0.01, float("nan"), float("inf"), -float("inf")):
            with pytest.raises(ValueError, match="roughness must be finite and not negative"):
                make(**kw, roughness=bad)
        with pytest.raises(ValueError, match="roughness"):
            make(**kw, roughness="frosted")


# ------------------------------------------------------------------------------------------------ batched_inference
def _models(mask_head=True):
    import mirror_nerf_amd as M
    return {name: M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=mask_head)
            for name in ("coarse", "fine")}


def _args(**over):
    a = dict(predict_normal=True, only_one_field=False, only_one_field_fine_epoch=2, max_recursive_level=1, near=0.05, root_dir="office")
    a.update(over)
    return SimpleNamespace(**a)


def _mirror(roughness=0.0):
    from mirror_nerf_amd import PlacedMirror
    return PlacedMirror(**FRAME, roughness=roughness)


def _object():
    from mirror_nerf_amd import PlacedObject
    return PlacedObject(SimpleNamespace(models={}, embeddings={}), dict(pose_align=None, scale=1.0, translation=(0, 0, 0)))


def _refuse(args, **kw):
    from mirror_nerf_amd.recursion import _refuse_apps
    return _refuse_apps(args, kw.pop("models", None) or _models(), dict(kw, _N_importance=64))


def test_allowed_combinations():
    objects = dict(placed_objects=[_object()])
    _refuse(_args(), rough_times=1)
    _refuse(_args(), rough_times=64, scene_roughness=0.01)
    _refuse(_args(), rough_times=np.int64(2), scene_roughness=np.float32(0.01))
    _refuse(_args(), rough_times=2, new_mirrors=[_mirror(0.03), _mirror()])
    _refuse(_args(), rough_times=2, scene_roughness=0.01, new_mirrors=[_mirror(0.03)] * 8)
    _refuse(_args(app_reflect_newly_placed_objects=True), rough_times=2, scene_roughness=0.01, **objects)
    _refuse(_args(app_reflect_newly_placed_objects=True), rough_times=2, new_mirrors=[_mirror(0.03)], **objects)
    # without the keywords nothing is new: polished mirrors and scene_roughness 0 pass as before
    _refuse(_args(), new_mirrors=[_mirror()])
    _refuse(_args(), new_mirrors=[_mirror()], scene_roughness=0.0)
    _refuse(_args(), rough_times=None)


@pytest.mark.parametrize("args,kw,msg", [
    (dict(app_control_mirror_roughness=True), {}, "rough_times= cannot be combined with app_control_mirror_roughness: one roughness rule per call"),
    (dict(app_control_mirror_roughness=True), dict(new_mirrors="m"), "rough_times= cannot be combined with app_control_mirror_roughness"),
    (dict(app_place_new_mirror=True), {}, "rough_times= cannot be combined with app_place_new_mirror or new_mirror="),
    (dict(), dict(new_mirror=dict(AXIS)), "rough_times= cannot be combined with app_place_new_mirror or new_mirror="),
    (dict(app_reflect_newly_placed_objects=True, obj_model_type="nerf_pl"), dict(system_obj=object()), r"rough_times= is combined with objects through placed_objects=.*system_obj="),
    (dict(app_reflect_newly_placed_objects=True), dict(render_kwargs_test_d_nerf={}, frame_time=0.5), "rough_times= is combined with objects through placed_objects="),
    (dict(app_reflect_newly_placed_objects=True), {}, "app_reflect_newly_placed_objects without placed_objects="),
    (dict(), dict(object_bounds="auto"), r"rough_times= is combined with objects.*object_bounds="),
    (dict(app_reflection_substitution=True), dict(system_substitution=object()), "rough_times= cannot be combined with app_reflection_substitution"),
    (dict(app_reflection_substitution=True), dict(system_substitution=object(), new_mirrors="m"), "rough_times= cannot be combined with app_reflection_substitution"),
], ids=["flag", "flag_beside_mirrors", "place", "new_mirror", "system_obj", "dnerf_keyword", "objects_without_list", "object_bounds", "subst",
        "subst_beside_mirrors"])
def test_refusals(args, kw, msg):
    if kw.get("new_mirrors") == "m":
        kw = dict(kw, new_mirrors=[_mirror(0.03)])
    with pytest.raises(ValueError, match=msg):
        _refuse(_args(**args), rough_times=2, scene_roughness=0.01, **kw)


def test_refusals_of_the_keywords_themselves():
    for bad in (0, -1, 2.0, "4", True):
        with pytest.raises(ValueError, match="rough_times is an int of at least 1"):
            _refuse(_args(), rough_times=bad)
    for bad in (-0.01, float("nan"), float("inf"), "rough"):
        with pytest.raises(ValueError, match="scene_roughness"):
            _refuse(_args(), rough_times=2, scene_roughness=bad)
    # without rough_times nobody would read them: refused with the reason
    with pytest.raises(ValueError, match=r"new_mirrors\[1\] has roughness .* pass rough_times=T"):
        _refuse(_args(), new_mirrors=[_mirror(), _mirror(0.03)])
    with pytest.raises(ValueError, match="scene_roughness=0.01 is read by the per-mirror roughness route alone: pass rough_times=T"):
        _refuse(_args(), scene_roughness=0.01)
    # the list's own refusals come first, as before
    with pytest.raises(ValueError, match="needs args.near"):
        _refuse(_args(near=None), new_mirrors=[_mirror(0.03)])


def test_refusal_through_batched_inference_and_the_flag_keeps_its_own():
    import mirror_nerf_amd as M
    rays = torch.zeros(4, 8)
    with pytest.raises(ValueError, match="one roughness rule per call"):
        M.batched_inference(_models(), {}, rays, 64, 64, False, 32, args=vars(_args(app_control_mirror_roughness=True)), rough_times=2)
    with pytest.raises(ValueError, match="pass rough_times=T"):
        M.batched_inference(_models(), {}, rays, 64, 64, False, 32, args=vars(_args()), new_mirrors=[_mirror(0.03)])
    # args.app_control_mirror_roughness without the new keywords: the refusals of before, word for word
    with pytest.raises(ValueError, match="app_control_mirror_roughness cannot be combined with new_mirrors="):
        _refuse(_args(app_control_mirror_roughness=True), new_mirrors=[_mirror()])
    with pytest.raises(ValueError, match="app_control_mirror_roughness cannot be combined with app_place_new_mirror"):
        _refuse(_args(app_control_mirror_roughness=True, app_place_new_mirror=True))


def test_roughness_row():
    from mirror_nerf_amd.placed_mirrors import roughness_row
    K, row = roughness_row([_mirror(0.1), _mirror(), _mirror(0.5)])
    assert K == 3 and list(row)[:3] == [float(F(0.1)), 0.0, 0.5]
    K, row = roughness_row(None)
    assert K == 0 and len(row) >= 1


# ------------------------------------------------------------------------------------------------ scripts/eval_scene.py
def _eval_scene():
    spec = importlib.util.spec_from_file_location("eval_scene", os.path.join(ROOT, "scripts", "eval_scene.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_mirrors_json_with_roughness(tmp_path):
    from mirror_nerf_amd import PlacedMirror
    ES = _eval_scene()
    path = tmp_path / "mirrors.json"
    path.write_text(json.dumps([dict(FRAME, roughness=0.03), dict(AXIS, shape="ellipse", roughness=0.1), FRAME, dict(AXIS, roughness=None)]))
    got = ES.read_mirrors_json(str(path))
    assert [m.roughness for m in got] == [float(F(0.03)), float(F(0.1)), 0.0, 0.0]
    assert got[0].as_dict() == PlacedMirror(**FRAME).as_dict() and got[1].as_dict() == PlacedMirror.axis_aligned(**AXIS, shape="ellipse").as_dict()
    for bad in (-1.0, "x"):
        path.write_text(json.dumps([FRAME, dict(FRAME, roughness=bad)]))
        with pytest.raises(SystemExit, match="mirror 1: .*roughness") as e:
            ES.read_mirrors_json(str(path))
        assert str(path) in str(e.value)


def test_rough_flags(capsys):
    ES = _eval_scene()
    base = ["--root_dir", "r", "--ckpt_path", "c", "--out_dir", "o"]
    a = ES.get_opts(base)
    assert a.rough_times is None and a.scene_roughness == 0.0
    a = ES.get_opts(base + ["--rough_times", "4", "--scene_roughness", "0.02", "--mirrors_json", "m.json", "--normal_noise_std_changes"])
    assert a.rough_times == 4 and a.scene_roughness == 0.02 and not a.app_control_mirror_roughness
    assert ES.get_opts(base + ["--rough_times", "1"]).scene_roughness == 0.0
    for extra, word in ((["--rough_times", "4", "--app_control_mirror_roughness"], "one roughness rule per call"),
                        (["--rough_times", "4", "--app_place_new_mirror"], "app_place_new_mirror"),
                        (["--rough_times", "4", "--app_reflect_newly_placed_objects", "--obj_ckpt_path", "x"], "--objects_json"),
                        (["--rough_times", "0"], "at least 1"),
                        (["--rough_times", "2", "--scene_roughness", "-1"], "--scene_roughness"),
                        (["--rough_times", "2", "--scene_roughness", "nan"], "--scene_roughness"),
                        (["--scene_roughness", "0.01"], "--rough_times")):
        with pytest.raises(SystemExit):
            ES.get_opts(base + extra)
        assert word in capsys.readouterr().err, extra


# ------------------------------------------------------------------------------------------------ the C entry points
@pytest.fixture(scope="module")
def L():
    from mirror_nerf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_argument_validation_without_a_launch(L):
    null, some = None, ctypes.c_void_p(256)            # (a pointer that is only compared with null: every call below returns before a launch)
    row = lambda *v: (ctypes.c_float * 8)(*v)  # noqa: E731

    def rows(n, K=1, rough=row(0.0), scene=0.0, ptrs=(null,) * 3):
        return L.mnrf_rough_rows(null, ptrs[0], n, K, rough, scene, ptrs[1], ptrs[2], null, null)

    assert rows(0) == 0 and rows(0, K=0, rough=None) == 0 and rows(0, K=8, rough=row(*[0.1] * 8)) == 0      # zero rays: a no-op
    assert rows(-1) < 0 and b"mnrf_rough_rows: bad size" in L.mnrf_last_error()
    assert rows(2 ** 31) < 0 and b"bad size" in L.mnrf_last_error()
    for K in (-1, 9):
        assert rows(4, K=K) < 0 and b"n_mirrors" in L.mnrf_last_error()
    assert rows(4, rough=None) < 0 and b"host array" in L.mnrf_last_error()
    for bad in (-0.5, float("nan"), float("inf")):
        assert rows(0, K=2, rough=row(0.1, bad)) < 0 and b"a roughness must be finite" in L.mnrf_last_error()
        assert rows(0, scene=bad) < 0 and b"scene_roughness must be finite" in L.mnrf_last_error()
    assert rows(4) < 0 and b"mnrf_rough_rows: null pointer" in L.mnrf_last_error()
    assert rows(4, ptrs=(some, some, null)) < 0 and b"null pointer" in L.mnrf_last_error()

    assert L.mnrf_perturb_normals(null, null, null, 0, null, null) == 0
    assert L.mnrf_perturb_normals(some, some, some, -1, some, null) < 0 and b"mnrf_perturb_normals: bad size" in L.mnrf_last_error()
    assert L.mnrf_perturb_normals(some, some, some, 2 ** 31, some, null) < 0 and b"bad size" in L.mnrf_last_error()
    for k in range(4):
        ptrs = [some] * 4
        ptrs[k] = null
        assert L.mnrf_perturb_normals(ptrs[0], ptrs[1], ptrs[2], 4, ptrs[3], null) < 0 and b"mnrf_perturb_normals: null pointer" in L.mnrf_last_error()

    def fan(m, n, n_jit, ptrs=(some,) * 6):
        return L.mnrf_reflect_jitter_fan_rows(ptrs[0], ptrs[1], ptrs[2], some, ptrs[3], ptrs[4], m, n, n_jit, 0.1, ptrs[5], null)

    assert fan(0, 4, 1) == 0 and fan(0, 0, 3, (null,) * 6) == 0           # m == 0: nothing is touched
    for m, n in ((-1, 4), (4, -1), (5, 4), (1, 2 ** 31)):
        assert fan(m, n, 1) < 0 and b"mnrf_reflect_jitter_fan_rows: bad size" in L.mnrf_last_error()
    for n_jit in (0, -3):
        assert fan(4, 4, n_jit) < 0 and b"n_jit must be at least 1" in L.mnrf_last_error()
        assert fan(0, 4, n_jit) < 0 and b"n_jit" in L.mnrf_last_error()
    for k in range(6):                                                     # rays, x_surface, normal, std_rows, index, sec
        ptrs = [some] * 6
        ptrs[k] = null
        assert fan(4, 4, 1, ptrs) < 0 and b"mnrf_reflect_jitter_fan_rows: null pointer" in L.mnrf_last_error()
    assert fan(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1) < 0 and b"too large for one launch" in L.mnrf_last_error()


# ------------------------------------------------------------------------------------------------ the restatements
def _case(n, seed):
    rs = np.random.RandomState(seed)
    rays, xs, nrm = rs.normal(size=(n, 8)).astype(F), rs.normal(size=(n, 3)).astype(F), rs.normal(size=(n, 3)).astype(F)
    noise = rs.normal(size=(3, n, 3)).astype(F)
    mask = rs.choice(np.array([0.0, 0.5, 1.0], F), size=n)
    if n > 3:
        nrm[1], nrm[2], noise[1, 3, 0] = 0.0, np.nan, np.nan
    return rays, xs, nrm, noise, mask


@pytest.mark.parametrize("n", [1, 65, 321])
def test_restatements_with_one_std_are_the_uniform_routes(n):
    rays, xs, nrm, noise, mask = _case(n, n)
    for std in (0.01, 0.3):
        rows = RW.rough_rows_ref(None, mask, [], std)
        assert (rows["std_rows"] == F(std)).all() and np.array_equal(rows["jitter_mask"], (mask != 0).astype(F))
        index = np.nonzero(rows["jitter_mask"])[0].astype(np.int32) if rows["any"] else np.arange(n, dtype=np.int32)
        got = RW.reflect_jitter_fan_rows_ref(rays, xs, nrm, noise, rows["std_rows"], index, 0.1)
        want = RR.reflect_jitter_fan_ref(rays, xs, nrm, noise, std, index, 0.1)
        assert np.array_equal(_bits(got), _bits(want))
        got = RW.reflect_jitter_fan_rows_ref(rays, xs, nrm, (2, None), rows["std_rows"], index, 0.1)
        assert np.array_equal(_bits(got), _bits(RR.reflect_jitter_fan_ref(rays, xs, nrm, (2, None), std, index, 0.1)))
        first = RW.first_reflection_ref(nrm, noise[0], rows["std_rows"], rays[:, 3:6])
        assert np.array_equal(_bits(first), _bits(RR.reflect_direction_ref(nrm, noise[0], std, rays[:, 3:6])))


def test_restatement_rules():
    """std by index, with the out-of-range rows; J; a std of 0 adds nothing -- a -0 stays -0 and a NaN draw does not reach the row."""
    index = np.array([-1, 0, 1, 2, 3, -5, 2 ** 31 - 1, 1], np.int32)
    mask = np.array([1, 1, 1, 0, 0.5, 1, 0, 1], F)
    rows = RW.rough_rows_ref(index, mask, [0.1, 0.0, 0.2], 0.05, any_in=4)
    assert rows["std_rows"].tolist() == [float(F(v)) for v in (0.05, 0.1, 0.0, 0.2, 0.05, 0.05, 0.05, 0.0)]
    assert rows["jitter_mask"].tolist() == [1, 1, 0, 0, 1, 1, 0, 0] and rows["any"] == 5
    assert RW.rough_rows_ref(index, mask, [0.0] * 3, 0.0, any_in=4)["any"] == 4
    assert RW.rough_rows_ref(None, np.zeros(5, F), [], 0.05)["any"] == 0
    nrm = np.array([[-0.0, 1.0, 0.0], [0.5, 0.5, 0.5]], F)
    draw = np.array([[1.0, np.nan, 2.0], [1.0, 2.0, 3.0]], F)
    out = RW.perturb_normals_ref(nrm, draw, np.array([0.0, 0.5], F))
    assert np.array_equal(_bits(out[0]), _bits(nrm[0])) and out[1].tolist() == [1.0, 1.5, 2.0]
    assert np.isnan(RW.perturb_normals_ref(nrm, draw, np.array([0.5, 0.5], F))[0, 1])
