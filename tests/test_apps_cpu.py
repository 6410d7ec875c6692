"""CPU-side checks of the scene-editing applications of batched_inference (app_place_new_mirror, app_reflection_substitution):
the preset tables against the reference's branch code (eval.py:369-433, 551-591), every refusal with its message, argument
validation of the two C-ABI entry points without a GPU, and a round trip of one fixture G19 through its generator (skipped
where the reference tree is absent)."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

# (plane_pos, root_dir) -> (axis, position, normal, rect) as eval.py:369-433 leaves them (last assignment wins)
PLACE = {
    ("plane_x", "/data/livingroom"): ("x", 0.0, (-1.0, 0.0, 0.0), (-1.0, 1.0, -0.5, 0.5)),
    ("plane_x", "/data/washroom"): ("x", -1.0, (1.0, 0.0, 0.0), (-1.0, 1.0, -1.0, 0.75)),
    ("plane_x", "/data/office"): ("x", 1.0, (1.0, 0.0, 0.0), (-1.0, 1.0, -1.0, 0.75)),
    ("plane_x", "/data/lego"): ("x", -1.0, (1.0, 0.0, 0.0), (-1.0, 1.0, -0.5, 0.5)),
    ("plane_y", "/data/washroom"): ("y", 1.3, (0.0, -1.0, 0.0), (-1.0, 1.0, -1.0, 1.0)),
    ("plane_y", "/data/livingroom"): ("y", 1.65, (0.0, -1.0, 0.0), (-0.3, 1.5, -0.5, 1.0)),
    ("plane_y", "/data/office"): ("y", 0.0, (0.0, -1.0, 0.0), (-1.0, 1.0, -0.5, 0.5)),
    ("plane_y", "/data/lego"): ("y", 1.0, (0.0, -1.0, 0.0), (-1.0, 1.0, -0.5, 0.5)),
}


@pytest.mark.parametrize("plane_pos,root_dir", list(PLACE), ids=[f"{a}:{b.rsplit('/', 1)[1]}" for a, b in PLACE])
def test_place_mirror_presets(plane_pos, root_dir):
    from mirror_nerf_amd.recursion import resolve_new_mirror
    axis, pos, normal, rect = PLACE[(plane_pos, root_dir)]
    got = resolve_new_mirror(SimpleNamespace(plane_pos=plane_pos, root_dir=root_dir))
    assert got == dict(axis=axis, position=pos, normal=normal, rect=rect)


def test_place_mirror_preset_order_and_override():
    from mirror_nerf_amd.recursion import resolve_new_mirror
    # the reference tests livingroom before washroom for plane_x and washroom first for plane_y (substring match, in order)
    assert resolve_new_mirror(SimpleNamespace(plane_pos="plane_x", root_dir="livingroom_washroom"))["position"] == 0.0
    assert resolve_new_mirror(SimpleNamespace(plane_pos="plane_y", root_dir="livingroom_washroom"))["position"] == 1.3
    # plane_pos defaults to plane_x as in eval.get_opt
    assert resolve_new_mirror(SimpleNamespace(root_dir="x"))["axis"] == "x"
    nm = dict(axis="y", position=0.25, normal=(0, 1, 0), rect=(0, 1, 2, 3))
    got = resolve_new_mirror(SimpleNamespace(plane_pos="plane_x", root_dir="office"), nm)
    assert got == dict(axis="y", position=0.25, normal=(0.0, 1.0, 0.0), rect=(0.0, 1.0, 2.0, 3.0))
    with pytest.raises(ValueError, match="axis must be"):
        resolve_new_mirror(None, dict(nm, axis="z"))
    with pytest.raises(ValueError, match="missing"):
        resolve_new_mirror(None, dict(axis="x", position=0.0))
    with pytest.raises(ValueError, match="plane_pos"):
        resolve_new_mirror(SimpleNamespace(plane_pos="plane_z", root_dir=""))


@pytest.mark.parametrize("root_dir,rotation,translation", [
    ("/data/office", None, (0.0, 1.0, 0.0)),
    ("/data/market", ((0.0, 1.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0)), (0.0, 0.0, 0.0)),
    ("/data/lego", None, (0.0, 0.0, 0.0)),
])
def test_substitution_presets(root_dir, rotation, translation):
    from mirror_nerf_amd.recursion import resolve_substitution
    assert resolve_substitution(SimpleNamespace(root_dir=root_dir)) == dict(rotation=rotation, scale=1.0, translation=translation)


def _models(mask_head=True):
    import mirror_nerf_amd as M
    return {"coarse": M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=mask_head)}


def _args(**over):
    a = dict(predict_normal=True, only_one_field=False, only_one_field_fine_epoch=2, max_recursive_level=1, near=0.05,
             root_dir="office")
    a.update(over)
    return a


@pytest.mark.parametrize("args,kw,exc,msg", [
    (_args(app_reflect_newly_placed_objects=True), {}, NotImplementedError, "UnboundLocalError"),
    (_args(app_place_new_mirror=True, app_control_mirror_roughness=True), {}, ValueError, "app_control_mirror_roughness cannot"),
    (_args(app_reflection_substitution=True, app_control_mirror_roughness=True), {"system_substitution": object()}, ValueError,
     "app_control_mirror_roughness cannot"),
    (_args(app_reflection_substitution=True), {}, ValueError, "needs system_substitution"),
    (_args(app_place_new_mirror=True, near=None), {}, ValueError, "needs args.near"),
], ids=["new_objects", "place_rough", "subst_rough", "subst_without_system", "place_without_near"])
def test_refusals(args, kw, exc, msg):
    import mirror_nerf_amd as M
    with pytest.raises(exc, match=msg):
        M.batched_inference(_models(), {}, torch.zeros(4, 8), 64, 64, False, 32, args=args, trace_secondary_rays=True, **kw)


def test_refusal_without_mirror_mask_head():
    import mirror_nerf_amd as M
    for flag in ("app_place_new_mirror", "app_reflection_substitution"):
        with pytest.raises(ValueError, match="needs a mirror-mask head"):
            M.batched_inference(_models(mask_head=False), {}, torch.zeros(4, 8), 64, 64, False, 32, args=_args(**{flag: True}),
                                system_substitution=object())


def test_place_and_substitution_together_are_not_refused():
    from mirror_nerf_amd.recursion import _refuse_apps
    _refuse_apps(SimpleNamespace(**_args(app_place_new_mirror=True, app_reflection_substitution=True)), _models(),
                 {"system_substitution": object()})


@pytest.fixture(scope="module")
def L():
    from mirror_nerf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_place_mirror_argument_validation(L):
    null = None
    f9 = [0.0] * 9

    def call(n, axis=0, ptrs=(null,) * 6):
        return L.mnrf_place_mirror(ptrs[0], n, axis, *f9, ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5], null, null)

    assert call(0) == 0                                        # zero rays: a no-op
    assert call(-1) < 0 and b"bad size" in L.mnrf_last_error()
    assert call(4) < 0 and b"null pointer" in L.mnrf_last_error()
    assert call(4, axis=2) < 0 and b"axis" in L.mnrf_last_error()


def test_transform_rays_argument_validation(L):
    assert L.mnrf_transform_rays(None, 0, None, 1.0, 0.0, 0.0, 0.0, None) == 0
    assert L.mnrf_transform_rays(None, -3, None, 1.0, 0.0, 0.0, 0.0, None) < 0 and b"bad size" in L.mnrf_last_error()
    assert L.mnrf_transform_rays(None, 4, None, 1.0, 0.0, 0.0, 0.0, None) < 0 and b"null pointer" in L.mnrf_last_error()


@pytest.mark.skipif(not os.path.isdir("/root/reference/models"), reason="the reference tree is not on this machine (GPU box)")
def test_g19_generator_reproduces_committed_fixture(tmp_path):
    name = "g19_place_y_livingroom"
    code = f"import sys; sys.path.insert(0, {GOLDEN!r}); import make_golden_apps as G; sys.argv[1:] = [{name!r}]; G.main()"
    env = dict(os.environ, MNRF_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", code], cwd=GOLDEN, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    new, old = np.load(tmp_path / f"{name}.npz"), np.load(os.path.join(GOLDEN, f"{name}.npz"))
    assert sorted(new.files) == sorted(old.files), sorted(set(new.files) ^ set(old.files))
    for k in old.files:
        if k == "meta":
            assert json.loads(str(new[k])) == json.loads(str(old[k]))
        else:
            assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape, k
            assert np.array_equal(new[k], old[k], equal_nan=True), k
