"""CPU-side checks of app_reflect_newly_placed_objects in batched_inference: the preset table against the reference's branch
code (eval.py:177-190), the `new_object=` override and its validation, every refusal with its message, argument validation of
the two C-ABI entry points without a GPU, load_object_system on a checkpoint in nerf_pl's layout, and a round trip of one
fixture G26 through its generator (skipped where the reference tree is absent)."""
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


@pytest.mark.parametrize("root_dir,scale,translation", [
    ("/data/livingroom", 2.0, (0.0, 0.0, 0.0)),
    ("/data/washroom", 2.0, (-0.5, -0.5, 0.0)),
    ("/data/office", 2.0, (0.0, 3.0, 0.5)),
    ("/data/lego", 1.0, (0.0, 0.0, 0.0)),
    ("", 1.0, (0.0, 0.0, 0.0)),
])
def test_object_presets(root_dir, scale, translation):
    from mirror_nerf_amd.recursion import resolve_new_object
    assert resolve_new_object(SimpleNamespace(root_dir=root_dir)) == dict(pose=None, scale=scale, translation=translation,
                                                                          pose_scale0=1.0)


def test_object_preset_order():
    """eval.py:180-190 is an if / elif chain: livingroom before washroom before office (substring match)."""
    from mirror_nerf_amd.recursion import OBJECT_PRESETS, resolve_new_object
    assert [k for k, _ in OBJECT_PRESETS] == ["livingroom", "washroom", "office", None]
    assert all(v["pose_align"] is None for _, v in OBJECT_PRESETS)
    assert resolve_new_object(SimpleNamespace(root_dir="office_washroom"))["translation"] == (-0.5, -0.5, 0.0)
    assert resolve_new_object(SimpleNamespace(root_dir="washroom_livingroom"))["translation"] == (0.0, 0.0, 0.0)
    assert resolve_new_object(SimpleNamespace(root_dir="office_livingroom"))["translation"] == (0.0, 0.0, 0.0)
    assert resolve_new_object(SimpleNamespace())["scale"] == 1.0          # no root_dir at all: the reference's `else`


def test_new_object_override_and_validation():
    from mirror_nerf_amd.recursion import resolve_new_object
    args = SimpleNamespace(root_dir="office")
    got = resolve_new_object(args, dict(pose_align=None, scale=3, translation=[1, 2, 3]))
    assert got == dict(pose=None, scale=3.0, translation=(1.0, 2.0, 3.0), pose_scale0=1.0)
    pose = np.eye(4)
    pose[:3, :3] = 1.25 * np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    pose[:3, 3] = (0.1, -0.2, 0.05)
    for p in (pose, pose[:3], pose.tolist()):
        got = resolve_new_object(args, dict(pose_align=p, scale=2.0, translation=(0, 0, 0)))
        assert got["pose"] == tuple(float(np.float32(v)) for v in pose[:3].reshape(-1))
        # the fp32 norm of the first column of the 3x3 (eval.py:194-196)
        assert got["pose_scale0"] == float(torch.norm(torch.tensor(pose[:3, 0], dtype=torch.float32)))
        assert abs(got["pose_scale0"] - 1.25) < 1e-6
    assert resolve_new_object(None, dict(pose_align=np.eye(4), scale=1, translation=(0, 0, 0)))["pose_scale0"] == 1.0
    with pytest.raises(ValueError, match="missing"):
        resolve_new_object(args, dict(scale=1.0))
    with pytest.raises(ValueError, match="3x4 or 4x4"):
        resolve_new_object(args, dict(pose_align=np.eye(3), scale=1.0, translation=(0, 0, 0)))
    with pytest.raises(ValueError, match="3 entries"):
        resolve_new_object(args, dict(pose_align=None, scale=1.0, translation=(0, 0)))
    with pytest.raises(ValueError, match="positive"):
        resolve_new_object(args, dict(pose_align=None, scale=0.0, translation=(0, 0, 0)))
    with pytest.raises(ValueError, match="first column"):
        resolve_new_object(args, dict(pose_align=np.zeros((3, 4)), scale=1.0, translation=(0, 0, 0)))


def _models(fine=True, mask_head=True):
    import mirror_nerf_amd as M
    make = lambda: M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=mask_head)  # noqa: E731
    return {"coarse": make(), "fine": make()} if fine else {"coarse": make()}


def _args(**over):
    a = dict(predict_normal=True, only_one_field=False, only_one_field_fine_epoch=2, max_recursive_level=1, near=0.05,
             root_dir="office", app_reflect_newly_placed_objects=True, obj_model_type="nerf_pl")
    a.update(over)
    return a


OBJ = {"system_obj": SimpleNamespace(models=[], embeddings=[])}


@pytest.mark.parametrize("args,kw,models,n_imp,exc,msg", [
    (_args(obj_model_type="d_nerf"), OBJ, _models, 64, NotImplementedError, "UnboundLocalError"),
    (_args(obj_model_type="d_nerf"), OBJ, _models, 64, NotImplementedError, "D-NeRF"),
    (_args(obj_model_type="d_nerf"), OBJ, _models, 64, NotImplementedError, "obj_model_type='nerf_pl'"),
    ({k: v for k, v in _args().items() if k != "obj_model_type"}, OBJ, _models, 64, NotImplementedError, "UnboundLocalError"),
    (_args(obj_model_type="tensorf"), OBJ, _models, 64, ValueError, "obj_model_type must be"),
    (_args(), {}, _models, 64, ValueError, "needs system_obj="),
    (_args(app_place_new_mirror=True), OBJ, _models, 64, ValueError, "cannot be combined with app_place_new_mirror"),
    (_args(app_reflection_substitution=True), dict(OBJ, system_substitution=object()), _models, 64, ValueError,
     "cannot be combined with app_reflection_substitution"),
    (_args(app_control_mirror_roughness=True), OBJ, _models, 64, ValueError, "cannot be combined with app_control_mirror_roughness"),
    (_args(), OBJ, _models, 0, ValueError, "needs a fine mirror mask"),
    (_args(only_one_field=True), OBJ, _models, 64, ValueError, "needs a fine mirror mask"),
    (_args(), OBJ, lambda: _models(fine=False), 64, ValueError, "needs a fine mirror mask"),
    (_args(), OBJ, lambda: _models(mask_head=False), 64, ValueError, "needs a fine mirror mask"),
    (_args(near=None), OBJ, _models, 64, ValueError, "needs args.near"),
], ids=["d_nerf", "d_nerf_names_the_model", "d_nerf_points_to_nerf_pl", "default_type_is_d_nerf", "unknown_type", "without_system",
        "with_place", "with_substitution", "with_roughness", "no_importance", "one_field", "no_fine_model", "no_mask_head",
        "without_near"])
def test_refusals(args, kw, models, n_imp, exc, msg):
    import mirror_nerf_amd as M
    with pytest.raises(exc, match=msg):
        M.batched_inference(models(), {}, torch.zeros(4, 8), 64, n_imp, False, 32, args=args, trace_secondary_rays=True, **kw)


@pytest.fixture(scope="module")
def L():
    from mirror_nerf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_object_entry_points_validate_their_arguments(L):
    null = None
    assert L.mnrf_object_rays(null, 0, null, 1.0, 0.0, 0.0, 0.0, null, null) == 0              # zero rays: a no-op
    assert L.mnrf_object_rays(null, -1, null, 1.0, 0.0, 0.0, 0.0, null, null) < 0 and b"bad size" in L.mnrf_last_error()
    assert L.mnrf_object_rays(null, 4, null, 1.0, 0.0, 0.0, 0.0, null, null) < 0 and b"null pointer" in L.mnrf_last_error()
    assert L.mnrf_object_rays(64, 4, null, 1.0, 0.0, 0.0, 0.0, 64, null) < 0 and b"out of place" in L.mnrf_last_error()
    assert L.mnrf_object_merge(null, null, null, 0, 1.0, 1.0, 0.05, null, null, null, null, null) == 0
    assert L.mnrf_object_merge(null, null, null, -2, 1.0, 1.0, 0.05, null, null, null, null, null) < 0 and b"bad size" in L.mnrf_last_error()
    assert L.mnrf_object_merge(null, null, null, 4, 1.0, 1.0, 0.05, null, null, null, null, null) < 0
    assert b"null pointer" in L.mnrf_last_error()


def test_load_object_system_reads_a_nerf_pl_checkpoint(tmp_path):
    """nerf_pl's NeRF (models/nerf_pl/nerf_nerfpl.py:42-109) names its parameters like MirrorNeRF without the optional heads."""
    from mirror_nerf_amd.recursion import _object_system, load_object_system
    from mirror_nerf_amd.synthetic import make_state_dict
    sds = make_state_dict(7, 2, predict_normal=False, predict_mirror_mask=False)
    assert list(sds[0]) == [f"xyz_encoding_{i}.0.{p}" for i in range(1, 9) for p in ("weight", "bias")] + \
        [f"{n}.{p}" for n in ("xyz_encoding_final", "dir_encoding.0", "sigma", "rgb.0") for p in ("weight", "bias")]
    state = {f"nerf_{n}.{k}": torch.from_numpy(v) for n, sd in zip(("coarse", "fine"), sds) for k, v in sd.items()}
    path = tmp_path / "object.ckpt"
    torch.save({"state_dict": state, "epoch": 3}, str(path))
    for src in (str(path), {"state_dict": state}):
        system = load_object_system(src, "cpu", 64)
        assert list(system.models) == ["coarse", "fine"] and (system.embeddings["xyz"].N_freqs, system.embeddings["dir"].N_freqs) == (10, 4)
        for sd, m in zip(sds, system.models.values()):
            assert not m.predict_normal and not m.predict_mirror_mask and not m.training
            got = m.state_dict()
            assert list(got) == list(sd)
            for k in sd:
                assert np.array_equal(got[k].numpy(), sd[k]), k
    assert list(load_object_system({"state_dict": state}, "cpu", 0).models) == ["coarse"]
    with pytest.raises(AssertionError, match="nerf_coarse"):
        load_object_system({"state_dict": {"model.sigma.weight": torch.zeros(1, 256)}}, "cpu", 64)
    # nerf_pl's own containers: lists
    models, embeddings = _object_system(SimpleNamespace(models=list(system.models.values()), embeddings=list(system.embeddings.values())))
    assert list(models) == ["coarse", "fine"] and list(embeddings) == ["xyz", "dir"]


def test_fixture_files_exist_and_are_small():
    src = open(os.path.join(GOLDEN, "make_golden_objects.py")).read()
    for name in ("g26_object_office_l2", "g26_object_default_chunk96", "g26_object_posed_l1"):
        assert name in src and os.path.isfile(os.path.join(GOLDEN, name + ".npz"))
        assert os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 400 * 1024


def test_fixture_conditions():
    """What the generator asserted, as stored: each class at level 0 holds >= 15 % of the rays, the object is seen in the
    mirrors, at most 5 % of the candidates sat on a decision edge."""
    from tests.golden import fixtures as FX
    for name in FX.names("g26_object_"):
        m = FX.Fixture(name).meta
        c = m["conditions"]
        n = c["per_level"]["0"]["rays"]
        assert n == c["candidates"] - c["dropped"] and c["dropped"] <= 0.05 * c["candidates"]
        for k in ("transparent", "blocked", "used"):
            assert c["per_level"]["0"][k] >= 0.15 * n, (name, k)
        assert c["per_level"]["1"]["used"] > 0
        assert m["args"]["obj_model_type"] == "nerf_pl" and len(m["obj_tweaks"]) == 2 and len(m["obj_checksum"]) == 2
    assert FX.Fixture("g26_object_default_chunk96").meta["chunk"] == 96
    assert FX.Fixture("g26_object_office_l2").meta["args"]["max_recursive_level"] == 2
    pose = np.asarray(FX.Fixture("g26_object_posed_l1").meta["new_object"]["pose_align"])
    assert abs(np.linalg.norm(pose[:3, 0]) - 1.25) < 1e-5 and np.abs(pose[:3, 3]).max() > 0 and abs(pose[0, 1]) > 0.1


@pytest.mark.skipif(not os.path.isdir("/root/reference/models"), reason="the reference tree is not on this machine (GPU box)")
def test_g26_generator_reproduces_committed_fixture(tmp_path):
    name = "g26_object_posed_l1"
    code = f"import sys; sys.path.insert(0, {GOLDEN!r}); import make_golden_objects as G; sys.argv[1:] = [{name!r}]; G.main()"
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
