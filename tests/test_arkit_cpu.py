"""`data.read_arkit` against the reference's own RealDatasetARKit (fixtures G24, G25: tests/golden/make_golden_poses.py) on the
scene of tests/arkit_scene.py, written here as lossless PNGs.  Focal, near and far exactly; poses to 1e-10 (float64 closed forms
on both sides); images and masks with tolerance zero -- through the reference's `rgbs` and `mirror_mask`, which are exact
functions of the bytes.  The masks' reader and resize are PIL and data._resize_nearest on both sides (the fixture's stand-ins
for cv2), so the fixture pins the class's logic around them, not cv2."""
import numpy as np
import pytest

from tests import arkit_scene as SC
from tests.golden.fixtures import Fixture

TOL = 1e-10


@pytest.fixture(scope="module")
def g25():
    return Fixture("g25_arkit_train")


@pytest.fixture(scope="module")
def scene(tmp_path_factory, g25):
    root = str(tmp_path_factory.mktemp("arkit") / "lounge")
    SC.write_scene(root, g25.inputs["poses"], g25.inputs["key_poses"])
    return root


def _read(root, split, **kw):
    from mirror_nerf_amd.data import read_arkit
    return read_arkit(root, split, SC.IMG_WH, SC.NEAR, SC.FAR, SC.SCALE_FACTOR, val_idx=SC.VAL_IDX, **kw)


def reference_rgbs(images):
    """datasets/real_arkit.py:238-243 on the bytes: ToTensor's / 255 and the alpha blend, in float32."""
    a = images.reshape(-1, images.shape[-1]).astype(np.float32) / np.float32(255)
    return a[:, :3] * a[:, 3:] + (1 - a[:, 3:]) if a.shape[1] == 4 else a


def test_train_split(scene, g25):
    """Largest pose difference seen: 0."""
    d = _read(scene, "train")
    o = g25.outputs
    assert [d["focal"], d["near"], d["far"]] == o["train__focal_near_far"].tolist()
    assert d["poses_f64"].shape == (6, 3, 4) and d["poses"].dtype == np.float32
    err = float(np.abs(d["poses_f64"] - o["poses"][:, :3, :4]).max())
    print(f"train poses: max abs difference {err:.3e}")
    assert err <= TOL
    assert np.array_equal(d["poses"], d["poses_f64"].astype(np.float32))
    assert np.abs(d["pose_avg"] - o["pose_avg"]).max() <= TOL
    assert d["images"].shape == (6, 6, 8, 4) and d["images"].dtype == np.uint8        # one RGBA frame: the others get alpha 255
    assert (d["images"][[0, 2, 3, 4, 5], ..., 3] == 255).all()
    assert np.array_equal(reference_rgbs(d["images"]), o["rgbs"])
    assert d["masks"].dtype == np.int8 and np.array_equal(d["masks"].reshape(-1).astype(np.float32), o["mirror_mask"])
    assert (d["masks"][SC.NO_MASK_FRAME] == -1).all() and set(np.unique(d["masks"][SC.MASK16_FRAME])) == {0, 1}
    from mirror_nerf_amd.data import frames_with_mask
    assert frames_with_mask(d["masks"]) == o["frames_with_mask"].tolist() == [0, 1, 3, 4, 5]
    assert np.array_equal(d["images"][SC.RGBA_FRAME, ..., 3].reshape(-1) > 0, o["valid_mask_rgba_frame"])
    assert d["file_paths"] == [SC.frame_name(k) for k in range(6)]


def test_skip_step_val_and_test_splits(scene, g25):
    full = _read(scene, "train")
    d = _read(scene, "train", train_skip_step=2)
    # frames 0, 2, 4: none of them is the RGBA frame, so this bank has three channels
    assert np.array_equal(d["images"], full["images"][::2, ..., :3]) and np.array_equal(d["poses_f64"], full["poses_f64"][::2])
    assert np.array_equal(d["masks"], full["masks"][::2])
    assert np.array_equal(d["pose_avg"], full["pose_avg"])                 # from transforms.json, whatever the split keeps
    # fx and cx at the top level; one frame, val_idx.  That frame is RGB and alone, so it keeps three channels
    v = _read(scene, "val")
    assert [v["focal"], v["near"], v["far"]] == g25.outputs["val__focal_near_far"].tolist()
    assert v["images"].shape == (1, 6, 8, 3) and np.array_equal(v["images"][0], full["images"][SC.VAL_IDX, ..., :3])
    assert np.array_equal(v["poses_f64"][0], full["poses_f64"][SC.VAL_IDX]) and v["file_paths"] == [SC.frame_name(SC.VAL_IDX)]
    # fx and cx from frame 0's intrinsics; every frame; the skip step is the train split's alone
    t = _read(scene, "test", train_skip_step=2)
    assert [t["focal"], t["near"], t["far"]] == g25.outputs["test__focal_near_far"].tolist()
    assert np.array_equal(t["images"], full["images"]) and np.array_equal(t["masks"], full["masks"])
    assert v["focal"] == t["focal"] == SC.FX * (8 / (SC.CX * 2)) and full["focal"] != v["focal"]
    with pytest.raises(ValueError, match="split"):
        _read(scene, "test_draw")


@pytest.mark.parametrize("split,n", [("test_rotate", 32), ("test_interpolation", 64)])
def test_path_splits(scene, split, n):
    """Largest pose difference seen: 0 (test_rotate), 4.4e-16 (test_interpolation)."""
    fx = Fixture("g24_arkit_paths")
    d = _read(scene, split)
    assert d["images"] is None and d["masks"] is None and d["file_paths"] is None
    want = fx.outputs[f"{split}__poses"]
    assert fx.meta["n_frames"][split] == n and d["poses_f64"].shape == (n, 3, 4)
    err = float(np.abs(d["poses_f64"] - want[:, :3, :4]).max())
    print(f"{split} poses: max abs difference {err:.3e}")
    assert err <= TOL
    assert [d["focal"], d["near"], d["far"]] == [float(fx.outputs[f"{split}__{k}"]) for k in ("focal", "near", "far")]


def test_rotate_preset_by_directory_name(tmp_path):
    """A directory whose name contains `market`: frame 77 of transforms.json, lowered by 0.3 (real_arkit.py:155-159); without
    transforms_test_rotate.json the intrinsics come from transforms.json.  (The test's own name must not contain the word:
    it is part of tmp_path.)"""
    import os
    fx = Fixture("g24_arkit_market")
    root = str(tmp_path / "market_small")
    SC.write_scene(root, fx.inputs["poses"], fx.inputs["key_poses"], images=False)
    d = _read(root, "test_rotate")
    assert np.abs(d["poses_f64"] - fx.outputs["test_rotate__poses"][:, :3, :4]).max() <= TOL
    other = str(tmp_path / "bazaar")
    SC.write_scene(other, fx.inputs["poses"], fx.inputs["key_poses"], images=False)
    assert np.abs(_read(other, "test_rotate")["poses_f64"] - d["poses_f64"]).max() > 0.1       # frame val_idx there
    os.remove(os.path.join(root, "transforms_test_rotate.json"))
    again = _read(root, "test_rotate")
    assert np.array_equal(again["poses_f64"], d["poses_f64"]) and again["focal"] == d["focal"]
