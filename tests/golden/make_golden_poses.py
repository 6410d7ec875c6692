#!/usr/bin/env python3
"""Fixtures G23-G25: the pose helpers and the real-capture reader captured from the reference.  Build-container only:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_poses.py

  g23_poses          datasets/geo_utils.py (numpy only, imported by path) on seeded inputs: every function poses.py restates
  g24_arkit_paths    the reference's own RealDatasetARKit for test_rotate and test_interpolation on the six-frame scene of
                     tests/arkit_scene.py at 8x6: the poses of the path and the rays of two frames per split
  g24_arkit_market   test_rotate again on a scene of 80 poses whose directory name contains "market" (frame 77, z - 0.3)
  g25_arkit_train    the class on the train split of that scene (lossless PNGs; one RGBA frame, one without a mask file, one
                     with a 16-bit mask): rays, rgbs and mirror_mask of every training ray, the frames of the *_wmask
                     buffers, the poses, valid_mask of the RGBA frame (from the test_train split), and focal / near / far
                     for the three ways the focal length is given

The class runs UNCHANGED, with the stand-ins of _ref_import.install() plus three installed here, none of which is pinned
against the package it stands in for:
  * torchvision.transforms.ToTensor: a PIL image or a uint8 array becomes float32 CHW / 255; any other array is converted
    unscaled (torchvision does not scale 16-bit input);
  * cv2.imread(path, IMREAD_ANYDEPTH): PIL -- a 16-bit file as uint16, anything else as 8-bit grey; None without a file;
  * cv2.resize(m, wh, interpolation=INTER_NEAREST): the repository's statement of that rule, data._resize_nearest.
The key frames of the interpolated path are drawn so that consecutive rotations differ by about 50 degrees, far below the
half turn where the log map loses its condition."""
import importlib
import os
import sys
import tempfile
import types
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

import _ref_import as R  # noqa: E402

from make_golden import save  # noqa: E402
from tests import arkit_scene as SC  # noqa: E402


def geo_utils():
    spec = importlib.util.spec_from_file_location("ref_geo_utils", os.path.join(R.REF_ROOT, "datasets", "geo_utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def arkit_class():
    """datasets/real_arkit.py imported as a module of a package that has the reference's datasets directory as its path (the
    package's own __init__ pulls every dataset class)."""
    R.install()
    import torch
    from PIL import Image
    from mirror_nerf_amd.data import _resize_nearest

    class ToTensor:
        def __call__(self, pic):
            if isinstance(pic, Image.Image):
                pic = np.asarray(pic)
            a = np.asarray(pic)
            if a.ndim == 2:
                a = a[:, :, None]
            t = torch.from_numpy(np.ascontiguousarray(a.transpose(2, 0, 1)).astype(np.float32 if a.dtype != np.float64 else np.float64))
            return t / 255 if a.dtype == np.uint8 else t

    def imread(path, flags=None):
        if not os.path.exists(path):
            return None
        m = Image.open(path)
        return np.asarray(m) if m.mode.startswith("I;16") else np.asarray(m.convert("L"))

    sys.modules["torchvision.transforms"].ToTensor = ToTensor
    cv2 = sys.modules["cv2"]
    cv2.IMREAD_ANYDEPTH, cv2.INTER_NEAREST, cv2.imread = 2, 0, imread
    cv2.resize = lambda m, wh, interpolation=None: _resize_nearest(m, wh)
    pkg = types.ModuleType("ref_datasets")
    pkg.__path__ = [os.path.join(R.REF_ROOT, "datasets")]
    sys.modules["ref_datasets"] = pkg
    return importlib.import_module("ref_datasets.real_arkit").RealDatasetARKit


def hparams(root):
    return SimpleNamespace(root_dir=root, near=SC.NEAR, far=SC.FAR, scale_factor=SC.SCALE_FACTOR, val_idx=SC.VAL_IDX,
                           train_skip_step=1, train_geometry_stage=False)


def path_split(cls, root, split, frames=(0, 5)):
    ds = cls(root, split, SC.IMG_WH, hparams(root))
    poses = np.stack([np.asarray(f["transform_matrix"], np.float64) for f in ds.meta["frames"]])
    out = {"poses": poses, "focal": np.float64(ds.focal), "near": np.float64(ds.near), "far": np.float64(ds.far)}
    for i in frames:
        out[f"rays_{i}"] = ds[i]["rays"].numpy()
    return out, len(ds)


def main():
    G = geo_utils()
    rng = np.random.RandomState(23)
    poses = SC.seeded_poses(9, 1)[:, :3, :4]
    centred, avg = G.center_poses(poses)
    one = SC.seeded_poses(1, 2)[0]
    radii, focus = rng.uniform(0.1, 0.5, 3), 3.5
    save("g23_poses", dict(radius=-1.3, n_spheric=7, focus_depth=focus, n_spiral=9, progress=0.3),
         {"poses": poses, "pose": one, "radii": radii},
         {"average_poses": G.average_poses(poses), "center_poses": centred, "pose_avg": avg,
          "center_pose_from_avg": G.center_pose_from_avg(avg, one),
          "create_spheric_poses": G.create_spheric_poses(-1.3, 7), "create_spiral_poses": G.create_spiral_poses(radii, focus, 9),
          "move_camera_pose_slightly": G.move_camera_pose_slightly(one, 0.3)})

    cls = arkit_class()
    scene_poses = SC.seeded_poses(SC.N_FRAMES, 3)
    key_poses = SC.seeded_poses(8, 4)[::2]
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "lounge")
        SC.write_scene(root, scene_poses, key_poses)
        outs, n_frames = {}, {}
        for split in ("test_rotate", "test_interpolation"):
            o, n_frames[split] = path_split(cls, root, split)
            outs.update({f"{split}__{k}": v for k, v in o.items()})
        # the centred key frames, by the reference's helper: what interpolate_poses is given
        pose_avg = G.center_poses(scene_poses[:, :3, :4])[1]
        keys = []
        for p in key_poses:
            c = G.center_pose_from_avg(pose_avg, p)
            c[..., 3] /= SC.SCALE_FACTOR
            keys.append(c[:3, :4])
        outs["centred_keys"] = np.stack(keys)
        save("g24_arkit_paths", dict(n_frames=n_frames, rays_of=[0, 5], img_wh=list(SC.IMG_WH)),
             {"poses": scene_poses, "key_poses": key_poses}, outs)

        market = os.path.join(tmp, "market_small")
        many = SC.seeded_poses(80, 5)
        SC.write_scene(market, many, key_poses, images=False)
        o, n = path_split(cls, market, "test_rotate", frames=(3,))
        save("g24_arkit_market", dict(n_frames=n, rays_of=[3], img_wh=list(SC.IMG_WH)), {"poses": many, "key_poses": key_poses},
             {f"test_rotate__{k}": v for k, v in o.items()})

        ds = cls(root, "train", SC.IMG_WH, hparams(root))
        hw = SC.IMG_WH[0] * SC.IMG_WH[1]
        masks = ds.all_mirror_masks.numpy().reshape(-1, hw)
        wmask = [f for f in range(len(masks)) if not (masks[f] < 0).any()]
        rays = ds.all_rays.numpy().reshape(-1, hw, 8)
        assert np.array_equal(ds.rays_wmask.numpy(), rays[wmask].reshape(-1, 8))          # the list is the *_wmask buffers'
        tt = cls(root, "test_train", SC.IMG_WH, hparams(root))
        sample = tt[SC.RGBA_FRAME]
        assert np.array_equal(sample["rgbs"].numpy(), ds.all_rgbs.numpy().reshape(-1, hw, 3)[SC.RGBA_FRAME])
        out = {"rays": ds.all_rays.numpy(), "rgbs": ds.all_rgbs.numpy(), "mirror_mask": ds.all_mirror_masks.numpy().astype(np.float32),
               "poses": np.asarray(ds.poses, np.float64), "pose_avg": ds.pose_avg, "frames_with_mask": np.array(wmask),
               "valid_mask_rgba_frame": sample["valid_mask"].numpy()}
        for split in ("train", "val", "test"):
            d = ds if split == "train" else cls(root, split, SC.IMG_WH, hparams(root))
            out[f"{split}__focal_near_far"] = np.array([d.focal, d.near, d.far], np.float64)
        save("g25_arkit_train", dict(img_wh=list(SC.IMG_WH), rgba_frame=SC.RGBA_FRAME), {"poses": scene_poses, "key_poses": key_poses}, out)


if __name__ == "__main__":
    main()
