"""The small real-capture scene of fixtures G24 / G25 (tests/golden/make_golden_poses.py), written as the directory
datasets/real_arkit.py reads: transforms*.json, lossless PNGs and masks/.  The generator and the tests both write it with
`write_scene` from the poses the fixture stores; the pixels are the integer hash of tests/resample_ref.py.

Six frames at 20x15, trained at 8x6 (a ratio of 2.5: the resize is not a plain decimation).  Frame 1 is RGBA, frame 2 has no
mask file, frame 3 has a 16-bit mask; the others are RGB with an 8-bit mask.  The focal length comes from `camera_angle_x` in
transforms.json, transforms_train.json, transforms_test_train.json and the two path splits, from a top-level fx / cx in
transforms_val.json and from frame 0's `intrinsics` in transforms_test.json."""
import json
import os

import numpy as np

from tests import resample_ref as RR

NATIVE_HW = (15, 20)
IMG_WH = (8, 6)
N_FRAMES = 6
CAMERA_ANGLE_X = 0.9
FX, CX = 1450.5, 957.25
NEAR, FAR, SCALE_FACTOR, VAL_IDX = 0.05, 8.0, 2.0, 2
RGBA_FRAME, NO_MASK_FRAME, MASK16_FRAME = 1, 2, 3


def frame_name(k):
    return f"images/frame_{k:04d}.png"


def image_of(k):
    return RR.make_source(NATIVE_HW, 4 if k == RGBA_FRAME else 3, "noise" if k % 2 else "ramp", seed=300 + k)


def mask_of(k):
    """The native mask of frame k (uint8 or uint16), or None."""
    if k == NO_MASK_FRAME:
        return None
    h, w = NATIVE_HW
    m = RR.make_source(NATIVE_HW, 3, "noise", seed=400 + k)[..., 0]
    if k == MASK16_FRAME:
        m16 = m.astype(np.uint16) * 257
        m16[m < 100] = 0
        m16[0, :3] = (0, 1, 65535)
        return m16
    m[0, :4] = (0, 127, 128, 255)
    return m


def seeded_poses(n, seed):
    """n camera-to-world (4, 4) float64 poses on an arc, looking roughly at the origin, with a seeded wobble: consecutive
    rotations are about 25 degrees apart."""
    rng = np.random.RandomState(seed)
    out = []
    for k in range(n):
        a = 0.45 * k + 0.05 * rng.uniform(-1, 1)
        eye = np.array([3.0 * np.cos(a), 3.0 * np.sin(a), 1.0 + 0.3 * rng.uniform(-1, 1)]) + np.array([0.7, -0.4, 0.2])
        z = eye - np.array([0.7, -0.4, 0.2]) + 0.1 * rng.uniform(-1, 1, 3)
        z /= np.linalg.norm(z)
        x = np.cross(np.array([0.0, 0.0, 1.0]), z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        p = np.eye(4)
        p[:3, :4] = np.stack([x, y, z, eye], 1)
        out.append(p)
    return np.stack(out)


def write_scene(root, poses, key_poses, images=True):
    """The scene under `root`: poses (N, 4, 4) of transforms.json, key_poses (K, 4, 4) of transforms_test_interpolation.json.
    With images=False only the JSON files are written (the path splits read nothing else)."""
    from PIL import Image
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    os.makedirs(os.path.join(root, "masks"), exist_ok=True)
    frames = [{"file_path": frame_name(k), "transform_matrix": np.asarray(p).tolist()} for k, p in enumerate(poses)]
    by_angle = {"camera_angle_x": CAMERA_ANGLE_X, "frames": frames}
    intr = [[FX, 0.0, CX], [0.0, FX, 720.0], [0.0, 0.0, 1.0]]
    files = {"transforms.json": by_angle, "transforms_train.json": by_angle, "transforms_test_train.json": by_angle,
             "transforms_test_rotate.json": by_angle,
             "transforms_val.json": {"fx": FX, "cx": CX, "frames": frames},
             "transforms_test.json": {"frames": [dict(f, intrinsics=intr) for f in frames]},
             "transforms_test_interpolation.json": {"camera_angle_x": CAMERA_ANGLE_X, "frames": [
                 {"file_path": "", "transform_matrix": np.asarray(p).tolist()} for p in key_poses]}}
    for name, meta in files.items():
        with open(os.path.join(root, name), "w") as f:
            json.dump(meta, f)
    if not images:
        return
    for k in range(min(N_FRAMES, len(poses))):
        Image.fromarray(image_of(k)).save(os.path.join(root, frame_name(k)))
        m = mask_of(k)
        if m is not None:
            Image.fromarray(m).save(os.path.join(root, "masks", os.path.basename(frame_name(k))))
