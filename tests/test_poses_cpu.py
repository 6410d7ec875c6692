"""mirror_nerf_amd/poses.py against the reference's datasets/geo_utils.py and the interpolated path of its real-capture class
(fixtures G23, G24: tests/golden/make_golden_poses.py).

The bound is 1e-10 absolute: the entries are O(1) to O(10) and both sides are float64 closed forms, so what separates them is
rounding of order 1e-15 to 1e-13 (the interpolated path goes through a quaternion here and through scipy's there)."""
import numpy as np
import pytest

from mirror_nerf_amd import poses as P
from tests.golden.fixtures import Fixture

TOL = 1e-10


@pytest.fixture(scope="module")
def g23():
    return Fixture("g23_poses")


def _close(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.float64, (what, got.shape, want.shape, got.dtype)
    err = float(np.abs(got - want).max())
    print(f"{what}: max abs difference {err:.3e}")
    assert err <= TOL, (what, err)


def test_geo_utils_functions(g23):
    """Largest difference seen: 0 for every function."""
    i, o, m = g23.inputs, g23.outputs, g23.meta
    _close(P.average_poses(i["poses"]), o["average_poses"], "average_poses")
    centred, avg = P.center_poses(i["poses"])
    _close(centred, o["center_poses"], "center_poses")
    _close(avg, o["pose_avg"], "pose_avg")
    _close(P.center_pose_from_avg(o["pose_avg"], i["pose"]), o["center_pose_from_avg"], "center_pose_from_avg")
    _close(P.center_pose_from_avg(o["pose_avg"], i["pose"][:3]), o["center_pose_from_avg"], "center_pose_from_avg (3, 4)")
    _close(P.create_spheric_poses(m["radius"], m["n_spheric"]), o["create_spheric_poses"], "create_spheric_poses")
    _close(P.create_spiral_poses(i["radii"], m["focus_depth"], m["n_spiral"]), o["create_spiral_poses"], "create_spiral_poses")
    _close(P.move_camera_pose_slightly(i["pose"], m["progress"]), o["move_camera_pose_slightly"], "move_camera_pose_slightly")
    before = i["pose"].copy()
    P.move_camera_pose_slightly(i["pose"], 0.7)
    assert np.array_equal(i["pose"], before)            # the argument is left alone


def test_interpolated_path():
    """The 64 poses of real_arkit.py:170-200 (scipy's Slerp and interp1d) from the centred key frames.  Largest difference
    seen: 4.4e-16."""
    fx = Fixture("g24_arkit_paths")
    got = P.interpolate_poses(fx.outputs["centred_keys"], 64)
    _close(got, fx.outputs["test_interpolation__poses"], "interpolate_poses")
    assert np.array_equal(got[0, :3, :4], fx.outputs["centred_keys"][0]) or np.abs(got[0, :3, :4] - fx.outputs["centred_keys"][0]).max() < 1e-15
    assert np.array_equal(got[:, 3], np.tile([0.0, 0.0, 0.0, 1.0], (64, 1)))
    with pytest.raises(ValueError):
        P.interpolate_poses(fx.outputs["centred_keys"][:1])


def test_interpolation_is_a_rotation_and_handles_equal_keys():
    """Properties no fixture covers: every frame is a rotation; two equal keys give a constant segment; a key is hit exactly at
    its own time; a turn of 170 degrees between two keys is followed the shorter way round at a constant rate."""
    a = np.deg2rad(170.0)
    rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    keys = np.zeros((3, 3, 4))
    keys[0, :, :3], keys[1, :, :3], keys[2, :, :3] = np.eye(3), np.eye(3), rz
    keys[:, :, 3] = [[0, 0, 0], [1, 2, 3], [1, 2, 3]]
    got = P.interpolate_poses(keys, 8)          # times 0, .25, ... 1.75
    for c in got:
        assert np.abs(c[:3, :3] @ c[:3, :3].T - np.eye(3)).max() < 1e-14 and abs(np.linalg.det(c[:3, :3]) - 1) < 1e-14
    assert all(np.abs(c[:3, :3] - np.eye(3)).max() < 1e-15 for c in got[:5])
    assert np.abs(got[2, :3, 3] - [0.5, 1.0, 1.5]).max() < 1e-15 and np.array_equal(got[4, :3, 3], [1.0, 2.0, 3.0])
    for k in (5, 6, 7):
        b = a * (k - 4) / 4
        want = np.array([[np.cos(b), -np.sin(b), 0], [np.sin(b), np.cos(b), 0], [0, 0, 1.0]])
        assert np.abs(got[k, :3, :3] - want).max() < 1e-14
