"""Camera poses on the host, numpy float64: the pose centring and the camera paths of datasets/geo_utils.py, and the
interpolated fly-through of datasets/real_arkit.py:170-200 without scipy.

A pose is a camera-to-world (3, 4) or (4, 4) matrix, [x y z | centre] in its columns (OpenGL convention: the camera looks
along -z).  Everything here is a closed form in float64; tests/test_poses_cpu.py holds each function against the reference's
own output to 1e-10."""
import numpy as np


def _normalize(v):
    return v / np.linalg.norm(v)


def _homo(pose34):
    h = np.eye(4)
    h[:3] = pose34
    return h


def average_poses(poses):
    """The average pose (3, 4) of poses (N, 3, 4) (geo_utils.py:9-45): the mean centre, z = the normalised mean z axis,
    x = normalise(mean y axis x z), y = z x x."""
    poses = np.asarray(poses, dtype=np.float64)
    center = poses[..., 3].mean(0)
    z = _normalize(poses[..., 2].mean(0))
    y_ = poses[..., 1].mean(0)
    x = _normalize(np.cross(y_, z))
    y = np.cross(z, x)
    return np.stack([x, y, z, center], 1)


def center_poses(poses):
    """(centred (N, 3, 4), pose_avg (3, 4)): every pose of (N, 3, 4) left-multiplied by the inverse of the average pose
    (geo_utils.py:48-75)."""
    poses = np.asarray(poses, dtype=np.float64)
    pose_avg = average_poses(poses)
    last_row = np.tile(np.array([0, 0, 0, 1]), (len(poses), 1, 1))
    poses_homo = np.concatenate([poses, last_row], 1)
    centred = np.linalg.inv(_homo(pose_avg)) @ poses_homo
    return centred[:, :3], pose_avg


def center_pose_from_avg(pose_avg, pose):
    """One pose ((3, 4) or (4, 4)) centred with a given average pose: (4, 4) (geo_utils.py:78-87)."""
    pose = np.asarray(pose, dtype=np.float64)
    return np.linalg.inv(_homo(pose_avg)) @ _homo(pose[:3])


def create_spiral_poses(radii, focus_depth, n_poses=120):
    """(n_poses, 3, 4) along a spiral of two rounds that looks at the plane z = -focus_depth (geo_utils.py:107-139)."""
    out = []
    for t in np.linspace(0, 4 * np.pi, n_poses + 1)[:-1]:
        center = np.array([np.cos(t), -np.sin(t), -np.sin(0.5 * t)]) * radii
        z = _normalize(center - np.array([0, 0, -focus_depth]))
        x = _normalize(np.cross(np.array([0, 1, 0]), z))
        y = np.cross(z, x)
        out.append(np.stack([x, y, z, center], 1))
    return np.stack(out, 0)


def create_spheric_poses(radius, n_poses=120):
    """(n_poses, 3, 4) on a circle around the z axis, looking 36 degrees downwards (geo_utils.py:142-189)."""
    def spheric_pose(theta, phi, t):
        trans_t = np.array([[1, 0, 0, 0], [0, 1, 0, -0.9 * t], [0, 0, 1, t], [0, 0, 0, 1]])
        rot_phi = np.array([[1, 0, 0, 0], [0, np.cos(phi), -np.sin(phi), 0], [0, np.sin(phi), np.cos(phi), 0], [0, 0, 0, 1]])
        rot_theta = np.array([[np.cos(theta), 0, -np.sin(theta), 0], [0, 1, 0, 0], [np.sin(theta), 0, np.cos(theta), 0],
                              [0, 0, 0, 1]])
        c2w = rot_theta @ rot_phi @ trans_t
        c2w = np.array([[-1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]]) @ c2w
        return c2w[:3]

    return np.stack([spheric_pose(th, -np.pi / 5, radius) for th in np.linspace(0, 2 * np.pi, n_poses + 1)[:-1]], 0)


def move_camera_pose_slightly(pose, progress):
    """The pose moved along a small spiral (radius 0.1, two rounds over progress 0..1) in its own frame (geo_utils.py:192-199)."""
    t = progress * np.pi * 4
    center = np.array([np.cos(t), -np.sin(t), -np.sin(0.5 * t)]) * 0.1
    pose_ = np.array(pose, dtype=np.float64)
    pose_[:3, 3] += pose_[:3, :3] @ center
    return pose_


# ----------------------------------------------------------------------------- the interpolated path
def _quat_from_matrix(m):
    """Unit quaternion (w, x, y, z) of a rotation matrix: the branch with the largest pivot, so nothing small is divided by."""
    t = np.trace(m)
    c = [t, m[0, 0], m[1, 1], m[2, 2]]
    k = int(np.argmax(c))
    if k == 0:
        q = np.array([1.0 + t, m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1]])
    elif k == 1:
        q = np.array([m[2, 1] - m[1, 2], 1.0 + 2.0 * m[0, 0] - t, m[0, 1] + m[1, 0], m[0, 2] + m[2, 0]])
    elif k == 2:
        q = np.array([m[0, 2] - m[2, 0], m[0, 1] + m[1, 0], 1.0 + 2.0 * m[1, 1] - t, m[1, 2] + m[2, 1]])
    else:
        q = np.array([m[1, 0] - m[0, 1], m[0, 2] + m[2, 0], m[1, 2] + m[2, 1], 1.0 + 2.0 * m[2, 2] - t])
    return q / np.linalg.norm(q)


def _matrix_from_quat(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def _rotvec_from_quat(q):
    """The log map: axis * angle with the angle in [0, pi] (the shorter way round)."""
    if q[0] < 0:
        q = -q
    s = np.linalg.norm(q[1:])
    if s < 1e-12:
        return 2.0 * q[1:]
    return q[1:] * (2.0 * np.arctan2(s, q[0]) / s)


def _quat_from_rotvec(v):
    a = np.linalg.norm(v)
    if a < 1e-12:
        q = np.array([1.0, 0.5 * v[0], 0.5 * v[1], 0.5 * v[2]])
        return q / np.linalg.norm(q)
    return np.concatenate([[np.cos(0.5 * a)], v * (np.sin(0.5 * a) / a)])


def interpolate_poses(c2ws, n=64):
    """(n, 4, 4) poses through the K key poses c2ws (K, 3 or 4, 4), the path of real_arkit.py:170-200: frame i sits at time
    i / n * (K - 1), key k at time k; the rotation is the spherical interpolation between the two neighbouring key rotations
    (R_k exp(a log(R_k^T R_{k+1})), the shorter way round), the position the linear one.  The last key is approached and not
    reached, as in the reference.  Key rotations half a turn apart have no unique path; up to there the log map used here
    (through unit quaternions) is well conditioned."""
    c2ws = np.asarray(c2ws, dtype=np.float64)
    K = len(c2ws)
    if K < 2:
        raise ValueError("interpolate_poses: at least two key poses are needed")
    quats = [_quat_from_matrix(c[:3, :3]) for c in c2ws]
    out = []
    for i in range(n):
        time = float(i) / n * (K - 1)
        k = min(int(np.floor(time)), K - 2)
        a = time - k
        rel = _quat_mul(quats[k] * np.array([1.0, -1.0, -1.0, -1.0]), quats[k + 1])
        q = _quat_mul(quats[k], _quat_from_rotvec(a * _rotvec_from_quat(rel)))
        c2w = np.eye(4)
        c2w[:3, :3] = _matrix_from_quat(q / np.linalg.norm(q))
        # scipy's interp1d: slope * (t - t_k) + y_k
        c2w[:3, 3] = (c2ws[k + 1, :3, 3] - c2ws[k, :3, 3]) * a + c2ws[k, :3, 3]
        out.append(c2w)
    return np.stack(out, 0)
