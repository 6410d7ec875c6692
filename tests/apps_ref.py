"""A numpy restatement of the two scene-editing entry points of csrc/mnrf_apps.hip, mnrf_place_mirror and mnrf_transform_rays,
written from their contract in include/mnrf.h, evaluated in the `dtype` asked for.  In float32 every step below is one IEEE
operation in the kernel's documented order (the kernels are compiled without contraction, with correctly rounded division and
square root), so the float32 run is what the kernels must return bit for bit (tests/test_hip_apps_kernels.py); the float64 run is
what the float32 run is judged by (tests/test_apps_ref_cpu.py).  The scalars (position, rectangle, near, rotation, scale,
translation) are the C floats the entry points receive: they are rounded to float32 first in either run.

`seeded_case` makes the rays both test files use."""
import numpy as np

PLANE_X, PLANE_Y = 0, 1                       # MNRF_PLANE_X / MNRF_PLANE_Y
EPS32 = np.float32(1.1920928955078125e-07)    # torch.finfo(float32).eps

# (axis, position, normal, rect): the two presets the issue names and one plane that is no preset
PLANES = {
    "x_default": (PLANE_X, -1.0, (1.0, 0.0, 0.0), (-1.0, 1.0, -0.5, 0.5)),
    "y_livingroom": (PLANE_Y, 1.65, (0.0, -1.0, 0.0), (-0.3, 1.5, -0.5, 1.0)),
    "y_free": (PLANE_Y, -0.37, (0.6, 0.0, -0.8), (-2.25, -0.4, 0.3, 0.9)),
}


def _c(v, dtype):
    """A C float argument in the run's dtype."""
    return dtype(np.float32(v))


def place_mirror(rays, depth, mask, normal, x_surface, axis, position, plane_normal, rect, near, any_in=0, dtype=np.float32):
    """-> dict: the edited copies `depth`, `mask`, `normal`, `x_surface`, the byte mask `mask_bool`, the flag `any`
    (any_in OR-ed with "some ray is in the merged mask"), and what decided: `u`, `w`, `dist`, `s`, `in_rect`, `blocked`, `hit`."""
    assert axis in (PLANE_X, PLANE_Y)
    rays = np.asarray(rays).astype(dtype)
    depth, mask = np.asarray(depth).astype(dtype), np.asarray(mask).astype(dtype)
    normal, x_surface = np.asarray(normal).astype(dtype), np.asarray(x_surface).astype(dtype)
    o, d = rays[:, 0:3], rays[:, 3:6]
    a = 1 if axis == PLANE_Y else 0
    b = 1 - a
    pos, near = _c(position, dtype), _c(near, dtype)
    r0, r1, r2, r3 = (_c(v, dtype) for v in rect)
    with np.errstate(all="ignore"):
        t = (pos - o[:, a]) / d[:, a]
        u = t * d[:, b] + o[:, b]
        w = t * d[:, 2] + o[:, 2]
        x = np.empty_like(o)
        x[:, a], x[:, b], x[:, 2] = pos, u, w
        in_rect = ~((u < r0) | (w < r2) | (u > r1) | (w > r3))      # every comparison with a NaN is false: NaN counts as inside
        normal[in_rect] = np.array([_c(v, dtype) for v in plane_normal], dtype)          # before the two filters
        e = o - x
        dist = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2])
        f = x - o
        s = (f[:, 0] * d[:, 0] + f[:, 1] * d[:, 1]) + f[:, 2] * d[:, 2]
        blocked = (dist > depth) & (depth > near)                    # the depth of before this call
        hit = in_rect & (s > 0) & ~blocked
    merged = (mask != 0) | hit
    x_surface[hit] = x[hit]
    depth[hit] = dist[hit]
    return dict(depth=depth, mask=merged.astype(dtype), normal=normal, x_surface=x_surface, mask_bool=merged.astype(np.uint8),
                any=int(any_in) | int(merged.any()), u=u, w=w, dist=dist, s=s, in_rect=in_rect, blocked=blocked, hit=hit)


def transform_rays(rays, rotation, scale, translation, dtype=np.float32):
    """-> the transformed copy of rays (n,8).  rotation: 9 floats row-major or None."""
    out = np.asarray(rays).astype(dtype)
    o = [out[:, k].copy() for k in range(3)]
    with np.errstate(all="ignore"):
        if rotation is not None:
            R = [_c(v, dtype) for v in np.asarray(rotation, np.float32).reshape(9)]
            v = [out[:, 3 + k].copy() for k in range(3)]
            ro = [(R[3 * k] * o[0] + R[3 * k + 1] * o[1]) + R[3 * k + 2] * o[2] for k in range(3)]
            rd = [(R[3 * k] * v[0] + R[3 * k + 1] * v[1]) + R[3 * k + 2] * v[2] for k in range(3)]
            # fmaxf: a NaN sum gives the clamp
            length = np.sqrt(np.fmax((rd[0] * rd[0] + rd[1] * rd[1]) + rd[2] * rd[2], dtype(EPS32)))
            for k in range(3):
                out[:, 3 + k] = rd[k] / length
            o = ro
        for k in range(3):
            out[:, k] = o[k] * _c(scale, dtype) + _c(translation[k], dtype)
    return out


def seeded_case(n, seed, axis, position, rect, near):
    """n rays aimed at the plane's rectangle, as float32 arrays: dict(rays (n,8), depth, mask, normal, x_surface).  Targets are
    uniform over the rectangle enlarged 1.5 x about its centre, origins the target plus N(0, 1.5^2), directions unit vectors
    towards the target with 30 % of the rays flipped, depth the distance x U(0.5, 1.5) with 30 % of the rays at near / 2, 20 % of
    the rays masked already.  Expected shares: 0.56 outside (1 - 1 / 1.5^2), 0.13 behind (0.44 x 0.3), 0.11 blocked
    (0.44 x 0.7 x 0.7 x 0.5), 0.20 hit, of which 0.09 with depth <= near (0.44 x 0.7 x 0.3): far enough above 5 % for 257 rays."""
    rs = np.random.RandomState(seed)
    a = 1 if axis == PLANE_Y else 0
    b = 1 - a
    cu, cw = 0.5 * (rect[0] + rect[1]), 0.5 * (rect[2] + rect[3])
    hu, hw = 0.75 * (rect[1] - rect[0]), 0.75 * (rect[3] - rect[2])
    target = np.empty((n, 3))
    target[:, a] = position
    target[:, b] = cu + hu * rs.uniform(-1.0, 1.0, n)
    target[:, 2] = cw + hw * rs.uniform(-1.0, 1.0, n)
    origin = target + rs.normal(0.0, 1.5, (n, 3))
    to = target - origin
    length = np.linalg.norm(to, axis=1)
    direction = to / length[:, None] * np.where(rs.uniform(size=n) < 0.3, -1.0, 1.0)[:, None]
    depth = length * rs.uniform(0.5, 1.5, n)
    depth[rs.uniform(size=n) < 0.3] = 0.5 * near
    rays = np.zeros((n, 8), np.float32)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = origin, direction, 0.05, rs.uniform(4.0, 9.0, n)
    return dict(rays=rays, depth=depth.astype(np.float32), mask=(rs.uniform(size=n) < 0.2).astype(np.float32),
                normal=rs.normal(size=(n, 3)).astype(np.float32), x_surface=rs.normal(size=(n, 3)).astype(np.float32))


def plane_case(name, n, near):
    """-> (the plane's keyword arguments for place_mirror, the seeded arrays) of PLANES[name] at n rays."""
    axis, pos, normal, rect = PLANES[name]
    seed = 1000 + n + 100000 * sorted(PLANES).index(name)
    return dict(axis=axis, position=pos, plane_normal=normal, rect=rect, near=near), seeded_case(n, seed, axis, pos, rect, near)
