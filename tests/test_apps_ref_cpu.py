"""Pins tests/apps_ref.py, the restatement that tests/test_hip_apps_kernels.py holds mnrf_place_mirror and mnrf_transform_rays to
bit for bit, without a GPU: hand-made rays through every branch with the expected values worked out here, and the float32 run
against the float64 run on the seeded rays the GPU test uses."""
import numpy as np
import pytest

from tests import apps_ref as AR

NEAR = 0.05
U24 = 2.0 ** -24          # half a float32 ulp of 1: the relative size of one rounding


def _state(n, depth):
    return dict(depth=np.asarray(depth, np.float32), mask=np.zeros(n, np.float32), normal=np.full((n, 3), 7.0, np.float32),
                x_surface=np.full((n, 3), 9.0, np.float32))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_place_mirror_by_hand_plane_x(dtype):
    """Plane x = 1, rectangle y in [-1, 1], z in [-0.5, 0.5], near 0.05.  All values below are exact in binary."""
    rays = np.array([
        [0, 0, 0, 1, 0, 0, 0, 0],                 # 0 straight at the plane: t = 1, (u, w) = (0, 0), |o - x| = 1, s = 1: a hit
        [0, 0, 0.25, 0.5, 0.25, -0.125, 0, 0],    # 1 oblique: t = 2, u = 0.5, w = 2 * -0.125 + 0.25 = 0; e = (-1, -0.5, 0.25),
                                                  #   |e|^2 = 1.3125; s = 1 * 0.5 + 0.5 * 0.25 + 0.25 * 0.125 = 0.65625: a hit
        [-1, 0.25, 0, 0.5, 0.5, 0, 0, 0],         # 2 t = 4, u = 2.25 > 1: outside
        [2, 0, 0, 1, 0, 0, 0, 0],                 # 3 t = -1: inside, s = -1: behind the origin
        [0, 0, 0, 1, 0, 0, 0, 0],                 # 4 depth 0.5: 1 > 0.5 and 0.5 > near: blocked
        [0, 0, 0, 1, 0, 0, 0, 0],                 # 5 depth 0.01 <= near: the foreground does not count, a hit
        [0, 3, 0, 1, 0, 0, 0, 0],                 # 6 u = 3: outside, but masked already
        [1, 0, 0, 0, 1, 0, 0, 0],                 # 7 in the plane and parallel to it: t = 0 / 0
        [0, 0, -0.75, 1, 0, 0, 0, 0],             # 8 w = -0.75 < -0.5: outside
    ], np.float32)
    st = _state(9, [5, 9, 5, 5, 0.5, 0.01, 5, 5, 5])
    st["mask"][6] = 1
    r = AR.place_mirror(rays, axis=AR.PLANE_X, position=1.0, plane_normal=(1, 0, 0), rect=(-1, 1, -0.5, 0.5), near=NEAR, dtype=dtype, **st)
    assert r["depth"].dtype == dtype
    assert r["in_rect"].tolist() == [True, True, False, True, True, True, False, True, False]
    assert r["hit"].tolist() == [True, True, False, False, False, True, False, False, False]
    assert r["blocked"].tolist() == [False, False, False, False, True, False, False, False, False]
    assert r["mask"].tolist() == [1, 1, 0, 0, 0, 1, 1, 0, 0] and r["mask_bool"].tolist() == [1, 1, 0, 0, 0, 1, 1, 0, 0]
    assert r["mask_bool"].dtype == np.uint8 and r["any"] == 1
    assert np.isnan(r["u"][7]) and np.isnan(r["s"][7])
    assert r["u"][:4].tolist() == [0, 0.5, 2.25, 0] and r["w"][:4].tolist() == [0, 0, 0, 0] and r["s"][:4].tolist() == [1, 0.65625, 2, -1]
    want_n = np.where(r["in_rect"][:, None], np.array([1, 0, 0]), 7.0)          # the normal of every ray inside, hit or not
    assert np.array_equal(r["normal"], want_n)
    want_x = np.full((9, 3), 9.0)
    want_x[0], want_x[1], want_x[5] = (1, 0, 0), (1, 0.5, 0), (1, 0, 0)
    assert np.array_equal(r["x_surface"], want_x)
    assert np.array_equal(r["depth"], np.array([1, np.sqrt(dtype(1.3125)), 5, 5, 0.5, 1, 5, 5, 5], dtype))
    assert st["depth"].tolist() == [5, 9, 5, 5, 0.5, np.float32(0.01), 5, 5, 5] and (st["x_surface"] == 9).all()      # the caller's arrays stay


def test_place_mirror_by_hand_plane_y():
    """Plane y = 1.5: the rectangle bounds (x, z) = [0, 2] x [-1, 1]."""
    rays = np.array([
        [1, 0, 0, 0, 1, 0, 0, 0],                 # t = 1.5, (u, w) = (1, 0): a hit at (1, 1.5, 0), 1.5 away
        [-0.5, 0, 0, 0, 1, 0, 0, 0],              # u = -0.5 < 0: outside (inside if the bounds were applied to (z, x))
        [1, 3, 0.5, 0, -0.5, 0, 0, 0],            # from the other side: t = 3, a hit at (1, 1.5, 0.5)
        [1, 0, 0, 1, 0, 0, 0, 0],                 # parallel, off the plane: t = inf, u = inf: outside
    ], np.float32)
    st = _state(4, [5, 5, 5, 5])
    r = AR.place_mirror(rays, axis=AR.PLANE_Y, position=1.5, plane_normal=(0, -1, 0), rect=(0, 2, -1, 1), near=NEAR, **st)
    assert r["hit"].tolist() == [True, False, True, False] and r["in_rect"].tolist() == [True, False, True, False]
    assert r["x_surface"].tolist() == [[1, 1.5, 0], [9, 9, 9], [1, 1.5, 0.5], [9, 9, 9]]
    assert r["depth"].tolist() == [1.5, 5, 1.5, 5] and r["normal"][0].tolist() == [0, -1, 0] and r["normal"][1].tolist() == [7, 7, 7]
    assert np.isinf(r["u"][3])


def test_the_flag_is_or_ed():
    rays = np.array([[0, 3, 0, 1, 0, 0, 0, 0]], np.float32)                      # outside
    kw = dict(axis=AR.PLANE_X, position=1.0, plane_normal=(1, 0, 0), rect=(-1, 1, -0.5, 0.5), near=NEAR)
    assert AR.place_mirror(rays, **_state(1, [5]), **kw)["any"] == 0
    assert AR.place_mirror(rays, any_in=4, **_state(1, [5]), **kw)["any"] == 4
    st = _state(1, [5])
    st["mask"][0] = 0.25                                                          # the old mask alone; any non-zero value counts
    r = AR.place_mirror(rays, any_in=4, **st, **kw)
    assert r["any"] == 5 and r["mask"].tolist() == [1] and not r["hit"][0]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_transform_rays_by_hand(dtype):
    rays = np.array([[1, 2, 3, 0, 2, 0, 0.1, 7], [1, 2, 3, 0, 0, 0, 0.2, 8]], np.float32)
    market = [0, 1, 0, -1, 0, 0, 0, 0, 1]
    # R o = (2, -1, 3), R d = (2, 0, 0) -> (1, 0, 0); o * 2 + (0.5, 0, -1) = (4.5, -2, 5).  A zero direction stays zero: 0 / sqrt(eps)
    got = AR.transform_rays(rays, market, 2.0, (0.5, 0.0, -1.0), dtype)
    assert got.dtype == dtype
    assert got.tolist() == [[4.5, -2, 5, 1, 0, 0, np.float32(0.1), 7], [4.5, -2, 5, 0, 0, 0, np.float32(0.2), 8]]
    # without a rotation the directions are not touched, not even normalised
    got = AR.transform_rays(rays, None, 2.0, (0.5, 0.0, -1.0), dtype)
    assert got.tolist() == [[2.5, 4, 5, 0, 2, 0, np.float32(0.1), 7], [2.5, 4, 5, 0, 0, 0, np.float32(0.2), 8]]
    # below the clamp: |R d|^2 = 1e-10 < eps, so the length is sqrt(eps) and not 1e-5
    tiny = np.array([[0, 0, 0, 1e-5, 0, 0, 0, 0]], np.float32)
    got = AR.transform_rays(tiny, market, 1.0, (0, 0, 0), np.float64)
    assert got[0, 4] == -np.float64(np.float32(1e-5)) / np.sqrt(np.float64(AR.EPS32)) and abs(got[0, 4]) < 0.03
    # sums associate to the left: (R0 v0 + R1 v1) + R2 v2 with 2^24 + 1 - 2^24 = 0 in float32, 1 the other way round
    big = np.array([[2.0 ** 24, 1, -2.0 ** 24, 1, 0, 0, 0, 0]], np.float32)
    got = AR.transform_rays(big, [1, 1, 1, 0, 1, 0, 0, 0, 1], 1.0, (0, 0, 0), np.float32)
    assert got[0, 0] == 0.0
    assert rays.tolist()[0][:3] == [1, 2, 3]                                       # the input is not touched


CASES = [(name, n) for name in AR.PLANES for n in (257, 4099)]


@pytest.mark.parametrize("name,n", CASES)
def test_seeded_rays_fill_every_class(name, n):
    kw, c = AR.plane_case(name, n, NEAR)
    r = AR.place_mirror(**kw, **c)
    ahead = r["s"] > 0
    share = {"outside": np.mean(~r["in_rect"]), "behind": np.mean(r["in_rect"] & ~ahead), "blocked": np.mean(r["in_rect"] & ahead & r["blocked"]),
             "hit": np.mean(r["hit"]), "hit_below_near": np.mean(r["hit"] & (c["depth"] <= np.float32(NEAR))),
             "masked_miss": np.mean((c["mask"] != 0) & ~r["hit"])}
    print(f"apps classes {name} n={n}: " + ", ".join(f"{k} {v:.3f}" for k, v in share.items()))
    for k, v in share.items():
        assert v >= 0.05, (k, v)
    assert abs(sum(share[k] for k in ("outside", "behind", "blocked", "hit")) - 1.0) < 1e-12      # the four are a partition


@pytest.mark.parametrize("name,n", CASES)
def test_float32_run_against_float64(name, n):
    """Decisions agree wherever no comparison is within 1e-5 (relative to max(1, |value|)) of equality in float64, and such rays
    are at most 1 % of all.  On the hits, x and the distance are a few roundings off.  x = t * d + o with t = (p - o_a) / d_a is a
    subtraction, a division, a product and a sum: the first three each move the product by 2^-24 of itself, the sum by 2^-24 of
    x, so |error| <= 4 * 2^-24 * M with M = max(|t d|, |x|) to first order.  e = o - x adds 2^-24 |e| to that per component;
    squares, two sums and the root move the length by another 2.5 * 2^-24 of itself: |error| <= 2^-24 * (4 sqrt(2) M + 3.5 dist)
    (two components of x carry an error)."""
    kw, c = AR.plane_case(name, n, NEAR)
    axis, pos, rect = kw["axis"], kw["position"], kw["rect"]
    r32, r64 = AR.place_mirror(dtype=np.float32, **kw, **c), AR.place_mirror(dtype=np.float64, **kw, **c)
    rel = lambda v, edge: np.abs(v - edge) <= 1e-5 * max(1.0, abs(edge))  # noqa: E731
    f = [float(np.float32(v)) for v in rect]
    band = rel(r64["u"], f[0]) | rel(r64["u"], f[1]) | rel(r64["w"], f[2]) | rel(r64["w"], f[3]) | (np.abs(r64["s"]) <= 1e-5)
    depth = c["depth"].astype(np.float64)                                        # the depth of before the call decides
    band |= np.abs(r64["dist"] - depth) <= 1e-5 * np.maximum(1.0, np.abs(depth))
    flips = sum(int((r32[k] != r64[k]).sum()) for k in ("in_rect", "blocked", "hit"))
    print(f"apps f32/f64 {name} n={n}: band share {band.mean():.4f}, decisions that differ {flips}")
    assert band.mean() <= 0.01
    for k in ("in_rect", "blocked", "hit", "mask_bool"):
        assert np.array_equal(r32[k][~band], r64[k][~band]), k
    assert np.array_equal((r32["s"] > 0)[~band], (r64["s"] > 0)[~band])
    h = r32["hit"] & r64["hit"]
    a = 1 if axis == AR.PLANE_Y else 0
    o, d = c["rays"][:, 0:3].astype(np.float64), c["rays"][:, 3:6].astype(np.float64)
    t = (float(np.float32(pos)) - o[:, a]) / d[:, a]
    M = np.maximum(np.abs(t[:, None] * d).max(1), np.abs(r64["x_surface"]).max(1))
    ex = np.abs(r32["x_surface"].astype(np.float64) - r64["x_surface"]).max(1)[h] / (U24 * M[h])
    ed = np.abs(r32["depth"].astype(np.float64) - r64["depth"])[h] / (U24 * (4 * np.sqrt(2) * M[h] + 3.5 * r64["depth"][h]))
    print(f"apps f32/f64 {name} n={n}: x off by {ex.max():.2f} x 2^-24 M (bar 4), dist by {ed.max():.3f} of its bar, on {h.sum()} hits")
    assert h.sum() >= 0.15 * n and ex.max() <= 4.0 and ed.max() <= 1.0
    # the transform: R v is two products and two sums, the length three more and a root, then a division; o * scale + t
    rs = np.random.RandomState(n)
    R = rs.normal(size=9).astype(np.float32)
    t32, t64 = (AR.transform_rays(c["rays"], R, 1.25, (0.5, -1.0, 2.0), dt) for dt in (np.float32, np.float64))
    scale = np.maximum(1.0, np.abs(t64).max(1))
    # |R_k0 v0| + |R_k1 v1| + |R_k2 v2| <= |R|_1 |v|_inf bounds every partial sum: 3 roundings of at most that size each
    amp = np.abs(R.astype(np.float64)).reshape(3, 3).sum(1).max() * np.abs(c["rays"][:, :3]).max(1)
    eo = (np.abs(t32[:, :3].astype(np.float64) - t64[:, :3]).max(1) / (U24 * (1.25 * 3 * amp + 2 * scale))).max()
    print(f"apps f32/f64 transform n={n}: origins at {eo:.3f} of their bar")
    assert eo <= 1.0 and np.array_equal(t32[:, 6:], c["rays"][:, 6:])
