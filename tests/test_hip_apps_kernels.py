"""mnrf_place_mirror and mnrf_transform_rays (csrc/mnrf_apps.hip) against the float32 run of their numpy restatement
(tests/apps_ref.py, pinned on the CPU by tests/test_apps_ref_cpu.py), bit for bit.

The tolerance is zero, and it is derived, not measured: the file is compiled with -ffp-contract=off, HIP's float division and
square root are correctly rounded, and every step of either kernel is one IEEE float32 operation that the restatement repeats in
the same order on the same float32 values.  Arrays are compared as bytes (so a NaN that came in must come out with its bits, and
-0 is not 0); a last-bit difference is a finding to explain, not a reason for a tolerance.

Sizes run from one thread to a second block with a partial tail wave (256 threads per block, 64 per wave); every array written in
place has sentinel rows behind row n, and the flag sits between two guard words."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import apps_ref as AR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEAR = 0.05
SIZES = [1, 63, 64, 65, 255, 256, 257, 4099]
PAD = 5                  # sentinel rows behind row n
SENT = -777.25
SENT_BYTE = 0xAB
GUARD_WORD = 0x5A5A5A5A
UINT = {1: np.uint8, 4: np.uint32}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.itemsize])


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, f"{what}: {len(bad)} entries differ, the first at {bad[0].tolist()}: got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}"


def _padded(a, fill=SENT):
    tail = np.full((PAD,) + a.shape[1:], fill, a.dtype)
    return np.concatenate([a, tail])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def hip_place(c, kw, with_bool=True, any_in=0):
    """One launch on copies of c's arrays with sentinel rows behind.  any_in None: a null flag.  -> every array as it came back,
    sentinel rows included; `any` as the three words [guard, flag, guard]."""
    from mirror_nerf_amd import _lib
    n = c["rays"].shape[0]
    rays = _dev(c["rays"])
    t = {k: _dev(_padded(c[k])) for k in ("depth", "mask", "normal", "x_surface")}
    mb = torch.full((n + PAD,), SENT_BYTE, dtype=torch.uint8, device=DEV)
    flag = torch.tensor([GUARD_WORD, 0 if any_in is None else any_in, GUARD_WORD], dtype=torch.int32, device=DEV)
    p = _lib.ptr
    u0, u1, w0, w1 = kw["rect"]
    nx, ny, nz = kw["plane_normal"]
    _lib.check(_lib.lib().mnrf_place_mirror(
        p(rays), n, kw["axis"], kw["position"], nx, ny, nz, u0, u1, w0, w1, kw["near"], p(t["depth"]), p(t["mask"]), p(t["normal"]),
        p(t["x_surface"]), ctypes.c_void_p(mb.data_ptr()) if with_bool else None,
        None if any_in is None else ctypes.c_void_p(flag.data_ptr() + 4), _lib.stream()), "mnrf_place_mirror")
    out = {k: v.cpu().numpy() for k, v in t.items()}
    out.update(rays=rays.cpu().numpy(), mask_bool=mb.cpu().numpy(), any=flag.cpu().numpy())
    return out


def check_place(c, kw, with_bool=True, any_in=0, tag=""):
    """Launch, compare every array with the float32 restatement as bytes; -> (the kernel's arrays, the restatement's)."""
    want = AR.place_mirror(any_in=any_in or 0, dtype=np.float32, **kw, **c)
    got = hip_place(c, kw, with_bool, any_in)
    _same(got["rays"], c["rays"], f"{tag} rays (an input)")
    for k in ("depth", "mask", "normal", "x_surface"):
        _same(got[k], _padded(want[k]), f"{tag} {k}")
    wb = _padded(want["mask_bool"], SENT_BYTE) if with_bool else np.full(len(c["rays"]) + PAD, SENT_BYTE, np.uint8)
    _same(got["mask_bool"], wb, f"{tag} mask_bool")
    flag = [GUARD_WORD, 0 if any_in is None else want["any"], GUARD_WORD]
    assert got["any"].tolist() == flag, f"{tag} any: {got['any'].tolist()} for {flag}"
    return got, want


# ------------------------------------------------------------------------------------------------------------ edge rows
EDGE_NAMES = ["u_on_r0", "u_on_r1", "w_on_r2", "w_on_r3", "origin_in_plane", "depth_is_dist", "depth_is_near", "depth_above_near",
              "parallel_in_plane", "parallel_off_plane", "parallel_off_plane_nan_u", "negative_depth", "nan_depth_hit", "nan_depth_outside",
              "masked_no_hit", "masked_fraction_behind"]
E = len(EDGE_NAMES)


def edge_rows(kw):
    """The E rays of EDGE_NAMES for the plane kw, as a case dict.  A `straight` ray runs along the plane's axis from one unit in
    front of it, so (u, w) are its own two other origin coordinates exactly: t * 0 + o = o."""
    a = 1 if kw["axis"] == AR.PLANE_Y else 0
    b = 1 - a
    f = np.float32
    pos, near = f(kw["position"]), f(kw["near"])
    r0, r1, r2, r3 = (f(v) for v in kw["rect"])
    mu, mw = f(0.5) * (r0 + r1), f(0.5) * (r2 + r3)
    front = pos - f(1.0)

    def ray(oa, ob, o2, da, db, d2):
        r = np.zeros(8, np.float32)
        r[a], r[b], r[2], r[3 + a], r[3 + b], r[5] = oa, ob, o2, da, db, d2
        r[6], r[7] = 0.05, 6.0
        return r
    straight = lambda ob, o2, oa=front: ray(oa, ob, o2, 1.0, 0.0, 0.0)  # noqa: E731
    ob_d = np.array([0.8, 0.1, -0.15]) / np.linalg.norm([0.8, 0.1, -0.15])
    oblique = ray(front, mu, mw, *ob_d)                 # ends 0.16 and 0.23 beside the centre: inside every rectangle of PLANES
    rows = {
        "u_on_r0": (straight(r0, mw), 10.0, 0.0), "u_on_r1": (straight(r1, mw), 10.0, 0.0),
        "w_on_r2": (straight(mu, r2), 10.0, 0.0), "w_on_r3": (straight(mu, r3), 10.0, 0.0),
        "origin_in_plane": (straight(mu, mw, oa=pos), 10.0, 0.0),
        "depth_is_dist": (oblique, None, 0.0),           # filled in below
        "depth_is_near": (oblique, near, 0.0),
        "depth_above_near": (oblique, np.nextafter(near, f(np.inf)), 0.0),
        "parallel_in_plane": (ray(pos, mu, mw, 0.0, 0.6, 0.8), 10.0, 0.0),
        "parallel_off_plane": (ray(front, mu, mw, 0.0, 0.6, 0.8), 10.0, 0.0),
        "parallel_off_plane_nan_u": (ray(front, mu, mw, 0.0, 0.0, 1.0), 10.0, 0.0),
        "negative_depth": (oblique, -1.0, 0.0),
        "nan_depth_hit": (oblique, np.nan, 0.0),
        "nan_depth_outside": (straight(r1 + f(1.0), mw), np.nan, 0.0),
        "masked_no_hit": (straight(r1 + f(1.0), mw), 10.0, 1.0),
        "masked_fraction_behind": (straight(mu, mw, oa=pos + f(1.0)), 10.0, 0.25),
    }
    assert list(rows) == EDGE_NAMES
    rs = np.random.RandomState(5)
    c = dict(rays=np.stack([rows[k][0] for k in EDGE_NAMES]), depth=np.array([rows[k][1] or 0.0 for k in EDGE_NAMES], np.float32),
             mask=np.array([rows[k][2] for k in EDGE_NAMES], np.float32), normal=rs.normal(size=(E, 3)).astype(np.float32),
             x_surface=rs.normal(size=(E, 3)).astype(np.float32))
    i = EDGE_NAMES.index("depth_is_dist")
    c["depth"][i] = AR.place_mirror(dtype=np.float32, **kw, **c)["dist"][i]      # the restatement's own float32 distance
    return c


def full_case(name, n):
    """n rays of plane `name`: seeded ones, and behind them the edge rows where n has room for them (so they sit in the last
    wave of the launch: at n = 257 the last of them is the only thread of the second block)."""
    if n < E:
        return AR.plane_case(name, n, NEAR)
    kw, c = AR.plane_case(name, n - E, NEAR)
    e = edge_rows(kw)
    return kw, {k: np.concatenate([c[k], e[k]]) for k in c}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", list(AR.PLANES))
def test_place_mirror_bit_exact(name, n):
    """Every output of the four launches (mask_bool and the flag given or null) equals the float32 restatement as bytes."""
    kw, c = full_case(name, n)
    for with_bool in (True, False):
        for any_in in (0, None):
            check_place(c, kw, with_bool, any_in, tag=f"{name} n={n} bool={with_bool} any={any_in}")


@pytest.mark.parametrize("name", list(AR.PLANES))
def test_edge_rows_by_name(name):
    """What each edge row is there for holds in the restatement (the row is on the edge it was built for) and in the kernel's
    own arrays."""
    n = 257
    kw, c = full_case(name, n)
    got, want = check_place(c, kw, tag=name)
    row = {k: n - E + i for i, k in enumerate(EDGE_NAMES)}
    f = np.float32
    r0, r1, r2, r3 = (f(v) for v in kw["rect"])
    nrm = np.array(kw["plane_normal"], np.float32)
    a = 1 if kw["axis"] == AR.PLANE_Y else 0

    def state(k):
        i = row[k]
        return SimpleNamespace(i=i, hit=bool(want["hit"][i]), inside=bool(want["in_rect"][i]), mask=got["mask"][i], mb=got["mask_bool"][i],
                               normal_written=np.array_equal(got["normal"][i], nrm), normal_kept=np.array_equal(got["normal"][i], c["normal"][i]),
                               x_kept=np.array_equal(_bits(got["x_surface"][i]), _bits(c["x_surface"][i])),
                               depth_kept=_bits(got["depth"])[i] == _bits(c["depth"])[i], depth=got["depth"][i], x=got["x_surface"][i])

    def is_hit(s):      # the kernel's arrays of a ray that hit
        return s.mask == 1 and s.mb == 1 and s.normal_written and s.x[a] == f(kw["position"]) and s.depth == want["dist"][s.i]
    # on each of the four edges: inside
    for k, v, edge in (("u_on_r0", "u", r0), ("u_on_r1", "u", r1), ("w_on_r2", "w", r2), ("w_on_r3", "w", r3)):
        s = state(k)
        assert want[v][s.i] == edge, (k, want[v][s.i], edge)
        assert s.inside and s.hit and is_hit(s), k
    s = state("origin_in_plane")
    assert want["s"][s.i] == 0 and s.inside and not s.hit, "origin_in_plane"
    assert s.normal_written and s.x_kept and s.depth_kept and s.mask == 0 and s.mb == 0, "origin_in_plane: the normal only"
    s = state("depth_is_dist")
    assert c["depth"][s.i] == want["dist"][s.i] > f(NEAR) and not want["blocked"][s.i] and is_hit(s), "depth_is_dist: not blocked"
    s = state("depth_is_near")
    assert c["depth"][s.i] == f(NEAR) < want["dist"][s.i] and not want["blocked"][s.i] and is_hit(s), "depth_is_near: a hit"
    s = state("depth_above_near")
    assert f(NEAR) < c["depth"][s.i] < f(NEAR) * f(1.000001) and want["blocked"][s.i] and not s.hit, "depth_above_near: blocked"
    assert s.normal_written and s.x_kept and s.depth_kept and s.mask == 0 and s.mb == 0, "depth_above_near: the normal only"
    s = state("parallel_in_plane")
    assert np.isnan(want["u"][s.i]) and np.isnan(want["w"][s.i]) and s.inside and not s.hit, "parallel_in_plane: NaN coordinates count as inside"
    assert s.normal_written and s.x_kept and s.depth_kept and s.mask == 0 and s.mb == 0, "parallel_in_plane: the normal only"
    for k in ("parallel_off_plane", "parallel_off_plane_nan_u", "nan_depth_outside"):
        s = state(k)
        assert not s.inside and s.normal_kept and s.x_kept and s.depth_kept and s.mask == 0 and s.mb == 0, f"{k}: nothing changes"
    assert np.isinf(want["u"][row["parallel_off_plane"]]) and np.isnan(want["u"][row["parallel_off_plane_nan_u"]])
    assert np.isnan(got["depth"][row["nan_depth_outside"]])
    for k in ("negative_depth", "nan_depth_hit"):
        s = state(k)
        assert not want["blocked"][s.i] and is_hit(s), k
    s = state("masked_no_hit")
    assert not s.inside and s.mask == 1 and s.mb == 1 and s.normal_kept and s.x_kept and s.depth_kept, "masked_no_hit: stays in the mask"
    s = state("masked_fraction_behind")
    assert s.inside and not s.hit and want["s"][s.i] < 0 and s.mask == 1 and s.mb == 1 and s.normal_written and s.x_kept and s.depth_kept


# ------------------------------------------------------------------------------------------------------------ the flag
def _miss_case(n, kw):
    """n rays that run along the axis past the rectangle: nothing merges."""
    e = edge_rows(kw)
    i = EDGE_NAMES.index("nan_depth_outside")
    c = {k: np.repeat(v[i:i + 1], n, axis=0) for k, v in e.items()}
    c["depth"][:] = 10.0
    return c, e


ANY_AT = [(1, 0), (65, 0), (65, 63), (65, 64), (257, 256), (321, 320), (300, 299)]


@pytest.mark.parametrize("n,idx", ANY_AT, ids=[f"{i}_of_{n}" for n, i in ANY_AT])
def test_any_flag(n, idx):
    """The flag is the OR over `merged` of every wave, the tail wave of the second block included: 0 while nothing merges, 1 for
    exactly one merged ray wherever it sits, whether it merged by a hit or by the old mask alone; the caller's bits stay."""
    kw = AR.plane_case("x_default", 1, NEAR)[0]
    c, e = _miss_case(n, kw)
    got, want = check_place(c, kw, any_in=0, tag="no ray merges")
    assert want["any"] == 0 and got["any"][1] == 0 and not got["mask_bool"][:n].any()
    got, _ = check_place(c, kw, any_in=4, tag="no ray merges, caller's 4")
    assert got["any"][1] == 4
    hit = {k: v.copy() for k, v in c.items()}
    for k in hit:
        hit[k][idx] = e[k][EDGE_NAMES.index("u_on_r1")]
    old = {k: v.copy() for k, v in c.items()}
    old["mask"][idx] = 1.0
    for what, case, is_hit in (("one hit", hit, True), ("the old mask alone", old, False)):
        for any_in, flag in ((0, 1), (4, 5)):
            got, want = check_place(case, kw, any_in=any_in, tag=f"{what} at {idx} of {n}")
            assert bool(want["hit"][idx]) == is_hit and int(want["hit"].sum()) == int(is_hit), what
            assert got["any"][1] == flag, f"{what} at {idx} of {n}: the flag is {got['any'][1]} for {flag}"
            assert got["mask_bool"][:n].sum() == 1 and got["mask_bool"][idx] == 1, what
        check_place(case, kw, with_bool=False, any_in=None, tag=f"{what}, null flag")


# ------------------------------------------------------------------------------------------------------------ transform
def _market():
    from mirror_nerf_amd.recursion import resolve_substitution
    rot = resolve_substitution(SimpleNamespace(root_dir="/data/market"))["rotation"]
    assert rot is not None
    return [float(v) for row in rot for v in row]


def _rotation(kind):
    if kind == "none":
        return None
    if kind == "market":
        return _market()
    return np.random.RandomState(11).normal(size=9).astype(np.float32).tolist()


def _xform_rays(n):
    """Seeded rays; behind them, where n has room, a zero direction, two below the clamp (|d|^2 < eps) and a large ray."""
    extra = np.array([[0.3, -0.2, 0.1, 0, 0, 0, 0.1, 6], [1, 2, 3, 1e-5, 0, 0, 0.1, 6], [1, 2, 3, 1e-4, -2e-4, 1e-4, 0.1, 6],
                      [3e4, -2e4, 1e4, 300, 400, -1200, 0.1, 6]], np.float32)
    if n < len(extra):
        return AR.plane_case("y_free", n, NEAR)[1]["rays"], 0
    return np.concatenate([AR.plane_case("y_free", n - len(extra), NEAR)[1]["rays"], extra]), len(extra)


def hip_transform(rays, rotation, scale, translation):
    from mirror_nerf_amd import _lib
    n = rays.shape[0]
    t = _dev(_padded(rays))
    rot = (ctypes.c_float * 9)(*rotation) if rotation is not None else None
    _lib.check(_lib.lib().mnrf_transform_rays(_lib.ptr(t), n, rot, scale, *translation, _lib.stream()), "mnrf_transform_rays")
    return t.cpu().numpy()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind,scale,translation", [
    ("none", 1.0, (0.0, 1.0, 0.0)), ("none", 1.25, (0.5, -1.0, 2.0)), ("market", 1.0, (0.0, 0.0, 0.0)), ("market", 1.25, (0.5, -1.0, 2.0)),
    ("general", 0.75, (0.5, -1.0, 2.0))], ids=["office", "scaled", "market", "market_scaled", "general"])
def test_transform_rays_bit_exact(kind, scale, translation, n):
    rays, n_extra = _xform_rays(n)
    rot = _rotation(kind)
    want = AR.transform_rays(rays, rot, scale, translation, np.float32)
    got = hip_transform(rays, rot, scale, translation)
    _same(got, _padded(want), f"{kind} n={n}")
    _same(got[:n, 6:], rays[:, 6:], "columns 6..7")                # (said once more by name)
    if rot is None:
        _same(got[:n, 3:6], rays[:, 3:6], "directions without a rotation")
    elif n_extra:
        zero, tiny = got[n - 4, 3:6], got[n - 3, 3:6]
        assert not zero.any() and np.isfinite(got[:n]).all(), "a zero direction stays zero: the length is clamped at sqrt(eps)"
        # below the clamp the direction is divided by sqrt(eps), not normalised
        assert 0 < np.linalg.norm(tiny.astype(np.float64)) < 0.5
