"""GPU tests of object bounds: mnrf_occupancy_bits, mnrf_object_cull and mnrf_object_merge_indexed against the float64
restatement of the rule (tests/object_cull_ref.py) at tolerance zero, and batched_inference(object_bounds=) against the run
without bounds on the smallest scene fixtures of G26 (nerf_pl object) and G27 (D-NeRF object).

The cull is held to the two certain classes of the rule -- every must-keep ray is kept, no must-cull ray is -- and the band
between them (either answer is right there) is held to at most 20 % of the random rays, so that it cannot hide a failure
(tests/test_object_cull_cpu.py checks the same share on the CPU).  Kept rows are compared as bytes with mnrf_object_rays."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import object_cull_ref as R
from tests.golden import fixtures as FX

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32 = np.float32
SIZES = [0, 1, 63, 64, 65, 257, 4099]      # wave, block (1024) and multi-block edges of the compaction


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits32(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.fixture(params=["split", "fp32"])
def precision(request):
    from mirror_nerf_amd import mirror_nerf as MN
    old = MN.PRECISION
    MN.set_precision(request.param)
    yield request.param
    MN.set_precision(old)


# ----------------------------------------------------------------------------------------------- occupancy bits
def _volume(rx, ry, rz, sigma_min, seed):
    """Corner samples around the threshold: below, above, exactly equal (sets the cell), NaN (sets it), and wide empty parts."""
    rs = np.random.RandomState(seed)
    v = rs.uniform(0.0, 0.9 * sigma_min, (rz + 1, ry + 1, rx + 1)).astype(F32)
    n = v.size
    flat = v.reshape(-1)
    pick = rs.choice(n, max(3, n // 40), replace=False)
    third = len(pick) // 3
    flat[pick[:third]] = rs.uniform(1.1, 5.0, third) * sigma_min
    flat[pick[third:2 * third]] = F32(sigma_min)
    flat[pick[2 * third:]] = np.nan
    if rx > 8:
        v[:, :, rx // 2:rx // 2 + 4] = 0.0           # an empty slab, so that dilation has something to grow into
    return v


@pytest.mark.parametrize("dilate", [0, 1])
@pytest.mark.parametrize("res", [(1, 1, 1), (4, 4, 4), (33, 5, 7), (64, 64, 64), (32, 3, 2), (65, 2, 3)], ids=lambda r: "x".join(map(str, r)))
def test_occupancy_bits_equal_the_reference(res, dilate):
    from mirror_nerf_amd import _lib
    rx, ry, rz = res
    sigma_min = 0.37
    v = _volume(rx, ry, rz, sigma_min, seed=rx + 7 * dilate)
    want_cells = R.occupancy_cells(v, sigma_min, dilate)
    want = R.pack_bits(want_cells)
    assert np.isnan(v).any() and (v == F32(sigma_min)).any()
    if res != (1, 1, 1):
        assert 0 < want_cells.sum() < want_cells.size or dilate
    vol = _dev(v)
    words = (rx + 31) // 32
    bits = torch.full((rz, ry, words), -1, dtype=torch.int32, device=DEV)
    n_set = torch.full((1,), 12345, dtype=torch.int32, device=DEV)
    p = _lib.ptr
    _lib.check(_lib.lib().mnrf_occupancy_bits(p(vol), rx, ry, rz, sigma_min, dilate, p(bits), p(n_set), _lib.stream()), "mnrf_occupancy_bits")
    got = bits.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want)                                             # bit for bit, the padding bits (zero in `want`) included
    if rx % 32:
        assert not (got[:, :, -1] >> np.uint32(rx % 32)).any()
    assert int(n_set.item()) == int(want_cells.sum())
    assert np.array_equal(_bits32(vol.cpu().numpy()), _bits32(v))               # the volume is read only
    # the same bits twice, and without the counter
    bits2 = torch.empty_like(bits)
    _lib.check(_lib.lib().mnrf_occupancy_bits(p(vol), rx, ry, rz, sigma_min, dilate, p(bits2), None, _lib.stream()), "mnrf_occupancy_bits")
    assert torch.equal(bits, bits2)


# ----------------------------------------------------------------------------------------------- the cull
class _Case:
    """One grid and one pose: the scene rays of every family (shuffled), their object-frame rows from mnrf_object_rays on the
    device, and the reference's two classes of them -- computed once, shared by the sizes."""
    _cache = {}

    def __init__(self, grid, pose_name):
        from mirror_nerf_amd import _lib
        self.cells = R.grid_cells(grid)
        self.pose = R.POSES[pose_name]
        self.lo = tuple(float(F32(v)) for v in R.BOX_LO)
        self.hi = tuple(float(F32(v)) for v in R.BOX_HI)
        fam = R.ray_families(self.cells, R.BOX_LO, R.BOX_HI, 4100, seed=3)
        rows = np.concatenate(list(fam.values()))
        self.random = np.concatenate([np.full(len(v), k in ("through", "missing")) for k, v in fam.items()])
        order = np.random.RandomState(5).permutation(len(rows))
        self.random = self.random[order]
        self.rays = R.to_scene(rows, self.pose, **R.MOVE).astype(F32)[order]
        assert len(self.rays) >= SIZES[-1]
        src = _dev(self.rays)
        self.q = torch.empty_like(src)
        _lib.check(_lib.lib().mnrf_object_rays(_lib.ptr(src), len(self.rays), self.pose_c(), R.MOVE["scale"], *R.MOVE["translation"],
                                               _lib.ptr(self.q), _lib.stream()), "mnrf_object_rays")
        self.q = self.q.cpu().numpy()
        self.must_keep, self.must_cull = R.classify(self.q, self.cells, self.lo, self.hi)
        self.bits = _dev(R.pack_bits(self.cells).view(np.int32))

    def pose_c(self):
        return (ctypes.c_float * 12)(*np.asarray(self.pose, F32).reshape(-1).tolist()) if self.pose is not None else None

    @classmethod
    def get(cls, grid, pose_name):
        key = (grid, pose_name)
        if key not in cls._cache:
            cls._cache[key] = cls(grid, pose_name)
        return cls._cache[key]


def _cull(case, n, with_bits=True):
    from mirror_nerf_amd import _lib
    src = _dev(case.rays[:n])
    out = torch.full((n, 8), -7.0, dtype=torch.float32, device=DEV)
    index = torch.full((n,), -3, dtype=torch.int32, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    rz, ry, rx = case.cells.shape
    p = _lib.ptr
    _lib.check(_lib.lib().mnrf_object_cull(p(src), n, case.pose_c(), R.MOVE["scale"], *R.MOVE["translation"],
                                           (ctypes.c_float * 3)(*case.lo), (ctypes.c_float * 3)(*case.hi), rx, ry, rz,
                                           p(case.bits) if with_bits else None, p(out), p(index), p(count), _lib.stream()),
               "mnrf_object_cull")
    torch.cuda.synchronize()
    assert np.array_equal(_bits32(src.cpu().numpy()), _bits32(case.rays[:n])), "the source rays were written"
    return out.cpu().numpy(), index.cpu().numpy(), int(count.item())


def _check_cull(case, n, out, index, count, must_keep, must_cull):
    assert 0 <= count <= n
    idx = index[:count]
    assert (np.diff(idx) > 0).all() and (count == 0 or (idx[0] >= 0 and idx[-1] < n))       # strictly increasing rows of the source
    assert np.array_equal(_bits32(out[:count]), _bits32(case.q[:n][idx]))                   # mnrf_object_rays' own bytes
    kept = np.zeros(n, bool)
    kept[idx] = True
    lost = np.nonzero(must_keep[:n] & ~kept)[0]
    wrong = np.nonzero(must_cull[:n] & kept)[0]
    assert lost.size == 0, f"{lost.size} rays that meet a set cell were culled, first rows {lost[:5]}: {case.q[lost[:2]]}"
    assert wrong.size == 0, f"{wrong.size} rays that miss the grown cells were kept, first rows {wrong[:5]}: {case.q[wrong[:2]]}"
    return kept


@pytest.mark.parametrize("pose", list(R.POSES))
@pytest.mark.parametrize("grid", R.GRIDS)
def test_cull_follows_the_rule(grid, pose):
    case = _Case.get(grid, pose)
    n = len(case.rays)
    rnd = case.random
    band = ~(case.must_keep | case.must_cull)
    share = band[rnd].mean()
    print(f"{grid} {pose}: {n} rays, must keep {case.must_keep.mean():.3f}, must cull {case.must_cull.mean():.3f}, "
          f"band share of the random families {share:.3f}")
    assert share <= 0.20 and case.must_keep[rnd].mean() >= 0.2 and case.must_cull[rnd].mean() >= 0.2
    out, index, count = _cull(case, n)
    kept = _check_cull(case, n, out, index, count, case.must_keep, case.must_cull)
    print(f"  kept {count}, of the band {int((kept & band).sum())} of {int(band.sum())}")
    assert np.isnan(case.rays).any(1).sum() >= 8 and np.isinf(case.rays).any(1).sum() >= 8
    assert kept[~np.isfinite(case.rays).all(1)].all()
    # the same call again gives the same bytes: nothing depends on the order of execution
    out2, index2, count2 = _cull(case, n)
    assert count2 == count and np.array_equal(index2[:count], index[:count]) and np.array_equal(_bits32(out2[:count]), _bits32(out[:count]))


@pytest.mark.parametrize("n", SIZES)
def test_cull_sizes(n):
    case = _Case.get("4x4x4", "similarity")
    out, index, count = _cull(case, n)
    _check_cull(case, n, out, index, count, case.must_keep, case.must_cull)
    if n == 0:
        assert count == 0 and out.size == 0
    if n >= 63:
        assert 0 < count < n


@pytest.mark.parametrize("pose", ["no_pose", "similarity"])
def test_cull_without_bits_is_the_box(pose):
    """bits = null: the whole box counts as one set cell, whatever Rx, Ry, Rz say."""
    case = _Case.get("1x1x1", pose)
    n = len(case.rays)
    a = _cull(case, n, with_bits=False)
    b = _cull(case, n, with_bits=True)
    _check_cull(case, n, *a, case.must_keep, case.must_cull)
    assert a[2] == b[2] and np.array_equal(a[1][:a[2]], b[1][:b[2]])
    other = _Case.get("33x5x7", pose)                      # the same box with a grid that is not looked at
    c = _cull(other, n, with_bits=False)
    keep, cull = R.classify(other.q, np.ones((1, 1, 1), bool), other.lo, other.hi)
    _check_cull(other, n, *c, keep, cull)


def test_cull_keeps_everything_and_nothing():
    case = _Case.get("4x4x4", "no_pose")
    n = 1500                                               # a full round of the compaction and a partial one
    full = SimpleNamespace(**vars(case))
    full.pose_c = case.pose_c
    full.lo, full.hi = (-1e6,) * 3, (1e6,) * 3
    full.bits = torch.full((4, 4, 1), 15, dtype=torch.int32, device=DEV)
    out, index, count = _cull(full, n)
    finite = np.isfinite(case.q[:n]).all(1)
    empty_seg = finite & (case.q[:n, 7] < case.q[:n, 6])
    assert count == n - int(empty_seg.sum()) and not np.isin(np.nonzero(empty_seg)[0], index[:count]).any()
    none = SimpleNamespace(**vars(case))
    none.pose_c = case.pose_c
    none.bits = torch.zeros((4, 4, 1), dtype=torch.int32, device=DEV)
    out, index, count = _cull(none, n)
    assert count == int((~finite).sum()) and np.array_equal(index[:count], np.nonzero(~finite)[0])


# ----------------------------------------------------------------------------------------------- the indexed merge
@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "null_mask"])
@pytest.mark.parametrize("n,m", [(1000, 300), (1000, 1000), (257, 1), (64, 0)])
def test_indexed_merge_equals_the_merge_on_the_listed_rows(n, m, with_mask):
    from mirror_nerf_amd import _lib
    from tests.test_hip_objects import _merge_inputs
    scale, ps0, near = 3.0, 0.7, 0.05
    rs = np.random.RandomState(n + m)
    index = np.sort(rs.choice(n, m, replace=False)).astype(np.int32)
    # the level's maps: rows of every branch of the rule (test_hip_objects._merge_inputs); the object's maps of the listed rows
    obj_rgb, obj_depth, obj_opacity, rgb, depth, mask = _merge_inputs(n, scale, ps0, near, seed=3)
    if m >= 300:
        assert np.isin(np.arange(48), index).sum() >= 8           # some of the hand-made edge rows are listed
    c_rgb, c_depth, c_op = obj_rgb[index], obj_depth[index], obj_opacity[index]
    p = _lib.ptr
    # reference: mnrf_object_merge on the gathered rows
    g = [_dev(a) for a in (c_rgb, c_depth, c_op, rgb[index], depth[index], mask[index])]
    used_ref = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().mnrf_object_merge(p(g[0]), p(g[1]), p(g[2]), m, scale, ps0, near, p(g[3]), p(g[4]), p(g[5]) if with_mask else None,
                                            p(used_ref), _lib.stream()), "mnrf_object_merge")
    want_rgb, want_depth, want_mask = rgb.copy(), depth.copy(), mask.copy()
    want_rgb[index], want_depth[index], want_mask[index] = g[3].cpu().numpy(), g[4].cpu().numpy(), g[5].cpu().numpy()
    # capacity above the count: the count on the device decides; rows of the object's maps behind it are never read as rows to merge
    cap = m + 5
    pad = lambda a: np.concatenate([a, np.full((5,) + a.shape[1:], 0.9, F32)])  # noqa: E731
    t = [_dev(a) for a in (pad(c_rgb), pad(c_depth), pad(c_op), rgb, depth, mask)]
    idx = _dev(np.concatenate([index, np.zeros(5, np.int32)]))
    count = _dev(np.array([m], np.int32))
    used = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().mnrf_object_merge_indexed(p(t[0]), p(t[1]), p(t[2]), p(idx), p(count), cap, scale, ps0, near, p(t[3]), p(t[4]),
                                                    p(t[5]) if with_mask else None, p(used), _lib.stream()), "mnrf_object_merge_indexed")
    torch.cuda.synchronize()
    assert int(used.item()) == int(used_ref.item())
    if m >= 300:
        assert 0 < int(used.item()) < m
    assert np.array_equal(_bits32(t[3].cpu().numpy()), _bits32(want_rgb))        # listed rows as the merge leaves them, the others untouched
    assert np.array_equal(_bits32(t[4].cpu().numpy()), _bits32(want_depth))
    assert np.array_equal(_bits32(t[5].cpu().numpy()), _bits32(want_mask if with_mask else mask))
    # a capacity below the count clips it
    if m == 300:
        t2 = [_dev(a) for a in (rgb, depth)]
        _lib.check(_lib.lib().mnrf_object_merge_indexed(p(t[0]), p(t[1]), p(t[2]), p(idx), p(count), 100, scale, ps0, near, p(t2[0]), p(t2[1]),
                                                        None, None, _lib.stream()), "mnrf_object_merge_indexed")
        w = depth.copy()
        w[index[:100]] = want_depth[index[:100]]
        assert np.array_equal(_bits32(t2[1].cpu().numpy()), _bits32(w))


# ----------------------------------------------------------------------------------------------- batched_inference
def _smallest(prefix):
    """The scene fixture with the fewest rays (then the fewest levels)."""
    best = None
    for name in FX.names(prefix):
        fx = FX.Fixture(name)
        if "rays" not in fx.inputs:
            continue
        key = (fx.inputs["rays"].shape[0], fx.meta["args"]["max_recursive_level"], name)
        if best is None or key < best[0]:
            best = (key, fx)
    return best[1]


def _runner(kind):
    """(fixture, run(fx, args=None, **extra) -> dict of numpy maps) of the nerf_pl (G26) or the D-NeRF (G27) object."""
    if kind == "nerf_pl":
        from tests import test_hip_objects as T
        return _smallest("g26_object_"), T._run
    from tests import test_hip_dnerf as T

    def run(fx, args=None, **extra):
        if args is None:
            return T._run(fx, **extra)
        import mirror_nerf_amd as M
        m = fx.meta
        sds = fx.state_dicts()
        models = {"coarse": T._scene_module(sds[0]), "fine": T._scene_module(sds[1])}
        emb = {"xyz": M.Embedding(10), "dir": M.Embedding(4)}
        kw = dict(new_object=m["new_object"], render_kwargs_test_d_nerf=T._object_kwargs(m), frame_time=m["frame_time"]) \
            if args.get("app_reflect_newly_placed_objects") else {}
        out = M.batched_inference(models, emb, _dev(fx.inputs["rays"]), m["N_samples"], m["N_importance"], False, m["chunk"], args=args,
                                  trace_secondary_rays=True, **kw, **extra)
        return {k: v.detach().cpu().numpy() for k, v in out.items()}
    return _smallest("g27_dnerf_"), run


def _same(a, b, keys=None):
    assert set(a) == set(b), set(a) ^ set(b)
    for k in keys or a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_the_smallest_fixtures():
    assert _smallest("g26_object_").name == "g26_object_default_chunk96" and _smallest("g27_dnerf_").name == "g27_dnerf_single_posed_l1"


@pytest.mark.parametrize("kind", ["nerf_pl", "d_nerf"])
def test_all_keeping_bounds_change_nothing(kind, precision):
    """Bounds that keep every ray: each returned map and object_used are bit for bit those of object_bounds=None, at the
    fixture's own recursion level (the object is seen in the mirrors too)."""
    from mirror_nerf_amd import ObjectBounds
    fx, run = _runner(kind)
    used = torch.zeros(1, dtype=torch.int32, device=DEV)
    base = run(fx, object_used=used)
    n_base = int(used.item())
    assert n_base > 0
    box = ObjectBounds((-1e6,) * 3, (1e6,) * 3)
    grid = ObjectBounds((-1e6,) * 3, (1e6,) * 3, (4, 4, 4), torch.full((4, 4, 1), 15, dtype=torch.int32))      # (CPU bits: moved to the rays' device)
    for bounds in (box, grid):
        got = run(fx, object_used=used, object_bounds=bounds)
        assert int(used.item()) == n_base
        _same(base, got)


def _off(args):
    return {k: v for k, v in args.items() if k not in ("app_reflect_newly_placed_objects", "obj_model_type")}


def _count_object_renders(monkeypatch, kind, object_modules):
    """Counts the launches of the object's field inside batched_inference: calls of render_rays on the object's models
    (nerf_pl), calls of render_rays_dnerf (D-NeRF)."""
    from mirror_nerf_amd import recursion
    calls = []
    if kind == "nerf_pl":
        real = recursion.render_rays

        def counting(models, *a, **kw):
            if any(m in object_modules for m in models.values()):
                calls.append(a[1].shape[0])
            return real(models, *a, **kw)
        monkeypatch.setattr(recursion, "render_rays", counting)
    else:
        real = recursion.render_rays_dnerf

        def counting(batch, **kw):
            calls.append(batch.shape[0])
            return real(batch, **kw)
        monkeypatch.setattr(recursion, "render_rays_dnerf", counting)
    return calls


@pytest.mark.parametrize("kind", ["nerf_pl", "d_nerf"])
def test_partial_bounds_three_ways(kind, precision, monkeypatch):
    """max_recursive_level 0, a box that part of the primary rays miss: the rays mnrf_object_cull keeps equal the run without
    bounds, the others the run without the application.  A box no ray hits: the run without the application, and the object's
    field is not launched at all."""
    from mirror_nerf_amd import ObjectBounds, _lib, recursion
    fx, run = _runner(kind)
    args = dict(fx.meta["args"], max_recursive_level=0)
    rays = _dev(fx.inputs["rays"])
    N = rays.shape[0]
    xform = recursion.resolve_new_object(SimpleNamespace(**args), fx.meta["new_object"])
    q = torch.empty_like(rays)
    pose = (ctypes.c_float * 12)(*xform["pose"]) if xform["pose"] is not None else None
    _lib.check(_lib.lib().mnrf_object_rays(_lib.ptr(rays), N, pose, xform["scale"], *xform["translation"], _lib.ptr(q), _lib.stream()),
               "mnrf_object_rays")
    q = q.cpu().numpy().astype(np.float64)
    extra, modules = {}, set()
    if kind == "nerf_pl":
        from tests import test_hip_objects as T
        extra["system_obj"] = T._object_system(fx.meta)
        modules = set(extra["system_obj"].models.values())
    calls = _count_object_renders(monkeypatch, kind, modules)
    used = torch.zeros(1, dtype=torch.int32, device=DEV)
    full = run(fx, args=args, object_used=used, **extra)
    n_full = int(used.item())
    assert sum(calls) == N and n_full > 0                                                 # the counter sees the object's renders
    calls.clear()
    off = run(fx, args=_off(args), **extra)
    assert calls == []
    took = (full["rgb_fine"] != off["rgb_fine"]).any(1) | (full["depth_fine"] != off["depth_fine"])
    assert took.sum() >= 8
    # a box around a point where a ray saw the object (the merged depth, back in the object's units), a fraction of the seen
    # surface wide: that ray is kept and takes the object.  The first such box that part of the rays miss.
    surface = q[:, :3] + q[:, 3:6] * (full["depth_fine"].astype(np.float64) * xform["scale"] * xform["pose_scale0"])[:, None]
    half = 0.15 * (surface[took].max(0) - surface[took].min(0))
    bounds = None
    for i in np.nonzero(took)[0]:
        bounds = ObjectBounds(surface[i] - half, surface[i] + half)
        _, index, count = bounds.cull(rays, xform)
        count = int(count.item())
        if 0 < count <= 0.8 * N:
            break
    else:
        pytest.fail("no box around a seen point of the object is missed by a fifth of the rays")
    kept = np.zeros(N, bool)
    kept[index[:count].cpu().numpy()] = True
    print(f"{fx.name}: {count} of {N} primary rays kept, {int(took[kept].sum())} of them take the object ({int(took.sum())} without bounds)")
    assert kept[i] and took[kept].any()
    part = run(fx, args=args, object_used=used, object_bounds=bounds, **extra)
    assert 0 < int(used.item()) <= n_full
    assert 1 <= len(calls) <= -(-N // fx.meta["chunk"]) and sum(calls) == count           # the object rendered on the kept rows alone
    for k in ("rgb_fine", "depth_fine", "mirror_mask_fine"):
        assert np.array_equal(_bits32(part[k][kept]), _bits32(full[k][kept])), k          # kept rays: the run without bounds
        assert np.array_equal(_bits32(part[k][~kept]), _bits32(off[k][~kept])), k         # culled rays: the scene alone
    # a box that no ray hits
    calls.clear()
    none = run(fx, args=args, object_used=used, object_bounds=ObjectBounds((1e5,) * 3, (1e5 + 1,) * 3), **extra)
    assert calls == [], f"the object's field was launched {len(calls)} times for a box no ray hits"
    assert int(used.item()) == 0
    _same(off, none)


# ----------------------------------------------------------------------------------------------- the estimator
@pytest.mark.parametrize("dilate", [0, 1])
def test_tight_box_of_a_ball(dilate):
    """A ball of density through mnrf_occupancy_bits: the tight box contains it and lies within one cell of it (two with the
    dilation).  The centre sits on a grid corner, so that the ball's six extreme points lie on grid lines, where the corner
    sampling sees them."""
    from mirror_nerf_amd import ObjectBounds
    from mirror_nerf_amd.object_bounds import occupancy_bits
    res, lo, hi = 24, np.array([-1.5, -1.0, -2.0]), np.array([1.5, 2.0, 1.0])
    cell = (hi - lo) / res
    centre, radius = lo + cell * (13, 10, 12), 0.61
    ax = [lo[a] + cell[a] * np.arange(res + 1) for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    inside = (x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2 <= radius ** 2
    volume = np.where(inside, 10.0, 0.0).astype(F32)
    bits, n_set = occupancy_bits(_dev(volume), 0.5, dilate)
    b = ObjectBounds(lo, hi, res, bits)
    assert b.n_set == int(n_set.item()) == int(R.occupancy_cells(volume, 0.5, dilate).sum()) > 0
    assert not b.touches_region_border()
    t_lo, t_hi = (np.array(v) for v in b.tight_box())
    slack = cell * (1 + dilate) + 1e-9
    assert (t_lo <= centre - radius).all() and (t_hi >= centre + radius).all()
    assert (t_lo >= centre - radius - slack).all() and (t_hi <= centre + radius + slack).all()


def test_auto_bounds_of_a_nerf_pl_object(precision):
    """object_bounds="auto" with a region: the frame of the ObjectBounds the estimator returns for that region; estimated once
    and kept on the object."""
    from mirror_nerf_amd import estimate_object_bounds
    from tests import test_hip_objects as T
    fx = _smallest("g26_object_")
    system_obj = T._object_system(fx.meta)
    region = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))
    bounds = estimate_object_bounds(system_obj, *region, res=12)
    print(f"{fx.name}: {bounds.n_set} of {12 ** 3} cells set, tight box {bounds.tight_box()}, touches the border: {bounds.touches_region_border()}")
    assert bounds.res == (12, 12, 12) and bounds.bits.is_cuda and bounds.n_set > 0
    used = torch.zeros(1, dtype=torch.int32, device=DEV)
    want = T._run(fx, system_obj=system_obj, object_used=used, object_bounds=bounds)
    n_want = int(used.item())
    got = T._run(fx, system_obj=system_obj, object_used=used, object_bounds="auto", object_region=region, object_bounds_res=12)
    assert int(used.item()) == n_want
    _same(want, got)
    cached = system_obj._mnrf_object_bounds[1]
    assert torch.equal(cached.bits, bounds.bits)
    T._run(fx, system_obj=system_obj, object_bounds="auto", object_region=region, object_bounds_res=12)
    assert system_obj._mnrf_object_bounds[1] is cached                           # not estimated again


def test_auto_bounds_of_a_dnerf_object():
    """A D-NeRF object is estimated per call at frame_time, through the sigma-only launch of its field: the estimator's bits
    are those of the reference restatement on the same density samples."""
    from mirror_nerf_amd import estimate_object_bounds, mesh
    from mirror_nerf_amd.dnerf import dnerf_field
    from mirror_nerf_amd.object_bounds import default_sigma_min
    from tests import test_hip_dnerf as T
    fx = _smallest("g27_dnerf_")
    kw = T._object_kwargs(fx.meta)
    lo, hi, res = (-1.0, -1.2, -0.8), (1.1, 0.9, 1.0), 9
    t = fx.meta["frame_time"]
    bounds = estimate_object_bounds(kw, lo, hi, res=res, frame_time=t, dilate=0)
    net = kw["network_fine"] if kw["network_fine"] is not None else kw["network_fn"]
    n = res + 1
    xyz = mesh.grid_points((lo[0], hi[0]), (lo[1], hi[1]), (lo[2], hi[2]), n, 0, n ** 3, device=DEV)
    sigma = dnerf_field(net, n ** 3, t, xyz=xyz, sigma_only=True, want_dx=False)["sigma"].view(n, n, n)      # [y, x, z]
    # the points are where the cells' corners are, to fp32 rounding
    ax = [np.linspace(lo[a], hi[a], n) for a in range(3)]
    assert np.abs(xyz.view(n, n, n, 3)[2, 5, 7].cpu().numpy() - (ax[0][5], ax[1][2], ax[2][7])).max() < 1e-6
    want = R.occupancy_cells(sigma.permute(2, 0, 1).cpu().numpy(), default_sigma_min(lo, hi), 0)
    assert np.array_equal(bounds.cells(), want)
    with pytest.raises(ValueError, match="frame_time"):
        estimate_object_bounds(kw, lo, hi, res=res)
