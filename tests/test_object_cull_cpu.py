"""CPU-side checks of object bounds (mirror_nerf_amd/object_bounds.py, csrc/mnrf_object_cull.hip): argument validation of the
three C-ABI entry points without a GPU, ObjectBounds validation and its host-side views, the refusals of batched_inference, and
the float64 reference of the rule (tests/object_cull_ref.py) against hand-worked cases on a 2x2x2 grid -- plus the share of the
GPU test's random rays that falls into the band between "must keep" and "must cull", which that test relies on."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import object_cull_ref as R


@pytest.fixture(scope="module")
def L():
    from mirror_nerf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _f3(*v):
    return (ctypes.c_float * 3)(*v)


# ----------------------------------------------------------------------------------------------- the C ABI
def test_occupancy_bits_validates_its_arguments(L):
    null = None
    for bad in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (1025, 4, 4), (4, -1, 4), (4, 4, 1025)):
        assert L.mnrf_occupancy_bits(64, *bad, 0.5, 1, 64, null, null) < 0 and b"1..1024" in L.mnrf_last_error(), bad
    for dilate in (-1, 2):
        assert L.mnrf_occupancy_bits(64, 4, 4, 4, 0.5, dilate, 64, null, null) < 0 and b"dilate" in L.mnrf_last_error()
    assert L.mnrf_occupancy_bits(null, 4, 4, 4, 0.5, 1, 64, null, null) < 0 and b"null pointer" in L.mnrf_last_error()
    assert L.mnrf_occupancy_bits(64, 4, 4, 4, 0.5, 1, null, null, null) < 0 and b"null pointer" in L.mnrf_last_error()


def test_object_cull_validates_its_arguments(L):
    null = None
    lo, hi = _f3(0, 0, 0), _f3(1, 1, 1)
    assert L.mnrf_object_cull(null, 0, null, 1.0, 0.0, 0.0, 0.0, lo, hi, 1, 1, 1, null, null, null, null, null) == 0     # zero rays: a no-op
    assert L.mnrf_object_cull(null, -1, null, 1.0, 0.0, 0.0, 0.0, lo, hi, 1, 1, 1, null, null, null, null, null) < 0
    assert b"bad size" in L.mnrf_last_error()
    assert L.mnrf_object_cull(null, 2 ** 31, null, 1.0, 0.0, 0.0, 0.0, lo, hi, 1, 1, 1, null, null, null, null, null) < 0     # the index is int32
    assert b"bad size" in L.mnrf_last_error()
    assert L.mnrf_object_cull(null, 4, null, 1.0, 0.0, 0.0, 0.0, null, hi, 1, 1, 1, null, null, null, null, null) < 0
    assert b"box_lo" in L.mnrf_last_error()
    for blo, bhi in ((_f3(0, 1, 0), hi), (_f3(0, 2, 0), hi), (_f3(0, float("nan"), 0), hi), (lo, _f3(1, float("inf"), 1)),
                     (_f3(-3e38, 0, 0), _f3(3e38, 1, 1))):
        assert L.mnrf_object_cull(null, 4, null, 1.0, 0.0, 0.0, 0.0, blo, bhi, 1, 1, 1, null, null, null, null, null) < 0
        assert b"lo < hi" in L.mnrf_last_error()
    for bad in ((0, 1, 1), (1, 1025, 1), (1, 1, -2)):
        assert L.mnrf_object_cull(64, 4, null, 1.0, 0.0, 0.0, 0.0, lo, hi, *bad, 64, 128, 64, 64, null) < 0
        assert b"1..1024" in L.mnrf_last_error()
    for ptrs in ((null, 128, 64, 64), (64, null, 64, 64), (64, 128, null, 64), (64, 128, 64, null)):
        assert L.mnrf_object_cull(ptrs[0], 4, null, 1.0, 0.0, 0.0, 0.0, lo, hi, 1, 1, 1, null, *ptrs[1:], null) < 0
        assert b"null pointer" in L.mnrf_last_error()
    assert L.mnrf_object_cull(64, 4, null, 1.0, 0.0, 0.0, 0.0, lo, hi, 1, 1, 1, null, 64, 64, 64, null) < 0
    assert b"out of place" in L.mnrf_last_error()


def test_object_merge_indexed_validates_its_arguments(L):
    null = None
    assert L.mnrf_object_merge_indexed(null, null, null, null, null, 0, 1.0, 1.0, 0.05, null, null, null, null, null) == 0
    assert L.mnrf_object_merge_indexed(null, null, null, null, null, -1, 1.0, 1.0, 0.05, null, null, null, null, null) < 0
    assert b"bad size" in L.mnrf_last_error()
    good = [64, 64, 64, 64, 64, 64, 64]       # obj_rgb, obj_depth, obj_opacity, index, count, rgb, depth
    for miss in range(7):
        a = [null if i == miss else v for i, v in enumerate(good)]
        assert L.mnrf_object_merge_indexed(*a[:5], 4, 1.0, 1.0, 0.05, a[5], a[6], null, null, null) < 0, miss
        assert b"null pointer" in L.mnrf_last_error()


# ----------------------------------------------------------------------------------------------- ObjectBounds
def test_object_bounds_validation():
    from mirror_nerf_amd import ObjectBounds
    b = ObjectBounds((0, 0, 0), [1, 2, 3])
    assert (b.lo, b.hi, b.res, b.bits) == ((0.0, 0.0, 0.0), (1.0, 2.0, 3.0), (1, 1, 1), None)
    assert b.n_set == 1 and b.tight_box() == (b.lo, b.hi) and b.touches_region_border()
    assert ObjectBounds(np.zeros(3), torch.ones(3)).hi == (1.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="three numbers"):
        ObjectBounds((0, 0), (1, 1, 1))
    with pytest.raises(ValueError, match="finite"):
        ObjectBounds((0, 0, float("nan")), (1, 1, 1))
    with pytest.raises(ValueError, match="lo < hi"):
        ObjectBounds((0, 0, 0), (1, 0, 1))
    with pytest.raises(ValueError, match="float32"):
        ObjectBounds((0, 0, 1.0), (1, 1, 1.0 + 1e-12))
    for res in ((0, 1, 1), (1, 1025, 1), (2, 2), (1.0, 1, 1), (True, 1, 1)):
        with pytest.raises(ValueError, match="res must be"):
            ObjectBounds((0, 0, 0), (1, 1, 1), res, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError, match="without bits"):
        ObjectBounds((0, 0, 0), (1, 1, 1), (2, 2, 2))
    with pytest.raises(TypeError, match="torch tensor"):
        ObjectBounds((0, 0, 0), (1, 1, 1), (2, 2, 2), np.zeros(4, np.int32))
    with pytest.raises(ValueError, match="int32"):
        ObjectBounds((0, 0, 0), (1, 1, 1), (2, 2, 2), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match=r"= 70 words"):
        ObjectBounds((0, 0, 0), (1, 1, 1), (33, 5, 7), torch.zeros(35, dtype=torch.int32))
    assert ObjectBounds((0, 0, 0), (1, 1, 1), (33, 5, 7), torch.zeros(70, dtype=torch.int32)).bits.shape == (7, 5, 2)
    assert ObjectBounds((0, 0, 0), (1, 1, 1), 2, torch.zeros(4, dtype=torch.int32)).res == (2, 2, 2)
    with pytest.raises(ValueError, match="padding bit"):
        ObjectBounds((0, 0, 0), (1, 1, 1), (2, 2, 2), torch.full((4,), 4, dtype=torch.int32)).n_set
    # CPU bits are fine to hold and to look at; the cull wants them where the rays are
    cpu = ObjectBounds((0, 0, 0), (1, 1, 1), (2, 2, 2), torch.ones(4, dtype=torch.int32))
    with pytest.raises((ValueError, RuntimeError)):
        cpu.cull(torch.zeros(4, 8), dict(pose=None, scale=1.0, translation=(0, 0, 0), pose_scale0=1.0))


def test_object_bounds_views():
    from mirror_nerf_amd import ObjectBounds
    cells = R.grid_cells("33x5x7")
    bits = torch.from_numpy(R.pack_bits(cells).view(np.int32))
    b = ObjectBounds(R.BOX_LO, R.BOX_HI, (33, 5, 7), bits)
    assert np.array_equal(b.cells(), cells) and b.n_set == int(cells.sum())
    lo, hi = b.tight_box()
    k, j, i = np.nonzero(cells)
    size = (np.array(R.BOX_HI) - np.array(R.BOX_LO)) / (33, 5, 7)
    assert np.allclose(lo, np.array(R.BOX_LO) + size * (i.min(), j.min(), k.min()), rtol=0, atol=1e-12)
    assert np.allclose(hi, np.array(R.BOX_LO) + size * (i.max() + 1, j.max() + 1, k.max() + 1), rtol=0, atol=1e-12)
    assert b.touches_region_border()                       # cell x = 32 of the run into the last word
    inner = np.zeros((4, 4, 4), bool)
    inner[1:3, 1:3, 2] = True
    b = ObjectBounds((0, 0, 0), (4, 4, 4), 4, torch.from_numpy(R.pack_bits(inner).view(np.int32)))
    assert not b.touches_region_border() and b.tight_box() == ((2.0, 1.0, 1.0), (3.0, 3.0, 3.0)) and b.n_set == 4
    empty = ObjectBounds((0, 0, 0), (4, 4, 4), 4, torch.zeros(16, dtype=torch.int32))
    assert empty.n_set == 0 and empty.tight_box() is None and not empty.touches_region_border()


def test_default_sigma_min_is_the_stated_bound():
    from mirror_nerf_amd.object_bounds import default_sigma_min
    s = default_sigma_min((-1.5,) * 3, (1.5,) * 3)
    diag = 3.0 * np.sqrt(3.0)
    assert abs(s - (-np.log(0.9) / diag)) < 1e-15
    assert abs((1.0 - np.exp(-s * diag)) - 0.1) < 1e-12      # the longest segment of the region, at the threshold: opacity 0.1


# ----------------------------------------------------------------------------------------------- batched_inference
def _models():
    import mirror_nerf_amd as M
    make = lambda: M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=True)  # noqa: E731
    return {"coarse": make(), "fine": make()}


def _args(**over):
    a = dict(predict_normal=True, only_one_field=False, only_one_field_fine_epoch=2, max_recursive_level=1, near=0.05,
             root_dir="office", app_reflect_newly_placed_objects=True, obj_model_type="nerf_pl")
    a.update(over)
    return a


def test_batched_inference_refusals():
    import mirror_nerf_amd as M
    from types import SimpleNamespace
    box = M.ObjectBounds((-1, -1, -1), (1, 1, 1))
    obj = SimpleNamespace(models=[], embeddings=[])
    call = lambda args, **kw: M.batched_inference(_models(), {}, torch.zeros(4, 8), 64, 64, False, 32, args=args,  # noqa: E731
                                                  trace_secondary_rays=True, **kw)
    off = {k: v for k, v in _args().items() if k not in ("app_reflect_newly_placed_objects", "obj_model_type")}
    with pytest.raises(ValueError, match="application is not on"):
        call(off, object_bounds=box)
    with pytest.raises(ValueError, match="application is not on"):
        call(off, object_bounds="auto", object_region=((-1, -1, -1), (1, 1, 1)))
    with pytest.raises(ValueError, match="must be None, an ObjectBounds or 'auto'"):
        call(_args(), system_obj=obj, object_bounds=((-1, -1, -1), (1, 1, 1)))
    with pytest.raises(ValueError, match="must be None, an ObjectBounds or 'auto'"):
        call(_args(), system_obj=obj, object_bounds="tight")
    with pytest.raises(ValueError, match="needs object_region"):
        call(_args(), system_obj=obj, object_bounds="auto")
    with pytest.raises(ValueError, match="pass object_bounds='auto'"):
        call(_args(), system_obj=obj, object_region=((-1, -1, -1), (1, 1, 1)))
    with pytest.raises(ValueError, match="needs system_obj="):                       # the application's own refusals come first
        call(_args(), object_bounds=box)


# ----------------------------------------------------------------------------------------------- the reference itself
def test_reference_bits_by_hand():
    v = np.zeros((3, 3, 3), np.float32)                    # 2x2x2 cells, corners [z, y, x]
    v[0, 0, 0] = 1.0                                       # the corner of cell (0, 0, 0) alone
    c = R.occupancy_cells(v, 0.5, 0)
    assert c.sum() == 1 and c[0, 0, 0]
    assert R.occupancy_cells(v, 0.5, 1).all()              # every cell of a 2x2x2 grid neighbours it
    v[0, 0, 0], v[1, 1, 1] = 0.0, 0.5                      # the centre corner, equal to the threshold: !(0.5 < 0.5) sets all 8 cells
    assert R.occupancy_cells(v, 0.5, 0).all()
    assert not R.occupancy_cells(v, np.nextafter(np.float32(0.5), np.float32(1)), 0).any()
    v[1, 1, 1], v[2, 2, 0] = 0.0, np.nan                   # a NaN corner sets its cell: (x, y, z) = (0, 1, 1)
    c = R.occupancy_cells(v, 0.5, 0)
    assert c.sum() == 1 and c[1, 1, 0]
    three = np.zeros((1, 1, 3), bool)
    three[0, 0, 0] = True
    v = np.zeros((2, 2, 4), np.float32)
    v[:, :, 0] = 1.0
    assert np.array_equal(R.occupancy_cells(v, 0.5, 0), three)
    assert np.array_equal(R.occupancy_cells(v, 0.5, 1)[0, 0], [True, True, False])
    # packing: cell i is bit i % 32 of word i / 32, the padding stays zero
    row = np.zeros((1, 1, 33), bool)
    row[0, 0, [0, 5, 31, 32]] = True
    assert R.pack_bits(row).tolist() == [[[(1 << 0) | (1 << 5) | (1 << 31), 1]]]


def test_reference_rule_by_hand():
    """A 2x2x2 grid over [0, 2]^3 with the one set cell (1, 1, 1) = [1, 2]^3; grown by a cell that is [0, 3]^3."""
    cells = np.zeros((2, 2, 2), bool)
    cells[1, 1, 1] = True
    lo, hi = (0, 0, 0), (2, 2, 2)
    assert R.run_boxes(cells, lo, hi).tolist() == [[[1, 1, 1], [2, 2, 2]]]
    assert R.run_boxes(cells, lo, hi, grow=1.0).tolist() == [[[0, 0, 0], [3, 3, 3]]]
    nan, inf = np.nan, np.inf
    rays = np.array([
        # o            d            near far     keep   cull
        [-1, 1.5, 1.5, 1, 0, 0,     0, 10],    # through the cell along x                                     keep
        [-1, 1.5, 1.5, 1, 0, 0,     0, 1.5],   # ends at x = 0.5: in the grown cell, not in the cell           band
        [-1, 1.5, 1.5, 1, 0, 0,     0, 0.5],   # ends at x = -0.5, before the grown cell                       cull
        [-1, 1.5, 1.5, 1, 0, 0,     0, 2.0],   # ends exactly on the face x = 1: closed cells                  keep
        [-1, 1.5, 1.5, 1, 0, 0,     5, 10],    # starts at x = 4, behind the grown cell                        cull
        [-1, 1.5, 1.5, 1, 0, 0,     3.5, 10],  # starts at x = 2.5: in the grown cell only                     band
        [-1, 1.5, 1.5, 1, 0, 0,     10, 0],    # far < near                                                    cull
        [-1, 0.5, 1.5, 1, 0, 0,     0, 10],    # parallel, one cell beside (y = 0.5): the grown cell           band
        [-1, -0.5, 1.5, 1, 0, 0,    0, 10],    # parallel, outside the grown cell (y = -0.5)                   cull
        [-1, 2.0, 1.5, 1, 0, 0,     0, 10],    # parallel, in the face y = 2                                   keep
        [1.5, 1.5, 1.5, 0, 0, 1,    0, 0.1],   # origin inside the cell                                        keep
        [1.5, 1.5, 1.5, 0, 0, 0,    1, 2],     # zero direction, a point in the cell                           keep
        [3.5, 3.5, 3.5, 0, 0, 0,    1, 2],     # zero direction, a point outside the grown cell                cull
        [0, 0, 0, 1, 1, 1,          0, 1.0],   # the diagonal up to the corner (1, 1, 1) of the cell           keep
        [0, 4.5, 1.5, 1, -1, 0,     0, 10],    # x + y = 4.5: passes the cell's edge (2, 2) at a distance      band
        [0, 7, 1.5, 1, -1, 0,       0, 10],    # x + y = 7: passes the grown cell's edge (3, 3)                cull
        [nan, 1.5, 1.5, 1, 0, 0,    0, 10],    # non-finite rows are kept whatever they point at
        [-1, -9, 1.5, 1, 0, inf,    0, 10],
        [-1, -9, 1.5, 1, 0, 0,      0, inf],
        [-1, -9, 1.5, 1, 0, 0,      nan, 10],
    ], np.float64)
    want = ["keep", "band", "cull", "keep", "cull", "band", "cull", "band", "cull", "keep", "keep", "keep", "cull", "keep", "band",
            "cull", "keep", "keep", "keep", "keep"]
    keep, cull = R.classify(rays, cells, lo, hi)
    got = ["keep" if k else "cull" if c else "band" for k, c in zip(keep, cull)]
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    # two set cells in a row are one run, and the empty grid culls every finite ray
    cells[1, 1, 0] = True
    assert R.run_boxes(cells, lo, hi).tolist() == [[[0, 1, 1], [2, 2, 2]]]
    keep, cull = R.classify(rays, np.zeros((2, 2, 2), bool), lo, hi)
    assert keep.tolist() == [False] * 16 + [True] * 4 and cull.tolist() == [True] * 16 + [False] * 4


@pytest.mark.parametrize("pose", list(R.POSES))
@pytest.mark.parametrize("grid", R.GRIDS)
def test_band_share_of_the_random_families(grid, pose):
    """The construction the GPU test relies on: of its random rays (through / missing), classified by the reference alone on
    the float64 ray move, at most 20 % fall between the two rules; both certain classes are well populated."""
    cells = R.grid_cells(grid)
    fam = R.ray_families(cells, R.BOX_LO, R.BOX_HI, 4100, seed=3)
    rnd = np.concatenate([fam["through"], fam["missing"]])
    q = R.object_rays64(R.to_scene(rnd, R.POSES[pose], **R.MOVE).astype(np.float32), R.POSES[pose], **R.MOVE)
    keep, cull = R.classify(q, cells, R.BOX_LO, R.BOX_HI)
    assert not (keep & cull).any()
    band = 1.0 - keep.mean() - cull.mean()
    print(f"{grid} {pose}: must keep {keep.mean():.3f}, must cull {cull.mean():.3f}, band {band:.3f}")
    assert band <= 0.20 and keep.mean() >= 0.2 and cull.mean() >= 0.2
    # the deterministic families say what their names say
    cls = {}
    for name, rows in fam.items():
        k, c = R.classify(rows.astype(np.float32), cells, R.BOX_LO, R.BOX_HI)
        cls[name] = (k, c)
    assert cls["origin_inside"][0].all() and cls["nan"][0].all() and cls["inf"][0].all()
    assert cls["starts_behind"][1].all() and cls["far_below_near"][1].all()
    assert cls["axis_parallel"][0][0::2].all() and cls["axis_parallel"][1][1::2].all()
    assert cls["zero_direction"][0][:2].all() and cls["zero_direction"][1][2:].all()
    assert not cls["ends_before"][0].any()
