"""The output stage of eval.py without a GPU: tests/frames_ref.py (the numpy restatement of eval.py:743-978 the GPU tests
compare with) against cases worked out by hand, the default colour table, the running-extrema rule, and the argument
validation of the C entry points of csrc/mnrf_frames.hip, which happens before any launch."""
import ctypes
import os

import numpy as np
import pytest

from tests import frames_ref as FR

F32 = np.float32


@pytest.fixture(scope="module")
def L():
    from mirror_nerf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _ulp(v, up):
    return np.nextafter(F32(v), F32(2 if up else -2))


def test_cast_is_truncation_inside_the_byte_range():
    v = np.array([0.0, 0.999, 1.0, 1.5, 127.99999, 254.99998, 255.0, 255.99998], F32)
    assert (FR.u8(v) == v.astype(np.uint8)).all()
    assert FR.u8(v).tolist() == [0, 0, 1, 1, 127, 254, 255, 255]
    # the pinned values outside it
    assert FR.u8(np.array([np.nan, -0.5, -3.0, -np.inf, 256.0, 1e9, np.inf], F32)).tolist() == [0, 0, 0, 0, 255, 255, 255]


def test_rgb_edges_by_hand():
    """trunc(clip(v, 0, 1) * 255) at k/255 and one ulp either side: the float32 product decides, not the real one."""
    for k in (0, 1, 2, 3, 127, 128, 254, 255):
        for v in (F32(k / 255), _ulp(k / 255, True), _ulp(k / 255, False)):
            c = min(max(float(v), 0.0), 1.0)
            want = int(np.float32(c) * np.float32(255))         # one float32 multiply, truncated
            got = FR.rgb_image(np.full((1, 3), v, F32))
            assert got.tolist() == [[want] * 3], (k, v)
    # the product of float32(k / 255) and 255 need not be k: 1/255 rounds down and gives 0.99999994
    assert FR.rgb_image(np.full((1, 3), F32(1 / 255), F32))[0, 0] in (0, 1)
    assert FR.rgb_image(np.array([[-0.25, 1.5, 0.5]], F32)).tolist() == [[0, 255, 127]]
    assert FR.rgb_image(np.array([[-3.0, 7.0, 1.0]], F32)).tolist() == [[0, 255, 255]]


def test_mask_and_normals_by_hand():
    assert FR.mask_image(np.array([-0.5, 0.0, 0.5, 1.0, 1.7], F32)).tolist() == [[0] * 3, [0] * 3, [127] * 3, [255] * 3, [255] * 3]
    # (v + 1) / 2: -1 -> 0, 0 -> 127 (0.5 * 255 = 127.5), 1 -> 255, outside clipped
    assert FR.normal_image(np.array([[-1.0, 0.0, 1.0], [-2.0, 3.0, 0.5]], F32)).tolist() == [[0, 127, 255], [0, 255, 191]]


def test_x_surface_by_hand():
    assert (FR.x_surface_image(np.full((5, 3), -1.5, F32)) == 255).all()            # min == max: all ones
    xs = np.array([[0.0, 1.0, 2.0], [4.0, 3.0, 2.0]], F32)                          # extremes 0 and 4 over all channels
    assert FR.x_surface_image(xs).tolist() == [[0, 63, 127], [255, 191, 127]]
    mn, mx = FR.x_surface_extrema(xs)
    assert (mn, mx) == (0.0, 4.0) and mn.dtype == F32


def test_depth_by_hand():
    T = np.arange(768, dtype=np.int64).reshape(256, 3) % 251
    T = T.astype(np.uint8)
    d = np.array([2.0, 3.0, 4.0, 6.0], F32)                     # (d - 2) / 4 -> 0, .25, .5, 1 -> k = 0, 63, 127, 255
    assert (FR.depth_image(d, T) == T[[0, 63, 127, 255]]).all()
    # a constant map: the divisor is 1e-8, every index 0
    assert (FR.depth_image(np.full(7, 3.25, F32), T) == T[0]).all()
    # NaN -> 0, +inf -> FLT_MAX, -inf -> -FLT_MAX before the extremes are taken
    mi, ma = FR.depth_extrema(np.array([np.nan, 2.0, 5.0], F32))
    assert (mi, ma) == (0.0, 5.0)
    assert (FR.depth_image(np.array([np.nan, 2.0, 5.0], F32), T) == T[[0, 102, 255]]).all()
    mi, ma = FR.depth_extrema(np.array([np.inf, 2.0], F32))
    assert ma == np.finfo(F32).max and mi == 2.0
    assert (FR.depth_image(np.array([np.inf, 2.0, 5.0], F32), T) == T[[255, 0, 0]]).all()      # 3 / FLT_MAX is 0
    mi, ma = FR.depth_extrema(np.array([np.inf, -np.inf, 1.0], F32))
    assert (mi, ma) == (-np.finfo(F32).max, np.finfo(F32).max)
    # both infinities: ma - mi overflows to inf; FLT_MAX - mi is inf too and inf / inf is NaN -> index 0; finite / inf is 0
    assert (FR.depth_image(np.array([np.inf, -np.inf, 1.0], F32), T) == T[[0, 0, 0]]).all()
    # given extremes clip: below vmin -> 0, above vmax -> 255
    assert (FR.depth_image(np.array([0.0, 2.0, 4.0, 9.0], F32), T, vmin=F32(2), vmax=F32(6)) == T[[0, 0, 127, 255]]).all()
    # the ToTensor round trip (v / 255) * 255 is exact for every byte in float32
    b = np.arange(256, dtype=np.uint8)
    assert (FR.u8((b.astype(F32) / F32(255)) * 255) == b).all()


def test_depth_reflect_by_hand():
    T = np.full((256, 3), 200, np.uint8)
    d = np.array([1.0, 2.0, 3.0, 4.0], F32)
    m = np.array([-1.0, 0.5, 1.0, 2.0], F32)
    want = [int((F32(200) / F32(255)) * F32(c) * F32(255)) for c in (0.0, 0.5, 1.0, 1.0)]
    assert FR.depth_reflect_image(d, m, T).tolist() == [[w] * 3 for w in want]
    assert want[0] == 0 and want[2] == 200


def test_jet_table():
    from mirror_nerf_amd.frames import jet_table
    T = jet_table()
    assert T.shape == (256, 3) and T.dtype == np.uint8
    # BGR: entry 0 is the blue-most (no red), entry 255 the red-most (no blue)
    assert T[0, 0] > 0 and T[0, 2] == 0 and T[0, 1] == 0
    assert T[255, 2] > 0 and T[255, 0] == 0 and T[255, 1] == 0
    assert T[0, 0] == 128 and T[255, 2] == 128 and T[:, 0].max() == 255 and T[:, 1].max() == 255 and T[:, 2].max() == 255
    # every channel rises to its plateau and falls from it: one sign change of the slope at most
    for c in range(3):
        d = np.diff(T[:, c].astype(np.int64))
        d = d[d != 0]
        assert (np.diff(np.sign(d)) != 0).sum() <= 1, c
    assert T[:, 0].argmax() < T[:, 1].argmax() < T[:, 2].argmax()


def test_running_extrema_rule():
    """Three frames, the middle one with a NaN: its np.min / np.max are NaN and the `<` / `>` updates skip it, wherever it
    stands -- first included, the one difference from the reference."""
    a = np.array([2.0, 3.0, 5.0], F32)
    b = np.array([1.0, np.nan, 9.0], F32)
    c = np.array([2.5, 6.0, np.inf], F32)
    r = FR.RunningExtrema().update(a).update(b).update(c)
    assert (r.min, r.max) == (2.0, np.inf) and r.min.dtype == F32
    r = FR.RunningExtrema().update(b)
    assert (r.min, r.max) == (np.inf, -np.inf)
    r.update(a)
    assert (r.min, r.max) == (2.0, 5.0)
    # the unified image uses them as vmin / vmax
    T = np.arange(768).reshape(256, 3).astype(np.uint8)
    assert (FR.depth_image(b, T, r.min, r.max) == T[[0, 0, 255]]).all()      # 1 clips to 2, NaN -> 0 clips to 2, 9 clips to 5


def test_frame_images_presence_rules():
    m = FR.seeded_maps(11, 0)
    T = np.arange(768).reshape(256, 3).astype(np.uint8)
    full = {"rgb_fine": m["rgb"], "depth_fine": m["depth"], "mirror_mask_fine": m["mirror_mask"],
            "depth_fine_reflect": m["depth_reflect"], "surface_normal_fine": m["surface_normal"], "x_surface_fine": m["x_surface"]}
    assert set(FR.frame_images(full, T)) == {"rgb_fine", "depth_fine", "mirror_mask_fine", "depth_reflect_fine",
                                             "surface_normal_fine", "x_surface_fine"}
    no_mask = {k: v for k, v in full.items() if k != "mirror_mask_fine"}
    assert "depth_reflect_fine" not in FR.frame_images(no_mask, T)
    assert FR.frame_images({k: v for k, v in full.items() if k != "rgb_fine"}, T) == {}
    assert all(v.shape == (11, 3) and v.dtype == np.uint8 for v in FR.frame_images(full, T).values())


def test_abi_validates_before_any_launch(L):
    """Null stats, n < 0 and a missing table are refused with the entry point's name in mnrf_last_error; n == 0 is a no-op.
    Nothing here reaches a launch, so no GPU is needed."""
    from mirror_nerf_amd import frames as FM
    assert L.mnrf_frame_stats_floats() >= 6 and L.mnrf_split_extrema_floats() == 4
    stats = (ctypes.c_float * L.mnrf_frame_stats_floats())()
    sp = ctypes.cast(stats, ctypes.c_void_p)
    fake = ctypes.c_void_p(4096)        # never dereferenced: validation only
    assert L.mnrf_frame_extrema(fake, None, None, 16, None, None, None) < 0
    assert b"mnrf_frame_extrema" in L.mnrf_last_error()
    assert L.mnrf_frame_extrema(fake, None, None, -1, sp, None, None) < 0
    assert b"mnrf_frame_extrema" in L.mnrf_last_error()
    assert L.mnrf_frame_extrema(None, None, None, 0, sp, None, None) == 0

    maps, images = FM._Maps(), FM._Images()
    assert L.mnrf_frame_finish(None, ctypes.byref(images), 16, sp, None, None) < 0
    assert b"mnrf_frame_finish" in L.mnrf_last_error()
    assert L.mnrf_frame_finish(ctypes.byref(maps), ctypes.byref(images), 16, None, None, None) < 0
    assert b"mnrf_frame_finish" in L.mnrf_last_error() and b"stats" in L.mnrf_last_error()
    assert L.mnrf_frame_finish(ctypes.byref(maps), ctypes.byref(images), -5, sp, None, None) < 0
    assert b"mnrf_frame_finish" in L.mnrf_last_error()
    maps.depth, images.depth = 4096, 8192
    assert L.mnrf_frame_finish(ctypes.byref(maps), ctypes.byref(images), 16, sp, None, None) < 0
    assert b"mnrf_frame_finish" in L.mnrf_last_error() and b"table" in L.mnrf_last_error()
    maps, images = FM._Maps(), FM._Images()
    maps.depth_reflect, images.depth_reflect = 4096, 8192          # the reflected image needs the mask as well
    assert L.mnrf_frame_finish(ctypes.byref(maps), ctypes.byref(images), 16, sp, fake, None) < 0
    assert b"mirror mask" in L.mnrf_last_error()
    assert L.mnrf_frame_finish(ctypes.byref(FM._Maps()), ctypes.byref(FM._Images()), 0, sp, None, None) == 0

    assert L.mnrf_depth_colormap(fake, None, 2, 16, None, None, fake, fake, None) < 0          # neither extrema nor stats
    assert b"mnrf_depth_colormap" in L.mnrf_last_error()
    assert L.mnrf_depth_colormap(fake, None, 2, -1, fake, None, fake, fake, None) < 0
    assert L.mnrf_depth_colormap(fake, None, 2, 16, fake, None, None, fake, None) < 0
    assert b"mnrf_depth_colormap" in L.mnrf_last_error() and b"table" in L.mnrf_last_error()
    assert L.mnrf_depth_colormap(None, None, 0, 16, fake, None, fake, None, None) == 0
    assert L.mnrf_depth_colormap(None, None, 2, 0, fake, None, fake, None, None) == 0


def test_cpu_maps_are_rejected():
    import torch
    import mirror_nerf_amd as M
    with pytest.raises(RuntimeError, match="GPU only"):
        M.finish_frame({"rgb_fine": torch.zeros(4, 3)})
    with pytest.raises(RuntimeError, match="GPU only"):
        M.colormap_depth(torch.zeros(2, 4))
    with pytest.raises(RuntimeError, match="GPU only"):
        M.SplitExtrema("cpu")
    assert M.finish_frame({"depth_fine": torch.zeros(4)}) == {}      # nothing without rgb (eval.py:762)
