"""csrc/mnrf_resample.hip on the GPU: `resample_lanczos` gives Pillow's own bytes (fixture G22) on every shape, for RGB, RGBA
and the (F = 2) stack; a one-axis case runs one pass; the same-size case is a copy; `resize_mask_nearest` is
data._resize_nearest plus the thresholds.  Every comparison has tolerance zero: the arithmetic is integer."""
import ctypes

import numpy as np
import pytest
import torch

from tests import resample_ref as RR
from tests.golden.fixtures import Fixture

pytestmark = pytest.mark.gpu
CASES = RR.cases()


@pytest.fixture(scope="module")
def g22():
    return Fixture("g22_resample")


@pytest.mark.parametrize("name,src,wh", CASES, ids=[c[0] for c in CASES])
def test_resample_is_pillow_s(g22, name, src, wh):
    from mirror_nerf_amd.data import resample_lanczos
    got = resample_lanczos(torch.from_numpy(src).cuda(), wh)
    want = g22.outputs[name]
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    got = got.cpu().numpy()
    assert np.array_equal(got, want), (int((got != want).sum()), int(np.abs(got.astype(int) - want.astype(int)).max()))


def test_out_argument_and_a_view_of_a_larger_stack(g22):
    """Writing straight into a slice of a bank's array, as from_arkit does; the frames around it stay untouched."""
    from mirror_nerf_amd.data import resample_lanczos
    name, src, wh = next(c for c in CASES if c[0] == "stack2_c4")
    bank = torch.full((4, wh[1], wh[0], 4), 7, dtype=torch.uint8, device="cuda")
    assert resample_lanczos(torch.from_numpy(src).cuda(), wh, out=bank[1:3]).data_ptr() == bank[1:3].data_ptr()
    assert np.array_equal(bank[1:3].cpu().numpy(), g22.outputs[name]) and bool((bank[0] == 7).all()) and bool((bank[3] == 7).all())
    with pytest.raises(ValueError, match="out must be"):
        resample_lanczos(torch.from_numpy(src).cuda(), wh, out=bank[:, :, :, :3])


@pytest.mark.parametrize("name", ["30x40_to_20x30_c3_noise", "30x40_to_20x30_c4_ramp", "29x37_to_37x11_c3_noise", "29x37_to_37x11_c4_noise"])
def test_one_axis_cases_run_one_pass(g22, name):
    """Two passes need the buffer between them and are refused without it: a call that is given none, and only the tables of the
    axis that changes, can have run one pass at most -- and its bytes are right, so it ran that one."""
    from mirror_nerf_amd import _lib
    from mirror_nerf_amd.data import _taps_on
    _, src, (w, h) = next(c for c in CASES if c[0] == name)
    F, sh, sw, C = src.shape
    assert (sw == w) != (sh == h)
    L = _lib.lib()
    assert L.mnrf_resample_tmp_bytes(F, sh, sw, h, w, C) == 0
    s = torch.from_numpy(src).cuda()
    dst = torch.zeros(F, h, w, C, dtype=torch.uint8, device="cuda")
    t, b, k = _taps_on(sw, w, s.device) if sw != w else _taps_on(sh, h, s.device)
    x = (t.data_ptr(), b.data_ptr(), k) if sw != w else (None, None, 0)
    y = (t.data_ptr(), b.data_ptr(), k) if sh != h else (None, None, 0)
    _lib.check(L.mnrf_resample_u8(s.data_ptr(), F, sh, sw, C, dst.data_ptr(), h, w, *x, *y, None, _lib.stream()), "mnrf_resample_u8")
    assert np.array_equal(dst.cpu().numpy(), g22.outputs[name])


@pytest.mark.parametrize("c", [3, 4])
def test_same_size_returns_the_input_bytes(c):
    from mirror_nerf_amd.data import resample_lanczos
    src = RR.make_source((6, 8), c, "noise", seed=5)[None]
    s = torch.from_numpy(src).cuda()
    got = resample_lanczos(s, (8, 6))
    assert got.data_ptr() != s.data_ptr() and np.array_equal(got.cpu().numpy(), src)     # RGBA: no premultiply round trip


def test_a_wrong_table_reads_nothing_outside_the_frame():
    """The windows are clamped in the kernel: a bounds table that points past the source (and counts past ksize) gives wrong
    pixels, never a read outside.  The frame sits inside a larger allocation whose other bytes are 255: a pixel made from a
    zero frame with any all-positive table is 0 unless something outside was read."""
    from mirror_nerf_amd import _lib
    F, sh, sw, C, w = 1, 4, 8, 3, 5
    big = torch.full((3, sh, sw, C), 255, dtype=torch.uint8, device="cuda")
    big[1] = 0
    taps = torch.full((7, w), (1 << 22) // 7, dtype=torch.int32, device="cuda")
    bounds = torch.tensor([[-5, 7], [6, 7], [8, 7], [100, 1000], [2, -3]], dtype=torch.int32, device="cuda")
    dst = torch.full((F, sh, w, C), 9, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().mnrf_resample_u8(big[1].data_ptr(), F, sh, sw, C, dst.data_ptr(), sh, w, taps.data_ptr(), bounds.data_ptr(),
                                           7, None, None, 0, None, _lib.stream()), "mnrf_resample_u8")
    assert bool((dst == 0).all())


@pytest.mark.parametrize("src_hw,wh", [((30, 40), (12, 9)), ((9, 12), (40, 30))])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_mask_nearest(src_hw, wh, dtype):
    from mirror_nerf_amd.data import resize_mask_nearest
    h, w = src_hw
    m = np.stack([RR.make_source(src_hw, 3, "noise", seed=60 + f)[..., 0] for f in range(2)])
    if dtype == np.uint16:
        m = m.astype(np.uint16) * 257
        m[m < 100 * 257] = 0
        m[:, 0, :3] = (0, 1, 65535)
    else:
        m[:, 0, :4] = (0, 127, 128, 255)
    want = RR.mask_nearest(m, wh)
    got = resize_mask_nearest(m, wh)                                    # a numpy array is uploaded
    assert got.dtype == torch.int8 and np.array_equal(got.cpu().numpy(), want)
    raw = torch.from_numpy(m.view(np.int16) if dtype == np.uint16 else m).cuda()
    out = torch.full((2,) + (wh[1], wh[0]), -1, dtype=torch.int8, device="cuda")
    assert resize_mask_nearest(raw, wh, out=out) is out and np.array_equal(out.cpu().numpy(), want)
    assert set(np.unique(want)) == {0, 1}
