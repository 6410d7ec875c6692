"""csrc/mnrf_resample.hip on the GPU: `resample_lanczos` gives Pillow's own bytes (fixture G22) on every shape, for RGB, RGBA
and the (F = 2) stack; a one-axis case runs one pass; the same-size case is a copy; `resize_mask_nearest` is
data._resize_nearest plus the thresholds.  Every comparison has tolerance zero: the arithmetic is integer.

Shapes: those of `RR.cases()` all fit the first 256-thread x-block and one sweep of rows.  `RR.edge_cases()` (fixture
g22_resample_edges) leaves both: (3, 90) -> (300, 3) runs the pass along x alone into a second, ragged x-block (256 + 44);
(9, 300) -> (300, 4) the pass along y alone with ox >= 256; (5, 700) -> (260, 3) both passes with a ragged second block and a
260-wide buffer between them; (7, 1100) -> (520, 5) both passes over three x-blocks; and 3000 frames of (24, 10) -> (7, 23)
give the pass along x 72000 rows and the pass along y 69000, past the 65535 of gridDim.y, so `row += gridDim.y` runs in each.
The mask kernel gets the same edges: 300 and 260 columns, and 69000 rows with its threshold values in the last frame, whose
rows lie past 65535.  Every such case asserts its reach from its shape."""
import ctypes

import numpy as np
import pytest
import torch

from tests import resample_ref as RR
from tests.golden.fixtures import Fixture

pytestmark = pytest.mark.gpu
CASES = RR.cases()
EDGE_CASES = RR.edge_cases()


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


@pytest.fixture(scope="module")
def g22_edges():
    return Fixture("g22_resample_edges")


@pytest.mark.parametrize("name,src,wh", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_resample_is_pillow_s_past_one_launch_tile(g22_edges, name, src, wh):
    """Pillow's bytes past the first x-block and past one sweep of rows; then once more through `out=`, a slice of a larger
    allocation prefilled with 7 whose frames before and after keep that value."""
    import zlib
    from mirror_nerf_amd.data import lanczos_taps, resample_lanczos
    F, sh, sw, C = src.shape
    w, h = wh
    if name == RR.EDGE_STACK:
        assert F * sh > RR.ROWS_MAX and F * h > RR.ROWS_MAX and sw != w and sh != h      # both passes run, each strides
        want = RR.resample(src, wh, lanczos_taps)
        assert zlib.crc32(want.tobytes()) == g22_edges.meta["output_crc32"][name]
    else:
        assert w > RR.TPB and w % RR.TPB != 0
        want = g22_edges.outputs[name]
    s = torch.from_numpy(src).cuda()
    got = resample_lanczos(s, wh)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape == (F, h, w, C)
    got = got.cpu().numpy()
    assert np.array_equal(got, want), (int((got != want).sum()), int(np.abs(got.astype(int) - want.astype(int)).max()))
    if name == RR.EDGE_STACK:
        assert zlib.crc32(got.tobytes()) == g22_edges.meta["output_crc32"][name]
    bank = torch.full((F + 2, h, w, C), 7, dtype=torch.uint8, device="cuda")
    assert resample_lanczos(s, wh, out=bank[1:F + 1]).data_ptr() == bank[1:F + 1].data_ptr()
    assert np.array_equal(bank[1:F + 1].cpu().numpy(), want) and bool((bank[0] == 7).all()) and bool((bank[F + 1] == 7).all())


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


MASK_EDGES = [(1, (3, 90), (300, 3)), (1, (5, 700), (260, 3)), (RR.EDGE_STACK_FRAMES,) + RR.EDGE_STACK_SHAPE]


@pytest.mark.parametrize("F,src_hw,wh", MASK_EDGES, ids=["3x90_to_300x3", "5x700_to_260x3", RR.EDGE_STACK[:-3]])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_mask_nearest_past_one_launch_tile(F, src_hw, wh, dtype):
    """The second, ragged x-block, and rows past gridDim.y: every frame has its own hashed content (one hash over the whole
    stack), and the threshold values sit in the last frame, in the source samples its first output row picks."""
    from mirror_nerf_amd.data import resize_mask_nearest
    (h, w), (dw, dh) = src_hw, wh
    if F == 1:
        assert dw > RR.TPB and dw % RR.TPB != 0
    else:
        assert F * dh > RR.ROWS_MAX and (F - 1) * dh > RR.ROWS_MAX       # the last frame's rows all lie in the second sweep
    m = RR._noise(F * h * w, seed=70 + h).reshape(F, h, w)
    picked = np.minimum(np.floor(np.arange(dw) * (w / dw)).astype(np.int64), w - 1)      # the sample of every output column
    samples, columns = np.unique(picked, return_index=True)                              # ... and a column that shows each
    if dtype == np.uint16:
        m = m.astype(np.uint16) * 257
        m[m < 100 * 257] = 0
        m[F - 1, 0, samples[:3]] = (0, 1, 65535)
        edge = [0, 1, 1]
    else:
        m[F - 1, 0, samples[:4]] = (0, 127, 128, 255)
        edge = [0, 0, 1, 1]
    want = RR.mask_nearest(m, wh)
    assert want[F - 1, 0, columns[:len(edge)]].tolist() == edge and set(np.unique(want)) == {0, 1}
    got = resize_mask_nearest(m, wh)
    assert got.dtype == torch.int8 and tuple(got.shape) == (F, dh, dw)
    got = got.cpu().numpy()
    assert np.array_equal(got, want), (int((got != want).sum()), np.argwhere(got != want)[:3])
    raw = torch.from_numpy(m.view(np.int16) if dtype == np.uint16 else m).cuda()
    big = torch.full((F + 2, dh, dw), -1, dtype=torch.int8, device="cuda")
    assert resize_mask_nearest(raw, wh, out=big[1:F + 1]).data_ptr() == big[1:F + 1].data_ptr()
    assert np.array_equal(big[1:F + 1].cpu().numpy(), want) and bool((big[0] == -1).all()) and bool((big[F + 1] == -1).all())
