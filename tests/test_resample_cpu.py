"""The device resize without a GPU: `data.lanczos_taps`, fed through the numpy restatement of tests/resample_ref.py (what
csrc/mnrf_resample.hip is written from), reproduces Pillow's own LANCZOS resize (fixture G22) with tolerance zero; the C entry
points refuse bad arguments with a message before any launch.

Shapes: those of `RR.cases()`, each inside one 256-wide x-block of the device kernels, and those of `RR.edge_cases()` (fixture
g22_resample_edges), which tests/test_hip_resample.py runs on the device past that block and past 65535 rows: outputs 300, 260
and 520 wide, and a 3000-frame stack of which the fixture keeps Pillow's CRC-32.  Here they anchor the restatement to Pillow
at those shapes."""
import ctypes
import os
import zlib

import numpy as np
import pytest

from tests import resample_ref as RR
from tests.golden.fixtures import Fixture

CASES = RR.cases()
EDGE_CASES = RR.edge_cases()


@pytest.fixture(scope="module")
def g22():
    return Fixture("g22_resample")


def test_sources_are_the_fixture_s(g22):
    assert {n for n, _, _ in CASES} == set(g22.outputs)
    for name, src, _ in CASES:
        assert zlib.crc32(src.tobytes()) == g22.meta["source_crc32"][name], name


@pytest.mark.parametrize("name,src,wh", CASES, ids=[c[0] for c in CASES])
def test_taps_reproduce_pillow(g22, name, src, wh):
    from mirror_nerf_amd.data import lanczos_taps
    got = RR.resample(src, wh, lanczos_taps)
    want = g22.outputs[name]
    assert got.shape == want.shape == (src.shape[0], wh[1], wh[0], src.shape[3])
    assert np.array_equal(got, want), int(np.abs(got.astype(int) - want.astype(int)).max())


@pytest.fixture(scope="module")
def g22_edges():
    return Fixture("g22_resample_edges")


def test_edge_sources_are_the_fixture_s(g22_edges):
    """The stack's output is kept as a checksum only; every other case has its bytes."""
    assert {n for n, _, _ in EDGE_CASES} == set(g22_edges.outputs) | {RR.EDGE_STACK} == set(g22_edges.meta["source_crc32"])
    assert set(g22_edges.meta["output_crc32"]) == {RR.EDGE_STACK}
    for name, src, _ in EDGE_CASES:
        assert zlib.crc32(src.tobytes()) == g22_edges.meta["source_crc32"][name], name
    stack = dict((n, s) for n, s, _ in EDGE_CASES)[RR.EDGE_STACK]
    assert len({zlib.crc32(f.tobytes()) for f in stack}) == stack.shape[0]        # no two frames agree


@pytest.mark.parametrize("name,src,wh", EDGE_CASES, ids=[c[0] for c in EDGE_CASES])
def test_taps_reproduce_pillow_past_one_launch_tile(g22_edges, name, src, wh):
    from mirror_nerf_amd.data import lanczos_taps
    F, sh, sw, C = src.shape
    if name == RR.EDGE_STACK:
        assert RR.rows_strided(F, sh, wh[1]) and sw != wh[0]
    else:
        assert RR.past_one_x_block(wh[0])
    got = RR.resample(src, wh, lanczos_taps)
    assert got.dtype == np.uint8 and got.shape == (F, wh[1], wh[0], C)
    if name == RR.EDGE_STACK:
        assert zlib.crc32(got.tobytes()) == g22_edges.meta["output_crc32"][name]
    else:
        want = g22_edges.outputs[name]
        assert got.shape == want.shape
        assert np.array_equal(got, want), int(np.abs(got.astype(int) - want.astype(int)).max())


def test_same_size_is_a_copy_without_the_alpha_round_trip(g22):
    name = "6x8_to_8x6_c4_noise"
    src = dict((n, s) for n, s, _ in CASES)[name]
    assert np.array_equal(g22.outputs[name], src)
    assert not np.array_equal(RR.unpremultiply(RR.premultiply(src)), src)        # the round trip would have changed it


def test_tap_tables():
    from mirror_nerf_amd.data import lanczos_taps
    for n_in, n_out in ((37, 11), (23, 31), (7, 3), (64, 1), (1440, 360), (5, 64)):
        bounds, taps = lanczos_taps(n_in, n_out)
        support = 3.0 * max(n_in / n_out, 1.0)
        assert bounds.shape == (n_out, 2) and taps.shape == (n_out, 2 * int(np.ceil(support)) + 1)
        assert bounds.dtype == np.int32 and taps.dtype == np.int32
        lo, n = bounds[:, 0], bounds[:, 1]
        assert (lo >= 0).all() and (n >= 1).all() and (lo + n <= n_in).all() and (n <= taps.shape[1]).all()
        # normalised: the taps of a window sum to 2^22 up to the rounding of each (half a unit per tap)
        assert (np.abs(taps.sum(1) - (1 << 22)) <= taps.shape[1] / 2).all()
        assert all((taps[i, n[i]:] == 0).all() for i in range(n_out))
        # a constant image stays what it is, and 255 * the positive taps stays inside an int32
        assert (255 * np.where(taps > 0, taps, 0).astype(np.int64).sum(1) + (1 << 21) < 2 ** 31).all()
    assert lanczos_taps(37, 11)[0] is lanczos_taps(37, 11)[0]       # cached
    with pytest.raises(ValueError):
        lanczos_taps(0, 4)


def test_mask_reference_rule():
    m8 = np.array([[[0, 127, 128, 255]]], np.uint8)
    m16 = np.array([[[0, 1, 127, 65535]]], np.uint16)
    assert RR.mask_nearest(m8, (4, 1)).tolist() == [[[0, 0, 1, 1]]]
    assert RR.mask_nearest(m16, (4, 1)).tolist() == [[[0, 1, 1, 1]]]
    assert RR.mask_nearest(m8, (2, 2)).tolist() == [[[0, 1], [0, 1]]]        # floor(x * 4 / 2): samples 0 and 2


# --------------------------------------------------------------------------- the C entry points, no launch
def test_entry_points_validate_before_any_launch():
    from mirror_nerf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    fake = ctypes.c_void_p(256)

    def resample(src=fake, frames=2, sh=30, sw=40, c=3, dst=fake, dh=7, dw=11, tx=fake, bx=fake, kx=23, ty=fake, by=fake, ky=27, tmp=fake):
        return L.mnrf_resample_u8(src, frames, sh, sw, c, dst, dh, dw, tx, bx, kx, ty, by, ky, tmp, None)

    def refused(code, word):
        return code < 0 and word in L.mnrf_last_error()

    for c in (0, 1, 2, 5):
        assert refused(resample(c=c), b"channels")
    for kw in (dict(frames=0), dict(sh=0), dict(sw=-1), dict(dh=0), dict(dw=0)):
        assert refused(resample(**kw), b"at least 1"), kw
    assert refused(resample(sw=2 ** 31 - 1), b"too large")
    assert refused(resample(dh=30, dw=40), b"both passes skipped")
    assert refused(resample(src=None), b"null source") and refused(resample(dst=None), b"null source")
    assert refused(resample(tx=None), b"along x") and refused(resample(bx=None), b"along x") and refused(resample(kx=0), b"along x")
    assert refused(resample(ty=None), b"along y") and refused(resample(by=None), b"along y") and refused(resample(ky=0), b"along y")
    assert refused(resample(tmp=None), b"tmp")
    # the buffer between the passes: (frames, src_h, dst_w, C); nothing when at most one pass runs; -1 for what is refused
    assert L.mnrf_resample_tmp_bytes(2, 30, 40, 7, 11, 3) == 2 * 30 * 11 * 3
    assert L.mnrf_resample_tmp_bytes(2, 30, 40, 7, 11, 4) == 2 * 30 * 11 * 4
    assert L.mnrf_resample_tmp_bytes(2, 30, 40, 30, 11, 4) == 0 and L.mnrf_resample_tmp_bytes(2, 30, 40, 7, 40, 4) == 0
    assert L.mnrf_resample_tmp_bytes(2, 30, 40, 7, 11, 2) == -1 and L.mnrf_resample_tmp_bytes(0, 30, 40, 7, 11, 3) == -1

    def mask(src=fake, nbytes=1, frames=2, sh=30, sw=40, dst=fake, dh=9, dw=12):
        return L.mnrf_mask_nearest(src, nbytes, frames, sh, sw, dst, dh, dw, None)

    for nbytes in (0, 3, 4):
        assert refused(mask(nbytes=nbytes), b"1 or 2 bytes")
    for kw in (dict(frames=0), dict(sh=0), dict(sw=0), dict(dh=-3), dict(dw=0)):
        assert refused(mask(**kw), b"at least 1"), kw
    assert refused(mask(src=None), b"null source") and refused(mask(dst=None), b"null source")
    assert refused(mask(src=ctypes.c_void_p(257), nbytes=2), b"odd address")


def test_python_entry_points_need_the_gpu():
    import torch
    from mirror_nerf_amd import data
    with pytest.raises(RuntimeError, match="GPU only"):
        data.resample_lanczos(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), (2, 2))
    with pytest.raises(RuntimeError, match="GPU only"):
        data.resize_mask_nearest(torch.zeros(1, 4, 4, dtype=torch.uint8), (2, 2))
    with pytest.raises(RuntimeError, match="GPU only"):
        data.RayBank.from_arkit("nowhere", device="cpu")
