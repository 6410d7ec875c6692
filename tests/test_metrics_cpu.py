"""Structural similarity without a GPU: the numpy restatement of tests/ssim_ref.py against scipy's uniform filter (the one
scikit-image calls) and against closed forms, and the argument validation of mnrf_ssim, which refuses null pointers and
bad sizes before anything touches the GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from mirror_nerf_amd.metrics import ssim, structural_similarity      # what this file is about: it needs the feature
from tests import ssim_ref as R


@pytest.fixture(scope="module")
def L():
    from mirror_nerf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


@pytest.mark.parametrize("win_size", [3, 7, 11])
@pytest.mark.parametrize("kind", R.KINDS)
def test_restatement_agrees_with_scipy_uniform_filter(kind, win_size):
    """skimage.metrics.structural_similarity written out with scipy.ndimage.uniform_filter in float64 (its steps, in its
    order: filter, sample covariance, S, crop of (win_size - 1) // 2, mean; per channel, then the mean over channels)."""
    ndi = pytest.importorskip("scipy.ndimage")
    p, t = R.pair(kind, 40, 52)
    n = win_size * win_size
    cov_norm, c1, c2, pad = n / (n - 1.0), 0.01 ** 2, 0.03 ** 2, (win_size - 1) // 2
    per_channel = []
    for c in range(3):
        x, y = p[..., c].astype(np.float64), t[..., c].astype(np.float64)
        ux, uy = ndi.uniform_filter(x, size=win_size), ndi.uniform_filter(y, size=win_size)
        uxx, uyy, uxy = (ndi.uniform_filter(v, size=win_size) for v in (x * x, y * y, x * y))
        vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
        S = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
        per_channel.append(S[pad:-pad, pad:-pad].mean())
    assert abs(R.structural_similarity(p, t, win_size) - float(np.mean(per_channel))) <= 1e-12


@pytest.mark.parametrize("kind", R.KINDS)
def test_identical_images_give_exactly_one(kind):
    p, _ = R.pair(kind, 37, 53)
    assert R.structural_similarity(p, p) == 1.0
    q = np.ascontiguousarray(p.transpose(2, 0, 1))[None]
    assert R.ssim(q, q) == 1.0 and (R.ssim_map(q, q) == 1.0).all()


@pytest.mark.parametrize("kind", R.KINDS)
def test_symmetry(kind):
    p, t = R.pair(kind, 37, 53)
    assert R.structural_similarity(p, t) == R.structural_similarity(t, p)
    q, u = (np.ascontiguousarray(v.transpose(2, 0, 1))[None] for v in (p, t))
    assert R.ssim(q, u) == R.ssim(u, q)


def test_constant_images_give_the_luminance_term():
    """a = 0.2 against b = 0.6: every variance is 0, so S = (2ab + C1) / (a^2 + b^2 + C1) under both definitions."""
    a, b, c1 = np.float32(0.2), np.float32(0.6), 1e-4
    want = (2.0 * float(a) * float(b) + c1) / (float(a) ** 2 + float(b) ** 2 + c1)
    p, t = np.full((20, 24, 3), a, np.float32), np.full((20, 24, 3), b, np.float32)
    assert abs(R.structural_similarity(p, t) - want) <= 1e-12
    assert abs(R.ssim(p.transpose(2, 0, 1)[None], t.transpose(2, 0, 1)[None]) - want) <= 1e-12


def test_reflect_padding_is_torchs():
    """index -1 -> 1: the padded row of [0, 1, 2, 3] is [1, 0, 1, 2, 3, 2]; a one-hot window reads exactly that."""
    a = np.arange(4.0)[None].repeat(4, 0)
    assert (R._filter(a, [1.0, 0.0, 0.0], -1, True)[0] == [1, 0, 1, 2]).all()
    assert (R._filter(a, [0.0, 0.0, 1.0], -1, True)[0] == [1, 2, 3, 2]).all()


def test_mnrf_ssim_validates_arguments_without_gpu(L):
    null = None
    taps = (C.c_double * 11)(*([1.0 / 7] * 7 + [0.0] * 4))
    strides = (C.c_int64 * 4)(3, 192, 1, 64 * 64 * 3)
    fake = C.cast((C.c_float * 4)(), C.c_void_p)      # never dereferenced: every call below is refused before a launch

    def call(pred=fake, ps=strides, gt=fake, gs=strides, H=64, W=64, channels=3, frames=1, tp=taps, radius=3, partials=fake,
             out=fake):
        return L.mnrf_ssim(pred, ps, gt, gs, H, W, channels, frames, tp, radius, 0, 49.0 / 48.0, 1e-4, 9e-4, partials, out,
                           null, null)

    for missing in ("pred", "ps", "gt", "gs", "tp", "partials", "out"):
        assert call(**{missing: null}) < 0, missing
        assert b"mnrf_ssim: null pointer" in L.mnrf_last_error()
    assert call(radius=6) < 0 and b"radius" in L.mnrf_last_error()
    assert call(radius=-1) < 0
    assert call(H=6) < 0 and b"smaller than the window" in L.mnrf_last_error()       # H below the 7x7 window
    assert call(W=6) < 0 and b"smaller than the window" in L.mnrf_last_error()
    assert call(frames=0) < 0 and b"bad size" in L.mnrf_last_error()
    assert call(channels=0) < 0
    # the workspace size is plain arithmetic: one partial per 32x16 tile of the image, channel and frame (an upper bound on
    # the partials a launch writes: a cropped border leaves fewer output tiles)
    assert L.mnrf_ssim_blocks(800, 800, 1, 3) == 25 * 50 * 3
    assert L.mnrf_ssim_blocks(800, 800, 20, 3) == 20 * L.mnrf_ssim_blocks(800, 800, 1, 3)
    assert L.mnrf_ssim_blocks(37, 53, 1, 3) == 2 * 3 * 3


def test_python_entry_points_refuse_cpu_tensors_and_bad_windows(L):
    a = torch.zeros(16, 16, 3)
    with pytest.raises(RuntimeError, match="GPU only"):
        structural_similarity(a, a)
    with pytest.raises(RuntimeError, match="GPU only"):
        ssim(a.permute(2, 0, 1)[None], a.permute(2, 0, 1)[None])
    for w in (2, 8, 1, 13):
        with pytest.raises(ValueError):
            structural_similarity(a, a, win_size=w)
    with pytest.raises(RuntimeError, match="shape"):
        structural_similarity(a, torch.zeros(16, 17, 3))
