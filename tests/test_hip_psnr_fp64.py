"""metrics.mse / metrics.psnr / frame_metrics (mse_partial_kernel and mse_finish_kernel of csrc/mnrf_loss.hip) against the float64
mean of squared differences, past one wave, one block and one pass of the grid-stride loop.

Bar: derived per case from the kernels' float32 summation in tests/loss_ref.py (mse_bar, psnr_bar), not measured: at most
(3 + (q - 1) + 9 + (blocks - 1) + 1) * 2^-24 relative on the MSE, 10 / ln 10 of that plus 2 ulp of the value on the PSNR.
tests/test_loss_ref_cpu.py shows a float32 numpy emulation of the kernels' order inside the same bar on the same cases; its MSE,
count and per-block partials are the kernel's bit for bit, which is asserted here as well.

Every case states the edge it is there for (loss_ref.mse_geometry, the first selected element of a mask), so that another tile
size makes it fail instead of testing nothing.

Largest errors seen on an MI355X, as fractions of the bar: MSE 0.151, PSNR 0.299, count 0.001 (test_mse_psnr_against_float64)."""
import ctypes

import numpy as np
import pytest
import torch

from tests import loss_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -12345.0
PAD = 64


def _launch(c):
    """One mnrf_mse_psnr through the C entry point, `out` and the workspace inside larger buffers of sentinels:
    (out (3,) float32, partials (blocks, 2) float32), after asserting that nothing else was written."""
    from mirror_nerf_amd import _lib
    L = _lib.lib()
    a, b = torch.from_numpy(c["a"]).to(DEV), torch.from_numpy(c["b"]).to(DEV)
    m = None if c["mask"] is None else torch.from_numpy(c["mask"]).to(DEV)
    blocks, _ = R.mse_geometry(c["a"].size)
    n_part = 2 * L.mnrf_mse_blocks()
    assert n_part == 2 * R.MSE_MAX_BLOCKS
    out = torch.full((PAD + 3 + PAD,), SENTINEL, dtype=torch.float32, device=DEV)
    part = torch.full((PAD + n_part + PAD,), SENTINEL, dtype=torch.float32, device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(L.mnrf_mse_psnr(_lib.ptr(a), _lib.ptr(b), None if m is None else ctypes.c_void_p(m.data_ptr()), a.numel(), c["per"],
                                   ctypes.c_void_p(part.data_ptr() + 4 * PAD), ctypes.c_void_p(out.data_ptr() + 4 * PAD), _lib.stream()),
                   "mnrf_mse_psnr")
    out, part = out.cpu().numpy(), part.cpu().numpy()
    # exactly 3 and 2 x blocks floats are written
    assert (out[:PAD] == SENTINEL).all() and (out[PAD + 3:] == SENTINEL).all()
    assert (part[:PAD] == SENTINEL).all() and (part[PAD + 2 * blocks:] == SENTINEL).all()
    assert not (part[PAD:PAD + 2 * blocks] == SENTINEL).any()
    return out[PAD:PAD + 3].copy(), part[PAD:PAD + 2 * blocks].reshape(blocks, 2).copy()


def _metrics(c, shape=None, mask_shape=None):
    """metrics.mse and metrics.psnr on the case, the images viewed as `shape`."""
    from mirror_nerf_amd import metrics
    a, b = torch.from_numpy(c["a"]).to(DEV), torch.from_numpy(c["b"]).to(DEV)
    m = None if c["mask"] is None else torch.from_numpy(c["mask"]).to(DEV).bool()
    if shape is not None:
        a, b = a.view(shape), b.view(shape)
        m = None if m is None else m.view(mask_shape)
    return np.array([float(metrics.mse(a, b, m)), float(metrics.psnr(a, b, m))], dtype=np.float32)


@pytest.mark.parametrize("name", list(R.PSNR_CASES))
def test_mse_psnr_against_float64(name):
    """Largest errors on an MI355X over the cases, as fractions of the derived bar: MSE 0.151 (size_255), PSNR 0.299 (size_257),
    count 0.001 (2^24 + 257, the only case with a count error at all); the MSE, the count and every per-block partial equal
    the float32 emulation bit for bit."""
    c = R.psnr_case(name)
    n = c["a"].size
    blocks, q = R.mse_geometry(n)
    out, part = _launch(c)
    fm, fp, fc = R.psnr_errors(c, out)
    print(f"{name}: n = {n}, {blocks} blocks x {q} terms a thread: mse {float(out[0]):.6e} (fp64 {c['ref'][0]:.6e}), psnr "
          f"{float(out[1]):.5f} dB, errors as fractions of the bar: mse {fm:.3f}, psnr {fp:.3f}, count {fc:.3f}")
    assert fm <= 1 and fp <= 1 and fc <= 1
    if n < 2 ** 24:
        assert float(out[2]) == c["ref"][2]
    # the emulation of the kernels' order predicts the bits of everything but the logarithm
    epart, eout = R.mse_emulate(c["a"], c["b"], c["sel"])
    assert part.tobytes() == epart.tobytes()
    assert np.array_equal(out[[0, 2]], eout[[0, 2]], equal_nan=True)      # (0 / 0 has the other sign bit on the host)
    # the reach of the case
    if name.startswith("size_"):
        edge = {1: (1, 1), 63: (1, 1), 64: (1, 1), 65: (1, 1), 255: (1, 1), 256: (1, 1), 257: (2, 1), R.MSE_SWEEP - 1: (1024, 1),
                R.MSE_SWEEP: (1024, 1), R.MSE_SWEEP + 1: (1024, 2), 3 * R.MSE_SWEEP + 5: (1024, 4), 2 ** 24 + 257: (1024, 65)}[n]
        assert (blocks, q) == edge
        if n == 2 ** 24 + 257:
            assert float(np.float32(n)) != n and c["ref"][2] == n      # the count is no float32: held to the bar, not to equality
    if name.startswith("mask_"):
        assert q == 4 and c["mask"].size * c["per"] == n
    if name == "mask_late_passes":
        picked = np.nonzero(c["sel"])[0]
        assert picked[0] >= R.MSE_SWEEP and picked[-1] < 3 * R.MSE_SWEEP and len(picked) > 100000
    if name == "mask_last_only":
        assert c["ref"][2] == 1 and c["sel"][-1] and n - 1 >= 3 * R.MSE_SWEEP and (part[:, 1] != 0).sum() == 1
    if name == "mask_none_selected":
        assert np.isnan(out[0]) and np.isnan(out[1]) and out[2] == 0.0
    if name == "mask_all_true":      # the bits of the unmasked call
        plain, _ = _launch(dict(c, mask=None, per=1))
        assert plain.tobytes() == out.tobytes()
    if name == "identical":
        assert out[0] == 0.0 and out[1] == np.inf
    if name == "one_element_2^-20":
        assert 0.0 < float(out[0]) < 1e-15 and np.isfinite(out[1]) and float(out[1]) > 150.0      # tiny, not flushed
    if name == "scale_255":
        assert c["ref"][0] > 100.0 and c["ref"][1] < -20.0
    # metrics.mse / metrics.psnr give those very numbers
    if name in ("size_1", "size_257", "size_262145", "mask_element", "identical", "scale_255"):
        assert _metrics(c).tobytes() == out[:2].tobytes()
    if name in ("mask_pixel3", "mask_none_selected"):       # a per-pixel mask over 3 channels, as eval.py passes it
        assert _metrics(c, (n // 3, 3), (n // 3,)).tobytes() == out[:2].tobytes()
    if name == "mask_pixel5":
        assert _metrics(c, (n // 10, 2, 5), (n // 10, 2)).tobytes() == out[:2].tobytes()


def test_frame_metrics_psnr_per_frame():
    """A stack of 5 frames of 37 x 53: every frame's PSNR has the bits of metrics.psnr on that frame and lies inside the
    derived bar against float64 (n = 5883 a frame: 23 blocks, the last with 251 elements).  Measured on an MI355X: the worst
    frame is 0.266 of the bar off."""
    from mirror_nerf_amd import metrics
    rs = np.random.RandomState(3)
    gt = rs.uniform(0, 1, (5, 37, 53, 3)).astype(np.float32)
    pred = np.clip(gt + rs.normal(0, 1, (5, 1, 1, 1)) * 0.02 + rs.normal(0, 0.05, gt.shape), 0, 1).astype(np.float32)
    n = 37 * 53 * 3
    assert R.mse_geometry(n) == (23, 1) and n % 256 == 251
    p, s = metrics.frame_metrics(torch.from_numpy(pred).to(DEV), torch.from_numpy(gt).to(DEV))
    assert p.shape == (5,) and s.shape == (5,) and p.dtype == torch.float32
    p = p.cpu().numpy()
    worst = 0.0
    for f in range(5):
        one = metrics.psnr(torch.from_numpy(pred[f]).to(DEV), torch.from_numpy(gt[f]).to(DEV))
        assert np.float32(float(one)).tobytes() == p[f].tobytes()
        single, _ = metrics.frame_metrics(torch.from_numpy(pred[f]).to(DEV), torch.from_numpy(gt[f]).to(DEV))
        assert np.float32(float(single)).tobytes() == p[f].tobytes()
        _, want, _ = R.mse_fp64(pred[f], gt[f], np.ones(n, bool))
        worst = max(worst, abs(float(p[f]) - want) / R.psnr_bar(n, want))
    print(f"frame_metrics: PSNR {p.tolist()} dB, worst error {worst:.3f} of the bar")
    assert worst <= 1 and len(set(p.tolist())) == 5
