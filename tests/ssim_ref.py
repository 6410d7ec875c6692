"""numpy-only float64 restatement of the two structural-similarity definitions of the reference, the yardstick of
tests/test_metrics_cpu.py and tests/test_hip_metrics.py, and the seeded image pairs both use.

`structural_similarity`: scikit-image's `metrics.structural_similarity(p, t, channel_axis=-1, data_range=1)` as
tools/eval_metrics.py:25-27 calls it (uniform window, sample covariance, crop of the window radius).
`ssim_map` / `ssim`: metrics.ssim (metrics.py:18-23), kornia's 3x3 Gaussian window over reflect-padded images.
No scipy here (it may be missing where the GPU tests run); test_metrics_cpu.py pins `structural_similarity` to
`scipy.ndimage.uniform_filter`, the filter scikit-image itself calls, where scipy exists."""
import numpy as np


def _filter(a, taps, axis, reflect):
    """1-D correlation with `taps` along `axis`: "valid" part only, or the full length after a reflect pad (-1 -> 1)."""
    r = (len(taps) - 1) // 2
    if reflect:
        pad = [(0, 0)] * a.ndim
        pad[axis] = (r, r)
        a = np.pad(a, pad, mode="reflect")
    a = np.moveaxis(a, axis, -1)
    n = a.shape[-1] - 2 * r
    out = np.zeros(a.shape[:-1] + (n,))
    for k, w in enumerate(taps):
        out += w * a[..., k:k + n]
    return np.moveaxis(out, -1, axis)


def similarity_map(x, y, taps, reflect, cov_norm, c1, c2):
    """S over the last two axes of x and y (float64)."""
    x = np.asarray(x, np.float64)
    y = np.asarray(y, np.float64)

    def mean(a):
        return _filter(_filter(a, taps, -1, reflect), taps, -2, reflect)

    ux, uy, uxx, uyy, uxy = mean(x), mean(y), mean(x * x), mean(y * y), mean(x * y)
    vx = cov_norm * (uxx - ux * ux)
    vy = cov_norm * (uyy - uy * uy)
    vxy = cov_norm * (uxy - ux * uy)
    return ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))


def structural_similarity(p, t, win_size=7, data_range=1.0):
    """p, t: (H, W, C).  The mean over channels of the per-channel means of S over the cropped interior."""
    n = win_size * win_size
    S = similarity_map(np.moveaxis(p, -1, 0), np.moveaxis(t, -1, 0), [1.0 / win_size] * win_size, False, n / (n - 1.0),
                       (0.01 * data_range) ** 2, (0.03 * data_range) ** 2)
    return float(np.mean([S[c].mean() for c in range(S.shape[0])]))


def gaussian_taps3(sigma=1.5):
    g = np.exp(-np.array([-1.0, 0.0, 1.0]) ** 2 / (2.0 * sigma * sigma))
    return list(g / g.sum())


def ssim_map(p, t):
    """p, t: (B, 3, H, W) -> the (B, 3, H, W) map 1 - 2 * clamp((1 - S) / 2, 0, 1) in float64."""
    S = similarity_map(p, t, gaussian_taps3(), True, 1.0, 0.01 ** 2, 0.03 ** 2)
    return 1.0 - 2.0 * np.clip((1.0 - S) / 2.0, 0.0, 1.0)


def ssim(p, t):
    return float(ssim_map(p, t).mean())


# ---- seeded (H, W, 3) float32 pairs in [0, 1]
KINDS = ("smooth_noise", "near_white", "quantised", "hard_edge")


def pair(kind, H, W, seed=0):
    rng = np.random.default_rng([seed, H, W, KINDS.index(kind)])
    yy, xx = np.meshgrid(np.linspace(0.0, 1.0, H), np.linspace(0.0, 1.0, W), indexing="ij")
    phase = np.array([0.0, 0.7, 1.9])
    smooth = 0.5 + 0.35 * np.sin(6.0 * xx[..., None] + phase) * np.cos(4.0 * yy[..., None] - phase)
    if kind == "smooth_noise":
        a, b = smooth, smooth + 0.03 * rng.standard_normal((H, W, 3))
    elif kind == "near_white":      # a white background: variances next to nothing against C2
        a = 0.995 + 0.004 * rng.random((H, W, 3))
        b = a + 0.002 * rng.standard_normal((H, W, 3))
    elif kind == "quantised":       # 8-bit images, as read back from PNG files
        a = np.round(255.0 * smooth) / 255.0
        b = np.round(255.0 * np.clip(smooth + 0.02 * rng.standard_normal((H, W, 3)), 0.0, 1.0)) / 255.0
    elif kind == "hard_edge":
        a = np.where(xx[..., None] + 0.3 * yy[..., None] > 0.6, 0.9, 0.1) + 0.0 * phase
        b = np.where(xx[..., None] + 0.3 * yy[..., None] > 0.62, 0.85, 0.12) + 0.01 * rng.standard_normal((H, W, 3))
    else:
        raise KeyError(kind)
    return (np.clip(a, 0.0, 1.0).astype(np.float32), np.clip(b, 0.0, 1.0).astype(np.float32))
