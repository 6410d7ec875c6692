"""metrics.py of the reference (5-15) on the GPU: `mse` and `psnr` of a rendered frame against the ground truth without
moving either to the host (eval.py:804 computes PSNR on CPU copies of full frames).
`structural_similarity` (scikit-image's, what tools/eval_metrics.py reports) and `ssim` (metrics.py:18-23, kornia's) run on
the device too: one windowed-moments kernel (csrc/mnrf_metrics.hip) evaluates both in float64 from the float32 frames, reads
`(H, W, 3)` render outputs and `(B, 3, H, W)` tensors in place, takes the frames of a test split in one launch and never
synchronises with the host.  `frame_metrics` gives the PSNR and SSIM of a frame or of a stack of frames."""
import ctypes
import math

import torch

from . import _lib


def _launch_mse(a, b, m, per, part, out):
    L = _lib.lib()
    _lib.check(L.mnrf_mse_psnr(_lib.ptr(a), _lib.ptr(b), None if m is None else m.data_ptr(), a.numel(), per,
                               _lib.ptr(part), _lib.ptr(out), _lib.stream()), "mnrf_mse_psnr")


def _mse_workspace(device):
    return torch.empty(2 * _lib.lib().mnrf_mse_blocks(), dtype=torch.float32, device=device)


def _reduce(image_pred, image_gt, valid_mask):
    a = image_pred.detach().float().contiguous()
    b = image_gt.detach().float().contiguous()
    if a.shape != b.shape:
        raise RuntimeError(f"shape mismatch {tuple(a.shape)} vs {tuple(b.shape)}")
    per, m = 1, None
    if valid_mask is not None:
        m = valid_mask.to(torch.uint8).contiguous()
        if m.shape == a.shape:
            per = 1
        elif m.shape == a.shape[:-1]:
            per = a.shape[-1]          # value[valid_mask] with a per-pixel mask keeps whole pixels
        else:
            raise RuntimeError("valid_mask must have the image's shape or its shape without the channel axis")
    out = torch.empty(3, dtype=torch.float32, device=a.device)
    _launch_mse(a, b, m, per, _mse_workspace(a.device), out)
    return out


def mse(image_pred, image_gt, valid_mask=None, reduction="mean"):
    if reduction != "mean":
        raise NotImplementedError("only reduction='mean' (what eval.py uses) runs on the device")
    return _reduce(image_pred, image_gt, valid_mask)[0]


def psnr(image_pred, image_gt, valid_mask=None, reduction="mean"):
    if reduction != "mean":
        raise NotImplementedError("only reduction='mean' (what eval.py uses) runs on the device")
    return _reduce(image_pred, image_gt, valid_mask)[1]


def _windowed(pred, gt, taps, reflect, cov_norm, c1, c2, want_map):
    """pred, gt: (F, C, H, W) float32 VIEWS with any strides.  Returns (the (F,) means, the (F, C, rows, columns) map or None)."""
    L = _lib.lib()
    if pred.shape != gt.shape:
        raise RuntimeError(f"shape mismatch {tuple(pred.shape)} vs {tuple(gt.shape)}")
    dev = pred.device
    for t in (pred, gt):
        if not t.is_cuda or t.device != dev:
            raise RuntimeError("mirror_nerf_amd runs on the GPU only: both images must live on one device (got %s)" % t.device)
    if dev.index != _lib._cur_device():
        raise RuntimeError(f"tensor lives on cuda:{dev.index} but the current device is cuda:{_lib._cur_device()}; "
                           "call torch.cuda.set_device / use `with torch.cuda.device(t.device)`")
    F, C, H, W = pred.shape
    r = (len(taps) - 1) // 2
    strides = [(ctypes.c_int64 * 4)(t.stride(3), t.stride(2), t.stride(1), t.stride(0)) for t in (pred, gt)]
    n_part = max(1, L.mnrf_ssim_blocks(H, W, F, C))
    part = torch.empty(n_part, dtype=torch.float64, device=dev)
    out = torch.empty(max(F, 1), dtype=torch.float32, device=dev)
    rows, cols = (H, W) if reflect else (H - 2 * r, W - 2 * r)
    smap = torch.empty((F, C, max(rows, 0), max(cols, 0)), dtype=torch.float32, device=dev) if want_map else None
    _lib.check(L.mnrf_ssim(pred.data_ptr(), strides[0], gt.data_ptr(), strides[1], H, W, C, F, (ctypes.c_double * len(taps))(*taps),
                           r, int(reflect), cov_norm, c1, c2, part.data_ptr(), _lib.ptr(out),
                           None if smap is None else _lib.ptr(smap), _lib.stream()), "mnrf_ssim")
    return out, smap


def _frames_last(image_pred, image_gt):
    """(H, W, C) or (F, H, W, C) -> (F, C, H, W) views of the same memory, and whether a frame axis was given."""
    a, b = image_pred.detach().float(), image_gt.detach().float()
    if a.dim() not in (3, 4) or a.shape != b.shape:
        raise RuntimeError(f"expected two (H, W, C) or (F, H, W, C) images of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    stacked = a.dim() == 4
    if not stacked:
        a, b = a[None], b[None]
    return a.permute(0, 3, 1, 2), b.permute(0, 3, 1, 2), stacked


def structural_similarity(pred, gt, win_size=7, data_range=1.0):
    """scikit-image's `metrics.structural_similarity(p, t, channel_axis=-1, data_range=1)` the way tools/eval_metrics.py:25-27
    calls it: uniform win_size x win_size window, sample covariance (cov_norm = NP / (NP - 1), NP = win_size^2), K1 = 0.01,
    K2 = 0.03; per channel the mean of S over the interior left after cropping (win_size - 1) // 2 pixels on each side, then the
    mean over the channels (the border mode of the filter never shows: the crop equals the window radius).  Evaluated in
    float64 from the float32 frames.  pred, gt: (H, W, C) or (F, H, W, C) device tensors with any strides (read in place).
    Returns a 0-d or (F,) float32 device tensor; no host synchronisation."""
    if win_size % 2 != 1 or not 3 <= win_size <= 11:
        raise ValueError("win_size must be odd and in 3..11")
    a, b, stacked = _frames_last(pred, gt)
    n = win_size * win_size
    out, _ = _windowed(a, b, [1.0 / win_size] * win_size, False, n / (n - 1.0), (0.01 * data_range) ** 2, (0.03 * data_range) ** 2,
                       False)
    return out if stacked else out[0]


def ssim(image_pred, image_gt, reduction="mean"):
    """metrics.ssim of the reference (metrics.py:18-23) = 1 - 2 * kornia.losses.ssim(pred, gt, 3, reduction) on (B, 3, H, W):
    3x3 Gaussian window with sigma 1.5 (taps exp(-x^2 / 2 sigma^2) at x in {-1, 0, 1}, normalised), no covariance correction,
    C1 = 1e-4, C2 = 9e-4, and 1 - 2 * clamp((1 - S) / 2, 0, 1), which is S because |S| <= 1.  The reference does not pin kornia
    and its border handling changed between releases; this is a DECISION for the definition with `filter2D`'s default
    "reflect" padding (index -1 -> 1), so that S exists at every pixel.  Evaluated in float64 from the float32 images, read in
    place.  "mean": over every element, a 0-d float32 device tensor; "none": the (B, 3, H, W) map."""
    if reduction not in ("mean", "none"):
        raise NotImplementedError("reduction must be 'mean' or 'none'")
    a, b = image_pred.detach().float(), image_gt.detach().float()
    if a.dim() != 4 or a.shape != b.shape:
        raise RuntimeError(f"expected two (B, C, H, W) images of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    g = math.exp(-1.0 / (2.0 * 1.5 * 1.5))
    taps = [g / (1.0 + 2.0 * g), 1.0 / (1.0 + 2.0 * g), g / (1.0 + 2.0 * g)]
    out, smap = _windowed(a, b, taps, True, 1.0, 0.01 ** 2, 0.03 ** 2, reduction == "none")
    if reduction == "none":
        return smap
    return out[0] if out.numel() == 1 else out.mean()      # frames of one shape weigh the same


def frame_metrics(pred, gt):
    """(psnr, ssim) of a rendered frame (H, W, C) against its ground truth, or (F,) each for a stack (F, H, W, C): what
    tools/eval_metrics.py prints per frame, `psnr` as metrics.psnr gives it and `ssim` = structural_similarity.  The SSIM of
    the whole stack is two launches (tiles, finish) into one (F,) output.  The PSNR is metrics.psnr's own reduction once per
    frame -- F times its launches, over one workspace and into one (F, 3) output -- so that every frame's PSNR has the
    bits metrics.psnr gives for it; that reduction reads contiguous memory, so a strided input is copied once for it (what the
    renderer returns is contiguous and is not).  Nothing goes to the host."""
    s = structural_similarity(pred, gt)
    a, b, stacked = _frames_last(pred, gt)
    a, b = a.permute(0, 2, 3, 1).contiguous(), b.permute(0, 2, 3, 1).contiguous()
    out = torch.empty((a.shape[0], 3), dtype=torch.float32, device=a.device)
    part = _mse_workspace(a.device)
    for f in range(a.shape[0]):
        _launch_mse(a[f], b[f], None, 1, part, out[f])
    return (out[:, 1], s) if stacked else (out[0, 1], s)
