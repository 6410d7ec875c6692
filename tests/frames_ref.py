"""numpy float32 restatement of the output stage of the reference's eval.py (eval.py:743-978 with utils/visualization.py:10-23,
208-221), the yardstick of tests/test_frames_cpu.py and tests/test_hip_frames.py, written from reading it: every image is the
reference's own chain of numpy operations on float32 arrays, with `T[k]` in place of `cv2.applyColorMap(k, COLORMAP_JET)` (cv2
is not needed: the table is an argument) and float32 division by 255 in place of torchvision's ToTensor.

Maps are flat: (n,) or (n, 3) float32 arrays, images (n, 3) uint8 -- the reference's (H, W, 3) without the reshape.

`u8` is `astype(np.uint8)`.  Inside [0, 256) that is truncation and nothing else is done; outside it numpy leaves the result to
the platform (and warns), so the restatement pins those: NaN and negative values give 0, values from 256 up give 255 -- the
rule of csrc/mnrf_frames.hip.  They arise only from non-finite maps (an overflowing `ma - mi`, a NaN colour)."""
import numpy as np

F32 = np.float32
STEMS = ("rgb", "mirror_mask", "depth", "depth_reflect", "surface_normal", "surface_normal_grad", "x_surface")


def u8(v):
    v = np.asarray(v, F32)
    inside = (v >= 0) & (v < 256)           # False for a NaN
    safe = np.where(inside, v, F32(0)).astype(np.uint8)
    return np.where(inside, safe, np.where(v >= 256, 255, 0).astype(np.uint8)).astype(np.uint8)


def rgb_image(rgb):
    """eval.py:763, 797"""
    img = np.clip(np.asarray(rgb, F32), 0, 1)
    return u8(img * 255)


def mask_float(mask):
    """eval.py:807-816: the clipped mask in three channels (kept as `mirror_masks_float`)"""
    return np.clip(np.repeat(np.asarray(mask, F32)[:, None], 3, axis=1), 0, 1)


def mask_image(mask):
    """eval.py:818"""
    return u8(mask_float(mask) * 255)


def normal_image(v):
    """eval.py:853-880"""
    return u8(np.clip((np.asarray(v, F32) + 1) / 2, 0, 1) * 255)


def x_surface_extrema(xs):
    xs = np.asarray(xs, F32)
    return np.min(xs), np.max(xs)           # a NaN propagates, as in torch.min / torch.max


def x_surface_image(xs):
    """visualization.py:208-221, eval.py:882-891"""
    xs = np.asarray(xs, F32)
    mn, mx = x_surface_extrema(xs)
    if mn == mx:
        out = np.ones_like(xs)
    else:
        with np.errstate(all="ignore"):
            out = (xs - mn) / (mx - mn)
    return u8(np.clip(out, 0, 1) * 255)


def depth_extrema(depth):
    """mi, ma of visualize_depth without vmin / vmax"""
    x = np.nan_to_num(np.asarray(depth, F32))
    return np.min(x), np.max(x)


def depth_canvas(depth, table, vmin=None, vmax=None):
    """visualize_depth (visualization.py:10-23): the float canvas (n, 3) in [0, 1] ToTensor hands back"""
    x = np.nan_to_num(np.asarray(depth, F32))
    mi = np.min(x) if vmin is None else F32(vmin)
    ma = np.max(x) if vmax is None else F32(vmax)
    with np.errstate(all="ignore"):
        x = np.clip(x, mi, ma)
        x = (x - mi) / max(ma - mi, 1e-8)       # Python's max: the float32 difference, or the Python float 1e-8
        assert x.dtype == F32
        k = u8(255 * x)
    return np.asarray(table, np.uint8)[k].astype(F32) / F32(255)


def depth_image(depth, table, vmin=None, vmax=None):
    """eval.py:787-789, 945-951"""
    return u8(depth_canvas(depth, table, vmin, vmax) * 255)


def depth_reflect_image(depth_reflect, mask, table, vmin=None, vmax=None):
    """eval.py:842-847, 962-971"""
    canvas = depth_canvas(depth_reflect, table, vmin, vmax)
    with np.errstate(all="ignore"):
        canvas = canvas * mask_float(mask)
        return u8(canvas * 255)


class RunningExtrema:
    """eval.py:776-785, 829-840: the split-wide extremes of the raw maps.  The one difference from the reference:
    they start at (+inf, -inf) and a frame's np.min / np.max only ever replaces them through `<` / `>`, so a frame that holds a
    NaN (np.min and np.max are NaN) is skipped also when it is the first; the reference stores the first frame's unseen."""

    def __init__(self):
        self.min, self.max = F32(np.inf), F32(-np.inf)

    def update(self, depth):
        depth = np.asarray(depth, F32)
        lo, hi = np.min(depth), np.max(depth)
        if hi > self.max:
            self.max = hi
        if lo < self.min:
            self.min = lo
        return self


def frame_images(results, table, typ="fine"):
    """The images save_img_and_cal_psnr writes for one frame, keyed by file stem, from a dict of numpy maps (eval.py:762-894):
    nothing without rgb; depth_reflect only under a predicted mask."""
    out = {}
    if f"rgb_{typ}" not in results:
        return out
    if f"depth_{typ}" in results:
        out[f"depth_{typ}"] = depth_image(results[f"depth_{typ}"], table)
    out[f"rgb_{typ}"] = rgb_image(results[f"rgb_{typ}"])
    if f"mirror_mask_{typ}" in results:
        out[f"mirror_mask_{typ}"] = mask_image(results[f"mirror_mask_{typ}"])
        if f"depth_{typ}_reflect" in results:
            out[f"depth_reflect_{typ}"] = depth_reflect_image(results[f"depth_{typ}_reflect"], results[f"mirror_mask_{typ}"], table)
    for stem in ("surface_normal_grad", "surface_normal"):
        if f"{stem}_{typ}" in results:
            out[f"{stem}_{typ}"] = normal_image(results[f"{stem}_{typ}"])
    if f"x_surface_{typ}" in results:
        out[f"x_surface_{typ}"] = x_surface_image(results[f"x_surface_{typ}"])
    return out


def seeded_maps(n, seed, constant_depth=False, constant_xs=False, nonfinite="all"):
    """Seeded float32 maps of n pixels with the values an implementation can get wrong: the byte edges k/255 and their
    neighbours one ulp either side, values below 0 and above 1, a mask outside [0, 1], and NaN / +inf / -inf in the depths
    (`nonfinite`: "all", "nan", "inf" -- +inf alone -- or "none")."""
    rng = np.random.default_rng(seed)
    edges = np.array([k / 255 for k in (0, 1, 2, 3, 127, 128, 254, 255)], F32)
    edges = np.concatenate([edges, np.nextafter(edges, F32(2)), np.nextafter(edges, F32(-2)), F32([-0.25, 1.5, -3.0, 7.0])])

    def unit(shape):
        v = rng.uniform(-0.2, 1.2, size=shape).astype(F32)
        flat = v.reshape(-1)
        idx = rng.permutation(flat.size)[:min(flat.size, edges.size)]
        flat[idx] = edges[:idx.size]
        return v

    d = {"rgb": unit((n, 3)), "mirror_mask": unit((n,)),
         "surface_normal": (unit((n, 3)) * 2 - 1).astype(F32), "surface_normal_grad": (unit((n, 3)) * 2 - 1).astype(F32),
         "x_surface": rng.normal(0, 2, size=(n, 3)).astype(F32)}
    for name, lo, hi in (("depth", 2.0, 6.0), ("depth_reflect", 0.0, 9.0)):
        v = rng.uniform(lo, hi, size=n).astype(F32)
        # the byte edges of the normalised depth, as far as the map's own extremes allow
        v[rng.permutation(n)[:min(n, edges.size)]] = (F32(lo) + edges[:min(n, edges.size)] * F32(hi - lo)).astype(F32)
        bad = {"all": [np.nan, np.inf, -np.inf], "nan": [np.nan], "inf": [np.inf], "none": []}[nonfinite]
        if n > 8:
            for b in bad:
                v[rng.permutation(n)[:2]] = b
        if constant_depth:
            v[:] = F32(3.25)
        d[name] = v
    if constant_xs:
        d["x_surface"][:] = F32(-1.5)
    return d
