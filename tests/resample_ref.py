"""Pillow's 8-bit resampler in numpy integers: the restatement csrc/mnrf_resample.hip is written from, fed with the tables of
`data.lanczos_taps` (or any other).  tests/test_resample_cpu.py holds it against Pillow's own output with tolerance zero."""
import numpy as np

PRECISION_BITS = 32 - 8 - 2


def one_pass(a, bounds, taps, axis):
    """a (F, H, W, C) uint8 resampled along `axis` (1: rows / y, 2: columns / x): int32 accumulation from 1 << 21, an arithmetic
    shift by 22, a clamp to 0..255."""
    a = np.moveaxis(a, axis, 1)
    out = np.empty((a.shape[0], len(bounds)) + a.shape[2:], np.uint8)
    for i, (lo, n) in enumerate(bounds):
        w = taps[i, :n].astype(np.int64).reshape((1, n) + (1,) * (a.ndim - 2))
        acc = (1 << (PRECISION_BITS - 1)) + (a[:, lo:lo + n].astype(np.int64) * w).sum(1)
        acc = ((acc + 2 ** 31) % 2 ** 32) - 2 ** 31            # an int32 accumulator
        out[:, i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 1, axis)


def premultiply(a):
    a = a.copy()
    t = a[..., :3].astype(np.int64) * a[..., 3:].astype(np.int64) + 128
    a[..., :3] = ((t >> 8) + t) >> 8
    return a


def unpremultiply(a):
    a = a.copy()
    alpha = a[..., 3:].astype(np.int64)
    q = np.minimum(255, 255 * a[..., :3].astype(np.int64) // np.maximum(alpha, 1))
    keep = (alpha == 0) | (alpha == 255)
    a[..., :3] = np.where(keep, a[..., :3], q)
    return a


def resample(a, wh, taps_of):
    """`Image.resize(wh, LANCZOS)` of every frame of a (F, H, W, C) uint8: the pass along x, then along y, a pass whose sizes
    agree skipped, a plain copy when both agree; RGBA premultiplied before and divided out after.  taps_of(in, out) ->
    (bounds, taps)."""
    a = np.asarray(a, np.uint8)
    w, h = wh
    if (a.shape[2], a.shape[1]) == (w, h):
        return a.copy()
    rgba = a.shape[3] == 4
    if rgba:
        a = premultiply(a)
    if a.shape[2] != w:
        a = one_pass(a, *taps_of(a.shape[2], w), axis=2)
    if a.shape[1] != h:
        a = one_pass(a, *taps_of(a.shape[1], h), axis=1)
    return unpremultiply(a) if rgba else a


def mask_nearest(m, wh):
    """The bank's int8 mask of native-depth samples (F, H, W) uint8 / uint16: data._resize_nearest's pick, then the thresholds."""
    from mirror_nerf_amd.data import _resize_nearest
    on = m >= 128 if m.dtype == np.uint8 else m > 0
    return np.stack([_resize_nearest(f, wh) for f in on]).astype(np.int8)


# ----------------------------------------------------------------------------- the cases of fixture g22_resample
# source (H, W) -> target (w, h).  Both passes, the pass along x alone (30x40 -> 20x30), the pass along y alone
# (29x37 -> 37x11), up- and down-scaling, a window wider than the source (5x7), one output row, and the plain copy.
SHAPES = (((29, 37), (11, 7)), ((48, 64), (16, 12)), ((30, 40), (20, 30)), ((17, 23), (31, 40)), ((144, 192), (48, 36)),
          ((5, 7), (3, 2)), ((64, 64), (63, 1)), ((29, 37), (37, 11)), ((6, 8), (8, 6)))
STACK_SHAPE = ((29, 37), (11, 7))      # the (F = 2) stack: a wrong frame stride shows here


def _noise(n, seed):
    """n bytes of an integer hash of (index, seed): the same on every numpy."""
    x = (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) + np.uint64(seed) * np.uint64(40503) + np.uint64(12345)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(2246822519)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(3266489917)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(16)
    return (x >> np.uint64(24)).astype(np.uint8)


def make_source(hw, channels, kind, seed=0):
    """(H, W, channels) uint8.  kind "noise": hashed bytes (alpha too, with a few 0 and 255); "ramp": smooth gradients, and an
    alpha of 0 in the left third, 255 in the middle, hashed on the right."""
    h, w = hw
    if kind == "noise":
        a = _noise(h * w * channels, seed).reshape(h, w, channels)
        if channels == 4:
            a[::3, ::2, 3] = 0
            a[1::3, 1::2, 3] = 255
        return a
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (7 * x + 3 * y) % 256], -1).astype(np.uint8)
    if channels == 4:
        alpha = _noise(h * w, seed + 1).reshape(h, w)
        alpha[:, :w // 3] = 0
        alpha[:, w // 3:2 * w // 3] = 255
        a = np.concatenate([a, alpha[..., None]], -1)
    return a


def cases():
    """(name, source (F, H, W, C), (w, h)) of every case of the fixture."""
    out = []
    for k, (hw, wh) in enumerate(SHAPES):
        for c in (3, 4):
            for kind in ("noise", "ramp"):
                out.append((f"{hw[0]}x{hw[1]}_to_{wh[0]}x{wh[1]}_c{c}_{kind}", make_source(hw, c, kind, seed=10 * k + c)[None], wh))
    hw, wh = STACK_SHAPE
    for c in (3, 4):
        out.append((f"stack2_c{c}", np.stack([make_source(hw, c, "noise", seed=100 + c), make_source(hw, c, "ramp", seed=200 + c)]), wh))
    return out


# ----------------------------------------------------------------------------- the cases of fixture g22_resample_edges
# The launch geometry of csrc/mnrf_resample.hip: TPB threads along the output x, rows on gridDim.y up to ROWS_MAX and strided
# beyond.  Every shape of cases() fits one x-block and one sweep of rows; these are the smallest that do not:
#   (3, 90) -> (300, 3)     the pass along x alone, upscaling: a second x-block, ragged (300 = 256 + 44)
#   (9, 300) -> (300, 4)    the pass along y alone at 300 columns: ox >= 256 in the y pass
#   (5, 700) -> (260, 3)    both passes, downscaling; a ragged second block in both, the buffer between them 260 wide
#   (7, 1100) -> (520, 5)   both passes, three x-blocks
# and a stack of EDGE_STACK_FRAMES frames of (24, 10) -> (7, 23): the pass along x runs over frames * 24 = 72000 rows and the
# pass along y over frames * 23 = 69000, both past ROWS_MAX, so the stride over rows runs in each.
TPB = 256
ROWS_MAX = 65535
EDGE_SHAPES = (((3, 90), (300, 3)), ((9, 300), (300, 4)), ((5, 700), (260, 3)), ((7, 1100), (520, 5)))
EDGE_STACK_SHAPE = ((24, 10), (7, 23))
EDGE_STACK_FRAMES = 3000
EDGE_STACK = f"stack{EDGE_STACK_FRAMES}_c4"


def past_one_x_block(dst_w):
    """A second x-block, and a last one that is not full."""
    return dst_w > TPB and dst_w % TPB != 0


def rows_strided(frames, src_h, dst_h):
    """Both passes sweep their rows more than once: the pass along x has the source's rows, the pass along y the target's."""
    return frames * src_h > ROWS_MAX and frames * dst_h > ROWS_MAX


def edge_cases():
    """(name, source (F, H, W, C), (w, h)) of every case of the fixture: RGB and RGBA noise, an RGBA ramp (alpha 0 / 255 / mixed in thirds,
    so the unpremultiply's branches also run past column 256), and the stack, hashed as a whole so that no two frames agree."""
    out = []
    for k, (hw, wh) in enumerate(EDGE_SHAPES):
        assert past_one_x_block(wh[0])
        for c, kind in ((3, "noise"), (4, "noise"), (4, "ramp")):
            out.append((f"{hw[0]}x{hw[1]}_to_{wh[0]}x{wh[1]}_c{c}_{kind}", make_source(hw, c, kind, seed=300 + 10 * k + c)[None], wh))
    (h, w), wh = EDGE_STACK_SHAPE
    assert rows_strided(EDGE_STACK_FRAMES, h, wh[1])
    out.append((EDGE_STACK, make_source((EDGE_STACK_FRAMES * h, w), 4, "noise", seed=400).reshape(EDGE_STACK_FRAMES, h, w, 4), wh))
    return out
