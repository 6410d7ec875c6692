"""The output stage of the reference's eval.py on the GPU (eval.py:743-978, utils/visualization.py:10-23, 208-221): the 8-bit
images a test frame is saved as -- colour, mirror mask, the two normal maps, x_surface, the depth and reflected-depth colour
maps -- computed from the float32 maps `batched_inference(..., to_cpu=False, maps_only=True)` leaves on the device, in two
launches per frame (csrc/mnrf_frames.hip) and without a host read.  What then crosses to the host is 3 bytes per pixel and
image instead of the float maps (~100 B per ray), and nobody restates the reference's numpy expressions: every byte is what
numpy gives for them.

    extrema = SplitExtrema(device)                       # the running extremes of the split, resident
    images = finish_frame(results, "fine", split_extrema=extrema)        # {"rgb_fine": (n, 3) uint8, "depth_fine": ...}
    ...                                                  # after the last frame: save_depth_unified_normalization
    unified = colormap_depth(depth_stack, extrema.depth)

`val_panel(img_wh, batch, results)` is the training loop's counterpart (utils/visualization.py:26-184, add_text=False): the
(N_pics, 3, H, W) float32 panel the reference logs as val/GT_pred_depth, with the reference's tile labels, in two launches.

The colour table is an argument: `jet_table()` restates the classic piecewise-linear jet in the channel order cv2 emits; it
is not pinned against cv2.COLORMAP_JET (neither cv2 nor its table is available to this project)."""
import ctypes

import numpy as np
import torch

from . import _lib

STEMS = ("rgb", "mirror_mask", "depth", "depth_reflect", "surface_normal", "surface_normal_grad", "x_surface")


_Maps, _Images = _lib.STRUCTS["MnrfFrameMaps"], _lib.STRUCTS["MnrfFrameImages"]      # one field per stem


def jet_table():
    """(256, 3) uint8 numpy array: entry k is the colour of depth index k, t = k / 255, as clamp(1.5 - |4 t - c|, 0, 1) with
    c = 3, 2, 1 for red, green, blue, rounded to bytes and stored blue first -- cv2.applyColorMap returns BGR and the reference
    hands that array to PIL unchanged, so its depth PNGs have red and blue swapped; kept.  A restatement, not pinned against
    cv2's own table."""
    t = np.arange(256, dtype=np.float64) / 255.0
    bgr = [np.clip(1.5 - np.abs(4.0 * t - c), 0.0, 1.0) for c in (1.0, 2.0, 3.0)]
    return np.rint(np.stack(bgr, axis=1) * 255.0).astype(np.uint8)


_TABLES = {}


def _table(table, device):
    """The colour table on `device` as a contiguous (256, 3) uint8 tensor; the default is uploaded once per device."""
    if table is None:
        key = (device.type, device.index)
        if key not in _TABLES:
            _TABLES[key] = torch.from_numpy(jet_table()).to(device)
        return _TABLES[key]
    if isinstance(table, np.ndarray):
        table = torch.from_numpy(np.ascontiguousarray(table))
    if table.dtype != torch.uint8 or tuple(table.shape) != (256, 3):
        raise ValueError(f"the colour table must be (256, 3) uint8, got {table.dtype} {tuple(table.shape)}")
    return table.to(device).contiguous()


def _map(t, what, n=None, tail=()):
    """A float32 map as the kernels read it: on the current GPU, contiguous, (n,) + tail.  No copy of a map that already is."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"mirror_nerf_amd runs on the GPU only: {what} must be a device tensor "
                           f"(got {getattr(t, 'device', type(t).__name__)})")
    if t.dtype != torch.float32:
        raise ValueError(f"{what} must be float32, got {t.dtype}")
    if n is not None and tuple(t.shape) != (n,) + tuple(tail):
        raise ValueError(f"{what} must have shape {(n,) + tuple(tail)}, got {tuple(t.shape)}")
    t = t.detach().contiguous()
    _lib.ptr(t)         # the current-device check
    return t


def _stats(device, frames=1):
    """Stats blocks of the extrema launch; the reduction's state in them starts at zero and every launch leaves it zero."""
    return torch.zeros((frames, _lib.lib().mnrf_frame_stats_floats()), dtype=torch.float32, device=device)


class SplitExtrema:
    """The running extremes of a split, resident on the device (eval.py's all_depths_min / _max and all_depths_reflect_min /
    _max): `finish_frame(..., split_extrema=self)` folds every frame's raw depth and reflected-depth extremes into them on
    the device.  A frame that holds a NaN changes nothing, an infinity counts.  `depth` and `depth_reflect` are
    (2,) device views (min, max) for `colormap_depth`; `values()` is the only host read."""

    def __init__(self, device="cuda"):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"mirror_nerf_amd runs on the GPU only (SplitExtrema on {device})")
        self.block = torch.empty(_lib.lib().mnrf_split_extrema_floats(), dtype=torch.float32, device=device)
        self.reset()

    def reset(self):
        self.block[0::2].fill_(float("inf"))
        self.block[1::2].fill_(float("-inf"))
        return self

    @property
    def depth(self):
        return self.block[0:2]

    @property
    def depth_reflect(self):
        return self.block[2:4]

    def values(self):
        """dict(depth_min, depth_max, depth_reflect_min, depth_reflect_max) as Python floats (synchronises)."""
        v = self.block.tolist()
        return dict(depth_min=v[0], depth_max=v[1], depth_reflect_min=v[2], depth_reflect_max=v[3])


def finish_frame(results, typ="fine", table=None, split_extrema=None, want=None):
    """The images eval.py:762-894 saves for one frame, as a dict of (n, 3) uint8 device tensors keyed by the reference's file
    stems: rgb_{typ}, mirror_mask_{typ}, depth_{typ}, depth_reflect_{typ}, surface_normal_{typ}, surface_normal_grad_{typ},
    x_surface_{typ} -- those whose maps are in `results` (the dict batched_inference returns with to_cpu=False), under the
    reference's conditions: nothing without rgb_{typ}; depth_reflect (from depth_{typ}_reflect) only with a predicted mirror
    mask.  The maps are read in place and left unchanged.
    table: (256, 3) uint8 colours of the depth indices (default jet_table()).  split_extrema: a SplitExtrema the frame's raw
    depth extremes are folded into.  want: an iterable of stems ("rgb", "depth", ...) to restrict the images to.
    Two launches, no host synchronisation."""
    L = _lib.lib()
    if f"rgb_{typ}" not in results:
        return {}
    rgb = _map(results[f"rgb_{typ}"], f"rgb_{typ}")
    if rgb.dim() != 2 or rgb.shape[1] != 3:
        raise ValueError(f"rgb_{typ} must be (n, 3), got {tuple(rgb.shape)}")
    n, dev = rgb.shape[0], rgb.device
    keys = {"rgb": f"rgb_{typ}", "mirror_mask": f"mirror_mask_{typ}", "depth": f"depth_{typ}",
            "depth_reflect": f"depth_{typ}_reflect", "surface_normal": f"surface_normal_{typ}",
            "surface_normal_grad": f"surface_normal_grad_{typ}", "x_surface": f"x_surface_{typ}"}
    if want is not None:
        want = set(want)
        if not want <= set(STEMS):
            raise ValueError(f"want: unknown image(s) {sorted(want - set(STEMS))}; known: {STEMS}")
    maps = {"rgb": rgb}
    for stem, key in keys.items():
        if stem != "rgb" and key in results:
            maps[stem] = _map(results[key], key, n, (3,) if stem in ("surface_normal", "surface_normal_grad", "x_surface") else ())
    emit = [s for s in STEMS if s in maps and (want is None or s in want)]
    if "mirror_mask" not in maps and "depth_reflect" in emit:
        emit.remove("depth_reflect")                   # eval.py:806, 825: only under a predicted mask
    if split_extrema is not None and split_extrema.block.device != dev:
        raise RuntimeError(f"split_extrema lives on {split_extrema.block.device}, the frame on {dev}")
    tab = _table(table, dev) if ("depth" in emit or "depth_reflect" in emit) else None
    stats = _stats(dev)
    images = {s: torch.empty((n, 3), dtype=torch.uint8, device=dev) for s in emit}
    m, im = _Maps(), _Images()
    for s in emit:
        setattr(m, s, maps[s].data_ptr())
        setattr(im, s, images[s].data_ptr())
    if "depth_reflect" in emit:
        m.mirror_mask = maps["mirror_mask"].data_ptr()
    fold = split_extrema is not None
    # the running extremes take the frame's depths whether or not their images are asked for (eval.py:776-785, 829-840)
    d = maps.get("depth") if ("depth" in emit or fold) else None
    dr = maps.get("depth_reflect") if ("mirror_mask" in maps and ("depth_reflect" in emit or fold)) else None
    xs = maps.get("x_surface") if "x_surface" in emit else None
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731
    _lib.check(L.mnrf_frame_extrema(p(d), p(dr), p(xs), n, stats.data_ptr(), split_extrema.block.data_ptr() if fold else None,
                                    _lib.stream()), "mnrf_frame_extrema")
    _lib.check(L.mnrf_frame_finish(ctypes.byref(m), ctypes.byref(im), n, stats.data_ptr(), p(tab), _lib.stream()),
               "mnrf_frame_finish")
    return {(f"depth_reflect_{typ}" if s == "depth_reflect" else f"{s}_{typ}"): images[s] for s in emit}


def colormap_depth(depth_stack, extrema=None, mask_stack=None, table=None):
    """visualize_depth over a stack of resident depth maps: (F, n) float32 -> (F, n, 3) uint8, one launch.
    extrema: a (2,) float32 device tensor (vmin, vmax) -- SplitExtrema.depth or .depth_reflect for the reference's
    save_depth_unified_normalization (eval.py:931-978) -- or None for each frame's own extremes (one more launch reduces
    them).  mask_stack (F, n): the reflected variant, the colour multiplied by clip(mask, 0, 1) before the cast
    (eval.py:968-971).  A (n,) map is taken as a stack of one and gives (n, 3)."""
    L = _lib.lib()
    single = isinstance(depth_stack, torch.Tensor) and depth_stack.dim() == 1
    if single:
        depth_stack = depth_stack[None]
        mask_stack = None if mask_stack is None else mask_stack[None]
    d = _map(depth_stack, "depth_stack")
    if d.dim() != 2:
        raise ValueError(f"depth_stack must be (F, n) or (n,), got {tuple(d.shape)}")
    F, n = d.shape
    mk = None if mask_stack is None else _map(mask_stack, "mask_stack")
    if mk is not None and mk.shape != d.shape:
        raise ValueError(f"mask_stack must have the depth stack's shape {tuple(d.shape)}, got {tuple(mk.shape)}")
    ex = stats = None
    if extrema is None:
        stats = _stats(d.device, max(F, 1))
    else:
        ex = _map(extrema, "extrema", 2)
    tab = _table(table, d.device)
    out = torch.empty((F, n, 3), dtype=torch.uint8, device=d.device)
    _lib.check(L.mnrf_depth_colormap(d.data_ptr(), None if mk is None else mk.data_ptr(), F, n,
                                     None if ex is None else ex.data_ptr(), None if stats is None else stats.data_ptr(),
                                     tab.data_ptr(), out.data_ptr(), _lib.stream()), "mnrf_depth_colormap")
    return out[0] if single else out


_PANEL_VECTOR = (_lib.MNRF_PANEL_COPY, _lib.MNRF_PANEL_NORMAL, _lib.MNRF_PANEL_GLOBAL)


def val_panel_tiles(batch, results):
    """The tiles of visualize_val_image in its order (utils/visualization.py:32-179) as (name, kind, map) triples; a key that
    is absent from `results` or `batch` contributes no tile."""
    COPY, MASK, NORMAL = _lib.MNRF_PANEL_COPY, _lib.MNRF_PANEL_MASK, _lib.MNRF_PANEL_NORMAL
    GLOBAL, DEPTH = _lib.MNRF_PANEL_GLOBAL, _lib.MNRF_PANEL_DEPTH
    typs = ("fine", "coarse")
    tiles = [("gt_img", COPY, batch["rgbs"])]
    for key, name, kind in (("rgb_{}", "img_{}", COPY), ("rgb_{}_reflect", "img_reflect_{}", COPY),
                            ("rgb_{}_direct", "img_direct_{}", COPY), ("depth_{}", "depth_{}", DEPTH),
                            ("depth_{}_reflect", "depth_reflect_{}", DEPTH)):
        tiles += [(name.format(t), kind, results[key.format(t)]) for t in typs if key.format(t) in results]
    if "mirror_mask" in batch:
        tiles.append(("gt_mirror_mask", MASK, batch["mirror_mask"]))
    tiles += [(f"mirror_mask_pred_{t}", MASK, results[f"mirror_mask_{t}"]) for t in typs if f"mirror_mask_{t}" in results]
    for t in typs:
        if f"surface_normal_{t}" in results:
            tiles.append((f"normal_pred_{t}", NORMAL, results[f"surface_normal_{t}"]))
        if f"surface_normal_grad_{t}" in results:
            tiles.append((f"normal_grad_{t}", NORMAL, results[f"surface_normal_grad_{t}"]))
    for key in ("secondary_rays_o", "reflect_direction"):
        if key in results:
            tiles += [(key, COPY, results[key]), (f"{key}_vis", GLOBAL, results[key])]
    tiles += [(f"x_surface_{t}", GLOBAL, results[f"x_surface_{t}"]) for t in typs if f"x_surface_{t}" in results]
    return tiles


def val_panel(img_wh, batch, results, table=None):
    """visualize_val_image(img_wh, batch, results, add_text=False) (utils/visualization.py:26-184) on the device: `(stack,
    names)` with stack the (N_pics, 3, H, W) float32 panel the reference logs as val/GT_pred_depth and names the reference's
    label of every tile in the same order ("gt_img", "img_fine", ..., "x_surface_coarse").  batch: {"rgbs": (H W, 3)[,
    "mirror_mask": (H W)]} and results: the eval-semantics maps, all float32 on the device; they are read in place and left
    unchanged.  Every tile is the reference's expression in single fp32 operations; the depth tiles are coloured
    through `table` (default jet_table()).  Two launches (csrc/mnrf_frames.hip), no host synchronisation.  Only the
    reference's --for_vis form: no captions are drawn into the tiles."""
    L = _lib.lib()
    W, H = (int(v) for v in img_wh)
    n = H * W
    tiles = val_panel_tiles(batch, results)
    maps = []
    for name, kind, t in tiles:
        if isinstance(t, torch.Tensor) and kind not in _PANEL_VECTOR:
            t = t.reshape(-1)                  # the reference's .squeeze(): (1, n) and (n, 1) maps are (n)
        elif isinstance(t, torch.Tensor) and t.dim() == 3 and t.shape[0] == 1:
            t = t[0]
        maps.append(_map(t, name, n, (3,) if kind in _PANEL_VECTOR else ()))
    dev = maps[0].device
    names = [name for name, _, _ in tiles]
    kinds = (ctypes.c_int * len(tiles))(*[kind for _, kind, _ in tiles])
    ptrs = (ctypes.c_void_p * len(tiles))(*[m.data_ptr() for m in maps])
    tab = _table(table, dev) if _lib.MNRF_PANEL_DEPTH in list(kinds) else None
    stats = torch.zeros((len(tiles), L.mnrf_val_panel_stats_floats()), dtype=torch.float32, device=dev)
    stack = torch.empty((len(tiles), 3, H, W), dtype=torch.float32, device=dev)
    _lib.check(L.mnrf_val_panel_extrema(ptrs, kinds, len(tiles), H, W, stats.data_ptr(), _lib.stream()), "mnrf_val_panel_extrema")
    _lib.check(L.mnrf_val_panel_write(ptrs, kinds, len(tiles), H, W, stats.data_ptr(), None if tab is None else tab.data_ptr(),
                                      stack.data_ptr(), _lib.stream()), "mnrf_val_panel_write")
    return stack, names
