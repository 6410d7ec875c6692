"""The training set on the device: `RayBank` keeps the frames of a pin-hole dataset as the bytes they were decoded to --
poses (F, 3, 4) float32, images (F, H, W, C) uint8, mirror masks (F, H, W) int8 -- and produces a training batch
(`rays (B, 8)`, `rgbs (B, 3)`, `mirror_mask (B,)`) in ONE launch of csrc/mnrf_bank.hip, written into caller-owned tensors
(`GraphedTrainStep`'s own `rays` / `target` / `gt` buffers as they are).

The reference's route (datasets/blender.py:51-108) builds every ray of every training image on the host as float32 -- 12
floats, 48 B per ray -- and a shuffling DataLoader hands out batches: per step 1024 `__getitem__` calls, a collate and three
host-to-device copies.  The bank holds C + 1 bytes per pixel and draws from a shuffled stream that, like that loader, visits
every ray exactly once per epoch: the stream is one keyed permutation of [0, N) per epoch, made in registers (a Feistel
network with cycle walking; the contract is stated in the header comment of csrc/mnrf_bank.hip).

`read_blender` reads a Blender-format directory the way `BlenderDataset` does.  The reference's class needs cv2 and
torchvision, which the machines this package is developed on do not have, so this loader is a RESTATEMENT FROM READING
datasets/blender.py -- no fixture pins it against the reference's own output.  It uses PIL and numpy only.

`read_arkit` reads a real capture (datasets/real_arkit.py: poses centred with the average pose of transforms.json, the fly-through
splits) and is pinned against the reference class by tests/golden/make_golden_poses.py.  It resizes on the host with PIL: the
CPU route and the tests' reference.  `RayBank.from_arkit` decodes with PIL, uploads the frames at their native size and resizes
them on the device, straight into the bank's arrays (csrc/mnrf_resample.hip): `resample_lanczos` is Pillow's 8-bit LANCZOS
resize bit for bit, `resize_mask_nearest` the masks' nearest pick with the reference's thresholds."""
import ctypes
import functools
import json
import math
import os
import warnings
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from . import dist as D


_Bank = _lib.STRUCTS["MnrfBank"]


def _device_array(x, dtype, device, what):
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"RayBank: {what} must be a numpy array or a tensor")
    if t.dtype != dtype:
        raise TypeError(f"RayBank: {what} must be {dtype}, got {t.dtype} (the bank keeps the decoded bytes; it does not convert)")
    return t.to(device).contiguous()


def frames_with_mask(masks):
    """The frames of an (F, H, W) mask array without a -1: the reference's *_wmask subset (blender.py:91-95)."""
    m = torch.from_numpy(masks) if isinstance(masks, np.ndarray) else masks
    ok = (m.reshape(m.shape[0], -1).amin(1) >= 0).tolist()
    return [f for f, v in enumerate(ok) if v]


class RayBank:
    """A shared-intrinsics pin-hole training set resident on one GPU.

        bank = RayBank(poses, images, masks, focal, near, far, device)     # or RayBank.from_blender(root_dir, ...)
        rays, rgbs, mask = bank.draw(step, 1024, seed)                      # one launch; every ray once per epoch
        bank.select("with_mask").draw(step, 1024, seed, out=(g.rays, g.target, g.gt))

    poses (F, 3, 4) float32; images (F, H, W, C) uint8 with C 3 or 4; masks (F, H, W) int8 with -1 for "no ground-truth mask
    for this frame", 0 and 1 (None: every frame -1); one focal length, near and far.  A global ray index g addresses slot
    g // (H*W) of the selected frames and pixel g % (H*W)."""

    def __init__(self, poses, images, masks, focal, near, far, device="cuda"):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("mirror_nerf_amd runs on the GPU only: a RayBank lives on a cuda device (got %s)" % device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if masks is None:
            masks = np.full(tuple(images.shape[:3]), -1, np.int8)
        self.poses = _device_array(poses, torch.float32, device, "poses")
        self.images = _device_array(images, torch.uint8, device, "images")
        self.masks = _device_array(masks, torch.int8, device, "masks")
        if self.images.dim() != 4 or self.images.shape[3] not in (3, 4) or self.images.shape[0] < 1 or self.images.numel() == 0:
            raise ValueError(f"RayBank: images must be (F, H, W, 3 or 4) with F, H, W >= 1, got {tuple(self.images.shape)}")
        F, H, W, C = self.images.shape
        if tuple(self.poses.shape) != (F, 3, 4):
            raise ValueError(f"RayBank: poses must be ({F}, 3, 4), got {tuple(self.poses.shape)}")
        if tuple(self.masks.shape) != (F, H, W):
            raise ValueError(f"RayBank: masks must be ({F}, {H}, {W}), got {tuple(self.masks.shape)}")
        self.H, self.W, self.channels = int(H), int(W), int(C)
        self.focal, self.near, self.far = float(focal), float(near), float(far)
        self.device = device
        self.frames_with_mask = frames_with_mask(masks)      # (a host read when `masks` is a device tensor: once, here)
        self._set_frames(None)

    # ------------------------------------------------------------------ frame selection
    def _set_frames(self, frames):
        F = int(self.images.shape[0])
        self.frame_ids = list(range(F)) if frames is None else [int(f) for f in frames]
        self._frames = None if frames is None else torch.tensor(self.frame_ids, dtype=torch.int32, device=self.device)
        self._c = _Bank(self.poses.data_ptr(), self.images.data_ptr(), self.masks.data_ptr(),
                        None if self._frames is None else self._frames.data_ptr(), F, self.H, self.W, self.channels,
                        len(self.frame_ids), self.focal, self.near, self.far)

    def select(self, frames=None):
        """A bank over a subset of the frames that shares this one's device arrays: None = every frame, "with_mask" = the
        frames whose ground-truth mask is valid everywhere (the reference's *_wmask buffers, which its geometry stage
        trains on: blender.py:91-95, 193-198), or a list of frame numbers (slot k of the result is frame frames[k])."""
        if isinstance(frames, str):
            if frames != "with_mask":
                raise ValueError("RayBank.select: frames must be None, \"with_mask\" or a list of frame numbers")
            frames = self.frames_with_mask
        if frames is not None:
            frames = [int(f) for f in frames]
            F = int(self.images.shape[0])
            if not frames:
                raise ValueError("RayBank.select: no frame selected")
            if any(f < 0 or f >= F for f in frames):
                raise ValueError(f"RayBank.select: frame numbers must lie in [0, {F})")
        other = object.__new__(RayBank)
        other.__dict__.update(self.__dict__)
        other._set_frames(frames)
        return other

    @property
    def n_frames(self):
        return len(self.frame_ids)

    @property
    def n_rays(self):
        return self.n_frames * self.H * self.W

    def bytes_resident(self):
        return sum(t.numel() * t.element_size() for t in (self.poses, self.images, self.masks))

    # ------------------------------------------------------------------ outputs
    def _outs(self, n, out, want_valid):
        dev = self.device
        if dev.index != _lib._cur_device():
            raise RuntimeError(f"the bank lives on cuda:{dev.index} but the current device is cuda:{_lib._cur_device()}; "
                               "call torch.cuda.set_device / use `with torch.cuda.device(bank.device)`")
        if out is None:
            out = (torch.empty(n, 8, device=dev), torch.empty(n, 3, device=dev), torch.empty(n, device=dev))
        else:
            out = tuple(out)
            if len(out) != 3:
                raise ValueError("RayBank: out must be a (rays, rgbs, mirror_mask) triple")
            for t, shape, name in zip(out, ((n, 8), (n, 3), (n,)), ("rays", "rgbs", "mirror_mask")):
                if not isinstance(t, torch.Tensor) or not t.is_cuda or t.device != dev:
                    raise RuntimeError(f"RayBank: out {name} must be a tensor on {dev} (mirror_nerf_amd runs on the GPU only)")
                if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous():
                    raise ValueError(f"RayBank: out {name} must be a contiguous float32 tensor of shape {shape}, "
                                     f"got {t.dtype} {tuple(t.shape)}")
        valid = torch.empty(n, dtype=torch.bool, device=dev) if want_valid else None
        return out, valid

    def _gather(self, indices, start, n, out, want_valid):
        out, valid = self._outs(n, out, want_valid)
        _lib.check(_lib.lib().mnrf_bank_gather(ctypes.byref(self._c), None if indices is None else indices.data_ptr(), start, n,
                                               out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                               None if valid is None else valid.data_ptr(), _lib.stream()), "mnrf_bank_gather")
        return out, valid

    def gather(self, indices, out=None):
        """(rays, rgbs, mirror_mask) of the rays named by `indices`: a 1-D int64 tensor of global ray indices on the bank's
        device.  `out`: a (rays (n, 8), rgbs (n, 3), mirror_mask (n,)) triple of float32 device tensors to write into.  An
        index outside [0, n_rays) is not checked on the host (no synchronisation): its row comes back as NaN."""
        if not isinstance(indices, torch.Tensor) or not indices.is_cuda or indices.device != self.device:
            raise RuntimeError(f"RayBank.gather: indices must be a tensor on {self.device} (mirror_nerf_amd runs on the GPU only)")
        if indices.dtype != torch.int64 or indices.dim() != 1:
            raise ValueError(f"RayBank.gather: indices must be a 1-D int64 tensor, got {indices.dtype} {tuple(indices.shape)}")
        indices = indices.contiguous()
        return self._gather(indices, 0, indices.numel(), out, False)[0]

    def frame(self, f):
        """The dict `BlenderDataset.__getitem__` returns for a test or validation frame (blender.py:116-178): `rays`
        (H*W, 8), `rgbs` (H*W, 3), `mirror_mask` (H*W,), `valid_mask` (H*W,) bool -- of slot f of this bank, on the device."""
        f = int(f)
        if not 0 <= f < self.n_frames:
            raise IndexError(f"RayBank.frame: {f} is not in [0, {self.n_frames})")
        hw = self.H * self.W
        (rays, rgbs, mask), valid = self._gather(None, f * hw, hw, None, True)
        return {"rays": rays, "rgbs": rgbs, "mirror_mask": mask, "valid_mask": valid}

    def draw(self, step, batch, seed, rank=None, world=None, out=None, step_dev=None, return_indices=False):
        """The batch of `step` of the shuffled stream: (rays, rgbs, mirror_mask), and the drawn global indices (int64) as a
        fourth item with return_indices.  Lane l of `rank` in `world` (default: dist.world()) takes stream position
        (step * world + rank) * batch + l; position p lies in epoch p // n_rays and names ray perm(seed, epoch)(p % n_rays):
        every ray once per epoch, batches of a fixed size, a batch may straddle two epochs.  `step_dev`: a device int64
        tensor of one element whose value is added to `step` on the device -- capture the draw with it and `step_dev.add_(1)`
        in a graph and every replay draws the next batch.  `out` as in gather().  One launch, no host synchronisation."""
        if rank is None or world is None:
            r, w = D.world()
            rank, world = (r if rank is None else rank), (w if world is None else world)
        rank, world, batch, step = int(rank), int(world), int(batch), int(step)
        if world < 1 or not 0 <= rank < world:
            raise ValueError(f"RayBank.draw: rank {rank} must lie in [0, world = {world})")
        if batch < 0 or step < 0:
            raise ValueError("RayBank.draw: step and batch must not be negative")
        if step_dev is not None:
            if not isinstance(step_dev, torch.Tensor) or not step_dev.is_cuda or step_dev.device != self.device:
                raise RuntimeError(f"RayBank.draw: step_dev must be a tensor on {self.device}")
            if step_dev.dtype != torch.int64 or step_dev.numel() != 1:
                raise ValueError("RayBank.draw: step_dev must be an int64 tensor of one element")
        out, _ = self._outs(batch, out, False)
        idx = torch.empty(batch, dtype=torch.int64, device=self.device) if return_indices else None
        _lib.check(_lib.lib().mnrf_bank_draw(ctypes.byref(self._c), int(seed) & 0xFFFFFFFFFFFFFFFF, step,
                                             None if step_dev is None else step_dev.data_ptr(), rank, world, batch,
                                             out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), None,
                                             None if idx is None else idx.data_ptr(), _lib.stream()), "mnrf_bank_draw")
        return out + (idx,) if return_indices else out

    def epoch_of(self, step, batch, world=None):
        """The epoch the first ray of `step` lies in (host arithmetic): a driver compares it with the previous step's to know
        when to call set_epoch."""
        world = D.world()[1] if world is None else int(world)
        return (int(step) * world * int(batch)) // self.n_rays

    @classmethod
    def from_blender(cls, root_dir, split="train", img_wh=(800, 800), near=2.0, far=6.0, train_skip_step=1, device="cuda"):
        d = read_blender(root_dir, split, img_wh, near, far, train_skip_step)
        return cls(d["poses"], d["images"], d["masks"], d["focal"], d["near"], d["far"], device)

    @classmethod
    def from_arkit(cls, root_dir, split="train", img_wh=(480, 360), near=0.05, far=8.0, scale_factor=1.0, val_idx=0,
                   train_skip_step=1, device="cuda", workers=8):
        """The bank of a real capture (read_arkit's frames, poses and bounds) with the resize done on the device: the frames are
        decoded with PIL on `workers` threads (16 at most), uploaded at their native size and resized by resample_lanczos /
        resize_mask_nearest straight into the bank's arrays -- no host copy at img_wh is made.  The bytes are read_arkit's.
        The result also carries `pose_avg` and `file_paths`."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("mirror_nerf_amd runs on the GPU only: a RayBank lives on a cuda device (got %s)" % device)
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        m = _arkit_meta(root_dir, split, img_wh, near, far, scale_factor, val_idx, train_skip_step)
        if m["frames"] is None:
            raise ValueError(f"RayBank.from_arkit: the split {split} carries poses only; a bank needs images (use read_arkit)")
        from PIL import Image
        w, h = int(img_wh[0]), int(img_wh[1])
        paths = [os.path.join(root_dir, f["file_path"]) for f in m["frames"]]
        modes = []
        for p in paths:             # the header only: the bank's layout has to be known before its arrays are made
            with Image.open(p) as im:
                if im.mode not in ("RGB", "RGBA"):
                    raise ValueError(f"from_arkit: {p} has mode {im.mode}; RGB or RGBA expected")
                modes.append(im.mode)
        C = 4 if "RGBA" in modes else 3
        F = len(paths)
        with torch.cuda.device(device):
            images = torch.empty(F, h, w, C, dtype=torch.uint8, device=device)
            masks = torch.full((F, h, w), -1, dtype=torch.int8, device=device)
            n_threads = max(1, min(16, int(workers)))
            with ThreadPoolExecutor(max_workers=n_threads) as pool:
                for first in range(0, F, 2 * n_threads):       # a bounded number of native-size frames on the host at a time
                    chunk = range(first, min(F, first + 2 * n_threads))
                    for f, (img, mask) in zip(chunk, pool.map(lambda k: _decode_arkit_frame(root_dir, m["frames"][k]), chunk)):
                        src = _upload(img, device)[None]
                        if img.shape[2] == C:
                            resample_lanczos(src, (w, h), out=images[f:f + 1])
                        else:                                  # an RGB frame in an RGBA bank: alpha 255, as read_blender states
                            images[f, :, :, :3] = resample_lanczos(src, (w, h))[0]
                            images[f, :, :, 3] = 255
                        if mask is not None:
                            resize_mask_nearest(mask[None], (w, h), out=masks[f:f + 1])
            bank = cls(m["poses"], images, masks, m["focal"], m["near"], m["far"], device)
        bank.pose_avg, bank.file_paths = m["pose_avg"], [f["file_path"] for f in m["frames"]]
        return bank


def _resize_nearest(a, wh):
    """cv2.resize(a, wh, interpolation=cv2.INTER_NEAREST): source index floor(x * src / dst), clamped (not PIL's centred rule)."""
    w, h = wh
    ys = np.minimum(np.floor(np.arange(h) * (a.shape[0] / h)).astype(np.int64), a.shape[0] - 1)
    xs = np.minimum(np.floor(np.arange(w) * (a.shape[1] / w)).astype(np.int64), a.shape[1] - 1)
    return a[ys][:, xs]


def read_blender(root_dir, split="train", img_wh=(800, 800), near=2.0, far=6.0, train_skip_step=1):
    """The frames of `transforms_{split}.json` as host arrays: dict(poses (F, 3, 4) float32, images (F, H, W, C) uint8, masks
    (F, H, W) int8, focal, near, far, file_paths).  A restatement from reading datasets/blender.py (the reference's class
    imports cv2 and torchvision; nothing pins this against its output), with PIL and numpy only:
      * focal = 0.5 * 800 / tan(0.5 * camera_angle_x) * W / 800 (blender.py:33-39);
      * the train split keeps every train_skip_step-th frame (blender.py:53-58);
      * `{file_path}.png` resized to img_wh with PIL's LANCZOS and kept as uint8 RGB or RGBA -- the division by 255 and the
        alpha blend (blender.py:128-133) happen on the device, per drawn ray.  A bank has one layout: when RGB and RGBA
        frames are mixed, the RGB frames get an alpha of 255 (rgb * 1 + (1 - 1) is rgb bit for bit; their valid_mask is then
        all true instead of the reference's blue > 0);
      * the mask `masks/MirrorMask_{name[6:]}.png` at its own depth, resized with cv2's nearest-neighbour rule; an 8-bit value
        >= 128 gives 1 (/255, then the 0.5 thresholds, blender.py:141-154), a 16-bit value > 0 gives 1 (torchvision's
        ToTensor does not scale 16-bit input); a missing file makes the whole frame -1."""
    from PIL import Image
    with open(os.path.join(root_dir, f"transforms_{split}.json"), "r") as f:
        meta = json.load(f)
    w, h = int(img_wh[0]), int(img_wh[1])
    focal = 0.5 * 800 / np.tan(0.5 * meta["camera_angle_x"])
    focal *= w / 800
    frames = meta["frames"]
    if split == "train":
        frames = [frames[i] for i in np.arange(0, len(frames), train_skip_step)]
    poses, images, masks, paths = [], [], [], []
    for frame in frames:
        poses.append(np.array(frame["transform_matrix"], dtype=np.float64)[:3, :4].astype(np.float32))
        img = Image.open(os.path.join(root_dir, f"{frame['file_path']}.png"))
        if img.mode not in ("RGB", "RGBA"):
            raise ValueError(f"read_blender: {frame['file_path']}.png has mode {img.mode}; RGB or RGBA expected")
        images.append(np.asarray(img.resize((w, h), Image.LANCZOS), dtype=np.uint8))
        name = os.path.split(frame["file_path"])[-1]
        mask_path = os.path.join(root_dir, "masks", f"MirrorMask_{name[6:]}.png")
        if not os.path.exists(mask_path):
            masks.append(np.full((h, w), -1, np.int8))      # -1 marks an invalid GT mirror mask (blender.py:142-147)
        else:
            m = Image.open(mask_path)
            if m.mode in ("I;16", "I;16B", "I;16L", "I"):
                m = np.asarray(m).astype(np.int64) > 0      # unscaled by ToTensor: any value above 0.5 is 1
            else:
                m = np.asarray(m.convert("L"), dtype=np.uint8) >= 128
            masks.append(_resize_nearest(m, (w, h)).astype(np.int8))
        paths.append(frame["file_path"])
    channels = {im.shape[2] for im in images}
    if len(channels) > 1:
        images = [im if im.shape[2] == 4 else np.concatenate([im, np.full(im.shape[:2] + (1,), 255, np.uint8)], 2) for im in images]
    return dict(poses=np.stack(poses), images=np.stack(images), masks=np.stack(masks), focal=float(focal), near=float(near),
                far=float(far), file_paths=paths)


# ----------------------------------------------------------------------------- the resize on the device
PRECISION_BITS = 32 - 8 - 2          # Pillow's fixed point for 8-bit images


def _lanczos(x):
    if -3.0 <= x < 3.0:
        def sinc(v):
            if v == 0.0:
                return 1.0
            v = v * math.pi
            return math.sin(v) / v
        return sinc(x) * sinc(x / 3)
    return 0.0


@functools.lru_cache(maxsize=64)
def lanczos_taps(in_size, out_size):
    """The windows and fixed-point weights of Pillow's LANCZOS resize of one axis from in_size to out_size samples, made as
    Pillow makes them, in double: (bounds (out, 2) int32: first source sample and count, taps (out, ksize) int32: 22
    fraction bits, zero past the count).  scale = in / out; fs = max(scale, 1); support = 3 fs; ksize = 2 ceil(support) + 1;
    centre = (i + 0.5) scale; the window is [max(int(centre - support + 0.5), 0), min(int(centre + support + 0.5), in));
    weight k = lanczos((k + lo - centre + 0.5) * (1 / fs)), lanczos(x) = sinc(x) sinc(x / 3) on [-3, 3); the weights are divided
    by their sum (accumulated in index order) and converted as int(+-0.5 + w 2^22), the sign w's.  Cached; the arrays are
    read-only."""
    in_size, out_size = int(in_size), int(out_size)
    if in_size < 1 or out_size < 1:
        raise ValueError("lanczos_taps: sizes must be at least 1")
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ss = 1.0 / fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    taps = np.zeros((out_size, ksize), np.int32)
    one = float(1 << PRECISION_BITS)
    for i in range(out_size):
        center = (i + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - lo
        ws = [_lanczos((k + lo - center + 0.5) * ss) for k in range(n)]
        ww = 0.0
        for v in ws:
            ww += v
        if ww != 0.0:
            ws = [v / ww for v in ws]
        bounds[i] = (lo, n)
        taps[i, :n] = [int(-0.5 + v * one) if v < 0 else int(0.5 + v * one) for v in ws]
    bounds.setflags(write=False)
    taps.setflags(write=False)
    return bounds, taps


_device_taps = {}


def _taps_on(in_size, out_size, device):
    """(taps (ksize, out) int32 -- transposed: the kernel's layout --, bounds (out, 2) int32, ksize) on the device; cached."""
    key = (int(in_size), int(out_size), device.index)
    if key not in _device_taps:
        bounds, taps = lanczos_taps(in_size, out_size)
        _device_taps[key] = (torch.from_numpy(np.array(taps.T, order="C")).to(device), torch.from_numpy(bounds.copy()).to(device),
                             int(taps.shape[1]))
    return _device_taps[key]


def _upload(a, device):
    """A host array on the device.  PIL hands out read-only buffers and torch warns about tensors over them; this one is
    only read, so the array is not copied first."""
    with warnings.catch_warnings():
        warnings.filterwarnings("ignore", message="The given NumPy array is not writable")
        return torch.from_numpy(a).to(device)


def _check_stack(t, what, dtypes, dims):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{what} must be a tensor on a cuda device (mirror_nerf_amd runs on the GPU only)")
    if t.dtype not in dtypes or t.dim() != dims:
        raise ValueError(f"{what} must be a {dims}-D tensor of {' or '.join(str(d) for d in dtypes)}, got {t.dtype} {tuple(t.shape)}")
    if t.device.index != _lib._cur_device():
        raise RuntimeError(f"{what} lives on cuda:{t.device.index} but the current device is cuda:{_lib._cur_device()}; "
                           "call torch.cuda.set_device / use `with torch.cuda.device(t.device)`")
    return t.contiguous()


def _check_out(out, shape, dtype, like, what):
    if out is None:
        return torch.empty(shape, dtype=dtype, device=like.device)
    if not isinstance(out, torch.Tensor) or out.device != like.device or out.dtype != dtype or tuple(out.shape) != tuple(shape) \
            or not out.is_contiguous():
        raise ValueError(f"{what}: out must be a contiguous {dtype} tensor of shape {tuple(shape)} on {like.device}")
    return out


def resample_lanczos(images_u8, wh, out=None):
    """`Image.resize(wh, Image.LANCZOS)` of every frame of a (F, H, W, C) uint8 device tensor, C 3 (RGB) or 4 (RGBA), on the
    device and bit for bit Pillow's: (F, h, w, C) uint8 (into `out` when given).  A pass along x, rounded to 8 bits, then a pass
    along y; a pass whose sizes agree is not run, and when both agree the result is a plain copy (as Pillow returns one: RGBA
    does not make the premultiply round trip then) without a kernel launch.  The arithmetic is stated in
    csrc/mnrf_resample.hip, the tables in lanczos_taps."""
    src = _check_stack(images_u8, "resample_lanczos: images", (torch.uint8,), 4)
    F, sh, sw, C = (int(v) for v in src.shape)
    w, h = int(wh[0]), int(wh[1])
    if C not in (3, 4) or min(F, sh, sw, w, h) < 1:
        raise ValueError(f"resample_lanczos: images must be (F, H, W, 3 or 4) with every size at least 1, got {tuple(src.shape)} -> {(w, h)}")
    dst = _check_out(out, (F, h, w, C), torch.uint8, src, "resample_lanczos")
    if (sw, sh) == (w, h):
        dst.copy_(src)
        return dst
    L = _lib.lib()
    tx, bx, kx = _taps_on(sw, w, src.device) if sw != w else (None, None, 0)
    ty, by, ky = _taps_on(sh, h, src.device) if sh != h else (None, None, 0)
    n_tmp = L.mnrf_resample_tmp_bytes(F, sh, sw, h, w, C)
    if n_tmp < 0:
        raise ValueError(f"resample_lanczos: sizes out of range: {tuple(src.shape)} -> {(w, h)}")
    tmp = torch.empty(n_tmp, dtype=torch.uint8, device=src.device) if n_tmp else None
    _lib.check(L.mnrf_resample_u8(src.data_ptr(), F, sh, sw, C, dst.data_ptr(), h, w, _lib.ptr(tx), _lib.ptr(bx), kx,
                                  _lib.ptr(ty), _lib.ptr(by), ky, None if tmp is None else tmp.data_ptr(), _lib.stream()),
               "mnrf_resample_u8")
    return dst


def resize_mask_nearest(masks, wh, out=None):
    """Mirror masks at their native depth to the bank's int8 at wh = (w, h), on the device: masks (F, H, W) of uint8 or of 16-bit
    samples (a numpy uint8 / uint16 array, which is uploaded, or a device tensor of uint8, uint16 or int16 holding the raw
    samples) -> (F, h, w) int8 of 0 and 1 (into `out` when given).  The pick is `_resize_nearest`'s (cv2's INTER_NEAREST rule);
    an 8-bit sample >= 128 is 1, a 16-bit sample > 0 is 1 (read_blender states why)."""
    if isinstance(masks, np.ndarray):
        if masks.dtype not in (np.uint8, np.uint16):
            raise ValueError(f"resize_mask_nearest: a numpy mask must be uint8 or uint16, got {masks.dtype}")
        a = np.ascontiguousarray(masks)
        dev = out.device if isinstance(out, torch.Tensor) else torch.device("cuda", torch.cuda.current_device())
        masks = _upload(a.view(np.int16) if a.dtype == np.uint16 else a, dev)
    two = tuple(d for d in (torch.int16, getattr(torch, "uint16", None)) if d is not None)
    src = _check_stack(masks, "resize_mask_nearest: masks", (torch.uint8,) + two, 3)
    F, sh, sw = (int(v) for v in src.shape)
    w, h = int(wh[0]), int(wh[1])
    if min(F, sh, sw, w, h) < 1:
        raise ValueError(f"resize_mask_nearest: every size must be at least 1, got {tuple(src.shape)} -> {(w, h)}")
    dst = _check_out(out, (F, h, w), torch.int8, src, "resize_mask_nearest")
    _lib.check(_lib.lib().mnrf_mask_nearest(src.data_ptr(), src.element_size(), F, sh, sw, dst.data_ptr(), h, w, _lib.stream()),
               "mnrf_mask_nearest")
    return dst


# ----------------------------------------------------------------------------- real captures (datasets/real_arkit.py)
# test_rotate: the frame the camera is moved around and a shift of its z, chosen like recursion.PLACE_MIRROR_PRESETS by the first
# key that is a substring of root_dir (real_arkit.py:153-159); None: frame val_idx, no shift
ROTATE_PRESETS = (
    ("market", dict(frame=77, dz=-0.3)),
    (None, dict(frame=None, dz=0.0)),
)
IMAGE_SPLITS = ("train", "val", "test", "test_train")
PATH_SPLITS = ("test_rotate", "test_interpolation")


def _arkit_meta(root_dir, split, img_wh, near, far, scale_factor, val_idx, train_skip_step):
    """Everything of read_arkit but the pixels: dict(frames: the split's frame entries (None for the path splits), poses_f64
    (F, 3, 4), poses float32, focal, near, far, pose_avg)."""
    from . import poses as P
    if split not in IMAGE_SPLITS + PATH_SPLITS:
        raise ValueError(f"read_arkit: split must be one of {IMAGE_SPLITS + PATH_SPLITS}, not {split!r}")
    with open(os.path.join(root_dir, "transforms.json"), "r") as f:
        meta_all = json.load(f)
    split_file = os.path.join(root_dir, f"transforms_{split}.json")
    if split == "test_rotate" and not os.path.exists(split_file):
        meta = meta_all              # the split's file gives the reference nothing but the intrinsics
    else:
        with open(split_file, "r") as f:
            meta = json.load(f)
    w = int(img_wh[0])
    if "camera_angle_x" in meta:                                     # real_arkit.py:51-58
        focal = 0.5 * 1920 / np.tan(0.5 * meta["camera_angle_x"])
        focal *= w / 1920
    else:                                                            # real_arkit.py:59-74
        focal = meta["fx"] if "fx" in meta else meta["frames"][0]["intrinsics"][0][0]
        cx = meta["cx"] if "cx" in meta else meta["frames"][0]["intrinsics"][0][2]
        focal *= w / (cx * 2)
    near, far = near / scale_factor, far / scale_factor
    # the same average pose for every split: the one of all frames (real_arkit.py:86-89)
    poses_all = np.stack([np.array(f["transform_matrix"], dtype=np.float64) for f in meta_all["frames"]], 0)
    poses_all, pose_avg = P.center_poses(poses_all[:, :3, :4])
    poses_all[..., 3] /= scale_factor

    def centred(frame):
        pose = P.center_pose_from_avg(pose_avg, np.array(frame["transform_matrix"], dtype=np.float64))
        pose[..., 3] /= scale_factor
        return pose[:3, :4]

    frames = meta["frames"]
    if split == "test_rotate":                                       # real_arkit.py:153-169
        preset = _lib.preset(ROTATE_PRESETS, root_dir)
        idx = val_idx if preset["frame"] is None else preset["frame"]
        base = poses_all[idx].copy()
        base[2, 3] += preset["dz"]
        c2ws = np.stack([P.move_camera_pose_slightly(base, i / 32) for i in range(32)], 0)
        frames = None
    elif split == "test_interpolation":                              # real_arkit.py:170-200
        c2ws = P.interpolate_poses(np.stack([centred(f) for f in frames], 0), 64)[:, :3, :4]
        frames = None
    else:
        if split == "train":
            frames = [frames[i] for i in np.arange(0, len(frames), train_skip_step)]
        elif split == "val":
            frames = [frames[val_idx]]
        c2ws = np.stack([centred(f) for f in frames], 0)
    return dict(frames=frames, poses_f64=c2ws, poses=c2ws.astype(np.float32), focal=float(focal), near=float(near), far=float(far),
                pose_avg=pose_avg)


def _decode_arkit_frame(root_dir, frame):
    """(image (H, W, 3 or 4) uint8, mask (H, W) uint8 or uint16 at its native depth, or None without a mask file)."""
    from PIL import Image
    path = os.path.join(root_dir, frame["file_path"])
    img = Image.open(path)
    if img.mode not in ("RGB", "RGBA"):
        raise ValueError(f"read_arkit: {path} has mode {img.mode}; RGB or RGBA expected")
    image = np.asarray(img, dtype=np.uint8)
    mask_path = os.path.join(root_dir, "masks", os.path.split(frame["file_path"])[-1])
    if not os.path.exists(mask_path):
        return image, None
    m = Image.open(mask_path)
    if m.mode in ("I;16", "I;16B", "I;16L", "I"):
        a = np.asarray(m)
        mask = a if a.dtype == np.uint16 else (a.astype(np.int64) > 0).astype(np.uint16)
    else:
        mask = np.asarray(m.convert("L"), dtype=np.uint8)
    return image, np.ascontiguousarray(mask)


def read_arkit(root_dir, split="train", img_wh=(480, 360), near=0.05, far=8.0, scale_factor=1.0, val_idx=0, train_skip_step=1):
    """A real capture the way `RealDatasetARKit` reads it (datasets/real_arkit.py), as host arrays: the dict read_blender
    returns -- poses (F, 3, 4) float32, images (F, H, W, C) uint8, masks (F, H, W) int8, focal, near, far, file_paths -- plus
    `pose_avg` (3, 4) and `poses_f64`, the poses before the rounding to float32 that the reference applies when it makes rays.
      * focal: with `camera_angle_x`, 0.5 * 1920 / tan(0.5 * angle) * W / 1920; otherwise fx * W / (2 cx), fx and cx from the
        top level of the split's file or from its frame 0's `intrinsics`;
      * near and far are divided by scale_factor;
      * pose_avg is the average pose of transforms.json (all frames), whatever the split; a frame's pose is centred with it
        and its translation divided by scale_factor;
      * train keeps every train_skip_step-th frame, val the one frame val_idx, test and test_train every frame;
      * `{file_path}` (the name carries its extension), RGB or RGBA, resized to img_wh with PIL's LANCZOS; mixed frames as in
        read_blender; the mask `masks/{file name}` at its own depth under read_blender's rules (8 bit: >= 128 is 1; 16 bit:
        > 0 is 1; no file: the frame is -1).  cv2.imread / cv2.resize are stood in by PIL and `_resize_nearest`;
      * test_rotate: 32 poses, move_camera_pose_slightly(pose, i / 32) of the centred pose of frame val_idx of transforms.json
        (ROTATE_PRESETS: for a `market` scene frame 77 with z - 0.3); its intrinsics come from transforms_test_rotate.json,
        or from transforms.json where that file does not exist;
      * test_interpolation: 64 poses through the centred key frames of transforms_test_interpolation.json
        (poses.interpolate_poses).
    The two path splits carry poses only: images, masks and file_paths are None."""
    from PIL import Image
    m = _arkit_meta(root_dir, split, img_wh, near, far, scale_factor, val_idx, train_skip_step)
    out = dict(poses=m["poses"], poses_f64=m["poses_f64"], images=None, masks=None, focal=m["focal"], near=m["near"], far=m["far"],
               file_paths=None, pose_avg=m["pose_avg"])
    if m["frames"] is None:
        return out
    w, h = int(img_wh[0]), int(img_wh[1])
    images, masks = [], []
    for frame in m["frames"]:
        image, mask = _decode_arkit_frame(root_dir, frame)
        images.append(np.asarray(Image.fromarray(image).resize((w, h), Image.LANCZOS), dtype=np.uint8))
        if mask is None:
            masks.append(np.full((h, w), -1, np.int8))
        else:
            masks.append(_resize_nearest(mask >= 128 if mask.dtype == np.uint8 else mask > 0, (w, h)).astype(np.int8))
    if len({im.shape[2] for im in images}) > 1:
        images = [im if im.shape[2] == 4 else np.concatenate([im, np.full(im.shape[:2] + (1,), 255, np.uint8)], 2) for im in images]
    out.update(images=np.stack(images), masks=np.stack(masks), file_paths=[f["file_path"] for f in m["frames"]])
    return out
