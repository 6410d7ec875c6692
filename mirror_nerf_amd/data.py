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
datasets/blender.py -- no fixture pins it against the reference's own output.  It uses PIL and numpy only."""
import ctypes
import json
import os

import numpy as np
import torch

from . import _lib
from . import dist as D


class _Bank(ctypes.Structure):
    """MnrfBank of include/mnrf.h."""
    _fields_ = [("poses", ctypes.c_void_p), ("images", ctypes.c_void_p), ("masks", ctypes.c_void_p), ("frames", ctypes.c_void_p),
                ("n_frames", ctypes.c_int), ("H", ctypes.c_int), ("W", ctypes.c_int), ("channels", ctypes.c_int),
                ("slots", ctypes.c_int), ("focal", ctypes.c_float), ("near", ctypes.c_float), ("far", ctypes.c_float)]


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
