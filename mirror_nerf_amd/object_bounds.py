"""Object bounds for app_reflect_newly_placed_objects: where, in its own frame, a placed object may have density.

batched_inference renders the object at every recursion level; with bounds it renders it only along the rays whose segment can
touch them (mnrf_object_cull), and merges the result back through the kept rays' index (mnrf_object_merge_indexed).  Bounds
are a box [lo, hi] in the OBJECT's frame -- the frame its field is evaluated in, behind the ray move of mnrf_object_rays --
cut into res = (Rx, Ry, Rz) cells, with one bit per cell (`bits`, None: the whole box counts).

What is guaranteed (include/mnrf.h, mnrf_object_cull): a ray whose segment meets a set cell is always kept, and kept rays are
rendered and merged exactly as without bounds (the same samples, the same launches on fewer rows).  What is assumed: that the
object has no density that matters outside the set cells.  For bounds given by hand that is the caller's statement; for
estimated ones see estimate_object_bounds.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib

__all__ = ["ObjectBounds", "estimate_object_bounds", "occupancy_bits", "MAX_RES"]

MAX_RES = 1024      # MNRF_OBJECT_MAX_RES


def _vec3(v, name):
    v = [float(x) for x in (v.tolist() if hasattr(v, "tolist") else v)]
    if len(v) != 3:
        raise ValueError(f"{name} must hold three numbers, not {len(v)}")
    if not all(math.isfinite(x) for x in v):
        raise ValueError(f"{name} must be finite, not {v}")
    return tuple(v)


def _res3(res):
    if isinstance(res, (int, np.integer)):
        res = (res, res, res)
    res = tuple(res)
    if len(res) != 3 or not all(isinstance(r, (int, np.integer)) and not isinstance(r, bool) for r in res):
        raise ValueError(f"res must be an int or three ints (Rx, Ry, Rz), not {res!r}")
    if not all(1 <= r <= MAX_RES for r in res):
        raise ValueError(f"res must be in 1..{MAX_RES} on every axis, not {res}")
    return tuple(int(r) for r in res)


def _object_system(system_obj):
    """(models, embeddings) of system_obj as the dicts render_rays takes: nerf_pl keeps lists, [coarse, fine] and [xyz, dir]
    (models/nerf_pl/rendering_nerfpl.py:138-140, 197)."""
    models, embeddings = system_obj.models, system_obj.embeddings
    if not isinstance(models, dict):
        models = dict(zip(("coarse", "fine"), models))
    if not isinstance(embeddings, dict):
        embeddings = dict(zip(("xyz", "dir"), embeddings))
    return models, embeddings


def words_per_row(rx):
    return (int(rx) + 31) // 32


class ObjectBounds:
    """A box in the object's frame, optionally refined by a bit grid of occupied cells.

    lo, hi: three floats each, lo < hi.  res: (Rx, Ry, Rz), 1..1024 per axis (an int: the same on every axis).  bits: None, or
    an int32 tensor of Rz * Ry * ceil(Rx / 32) words in the layout of include/mnrf.h (cell i of row (k, j) is bit i % 32 of
    word i / 32; padding bits zero), on the CPU or on the device the rays will live on.  Without bits the whole box counts
    and res must be (1, 1, 1)."""

    def __init__(self, lo, hi, res=(1, 1, 1), bits=None):
        self.lo, self.hi = _vec3(lo, "lo"), _vec3(hi, "hi")
        if not all(a < b for a, b in zip(self.lo, self.hi)):
            raise ValueError(f"ObjectBounds needs lo < hi on every axis, not lo={self.lo}, hi={self.hi}")
        if not all(math.isfinite(np.float32(b) - np.float32(a)) and np.float32(a) < np.float32(b) for a, b in zip(self.lo, self.hi)):
            raise ValueError(f"ObjectBounds: lo < hi must hold in float32 with a finite extent, not lo={self.lo}, hi={self.hi}")
        self.res = _res3(res)
        if bits is None:
            if self.res != (1, 1, 1):
                raise ValueError(f"ObjectBounds without bits is one cell: res must be (1, 1, 1), not {self.res}")
        else:
            if not isinstance(bits, torch.Tensor):
                raise TypeError("bits must be a torch tensor (int32 words) or None")
            if bits.dtype != torch.int32:
                raise ValueError(f"bits must be int32 (32 cells per word), not {bits.dtype}")
            want = self.res[2] * self.res[1] * words_per_row(self.res[0])
            if bits.numel() != want:
                raise ValueError(f"bits must hold Rz * Ry * ceil(Rx / 32) = {want} words for res {self.res}, not {bits.numel()}")
            if bits.device.type not in ("cpu", "cuda"):
                raise ValueError(f"bits must live on the CPU or on a GPU, not on {bits.device}")
            bits = bits.contiguous().view(self.res[2], self.res[1], words_per_row(self.res[0]))
        self.bits = bits
        self._cells = None

    def __repr__(self):
        return f"ObjectBounds(lo={self.lo}, hi={self.hi}, res={self.res}, bits={'None' if self.bits is None else 'set: %d' % self.n_set})"

    # ---- host-side views of the cells
    def cells(self):
        """(Rz, Ry, Rx) numpy bool array of the set cells (host copy, made once)."""
        if self._cells is None:
            rx, ry, rz = self.res
            if self.bits is None:
                self._cells = np.ones((1, 1, 1), bool)
            else:
                w = self.bits.detach().cpu().numpy().view(np.uint32).reshape(rz, ry, -1)
                b = (w[..., None] >> np.arange(32, dtype=np.uint32)) & 1
                full = b.reshape(rz, ry, -1).astype(bool)
                if full[:, :, rx:].any():
                    raise ValueError("bits: a padding bit (behind cell Rx - 1 of a row) is set")
                self._cells = full[:, :, :rx]
        return self._cells

    @property
    def n_set(self):
        return int(self.cells().sum())

    @property
    def cell(self):
        return tuple((h - l) / r for l, h, r in zip(self.lo, self.hi, self.res))

    def tight_box(self):
        """(lo, hi) of the axis-aligned box around the set cells, or None when no cell is set."""
        c = self.cells()
        if not c.any():
            return None
        lo, hi = [], []
        for axis, (keep, l, s) in enumerate(zip(((0, 1), (0, 2), (1, 2)), self.lo, self.cell)):      # x, y, z <- array axes 2, 1, 0
            idx = np.nonzero(c.any(axis=keep))[0]
            lo.append(l + s * int(idx[0]))
            hi.append(l + s * (int(idx[-1]) + 1))
        return tuple(lo), tuple(hi)

    def touches_region_border(self):
        """True when a set cell lies on a face of the box: the object may continue outside the region it was looked for in."""
        c = self.cells()
        return bool(c[0].any() or c[-1].any() or c[:, 0].any() or c[:, -1].any() or c[:, :, 0].any() or c[:, :, -1].any())

    def to(self, device):
        """The same bounds with the bits on `device`."""
        if self.bits is None or self.bits.device == torch.device(device):
            return self
        out = ObjectBounds(self.lo, self.hi, self.res, self.bits.to(device))
        out._cells = self._cells
        return out

    # ---- the device passes
    def cull(self, rays, xform):
        """mnrf_object_cull on one level's rays (N, 8) with the ray move `xform` (placed_objects.resolve_new_object) ->
        (object-frame rays of the kept rays (N, 8), their rows (N,) int32, count (1,) int32 on the device): rows from count on
        are undefined.  rays of another precision or layout are converted."""
        return self._cull(_lib.f32_in(rays), xform)

    def _cull(self, rays, xform):
        """cull for the driver, whose rays are float32 rows already."""
        N = rays.shape[0]
        if self.bits is not None and self.bits.device != rays.device:
            raise ValueError(f"ObjectBounds: the bits live on {self.bits.device}, the rays on {rays.device} (use .to(device))")
        out = torch.empty_like(rays)
        index = torch.empty(N, dtype=torch.int32, device=rays.device)
        count = torch.full((1,), 0, dtype=torch.int32, device=rays.device)
        pose = (ctypes.c_float * 12)(*xform["pose"]) if xform["pose"] is not None else None
        tx, ty, tz = xform["translation"]
        p = _lib.ptr
        _lib.check(_lib.lib().mnrf_object_cull(
            p(rays), N, pose, xform["scale"], tx, ty, tz, (ctypes.c_float * 3)(*self.lo), (ctypes.c_float * 3)(*self.hi),
            self.res[0], self.res[1], self.res[2], p(self.bits), p(out), p(index), p(count), _lib.stream()), "mnrf_object_cull")
        return out, index, count


def occupancy_bits(volume, sigma_min, dilate=1):
    """mnrf_occupancy_bits: (Rz+1, Ry+1, Rx+1) float32 corner samples on the device -> (bits (Rz, Ry, ceil(Rx/32)) int32,
    n_set (1,) int32 on the device)."""
    if volume.dim() != 3 or volume.dtype != torch.float32 or min(volume.shape) < 2:
        raise ValueError("volume must be a float32 tensor of (Rz+1, Ry+1, Rx+1) corner samples, at least 2 per axis")
    if dilate not in (0, 1):
        raise ValueError(f"dilate must be 0 or 1, not {dilate!r}")
    rz, ry, rx = (int(s) - 1 for s in volume.shape)
    _res3((rx, ry, rz))
    volume = volume.contiguous()
    with torch.cuda.device(volume.device):
        bits = torch.empty(rz, ry, words_per_row(rx), dtype=torch.int32, device=volume.device)
        n_set = torch.empty(1, dtype=torch.int32, device=volume.device)
        _lib.check(_lib.lib().mnrf_occupancy_bits(_lib.ptr(volume), rx, ry, rz, float(sigma_min), int(dilate), _lib.ptr(bits),
                                                  _lib.ptr(n_set), _lib.stream()), "mnrf_occupancy_bits")
    return bits, n_set


def default_sigma_min(region_lo, region_hi):
    """-ln(0.9) / |region diagonal|: along any segment inside the region that touches only cells below this density the
    accumulated opacity 1 - exp(-integral of sigma) is at most 1 - 0.9 = 0.1, far under the 0.8 the merge asks for."""
    diag = math.sqrt(sum((h - l) ** 2 for l, h in zip(region_lo, region_hi)))
    return -math.log(0.9) / diag


@torch.no_grad()
def estimate_object_bounds(obj, region_lo, region_hi, res=64, frame_time=None, sigma_min=None, dilate=1):
    """Bounds of an object from its own density, sampled at the (res+1)^3 corners of a res^3 grid over the region
    [region_lo, region_hi] of the object's frame.

    obj: a nerf_pl `system_obj` (.models / .embeddings as batched_inference takes them: the density through the route of
    mesh.density_grid, on the fine model when there are two), or a `render_kwargs_test_d_nerf` dict (the density through
    dnerf.dnerf_field(xyz=, sigma_only=True) at `frame_time`, on network_fine when there are two models).
    sigma_min: a cell is set when one of its corners has a density >= sigma_min; the default is default_sigma_min(region).
    dilate: 1 (default) grows the set by one cell over the 26-neighbourhood, 0 does not.

    THE ASSUMPTION: the corner samples represent the cell.  Under it the default threshold is a bound -- a ray that touches no
    set cell accumulates an opacity of at most 0.1 inside the region and can never be taken by the merge (> 0.8) -- but a
    structure thinner than a cell can pass between the corners unseen; `dilate` is there for that, and so is a larger res.
    Density outside the region is not looked at at all: check touches_region_border() of the result."""
    lo, hi = _vec3(region_lo, "region_lo"), _vec3(region_hi, "region_hi")
    if not all(a < b for a, b in zip(lo, hi)):
        raise ValueError(f"the region needs lo < hi on every axis, not lo={lo}, hi={hi}")
    if not isinstance(res, (int, np.integer)) or isinstance(res, bool) or not 1 <= res <= MAX_RES:
        raise ValueError(f"res must be an int in 1..{MAX_RES}, not {res!r}")
    res = int(res)
    if sigma_min is None:
        sigma_min = default_sigma_min(lo, hi)
    from . import mesh
    n = res + 1
    ranges = ((lo[0], hi[0]), (lo[1], hi[1]), (lo[2], hi[2]))
    if isinstance(obj, dict):                                                    # D-NeRF
        if frame_time is None:
            raise ValueError("a D-NeRF object moves: estimate_object_bounds needs frame_time=")
        from .dnerf import dnerf_field
        net = obj["network_fn"] if obj.get("network_fine") is None else obj["network_fine"]
        dev = next(net.parameters()).device
        total, chunk = n ** 3, 1 << 20
        volume = torch.empty(total, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            for start in range(0, total, chunk):
                cnt = min(chunk, total - start)
                xyz = mesh.grid_points(*ranges, n, start, cnt, device=dev)
                volume[start:start + cnt] = dnerf_field(net, cnt, float(frame_time), xyz=xyz, sigma_only=True, want_dx=False)["sigma"]
        volume = volume.view(n, n, n)
    else:                                                                        # nerf_pl
        models, embeddings = _object_system(obj)
        model = models["fine"] if "fine" in models else models["coarse"]
        volume = mesh.density_grid(model, embeddings["xyz"], *ranges, n)
    # both routes index the volume [y, x, z] (numpy.meshgrid's "xy" order, mesh.grid_points): the bits want [z, y, x]
    volume = volume.permute(2, 0, 1).contiguous()
    bits, _ = occupancy_bits(volume, sigma_min, dilate)
    return ObjectBounds(lo, hi, (res, res, res), bits)
