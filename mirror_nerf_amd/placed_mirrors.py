"""Several new mirrors in one scene, on any plane: `batched_inference(..., new_mirrors=[PlacedMirror(...), ...])`.

app_place_new_mirror of the reference places exactly one mirror on a plane x = c or y = c (`new_mirror=` follows it).  A
PlacedMirror is either that axis-aligned mirror (`PlacedMirror.axis_aligned`, the keys of `new_mirror=`) or a mirror on any
plane, given by a centre, a normal, an up direction and a size; its shape is the rectangle or the ellipse inscribed in it.  A
list of 1..MAX_MIRRORS of them is applied at every recursion level below the last, right behind the threshold of the mirror
mask, by one rule (include/mnrf.h mnrf_place_mirrors):

    every mirror is tested against the level's depth as it is before any mirror of the call; per ray the nearest hit wins, an
    exact tie goes to the later mirror of the list, and the winner alone writes the ray's x_surface, depth and normal.

One deliberate difference from the single mirror: the reference writes the plane's normal to every ray inside the rectangle
BEFORE its two filters (eval.py:458-460), so a second mirror behind the first would overwrite the normal of rays that hit the
first.  Here the normal of a ray that is inside a shape but takes no mirror is kept.  The device pass is mnrf_place_mirrors,
one launch for the whole list.

A mirror may be frosted: `roughness` is the standard deviation of the normal jitter of the rays that take it, read by
`batched_inference(rough_times=T, scene_roughness=S)` alone (include/mnrf.h "A roughness per mirror"): those rays
get the mean of T + 1 reflections about jittered normals, the rays of a polished mirror are traced once.  roughness_row packs the
list's values for mnrf_rough_rows; without rough_times a list that holds a frosted mirror is refused.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .placed_objects import SINGLE_OBJECT_KEYWORDS

__all__ = ["PlacedMirror", "MAX_MIRRORS", "pack", "place_mirrors", "mirror_sources", "roughness_row", "PLACE_MIRROR_PRESETS",
           "resolve_new_mirror"]

MAX_MIRRORS = 8      # MNRF_MIRRORS_MAX
SHAPES = ("rect", "ellipse")

# app_place_new_mirror presets (eval.py:369-433), restated as data: the first entry whose key is a substring of args.root_dir
# wins (None: the reference's `else`).  position: the plane x = position (plane_x) or y = position (plane_y); rect: the
# rectangle (u0, u1, w0, w1) on the plane's (y, z) resp. (x, z).  The livingroom plane_y preset assigns position and rectangle
# twice (eval.py:421-425): the last assignment is the one the reference uses.
PLACE_MIRROR_PRESETS = {
    "plane_x": (
        ("livingroom", dict(position=0.0, normal=(-1.0, 0.0, 0.0), rect=(-1.0, 1.0, -0.5, 0.5))),     # eval.py:370-374
        ("washroom", dict(position=-1.0, normal=(1.0, 0.0, 0.0), rect=(-1.0, 1.0, -1.0, 0.75))),      # eval.py:375-378
        ("office", dict(position=1.0, normal=(1.0, 0.0, 0.0), rect=(-1.0, 1.0, -1.0, 0.75))),         # eval.py:379-382
        (None, dict(position=-1.0, normal=(1.0, 0.0, 0.0), rect=(-1.0, 1.0, -0.5, 0.5))),             # eval.py:383-386
    ),
    "plane_y": (
        ("washroom", dict(position=1.3, normal=(0.0, -1.0, 0.0), rect=(-1.0, 1.0, -1.0, 1.0))),       # eval.py:416-419
        ("livingroom", dict(position=1.65, normal=(0.0, -1.0, 0.0), rect=(-0.3, 1.5, -0.5, 1.0))),    # eval.py:420-425
        ("office", dict(position=0.0, normal=(0.0, -1.0, 0.0), rect=(-1.0, 1.0, -0.5, 0.5))),         # eval.py:426-429
        (None, dict(position=1.0, normal=(0.0, -1.0, 0.0), rect=(-1.0, 1.0, -0.5, 0.5))),             # eval.py:430-433
    ),
}


def resolve_new_mirror(args, new_mirror=None):
    """The plane of app_place_new_mirror: dict(axis="x"|"y", position, normal (3,), rect (u0, u1, w0, w1)).  `new_mirror`
    (same keys) overrides the preset that args.plane_pos / args.root_dir select (eval.py:369-433)."""
    if new_mirror is not None:
        nm = dict(new_mirror)
        missing = {"axis", "position", "normal", "rect"} - set(nm)
        if missing:
            raise ValueError(f"new_mirror needs the keys axis, position, normal, rect (missing: {sorted(missing)})")
        if nm["axis"] not in ("x", "y"):
            raise ValueError(f"new_mirror axis must be 'x' or 'y', not {nm['axis']!r}")
        if len(nm["normal"]) != 3 or len(nm["rect"]) != 4:
            raise ValueError("new_mirror normal has 3 entries and rect 4 (u0, u1, w0, w1)")
        return dict(axis=nm["axis"], position=float(nm["position"]), normal=tuple(float(v) for v in nm["normal"]),
                    rect=tuple(float(v) for v in nm["rect"]))
    plane_pos = getattr(args, "plane_pos", "plane_x")            # eval.py get_opt: default plane_x
    if plane_pos not in PLACE_MIRROR_PRESETS:
        raise ValueError(f"args.plane_pos must be 'plane_x' or 'plane_y', not {plane_pos!r}")
    p = _lib.preset(PLACE_MIRROR_PRESETS[plane_pos], getattr(args, "root_dir", ""))
    return dict(axis=plane_pos[-1], **p)


def _f32(v):
    return float(np.float32(v))


def _vec(v, n, what):
    try:
        a = np.asarray(v, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"PlacedMirror: {what} holds {n} numbers, not {v!r}") from None
    if a.shape != (n,):
        raise ValueError(f"PlacedMirror: {what} holds {n} numbers, not {v!r}")
    if not np.isfinite(a).all():
        raise ValueError(f"PlacedMirror: {what} must be finite, not {v!r}")
    return a


def _roughness(v, what="PlacedMirror: roughness"):
    """A standard deviation of the normal jitter: rounded once to float32; refused when negative, NaN or infinite."""
    try:
        s = np.float32(v)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"{what} is one number, not {v!r}") from None
    if np.ndim(s) != 0 or not np.isfinite(s) or s < 0:
        raise ValueError(f"{what} must be finite and not negative, not {v!r}")
    return float(s)


class PlacedMirror:
    """One mirror of `new_mirrors=`.

    PlacedMirror(center, normal, up, size=(width, height), shape="rect" | "ellipse", roughness=0.0): the plane through `center` with normal
    `normal` (the side the mirror faces); `up` fixes the rotation about the normal -- the height runs along the part of `up` that
    lies in the plane, the width along cross(that, normal).  The frame is built in float64 and rounded once to float32:
        n = normal / |normal|,  e_w = normalize(up - (up . n) n),  e_u = normalize(cross(e_w, n)),
        rect = (-width / 2, width / 2, -height / 2, height / 2) in (u, w).
    The float64 frame stays in .frame64 (rows n, e_u, e_w).  Refused: a zero normal, an up parallel to the normal, a size that is
    not positive, input that is not finite.

    PlacedMirror.axis_aligned(axis, position, normal, rect, shape="rect", roughness=0.0): the mirror of `new_mirror=`, on the
    plane x = position (axis "x", rect = (y0, y1, z0, z1)) or y = position (axis "y", rect = (x0, x1, z0, z1)); `normal` is what
    is written to the rays that take it, as given.

    roughness: the standard deviation of the normal jitter of the rays that take this mirror (0: polished), rounded once to
    float32 and kept as .roughness; negative, NaN and infinite are refused.  It is used by `batched_inference(rough_times=T)`
    alone -- a call without rough_times refuses a list that holds a mirror with roughness > 0.  It is not a key
    of as_dict(): mnrf_place_mirrors does not receive it."""

    def __init__(self, center, normal, up, size, shape="rect", roughness=0.0):
        if shape not in SHAPES:
            raise ValueError(f"PlacedMirror: shape must be 'rect' or 'ellipse', not {shape!r}")
        self.roughness = _roughness(roughness)
        c, n, up, size = _vec(center, 3, "center"), _vec(normal, 3, "normal"), _vec(up, 3, "up"), _vec(size, 2, "size")
        if not (size > 0.0).all():
            raise ValueError(f"PlacedMirror: size = (width, height) must be positive, not {tuple(size)}")
        length = np.linalg.norm(n)
        if not length > 0.0:
            raise ValueError("PlacedMirror: the normal is zero")
        n = n / length
        up = up / max(np.linalg.norm(up), np.finfo(np.float64).tiny)
        e_w = up - np.dot(up, n) * n
        length = np.linalg.norm(e_w)
        if not length > 1e-8:
            raise ValueError("PlacedMirror: up is parallel to the normal (or zero): it does not fix the mirror's rotation about it")
        e_w = e_w / length
        e_u = np.cross(e_w, n)
        e_u = e_u / np.linalg.norm(e_u)
        self.kind, self.shape = "frame", shape
        self.frame64 = np.stack([n, e_u, e_w])
        self.center = tuple(_f32(v) for v in c)
        self.normal = tuple(_f32(v) for v in n)
        self.e_u = tuple(_f32(v) for v in e_u)
        self.e_w = tuple(_f32(v) for v in e_w)
        self.rect = (_f32(-size[0] / 2), _f32(size[0] / 2), _f32(-size[1] / 2), _f32(size[1] / 2))
        self.axis, self.position = None, None

    @classmethod
    def axis_aligned(cls, axis, position, normal, rect, shape="rect", roughness=0.0):
        if shape not in SHAPES:
            raise ValueError(f"PlacedMirror: shape must be 'rect' or 'ellipse', not {shape!r}")
        if axis not in ("x", "y"):
            raise ValueError(f"PlacedMirror: axis must be 'x' or 'y', not {axis!r}")
        n, rect = _vec(normal, 3, "normal"), _vec(rect, 4, "rect")
        position = _vec([position], 1, "position")[0]
        self = cls.__new__(cls)
        self.roughness = _roughness(roughness)
        self.kind, self.shape, self.frame64 = "axis", shape, None
        self.axis, self.position = axis, _f32(position)
        self.normal = tuple(_f32(v) for v in n)
        self.rect = tuple(_f32(v) for v in rect)
        self.center = self.e_u = self.e_w = (0.0, 0.0, 0.0)
        return self

    def as_dict(self):
        """The mirror as the C entry point receives it (every number a float32 value)."""
        return dict(kind=self.kind, shape=self.shape, axis=self.axis, position=self.position, center=self.center, normal=self.normal,
                    e_u=self.e_u, e_w=self.e_w, rect=self.rect)

    def __repr__(self):
        rough = f", roughness={self.roughness}" if self.roughness != 0 else ""
        if self.kind == "axis":
            return f"PlacedMirror.axis_aligned({self.axis!r}, {self.position}, normal={self.normal}, rect={self.rect}, shape={self.shape!r}{rough})"
        return f"PlacedMirror(center={self.center}, normal={self.normal}, e_u={self.e_u}, e_w={self.e_w}, rect={self.rect}, shape={self.shape!r}{rough})"


def refuse(args, models, kwargs):
    """The refusals of `new_mirrors=`, each with its reason.  What the list is allowed beside -- placed_objects= and
    app_reflection_substitution -- keeps its own refusals (recursion._refuse_apps goes on with them)."""
    mirrors = kwargs["new_mirrors"]
    if isinstance(mirrors, PlacedMirror) or not isinstance(mirrors, (list, tuple)):
        raise TypeError(f"new_mirrors must be a list of PlacedMirror, not {type(mirrors).__name__}")
    if not 1 <= len(mirrors) <= MAX_MIRRORS:
        raise ValueError(f"new_mirrors holds 1..{MAX_MIRRORS} mirrors (MNRF_MIRRORS_MAX), not {len(mirrors)}")
    for k, m in enumerate(mirrors):
        if not isinstance(m, PlacedMirror):
            raise TypeError(f"new_mirrors[{k}] must be a PlacedMirror, not {type(m).__name__}")
    if getattr(args, "app_place_new_mirror", False) or kwargs.get("new_mirror") is not None:
        raise ValueError("new_mirrors= carries every mirror of the call: it cannot be combined with app_place_new_mirror or new_mirror= "
                         "(the single mirror; PlacedMirror.axis_aligned takes its keys)")
    given = [k for k in SINGLE_OBJECT_KEYWORDS if kwargs.get(k) is not None]
    if given or (getattr(args, "app_reflect_newly_placed_objects", False) and kwargs.get("placed_objects") is None):
        raise ValueError("new_mirrors= is combined with objects through placed_objects=[PlacedObject(...), ...], not with the "
                         f"single-object keywords ({', '.join(k + '=' for k in given) or 'app_reflect_newly_placed_objects without placed_objects='})")
    if getattr(args, "app_control_mirror_roughness", False):
        raise ValueError("app_control_mirror_roughness cannot be combined with new_mirrors= (one application at a time, except "
                         "placed mirrors with placed objects or substitution)")
    if not any(getattr(m, "predict_mirror_mask", False) for m in models.values()):
        raise ValueError("new_mirrors= needs a mirror-mask head (predict_mirror_mask=True): the new mirror is merged into the "
                         "predicted mirror mask, and substitution replaces what the mask marks")
    if getattr(args, "near", None) is None:
        raise ValueError("new_mirrors= needs args.near: the foreground test compares the depth with it (eval.py:169-171)")
    if kwargs.get("rough_times") is None:
        for k, m in enumerate(mirrors):
            if getattr(m, "roughness", 0.0) > 0:
                raise ValueError(f"new_mirrors[{k}] has roughness {m.roughness}, which only the per-mirror roughness route reads: pass "
                                 "rough_times=T (the number of jittered reflections beside the first) to batched_inference")


def roughness_row(mirrors):
    """The host array of mnrf_rough_rows for a list of PlacedMirror (or none): (K, roughness[K])."""
    K = len(mirrors) if mirrors is not None else 0
    row = (ctypes.c_float * max(K, 1))()
    for k in range(K):
        row[k] = mirrors[k].roughness
    return K, row


def pack(mirrors):
    """The host arrays of mnrf_place_mirrors for a list of PlacedMirror: (K, kinds, shapes, axes, positions, frames, normals, rects)."""
    K = len(mirrors)
    kinds, shapes, axes = (ctypes.c_int * K)(), (ctypes.c_int * K)(), (ctypes.c_int * K)()
    positions, frames = (ctypes.c_float * K)(), (ctypes.c_float * (9 * K))()
    normals, rects = (ctypes.c_float * (3 * K))(), (ctypes.c_float * (4 * K))()
    for k, m in enumerate(mirrors):
        kinds[k] = _lib.MNRF_MIRROR_AXIS if m.kind == "axis" else _lib.MNRF_MIRROR_FRAME
        shapes[k] = _lib.MNRF_MIRROR_ELLIPSE if m.shape == "ellipse" else _lib.MNRF_MIRROR_RECT
        axes[k] = _lib.MNRF_PLANE_Y if m.axis == "y" else _lib.MNRF_PLANE_X
        positions[k] = m.position if m.position is not None else 0.0
        frames[9 * k:9 * k + 9] = m.center + m.e_u + m.e_w
        normals[3 * k:3 * k + 3] = m.normal
        rects[4 * k:4 * k + 4] = m.rect
    return K, kinds, shapes, axes, positions, frames, normals, rects


def place_mirrors(rays, packed, near, depth, mask, normal, x_surface, mask_bool=None, flag=None, index=None, source=None):
    """mnrf_place_mirrors on one level's rays (N, 8) and maps, in place.  packed: pack(mirrors); mask_bool: (N,) torch.bool or
    None; flag: device int32 of one element, OR-ed with "any merged ray", or None; index: (N,) int32 or None.
    rays of another precision or layout are converted; the maps, mask_bool, flag and index are written: float32 (mask_bool an
    8-bit type, flag and index int32) and contiguous, or refused.
    source: (N,) integers, the placed mirror each ray left at the level above (-1: none), which the ray cannot hit
    (mnrf_place_mirrors_from; converted to int32 like any input), or None: mnrf_place_mirrors itself."""
    for name, t in (("depth", depth), ("mask", mask), ("normal", normal), ("x_surface", x_surface)):
        _lib.written(t, _lib.F32, name)
    _lib.written(mask_bool, _lib.BYTE, "mask_bool")
    _lib.written(flag, _lib.I32, "flag")
    _lib.written(index, _lib.I32, "index")
    if source is not None and tuple(source.shape) != (rays.shape[0],):
        raise ValueError(f"source holds one mirror index per ray, ({rays.shape[0]},), not {tuple(source.shape)}")
    _place_mirrors(_lib.f32_in(rays), packed, near, depth, mask, normal, x_surface, mask_bool, flag, index, _lib.i32_in(source), source is not None)


def _place_mirrors(rays, packed, near, depth, mask, normal, x_surface, mask_bool, flag, index, source=None, exclude=False):
    """place_mirrors for the driver, whose tensors are float32 / int32 rows already.  exclude: the launch is
    mnrf_place_mirrors_from, with `source` ((N,) int32, or None where no ray of the level has one)."""
    p = _lib.ptr
    K, kinds, shapes, axes, positions, frames, normals, rects = packed
    head = (p(rays), rays.shape[0], K, kinds, shapes, axes, positions, frames, normals, rects, float(near))
    tail = (p(depth), p(mask), p(normal), p(x_surface), ctypes.c_void_p(mask_bool.data_ptr()) if mask_bool is not None else None,
            p(flag), p(index), _lib.stream())
    if exclude:
        _lib.check(_lib.lib().mnrf_place_mirrors_from(*head, p(source), *tail), "mnrf_place_mirrors_from")
    else:
        _lib.check(_lib.lib().mnrf_place_mirrors(*head, *tail), "mnrf_place_mirrors")


def _edit_level(r, rays_chunk, sel, launch):
    """What placing one mirror and placing a list share, on one level's maps in place: the maps the launch writes are made
    contiguous, launch(depth, mask, normal, x_surface, merged) runs, the returned mirror mask becomes the merged bool tensor
    (eval.py:492-496) and depth_fine the edited depth (eval.py:497-500).  The normal is the composited predicted one, else the
    composited grad normal (eval.py:338-360); -> the level's float mask."""
    for k in (f"depth_{sel}", f"x_surface_{sel}", f"surface_normal_{sel}", f"surface_normal_grad_{sel}"):
        if k in r and not r[k].is_contiguous():
            r[k] = r[k].contiguous()
    mkey = next(k for k in (f"mirror_mask_{sel}", "mirror_mask_fine", "mirror_mask_coarse") if k in r)
    mask, depth = r[mkey], r[f"depth_{sel}"]
    merged = torch.empty(rays_chunk.shape[0], dtype=torch.bool, device=rays_chunk.device)
    normal = r[f"surface_normal_{sel}"] if f"surface_normal_{sel}" in r else r[f"surface_normal_grad_{sel}"]
    launch(depth, mask, normal, r[f"x_surface_{sel}"], merged)
    r["mirror_mask_fine" if "mirror_mask_fine" in r else "mirror_mask_coarse"] = merged
    if "depth_fine" in r:
        r["depth_fine"] = depth
    elif "depth_coarse" in r:
        r["depth_coarse"] = depth
    return mask


def _place_mirror_level(r, rays_chunk, sel, plane, near, flag):
    """eval.py:364-504 on one level's maps, in place (mnrf_place_mirror, _edit_level); `flag` (device int32) is OR-ed with "any
    mirror after the merge"."""
    def launch(depth, mask, nrm, x_surface, merged):
        p = _lib.ptr
        nx, ny, nz = plane["normal"]
        u0, u1, w0, w1 = plane["rect"]
        _lib.check(_lib.lib().mnrf_place_mirror(
            p(rays_chunk), rays_chunk.shape[0], _lib.MNRF_PLANE_Y if plane["axis"] == "y" else _lib.MNRF_PLANE_X, plane["position"],
            nx, ny, nz, u0, u1, w0, w1, float(near), p(depth), p(mask), p(nrm), p(x_surface), ctypes.c_void_p(merged.data_ptr()),
            p(flag), _lib.stream()), "mnrf_place_mirror")
    return _edit_level(r, rays_chunk, sel, launch)


def _place_mirrors_level(r, rays_chunk, sel, packed, near, flag, index, source=None, exclude=False):
    """The K-mirror rule on one level's maps, in place (mnrf_place_mirrors, _edit_level) for the mirrors `packed` (pack); index:
    (N,) int32 that receives the mirror each ray took, or None.  exclude: mnrf_place_mirrors_from with the level's `source`
    ((N,) int32: the placed mirror each ray left at the level above, which it cannot hit; None: no ray has one)."""
    return _edit_level(r, rays_chunk, sel, lambda depth, mask, nrm, x_surface, merged: _place_mirrors(
        rays_chunk, packed, near, depth, mask, nrm, x_surface, merged, flag, index, source, exclude))


def mirror_sources(level_index, compaction_index, m, n_rep=1, device=None):
    """The `source` row of the next level (mnrf_mirror_sources): (n_rep * m,) int32 with row j * m + p =
    level_index[compaction_index[p]].  level_index: the (N,) int32 index this level's mnrf_place_mirrors wrote, or None (-1
    everywhere); compaction_index: (m,) int32 rows of it, or None (p itself); device: where the row is made when both are None."""
    given = level_index if level_index is not None else compaction_index
    out = torch.empty(n_rep * m, dtype=torch.int32, device=given.device if given is not None else device)
    p = _lib.ptr
    _lib.check(_lib.lib().mnrf_mirror_sources(p(level_index), p(compaction_index), m, n_rep, p(out), _lib.stream()), "mnrf_mirror_sources")
    return out


def refuse_source(kwargs):
    """The refusals of exclude_source_mirror= and source_mirror= that need no look at the rays, each with its reason."""
    on = kwargs.get("exclude_source_mirror", False)
    if not isinstance(on, (bool, np.bool_)):
        raise ValueError(f"exclude_source_mirror is a bool, not {on!r}")
    if on and kwargs.get("new_mirrors") is None:
        raise ValueError("exclude_source_mirror=True keeps a ray from hitting the placed mirror it has just left: it needs new_mirrors=")
    if kwargs.get("source_mirror") is not None and not on:
        raise ValueError("source_mirror= is read by exclude_source_mirror=True alone (the placed mirror each ray of the call left)")


def resolve_source(kwargs, rays):
    """exclude_source_mirror=, source_mirror= -> (on, the (N,) int32 source of the call's own rays or None: all -1).  The tensor is an
    input, but one that says what it is by its dtype: another dtype, shape or device is refused, another layout is converted."""
    refuse_source(kwargs)
    on, source = bool(kwargs.get("exclude_source_mirror", False)), kwargs.get("source_mirror")
    if source is None:
        return on, None
    if not isinstance(source, torch.Tensor) or source.dtype != torch.int32:
        raise ValueError("source_mirror must be an int32 tensor (an index into new_mirrors= per ray, -1 for none), not "
                         f"{getattr(source, 'dtype', type(source).__name__)}")
    if tuple(source.shape) != (rays.shape[0],):
        raise ValueError(f"source_mirror holds one index per ray of the call, ({rays.shape[0]},), not {tuple(source.shape)}")
    if source.device != rays.device:
        raise ValueError(f"source_mirror is on {source.device}, the rays are on {rays.device}")
    return on, source.contiguous()
