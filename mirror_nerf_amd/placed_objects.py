"""Several placed objects in one scene: `batched_inference(..., placed_objects=[PlacedObject(...), ...])`.

app_reflect_newly_placed_objects of the reference places exactly one object; the single-object keywords of batched_inference
(system_obj= / render_kwargs_test_d_nerf=, new_object=, object_bounds=) follow it.  A PlacedObject carries what those keywords
carry for ONE object -- its field, its placement, optionally its bounds and, for a D-NeRF object, its own time -- and a list of
1..MAX_OBJECTS of them is rendered at every recursion level by one rule:

    for k = 0 .. K-1 in list order, the single-object merge of object k is applied to the ray's current (rgb, depth, mask),
    current meaning as left by the scene and by the objects 0 .. k-1.

That is the chain of K single-object applications, by definition.  The merge writes depth = d, so the nearest opaque object
wins; an exact tie in depth goes to the later object of the list; a current depth <= near hides nothing, as in the reference's
own rule (eval.py:275-281).  The device passes are mnrf_objects_cull (all K objects' bounds against a level's rays in two
launches, ONE read of the K counts) and mnrf_objects_merge (one launch); per object they evaluate the device functions of the
single-object kernels, so the result is that chain bit for bit.
"""
import ctypes
from types import SimpleNamespace

import torch

from . import _lib, checkpoint
from .mirror_nerf import Embedding, MirrorNeRF
from .object_bounds import ObjectBounds, _object_system, estimate_object_bounds

__all__ = ["PlacedObject", "MAX_OBJECTS", "cull_objects", "merge_objects", "OBJECT_PRESETS", "resolve_new_object",
           "resolve_object_bounds", "load_object_system"]

MAX_OBJECTS = 8      # MNRF_OBJECTS_MAX

SINGLE_OBJECT_KEYWORDS = ("system_obj", "render_kwargs_test_d_nerf", "new_object", "object_bounds", "object_region")

# app_reflect_newly_placed_objects presets (eval.py:177-190): how a level's rays are moved into the object's frame.  pose_align
# is None in every branch of the reference (eval.py:177); `new_object=` of batched_inference may give one.
OBJECT_PRESETS = (
    ("livingroom", dict(pose_align=None, scale=2.0, translation=(0.0, 0.0, 0.0))),                          # eval.py:180-184
    ("washroom", dict(pose_align=None, scale=2.0, translation=(-0.5, -0.5, 0.0))),                          # eval.py:185-187
    ("office", dict(pose_align=None, scale=2.0, translation=(0.0, 3.0, 0.5))),                              # eval.py:188-190
    (None, dict(pose_align=None, scale=1.0, translation=(0.0, 0.0, 0.0))),                                  # eval.py:178-179
)


def resolve_new_object(args, new_object=None):
    """The ray move of app_reflect_newly_placed_objects: dict(pose (12 floats, the row-major 3x4 [A | p], or None), scale,
    translation (3,), pose_scale0).  `new_object=dict(pose_align=None | 3x4 | 4x4, scale=, translation=)` overrides the preset
    that args.root_dir selects (eval.py:177-190).  pose_scale0 is the fp32 norm of the first column of A (eval.py:194-196) and
    1 without a pose: the reference leaves `pose_scale` unbound there (eval.py:264), and no alignment is a scale of 1."""
    if new_object is not None:
        cfg = dict(new_object)
        missing = {"pose_align", "scale", "translation"} - set(cfg)
        if missing:
            raise ValueError(f"new_object needs the keys pose_align, scale, translation (missing: {sorted(missing)})")
    else:
        cfg = _lib.preset(OBJECT_PRESETS, getattr(args, "root_dir", ""))
    if len(cfg["translation"]) != 3:
        raise ValueError("new_object translation has 3 entries")
    scale = float(cfg["scale"])
    if not scale > 0.0:
        raise ValueError(f"new_object scale must be positive, not {cfg['scale']!r}")
    pose, pose_scale0 = None, 1.0
    if cfg["pose_align"] is not None:
        m = torch.as_tensor(cfg["pose_align"], dtype=torch.float32)            # eval.py:193 (FloatTensor)
        if tuple(m.shape) not in ((3, 4), (4, 4)):
            raise ValueError(f"new_object pose_align must be None, 3x4 or 4x4, not {tuple(m.shape)}")
        pose = tuple(float(v) for v in m[:3, :4].reshape(-1))
        pose_scale0 = float(torch.norm(m[:3, 0]))                              # eval.py:194-196, the only entry that is read
        if not pose_scale0 > 0.0:
            raise ValueError("new_object pose_align: the first column of its 3x3 is zero")
    return dict(pose=pose, scale=scale, translation=tuple(float(v) for v in cfg["translation"]), pose_scale0=pose_scale0)


def load_object_system(ckpt_path, device, N_importance=64, trusted=False):
    """The object of app_reflect_newly_placed_objects from a nerf_pl checkpoint (eval.py:1041-1061): the pair of plain NeRF
    fields -- MirrorNeRF without the optional heads, whose parameter names are nerf_pl's (models/nerf_pl/nerf_nerfpl.py:42-109)
    -- filled from `nerf_coarse.*` and, with N_importance > 0, `nerf_fine.*`; .models / .embeddings are dicts."""
    models = {}
    for key in ("coarse", "fine") if N_importance > 0 else ("coarse",):
        m = MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=False, predict_mirror_mask=False)
        checkpoint.load_ckpt(m, ckpt_path, model_name="nerf_" + key, trusted=trusted)
        models[key] = m.to(device).eval()
    return SimpleNamespace(models=models, embeddings={"xyz": Embedding(10), "dir": Embedding(4)})


def resolve_object_bounds(bounds, region, res, kind, field, time, device):
    """`object_bounds=` (with object_region=, object_bounds_res=) of batched_inference, or bounds= (region=, bounds_res=) of a
    PlacedObject -> an ObjectBounds on `device`, or None.  kind: "nerf_pl" / "d_nerf", the object `field` is (None: the
    application is not on).  "auto" estimates the bounds from the object's own density inside region=(lo, hi) at res cells per
    axis (object_bounds.estimate_object_bounds): once for a nerf_pl object, kept on the field (its system_obj); per call, at
    `time`, for a D-NeRF object, which moves."""
    if bounds is None:
        if region is not None:
            raise ValueError("object_region= is the region object_bounds='auto' looks for the object in: pass object_bounds='auto'")
        return None
    if kind is None:
        raise ValueError("object_bounds= bounds the object of app_reflect_newly_placed_objects: the application is not on")
    if isinstance(bounds, ObjectBounds):
        return bounds.to(device)
    if not (isinstance(bounds, str) and bounds == "auto"):
        raise ValueError(f"object_bounds must be None, an ObjectBounds or 'auto', not {bounds!r}")
    if region is None or len(region) != 2:
        raise ValueError("object_bounds='auto' needs object_region=(lo, hi): the box of the object's frame to look for it in")
    lo, hi = (tuple(float(v) for v in c) for c in region)
    if kind == "d_nerf":
        return estimate_object_bounds(field, lo, hi, res=res, frame_time=time).to(device)
    key = (lo, hi, res, str(device))
    cached = getattr(field, "_mnrf_object_bounds", None)
    if cached is None or cached[0] != key:
        cached = (key, estimate_object_bounds(field, lo, hi, res=res).to(device))
        try:
            field._mnrf_object_bounds = cached
        except AttributeError:      # (an object without a __dict__: estimated per call)
            pass
    return cached[1]


class PlacedObject:
    """One object of `placed_objects=`.

    field: a nerf_pl `system_obj` (.models and .embeddings, load_object_system) or a `render_kwargs_test_d_nerf` dict
    (dnerf.load_dnerf_object); the kind is taken from the type.
    placement: what `new_object=` takes, dict(pose_align=None | 3x4 | 4x4, scale=, translation=); None: the args.root_dir preset
    of the call (resolve_new_object, with its refusals).
    bounds: None (every ray of a level renders the object), an ObjectBounds, or "auto" with region=(lo, hi) and bounds_res
    cells per axis (resolve_object_bounds: estimated once and kept on a nerf_pl object, per call at the object's
    time for a D-NeRF object).
    time: a D-NeRF object's own time; None: the call's frame_time=, which is then required."""

    def __init__(self, field, placement, bounds=None, region=None, bounds_res=64, time=None):
        if isinstance(field, dict):
            if field.get("network_fn") is None:
                raise TypeError("PlacedObject: a dict field is a render_kwargs_test_d_nerf (dnerf.load_dnerf_object): it has no network_fn")
            self.kind = "d_nerf"
        elif hasattr(field, "models") and hasattr(field, "embeddings"):
            self.kind = "nerf_pl"
        else:
            raise TypeError("PlacedObject: field must be a nerf_pl system_obj (.models and .embeddings, load_object_system) or a "
                            f"render_kwargs_test_d_nerf dict (dnerf.load_dnerf_object), not {type(field).__name__}")
        self.field = field
        if placement is not None:
            resolve_new_object(None, placement)          # its refusals, now and not at the first frame
        self.placement = placement
        if bounds is None:
            if region is not None:
                raise ValueError("PlacedObject: region= is the region bounds='auto' looks for the object in: pass bounds='auto'")
        elif isinstance(bounds, str) and bounds == "auto":
            if region is None or len(region) != 2:
                raise ValueError("PlacedObject: bounds='auto' needs region=(lo, hi): the box of the object's frame to look for it in")
        elif not isinstance(bounds, ObjectBounds):
            raise ValueError(f"PlacedObject: bounds must be None, an ObjectBounds or 'auto', not {bounds!r}")
        self.bounds, self.region, self.bounds_res = bounds, region, bounds_res
        if time is not None:
            if self.kind != "d_nerf":
                raise ValueError("PlacedObject: time= is a D-NeRF object's time; a nerf_pl object does not move")
            time = float(time)
        self.time = time

    def __repr__(self):
        return f"PlacedObject({self.kind}, placement={self.placement!r}, bounds={self.bounds!r}, time={self.time!r})"

    def resolve(self, args, frame_time, device):
        """What one call needs of this object: dict(kind, field, xform, bounds, time)."""
        time = None
        if self.kind == "d_nerf":
            time = self.time if self.time is not None else frame_time
            if time is None:
                raise ValueError("placed_objects: a D-NeRF object without time= needs frame_time= (the object's time in [0, 1])")
            time = float(time)
        bounds = resolve_object_bounds(self.bounds, self.region, self.bounds_res, self.kind, self.field, time, device)
        return dict(kind=self.kind, field=self.field, xform=resolve_new_object(args, self.placement), bounds=bounds, time=time)


def refuse(args, models, kwargs):
    """The refusals of `placed_objects=`, each with its reason; the conditions of the single-object path that do not name an
    object hold here too."""
    placed = kwargs["placed_objects"]
    given = [k for k in SINGLE_OBJECT_KEYWORDS if kwargs.get(k) is not None]
    if given:
        raise ValueError(f"placed_objects= carries every object's field, placement and bounds: it cannot be combined with "
                         f"{', '.join(k + '=' for k in given)} (the single-object keywords)")
    if not getattr(args, "app_reflect_newly_placed_objects", False):
        raise ValueError("placed_objects= lists the objects of app_reflect_newly_placed_objects: the application is not on")
    if isinstance(placed, PlacedObject) or not isinstance(placed, (list, tuple)):
        raise TypeError(f"placed_objects must be a list of PlacedObject, not {type(placed).__name__}")
    if not 1 <= len(placed) <= MAX_OBJECTS:
        raise ValueError(f"placed_objects holds 1..{MAX_OBJECTS} objects (MNRF_OBJECTS_MAX), not {len(placed)}")
    for k, obj in enumerate(placed):
        if not isinstance(obj, PlacedObject):
            raise TypeError(f"placed_objects[{k}] must be a PlacedObject, not {type(obj).__name__}")
        if obj.kind == "d_nerf" and obj.time is None and kwargs.get("frame_time") is None:
            raise ValueError(f"placed_objects[{k}] is a D-NeRF object without time=: it needs frame_time= (the object's time in "
                             "[0, 1], eval.py:1130, 1154)")
    for other in ("app_place_new_mirror", "app_reflection_substitution", "app_control_mirror_roughness"):
        if getattr(args, other, False):
            raise ValueError(f"app_reflect_newly_placed_objects cannot be combined with {other} (one application at a time)")
    if not ("fine" in models and kwargs.get("_N_importance", 1) > 0 and not getattr(args, "only_one_field", False)
            and getattr(models["fine"], "predict_mirror_mask", False)):
        raise ValueError("app_reflect_newly_placed_objects needs a fine mirror mask (N_importance > 0, not only_one_field, "
                         "predict_mirror_mask=True): the reference clears mirror_mask_fine where the object is seen "
                         "(eval.py:291)")
    if getattr(args, "near", None) is None:
        raise ValueError("app_reflect_newly_placed_objects needs args.near: the occlusion test compares the depth with it "
                         "(eval.py:169-171, 275-281)")


def cull_objects(rays, placed):
    """mnrf_objects_cull on one level's rays (N, 8) for the resolved objects `placed` (PlacedObject.resolve) ->
    (out_rays (K, N, 8), index (K, N) int32, slot (K, N) int32, counts (K,) int32 on the device): per object what
    ObjectBounds.cull returns -- for an object without bounds every ray, in order -- and slot, the inverse of index (-1: the
    ray is not in the object's list).  rays of another precision or layout are converted."""
    return _cull_objects(_lib.f32_in(rays), placed)


def _cull_objects(rays, placed):
    """cull_objects for the driver, whose rays are float32 rows already."""
    K, N, dev = len(placed), rays.shape[0], rays.device
    posed, poses, scales, trans = (ctypes.c_int * K)(), (ctypes.c_float * (12 * K))(), (ctypes.c_float * K)(), (ctypes.c_float * (3 * K))()
    unbounded, lo, hi, res = (ctypes.c_int * K)(), (ctypes.c_float * (3 * K))(), (ctypes.c_float * (3 * K))(), (ctypes.c_int * (3 * K))()
    bits = (ctypes.c_void_p * K)()
    for k, o in enumerate(placed):
        x, b = o["xform"], o["bounds"]
        posed[k] = x["pose"] is not None
        if x["pose"] is not None:
            poses[12 * k:12 * k + 12] = x["pose"]
        scales[k] = x["scale"]
        trans[3 * k:3 * k + 3] = x["translation"]
        unbounded[k] = b is None
        res[3 * k:3 * k + 3] = (1, 1, 1)
        if b is not None:
            if b.bits is not None and b.bits.device != dev:
                raise ValueError(f"ObjectBounds: the bits live on {b.bits.device}, the rays on {dev} (use .to(device))")
            lo[3 * k:3 * k + 3], hi[3 * k:3 * k + 3], res[3 * k:3 * k + 3] = b.lo, b.hi, b.res
            bits[k] = b.bits.data_ptr() if b.bits is not None else None
    out = torch.empty(K, N, 8, dtype=torch.float32, device=dev)
    index = torch.empty(K, N, dtype=torch.int32, device=dev)
    slot = torch.empty(K, N, dtype=torch.int32, device=dev)
    counts = torch.zeros(K, dtype=torch.int32, device=dev)
    p = _lib.ptr
    _lib.check(_lib.lib().mnrf_objects_cull(p(rays), N, K, posed, poses, scales, trans, unbounded, lo, hi, res, bits, p(out), p(index),
                                            p(slot), p(counts), _lib.stream()), "mnrf_objects_cull")
    return out, index, slot, counts


def merge_objects(maps, placed, slot, counts, capacity, near, rgb, depth, mask, n_used):
    """mnrf_objects_merge: maps[k] = (rgb, depth, opacity) of object k rendered on its kept rows, or None (not rendered), into
    the level's rgb, depth, mask (None: no mirror head) in place; n_used: (K,) int32 on the device or None.
    The objects' maps, slot and counts are converted where they are of another precision; rgb, depth, mask and n_used are
    written: float32 (n_used int32) and contiguous, or refused."""
    for name, t in (("rgb", rgb), ("depth", depth), ("mask", mask)):
        _lib.written(t, _lib.F32, name)
    _lib.written(n_used, _lib.I32, "n_used")
    maps = [None if m is None else tuple(_lib.f32_in(t) for t in m) for m in maps]
    _merge_objects(maps, placed, _lib.i32_in(slot), _lib.i32_in(counts), capacity, near, rgb, depth, mask, n_used)


def _merge_objects(maps, placed, slot, counts, capacity, near, rgb, depth, mask, n_used):
    """merge_objects for the driver, whose tensors are float32 / int32 rows already."""
    K, N = len(placed), rgb.shape[0]
    tables = [(ctypes.c_void_p * K)() for _ in range(3)]
    hold = []
    for k, m in enumerate(maps):
        if m is None:
            continue
        for table, t in zip(tables, m):
            t = t.contiguous()
            hold.append(t)
            table[k] = t.data_ptr()
    scales = (ctypes.c_float * K)(*[o["xform"]["scale"] for o in placed])
    ps0 = (ctypes.c_float * K)(*[o["xform"]["pose_scale0"] for o in placed])
    p = _lib.ptr
    _lib.check(_lib.lib().mnrf_objects_merge(tables[0], tables[1], tables[2], K, p(slot), p(counts), N, capacity, scales, ps0, float(near),
                                             p(rgb), p(depth), p(mask), p(n_used), _lib.stream()), "mnrf_objects_merge")


# ----------------------------------------------------------------------------- one level of batched_inference
def _contiguous_maps(r):
    """The maps of a level that the merge kernels write, made contiguous in the result dict."""
    for key in ("rgb_fine", "depth_fine", "mirror_mask_fine"):
        if key in r and not r[key].is_contiguous():
            r[key] = r[key].contiguous()


def _merge_object(r, rays_chunk, xform, near, n_used, render, bounds=None):
    """eval.py:173-291 on one level's maps, in place: the level's rays moved into the object's frame (mnrf_object_rays), the
    object field rendered for colour, depth and opacity (`render`: rays -> dict), and its maps merged where the object is
    opaque and not hidden by the scene (mnrf_object_merge).  The mirror flag is cleared there BEFORE the caller's hard clip,
    as in the reference; x_surface and the normals are not edited (the reference does not edit them either).

    bounds (an ObjectBounds): only the rays whose object-frame segment can touch a set cell are rendered -- mnrf_object_cull
    compacts them in order, ONE 4-byte device->host read says how many there are, `render` runs on those rows (not at all when
    there are none) and mnrf_object_merge_indexed applies the same per-ray rule through their index.  The other rays stay as
    the scene rendered them."""
    N = rays_chunk.shape[0]
    if N == 0:
        return
    p = _lib.ptr
    if bounds is not None:
        obj_rays, index, count = bounds._cull(rays_chunk, xform)
        M = int(count.item())
        if M == 0:
            return
        obj_rays = obj_rays[:M]
    else:
        obj_rays = torch.empty_like(rays_chunk)
        pose = (ctypes.c_float * 12)(*xform["pose"]) if xform["pose"] is not None else None
        tx, ty, tz = xform["translation"]
        _lib.check(_lib.lib().mnrf_object_rays(p(rays_chunk), N, pose, xform["scale"], tx, ty, tz, p(obj_rays), _lib.stream()),
                   "mnrf_object_rays")
    o = render(obj_rays)
    _contiguous_maps(r)
    held = [o[k].contiguous() for k in ("rgb_fine", "depth_fine", "opacity_fine")]      # (alive until the launch is queued)
    obj = [p(t) for t in held]
    tail = (xform["scale"], xform["pose_scale0"], float(near), p(r["rgb_fine"]), p(r["depth_fine"]), p(r.get("mirror_mask_fine")),
            p(n_used), _lib.stream())
    if bounds is not None:
        _lib.check(_lib.lib().mnrf_object_merge_indexed(*obj, p(index), p(count), M, *tail), "mnrf_object_merge_indexed")
    else:
        _lib.check(_lib.lib().mnrf_object_merge(*obj, N, *tail), "mnrf_object_merge")


def _merge_placed(r, rays_chunk, placed, near, n_used, renderers):
    """The K-object rule on one level's maps, in place: for k = 0 .. K-1 in list order, _merge_object's per-ray rule of object
    k on the ray's current maps.  ONE mnrf_objects_cull moves and culls the level's rays for every object, ONE device->host
    read brings the K counts, every object with a non-zero count is rendered on its kept rows (renderers[k]: rays -> dict;
    queued back to back, no read in between), ONE mnrf_objects_merge applies the chain.  placed: the resolved objects
    (PlacedObject.resolve); n_used: (K,) int32 on the device or None."""
    N = rays_chunk.shape[0]
    if N == 0:
        return
    obj_rays, _, slot, counts = _cull_objects(rays_chunk, placed)
    host = counts.tolist()                                    # the one read of this chunk and level
    maps = [None] * len(placed)
    for k, M in enumerate(host):
        if M > 0:
            o = renderers[k](obj_rays[k, :M])
            maps[k] = (o["rgb_fine"], o["depth_fine"], o["opacity_fine"])
    if not any(m is not None for m in maps):
        return
    _contiguous_maps(r)
    _merge_objects(maps, placed, slot, counts, N, near, r["rgb_fine"], r["depth_fine"], r.get("mirror_mask_fine"), n_used)
