"""Whitted-style reflected-ray recursion around render_rays, in both rule sets of the reference:

  * `NeRFSystem.forward` / `render_rays_chunk_recursively`  -- TRAIN semantics, train.py:102-348
  * `batched_inference`                                      -- EVAL semantics, eval.py:114-172,
    293-740: the core path, roughness (app_control_mirror_roughness) and the three scene-editing
    applications that need only MirrorNeRF fields -- a new planar mirror (app_place_new_mirror,
    eval.py:311-320, 364-504; run.sh MODE 3), reflection substitution (app_reflection_substitution,
    eval.py:550-613: the reflections are rendered by a second system) and a newly placed object
    (app_reflect_newly_placed_objects, eval.py:173-291; run.sh MODE 4) whose field is a nerf_pl model
    (the plain NeRF this package already runs: MirrorNeRF without the optional heads) or a D-NeRF
    model (a time-conditioned deformation network in front of a canonical NeRF: dnerf.py).

Python here is the recursion driver only: mask thresholding, reflected-ray construction,
order-preserving compaction and blending are the HIP kernels mnrf_threshold_mask,
mnrf_reflect_compact and mnrf_blend_scatter; the applications add mnrf_place_mirror,
mnrf_transform_rays, mnrf_object_rays and mnrf_object_merge (with object bounds: mnrf_object_cull and
mnrf_object_merge_indexed; several objects, placed_objects=: mnrf_objects_cull and mnrf_objects_merge; several mirrors on any
plane, new_mirrors=: mnrf_place_mirrors; with exclude_source_mirror=: mnrf_place_mirrors_from and mnrf_mirror_sources);
roughness adds mnrf_reflect_jitter_fan and mnrf_jitter_mean (a roughness per
mirror, rough_times=: mnrf_rough_rows, mnrf_perturb_normals and mnrf_reflect_jitter_fan_rows beside them).  One 4-byte device->host
read per level decides
whether (and how many) reflected rays are traced -- the reference syncs at the same place
through `mirror_mask.bool().any()` (train.py:175, eval.py:315).
"""
import ctypes
import os
from collections import defaultdict
import weakref
from types import SimpleNamespace

import numpy as np
import torch
from torch import nn

from . import _lib, placed_mirrors, placed_objects
from .mirror_nerf import Embedding, MirrorNeRF, check_guard, release_transient
from .dnerf import render_rays_dnerf
from .rendering import render_rays
# (re-exported: callers reach the presets and resolvers of the applications through this module)
from .object_bounds import _object_system
from .placed_mirrors import PLACE_MIRROR_PRESETS, resolve_new_mirror  # noqa: F401
from .placed_objects import OBJECT_PRESETS, load_object_system, resolve_new_object, resolve_object_bounds  # noqa: F401

RAY_FORWARD_OFFSET = 0.1   # train.py:232, eval.py:529 (absolute near of a reflected ray)
# Share of rays above the mirror threshold from which the blended-level launch is the faster route for a chunk of a level that
# traces (_stage_a): measured, profiles/blended_level_ab.txt section 4 -- 13.60 ms without and 12.55 ms with
# every ray a mirror, against 13.21 ms for the field launch and the compositing launch it replaces
BLENDED_BREAK_EVEN = 0.37
_MIRROR_FRACTION = weakref.WeakKeyDictionary()      # model of the selected pass -> {recursion level: share last counted}
# How the mean over the trace_ray_times + 1 samples of a mirror ray ends (eval.py:671-674 `rgb / (trace_ray_times + 1)`): on the
# device torch evaluates a division by a host scalar as a multiplication by the fp32 reciprocal, and so does mnrf_jitter_mean
# (tests/test_hip_rough_kernels.py compares the kernel with torch's own `/`); the driver forms 1 / (times + 1) in fp32.
ROUGH_FINISH = _lib.MNRF_MEAN_MULTIPLY
JITTER_RAYS = 262144      # rays per batched group of jittered reflections (roughness, eval.py:622-674)

# app_reflection_substitution presets (eval.py:551-591): how the reflected rays are moved into the substituted scene.
# rotation: the 3x3 of the market `pose_align` (its translation column is zero), directions re-normalised after it.
SUBSTITUTION_PRESETS = (
    ("office", dict(rotation=None, scale=1.0, translation=(0.0, 1.0, 0.0))),                                 # eval.py:552-554
    ("market", dict(rotation=((0.0, 1.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 0.0, 1.0)), scale=1.0,
                    translation=(0.0, 0.0, 0.0))),                                                          # eval.py:555-583
    (None, dict(rotation=None, scale=1.0, translation=(0.0, 0.0, 0.0))),                                    # eval.py:584-586
)


def resolve_substitution(args):
    """The ray transform of app_reflection_substitution chosen by args.root_dir (eval.py:551-591)."""
    return _lib.preset(SUBSTITUTION_PRESETS, getattr(args, "root_dir", ""))


def resolve_rough_rows(kwargs):
    """rough_times=, scene_roughness= -> (T, the scene's own std as a float32 value), or (None, 0.0) where rough_times is not given."""
    times = kwargs.get("rough_times")
    if times is None:
        return None, 0.0
    if isinstance(times, bool) or not isinstance(times, (int, np.integer)) or times < 1:
        raise ValueError(f"rough_times is an int of at least 1 (the jittered reflections beside the first; None: off), not {times!r}")
    return int(times), placed_mirrors._roughness(kwargs.get("scene_roughness", 0.0), "scene_roughness")


def _refuse_rough_rows(args, kwargs):
    """The refusals of rough_times= (a roughness per mirror), each with its reason."""
    resolve_rough_rows(kwargs)
    if getattr(args, "app_control_mirror_roughness", False):
        raise ValueError("rough_times= cannot be combined with app_control_mirror_roughness: one roughness rule per call (the flag "
                         "jitters every mirror ray with normal_noise_std=; rough_times= takes the std per mirror and scene_roughness=)")
    if getattr(args, "app_place_new_mirror", False) or kwargs.get("new_mirror") is not None:
        raise ValueError("rough_times= cannot be combined with app_place_new_mirror or new_mirror= (the single mirror carries no "
                         "roughness; PlacedMirror.axis_aligned(..., roughness=) in new_mirrors= takes its keys)")
    given = [k for k in placed_objects.SINGLE_OBJECT_KEYWORDS if kwargs.get(k) is not None]
    if given or (getattr(args, "app_reflect_newly_placed_objects", False) and kwargs.get("placed_objects") is None):
        raise ValueError("rough_times= is combined with objects through placed_objects=[PlacedObject(...), ...], not with the "
                         f"single-object keywords ({', '.join(k + '=' for k in given) or 'app_reflect_newly_placed_objects without placed_objects='})")
    if getattr(args, "app_reflection_substitution", False):
        raise ValueError("rough_times= cannot be combined with app_reflection_substitution (the substituted render is traced once, "
                         "without the recursion the jitters go through)")


def _refuse_apps(args, models, kwargs):
    """The application flags batched_inference cannot honour, refused up front with the reason."""
    place = bool(getattr(args, "app_place_new_mirror", False))
    subst = bool(getattr(args, "app_reflection_substitution", False))
    multi = kwargs.get("new_mirrors") is not None
    if kwargs.get("rough_times") is not None:         # a roughness per mirror: allowed alone, beside new_mirrors=
        _refuse_rough_rows(args, kwargs)              # and beside placed_objects=; those keep their own refusals, below
    elif kwargs.get("scene_roughness") not in (None, 0, 0.0):
        raise ValueError(f"scene_roughness={kwargs['scene_roughness']!r} is read by the per-mirror roughness route alone: pass "
                         "rough_times=T (the number of jittered reflections beside the first)")
    if kwargs.get("exclude_source_mirror", False) is not False or kwargs.get("source_mirror") is not None:
        placed_mirrors.refuse_source(kwargs)          # allowed wherever new_mirrors= is; the tensor is looked at with the rays
    if multi:                                         # its own refusals; what it is allowed beside keeps its own, below
        placed_mirrors.refuse(args, models, kwargs)
    if kwargs.get("placed_objects") is not None:      # the list carries the kinds: args.obj_model_type is not consulted
        return placed_objects.refuse(args, models, kwargs)
    if getattr(args, "app_reflect_newly_placed_objects", False):
        obj_type = getattr(args, "obj_model_type", "d_nerf")                   # eval.py:108: the reference's default
        if obj_type == "d_nerf":
            if kwargs.get("render_kwargs_test_d_nerf") is None:
                raise NotImplementedError(
                    "app_reflect_newly_placed_objects with obj_model_type='d_nerf' needs the D-NeRF object itself: pass "
                    "render_kwargs_test_d_nerf= (dnerf.load_dnerf_object: network_fn / network_fine are DirectTemporalNeRF "
                    "modules) and frame_time=, the reference's own keyword names.  (The reference cannot run the branch as it "
                    "stands: pose_align is always None there, so pose_scale at eval.py:264 is never bound: UnboundLocalError.)  "
                    "A nerf_pl object is passed as obj_model_type='nerf_pl' with system_obj= (load_object_system)")
            if kwargs.get("frame_time") is None:
                raise ValueError("app_reflect_newly_placed_objects with a D-NeRF object needs frame_time= (the object's time in "
                                 "[0, 1], eval.py:1130, 1154)")
        elif obj_type != "nerf_pl":
            raise ValueError(f"args.obj_model_type must be 'nerf_pl' or 'd_nerf', not {obj_type!r}")
        elif kwargs.get("system_obj") is None:
            raise ValueError("app_reflect_newly_placed_objects needs system_obj= (an object with .models and .embeddings, the "
                             "radiance field of the object; load_object_system)")
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
        return
    if not (place or subst):
        return
    which = "app_place_new_mirror" if place else "app_reflection_substitution"
    if getattr(args, "app_control_mirror_roughness", False):
        raise ValueError(f"app_control_mirror_roughness cannot be combined with {which} (one application at a time, except "
                         "place-mirror with substitution)")
    if not any(getattr(m, "predict_mirror_mask", False) for m in models.values()):
        raise ValueError(f"{which} needs a mirror-mask head (predict_mirror_mask=True): the new mirror is merged into the "
                         "predicted mirror mask, and substitution replaces what the mask marks")
    if subst and kwargs.get("system_substitution") is None:
        raise ValueError("app_reflection_substitution needs system_substitution= (an object with .models and .embeddings, "
                         "the radiance field rendered in the mirrors)")
    if place and getattr(args, "near", None) is None:
        raise ValueError("app_place_new_mirror needs args.near: the foreground test compares the depth with it (eval.py:169-171)")


def _transform_rays(sec, xform):
    """eval.py:551-594 in place on the (M,8) secondary rays (mnrf_transform_rays)."""
    rot = xform["rotation"]
    rot = (ctypes.c_float * 9)(*[float(v) for row in rot for v in row]) if rot is not None else None
    tx, ty, tz = xform["translation"]
    _lib.check(_lib.lib().mnrf_transform_rays(_lib.ptr(sec), sec.shape[0], rot, float(xform["scale"]), tx, ty, tz, _lib.stream()),
               "mnrf_transform_rays")


def _f(dev, *s):
    return torch.empty(*s, dtype=torch.float32, device=dev)


def _threshold_(mask, want_any=True, edit=None):
    """In place m[m>0.5]=1, m[m<0.5]=0 (exactly 0.5 untouched); returns any(m != 0) as a bool.
    want_any=False skips the device->host read of the flag (a stream sync) when the caller does not branch on it.
    edit(flag): launched behind the threshold (the new mirror of app_place_new_mirror), may OR into the flag."""
    n = mask.shape[0]
    flag = torch.full((1,), 0, dtype=torch.int32, device=mask.device)      # (not torch.zeros: that is a memset, ~40 us of idle GPU)
    if n:
        _lib.check(_lib.lib().mnrf_threshold_mask(_lib.ptr(mask), n, _lib.ptr(flag), _lib.stream()),
                   "mnrf_threshold_mask")
        if edit is not None:
            edit(flag)
    return bool(flag.item()) if want_any else False


def _threshold_async(mask, host_flags, slot, edit=None):
    """_threshold_ without the stream sync: the flag travels to pinned host memory behind the kernel and an event marks its
    arrival; `_flag_ready` waits for THAT event only, so launches queued meanwhile (the next chunk's primary pass) keep
    the GPU busy."""
    flag = torch.full((1,), 0, dtype=torch.int32, device=mask.device)      # (not torch.zeros: that is a memset, ~40 us of idle GPU)
    _lib.check(_lib.lib().mnrf_threshold_mask(_lib.ptr(mask), mask.shape[0], _lib.ptr(flag), _lib.stream()), "mnrf_threshold_mask")
    if edit is not None:
        edit(flag)
    host = host_flags[slot:slot + 1]
    host.copy_(flag, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    return host, ev, flag     # (flag: kept alive until the copy has run)


def _flag_ready(pending):
    host, ev, _ = pending
    ev.synchronize()
    return bool(host.item())


def _reflect(rays, x_surface, normal, mask, compact, normal_noise=None, noise_std=0.0, want_dir=True):
    """-> (secondary rays (M,8), index (M,) int32 or None when not compacted, reflect_dir (N,3))."""
    N = rays.shape[0]
    dev = rays.device
    sec = _f(dev, N, 8)
    index = torch.empty(N, dtype=torch.int32, device=dev)
    count = torch.full((1,), 0, dtype=torch.int32, device=dev)
    rdir = _f(dev, N, 3) if want_dir else None
    p = _lib.ptr
    _lib.check(_lib.lib().mnrf_reflect_compact(
        p(rays), p(x_surface.contiguous()), p(normal.contiguous()), p(normal_noise), float(noise_std),
        p(mask.contiguous()) if mask is not None else None, N, int(bool(compact)), RAY_FORWARD_OFFSET,
        p(sec), p(index), p(count), p(rdir), _lib.stream()), "mnrf_reflect_compact")
    M = int(count.item()) if compact else N
    return sec[:M], (index[:M] if compact else None), rdir


def _reflect_fan(rays, x_surface, normal, noise, noise_std, index):
    """The noise.shape[0] jittered reflections of the rays index names, block after block: (n_jit * M, 8)
    (mnrf_reflect_jitter_fan; block j is what _reflect(..., compact=True, noise[j]) gives)."""
    n_jit, m = noise.shape[0], index.shape[0]
    sec = _f(rays.device, n_jit * m, 8)
    p = _lib.ptr
    _lib.check(_lib.lib().mnrf_reflect_jitter_fan(
        p(rays), p(x_surface.contiguous()), p(normal.contiguous()), p(noise.contiguous()), float(noise_std), p(index), m,
        rays.shape[0], n_jit, RAY_FORWARD_OFFSET, p(sec), _lib.stream()), "mnrf_reflect_jitter_fan")
    return sec


def _rough_rows(index, mask, rough_row, scene_roughness, flag=None):
    """-> (std_rows (N,), jitter_mask (N,)): the std of every ray and the 0/1 mask of the jitter set J (mnrf_rough_rows).  index:
    (N,) int32 as mnrf_place_mirrors wrote it at this level, or None (all -1); rough_row: placed_mirrors.roughness_row."""
    N = mask.shape[0]
    std_rows, jitter_mask = _f(mask.device, N), _f(mask.device, N)
    p = _lib.ptr
    _lib.check(_lib.lib().mnrf_rough_rows(p(index), p(mask), N, rough_row[0], rough_row[1], float(scene_roughness), p(std_rows),
                                          p(jitter_mask), p(flag), _lib.stream()), "mnrf_rough_rows")
    return std_rows, jitter_mask


def _perturb_normals(normal, noise, std_rows):
    """normal + noise * std on the rows with std > 0, the others as they are (mnrf_perturb_normals): (N,3)."""
    out = torch.empty_like(noise)
    p = _lib.ptr
    _lib.check(_lib.lib().mnrf_perturb_normals(p(normal.contiguous()), p(noise), p(std_rows), noise.shape[0], p(out), _lib.stream()),
               "mnrf_perturb_normals")
    return out


def _reflect_fan_rows(rays, x_surface, normal, noise, std_rows, index):
    """_reflect_fan with the std of every ray in std_rows (N,) (mnrf_reflect_jitter_fan_rows)."""
    n_jit, m = noise.shape[0], index.shape[0]
    sec = _f(rays.device, n_jit * m, 8)
    p = _lib.ptr
    _lib.check(_lib.lib().mnrf_reflect_jitter_fan_rows(
        p(rays), p(x_surface.contiguous()), p(normal.contiguous()), p(noise.contiguous()), p(std_rows), p(index), m,
        rays.shape[0], n_jit, RAY_FORWARD_OFFSET, p(sec), _lib.stream()), "mnrf_reflect_jitter_fan_rows")
    return sec


def _jitter_mean(acc, pieces, index, m, n_jit, finish=None):
    """acc[row(p)] += pieces[0][p], then pieces[1][p], ... in place (row(p) = index[p], or p where index is None), then the
    finish of ROUGH_FINISH with `finish` unless it is None (mnrf_jitter_mean)."""
    p = _lib.ptr
    _lib.check(_lib.lib().mnrf_jitter_mean(
        p(acc), p(pieces.contiguous()), p(index), m, n_jit, acc.shape[0], _lib.MNRF_MEAN_NONE if finish is None else ROUGH_FINISH,
        0.0 if finish is None else finish, _lib.stream()), "mnrf_jitter_mean")


def _blend(base, sec, index, mask, want_reflect):
    """m*part + (1-m)*base with part = sec scattered through index (or sec itself)."""
    N, c = base.shape[0], (base.shape[1] if base.dim() == 2 else 1)
    dev = base.device
    out = torch.empty_like(base)
    refl = torch.empty_like(base) if want_reflect else None
    p = _lib.ptr
    _lib.check(_lib.lib().mnrf_blend_scatter(
        p(base.contiguous()), p(sec.contiguous()), p(index), sec.shape[0], p(mask), N, c, p(out), p(refl),
        _lib.stream()), "mnrf_blend_scatter")
    return out, refl


def _reflect_autograd(rays, x_surface, normal, mask, compact):
    """Reflected rays with gradient history (train.py:205 "not detach() to jointly optimize"): the same HIP
    kernel forward, mnrf_reflect_backward backward."""
    from .autograd import ReflectFn
    sec, index, rdir, _count = ReflectFn.apply(rays, x_surface, normal, mask, bool(compact))
    return sec, (index if compact else None), rdir


def _blend_autograd(base, sec, index, mask, want_reflect, detach_sec=False, n_sec_live=None, n_live=None):
    """train.py:263-296 with gradient history (BlendFn); the optional visualisation output is detached."""
    from .autograd import BlendFn
    compact = index is not None
    idx = index if compact else torch.empty(0, dtype=torch.int32, device=base.device)
    out = BlendFn.apply(base, sec, idx, mask, compact, detach_sec, n_sec_live, n_live)
    refl = None
    if want_reflect:
        refl = torch.zeros_like(base)
        if compact:
            refl[index.long()] = sec.detach()
        else:
            refl = sec.detach()
    return out, refl


def _pick_normal(r, sel):
    """train.py:194-215 / eval.py:338-360 -- composited predicted normal, else composited grad normal.  (The reference keys
    on `pred_normal_*`; `surface_normal_*` exists exactly when that does, and is all the ray-fused eval pass produces.)"""
    if f"surface_normal_{sel}" in r:
        return r[f"surface_normal_{sel}"]
    return r[f"surface_normal_grad_{sel}"]


# ----------------------------------------------------------------------------- train semantics
def render_rays_chunk_recursively(models, embeddings, hp, rays_chunk, mirror_mask_prev, recur_level,
                                  extra_chunk, white_back=False, train_geometry_stage=False):
    """train.py:129-348.

    STATIC STEP (round 5; extra_chunk["_static"], set by training.train_step / GraphedTrainStep): the training route without a
    single device->host read.  The reference decides on the host whether anything is traced (`mirror_mask.bool().any()`,
    train.py:175) and how many rays (`secondary_rays[mask.bool()]`, train.py:248-252: a stream sync in the middle of every
    step).  Here the count of the compacted reflections stays on the device (ReflectFn static=True): the reflected rays keep
    the CAPACITY of the chunk, every launch of the nested level takes the count as its live row count (`_n_live`,
    include/mnrf.h) and the blend reads it too.  Values and gradients are those of the host-driven route: with no mirror
    pixel the nested launches find nothing to do and the blend leaves every ray as it is (m = 0: m*x + (1-m)*base == base).
    Differences: `rgb_*_direct` is then present although the reference would not have traced (nothing reads it), and whether
    the ground-truth mask is valid (train.py:153 `(mask >= 0).all()`) is the caller's statement extra_chunk["_gt_valid"]."""
    static = bool(extra_chunk.get("_static")) and not extra_chunk.get("is_eval", False) and torch.is_grad_enabled()
    n_live = extra_chunk.get("_n_live")
    if recur_level == 0:
        rays_chunk = _lib.f32_in(rays_chunk)              # (a direct caller's chunk; NeRFSystem hands on float32 rows)
    if static and recur_level == 0 and "_rng_share" not in extra_chunk and hp.trace_secondary_rays and not train_geometry_stage:
        # every level of a static step renders the same capacity of rays: the first one draws the random numbers of all of them
        # (two generator launches per step instead of two per level)
        extra_chunk = dict(extra_chunk, _rng_share=(1 + max(0, hp.max_recursive_level), {}))
    r = render_rays(models, embeddings, rays_chunk, hp.N_samples, hp.use_disp, hp.perturb, hp.noise_std,
                    hp.N_importance, hp.chunk, white_back, compute_normal=hp.trace_secondary_rays,
                    **dict(extra_chunk, _guard=False))        # the range guard is read once, in NeRFSystem.forward
    N = rays_chunk.shape[0]
    dev = rays_chunk.device
    sel = "fine" if (hp.N_importance > 0 and not hp.only_one_field) else "coarse"
    if static and N:
        return _static_level(models, embeddings, hp, rays_chunk, mirror_mask_prev, recur_level, extra_chunk, white_back,
                             train_geometry_stage, r, sel, n_live)

    # -- mirror mask (train.py:153-168)
    gt = extra_chunk["mirror_mask"].float()
    any_mirror = None
    # nothing branches on "any mirror pixel" when this level cannot trace: no device->host reads (stream syncs) then
    can_trace = bool(hp.trace_secondary_rays and (not train_geometry_stage) and recur_level < hp.max_recursive_level)
    if recur_level > 0 or bool((gt < 0).any().item()):
        # the reference thresholds `results[...].detach()` in place: the returned predicted
        # mask is the hard one
        if "mirror_mask_fine" in r:
            mask = r["mirror_mask_fine"]
        elif "mirror_mask_coarse" in r:
            mask = r["mirror_mask_coarse"]
        else:
            mask = torch.zeros(N, device=dev)
        any_mirror = _threshold_(mask.detach(), want_any=can_trace)   # in place on the shared storage, like the reference
        mask = mask.detach()
    else:
        mask = gt.clone().contiguous()
    only_in = hp.only_trace_rays_in_mirrors
    if (not only_in) and recur_level > 0:
        mask = mask * mirror_mask_prev.float()
        any_mirror = None
    assumed_mirror = False
    if any_mirror is None:
        if N and can_trace and only_in and not hp.for_vis:
            # compacted reflections: "any mirror pixel" is "the compaction found a ray" -- ONE device->host read (the count the
            # reflect kernel returns) instead of two stream syncs per level
            any_mirror = assumed_mirror = True
        else:
            any_mirror = bool((mask != 0).any().item()) if (N and can_trace) else False

    # -- trace decision (train.py:170-178)
    trace = bool(hp.trace_secondary_rays and (not train_geometry_stage) and (any_mirror or hp.for_vis))
    if recur_level >= hp.max_recursive_level:
        trace = False
    is_eval = extra_chunk.get("is_eval", False)

    traced = False
    grad_path = torch.is_grad_enabled() and r[f"rgb_{sel}"].requires_grad
    reflect_fn, blend_fn = (_reflect_autograd, _blend_autograd) if grad_path else (_reflect, _blend)
    if grad_path and getattr(hp, "detach_ref_color_for_blend", False) and \
            extra_chunk.get("current_epoch", 0) >= getattr(hp, "train_geometry_stage_end_epoch", 4) + 1:
        # train.py:284-289 (the reference reads Lightning's self.current_epoch; here: extra["current_epoch"], which
        # training_step passes as the same number, train.py:426)
        blend_fn = lambda *a: _blend_autograd(*a, detach_sec=True)  # noqa: E731
    if trace and N:
        nrm = _pick_normal(r, sel)
        if getattr(hp, "detach_normal_in_reflection", False):
            nrm = nrm.detach()
        sec, index, rdir = reflect_fn(rays_chunk, r[f"x_surface_{sel}"], nrm, mask, only_in)
        if sec.shape[0] > 0:
            traced = True
            r2 = render_rays_chunk_recursively(models, embeddings, hp, sec.contiguous(), mask, recur_level + 1,
                                               extra_chunk, white_back, train_geometry_stage)
            for typ in ("coarse", "fine"):                               # train.py:263-311
                if f"rgb_{typ}" in r and f"rgb_{typ}" in r2:
                    r[f"rgb_{typ}_direct"] = r[f"rgb_{typ}"]
                    r[f"rgb_{typ}"], refl = blend_fn(r[f"rgb_{typ}"], r2[f"rgb_{typ}"], index, mask, is_eval)
                    if is_eval:
                        r[f"rgb_{typ}_reflect"] = refl
            if is_eval:                                                  # train.py:312-324
                if only_in:
                    d = torch.zeros_like(r[f"depth_{sel}"])
                    d[index.long()] = r2[f"depth_{sel}"]
                    r[f"depth_{sel}_reflect"] = d
                else:
                    r[f"depth_{sel}_reflect"] = r2[f"depth_{sel}"]
                r["secondary_rays_o"] = r[f"x_surface_{sel}"]
                r["reflect_direction"] = rdir
        elif assumed_mirror:
            trace = False       # the compaction found no mirror pixel: what mask.any() would have said up front
    if not trace and is_eval:                                            # train.py:325-346
        for typ in ("coarse", "fine"):
            if f"rgb_{typ}" in r:
                r[f"rgb_{typ}_reflect"] = torch.zeros_like(r[f"rgb_{typ}"])
                r[f"rgb_{typ}_direct"] = torch.zeros_like(r[f"rgb_{typ}"])
        r[f"depth_{sel}_reflect"] = torch.zeros_like(r[f"depth_{sel}"])
        r["secondary_rays_o"] = torch.zeros_like(r[f"rgb_{sel}"])
        r["reflect_direction"] = torch.zeros_like(r[f"rgb_{sel}"])
    del traced
    return r


def _static_level(models, embeddings, hp, rays_chunk, mirror_mask_prev, recur_level, extra_chunk, white_back,
                  train_geometry_stage, r, sel, n_live):
    """One level of render_rays_chunk_recursively in a static step (see there): train.py:153-296 with the mirror-ray count on
    the device.  `r`: this level's render_rays result; n_live: the live rows of rays_chunk (None at level 0)."""
    from .autograd import ReflectFn
    N = rays_chunk.shape[0]
    dev = rays_chunk.device
    can_trace = bool(hp.trace_secondary_rays and (not train_geometry_stage) and recur_level < hp.max_recursive_level)
    gt = extra_chunk["mirror_mask"].float()
    gt_valid = extra_chunk.get("_gt_valid")
    if gt_valid is None:
        raise RuntimeError("static step: extra['_gt_valid'] must say whether the batch's mirror masks are all valid (train.py:153)")
    if recur_level > 0 and not can_trace:
        return r      # (the reference thresholds this level's predicted mask in place, train.py:165-166, in a dict whose masks nobody reads:
                      #  the caller keeps rgb_* only, train.py:263-296 -- one launch less per step)
    if recur_level > 0 or not gt_valid:                           # train.py:155-166: predicted mask, thresholded in place
        if "mirror_mask_fine" in r:
            mask = r["mirror_mask_fine"]
        elif "mirror_mask_coarse" in r:
            mask = r["mirror_mask_coarse"]
        else:
            mask = torch.zeros(N, device=dev)
        md = mask.detach()
        _lib.check(_lib.lib().mnrf_threshold_mask_n(_lib.ptr(md), N, None, _lib.ptr(n_live), _lib.stream()), "mnrf_threshold_mask")
        mask = md
    else:
        mask = gt.contiguous()       # (never written: no clone needed)
    only_in = hp.only_trace_rays_in_mirrors
    if (not only_in) and recur_level > 0:
        mask = mask * mirror_mask_prev.float()                    # train.py:167-168
    if not can_trace:
        return r
    if not r[f"rgb_{sel}"].requires_grad:
        raise RuntimeError("static step: the render carries no gradient history (use the default route for evaluation)")
    detach_sec = bool(getattr(hp, "detach_ref_color_for_blend", False)) and \
        extra_chunk.get("current_epoch", 0) >= getattr(hp, "train_geometry_stage_end_epoch", 4) + 1      # train.py:284-289
    nrm = _pick_normal(r, sel)
    if getattr(hp, "detach_normal_in_reflection", False):
        nrm = nrm.detach()
    sec, index, _rdir, count = ReflectFn.apply(rays_chunk, r[f"x_surface_{sel}"], nrm, mask, bool(only_in), True, n_live)
    r2 = render_rays_chunk_recursively(models, embeddings, hp, sec, mask, recur_level + 1,
                                       dict(extra_chunk, _n_live=count, _compacted=bool(only_in) or bool(extra_chunk.get("_compacted"))),
                                       white_back, train_geometry_stage)
    # train.py:263-296 for both typs in one launch (gather form through the compaction's inverse index: autograd.Blend2Fn)
    from .autograd import Blend2Fn
    typs = [t for t in ("coarse", "fine") if f"rgb_{t}" in r and f"rgb_{t}" in r2]
    if typs:
        a = typs[0]
        b = typs[1] if len(typs) > 1 else None
        out_a, out_b = Blend2Fn.apply(r[f"rgb_{a}"], r2[f"rgb_{a}"], r[f"rgb_{b}"] if b else None, r2[f"rgb_{b}"] if b else None,
                                      count._mnrf_slot, mask, detach_sec, n_live)
        for t, o in ((a, out_a), (b, out_b)):
            if t:
                r[f"rgb_{t}_direct"] = r[f"rgb_{t}"]
                r[f"rgb_{t}"] = o
    return r


class NeRFSystem(nn.Module):
    """The model-holding part of train.NeRFSystem (train.py:33-127): same attribute names
    (`nerf_coarse`, `nerf_fine`, `embedding_xyz`, `embedding_dir`, `models`, `embeddings`) and the
    same `forward(rays, extra)`.  The Lightning training loop around it is out of scope."""

    def __init__(self, hparams, white_back=False):
        super().__init__()
        self.hparams = hparams if not isinstance(hparams, dict) else SimpleNamespace(**hparams)
        hp = self.hparams
        self.train_geometry_stage = getattr(hp, "train_geometry_stage", False)
        self.white_back = white_back
        if getattr(hp, "model_type", "nerf") == "nerf_tcnn":                       # train.py:67-99
            from .mirror_nerf_tcnn import MirrorNeRFTcnn
            self.embedding_xyz = Embedding(0)
            self.embedding_dir = Embedding(0)
            make = lambda: MirrorNeRFTcnn(encoding="hashgrid", bound=hp.bound, predict_normal=hp.predict_normal,  # noqa: E731
                                          predict_mirror_mask=hp.predict_mirror_mask)
        else:
            self.embedding_xyz = Embedding(hp.N_emb_xyz)
            self.embedding_dir = Embedding(hp.N_emb_dir)
            kw = dict(in_channels_xyz=6 * hp.N_emb_xyz + 3, in_channels_dir=6 * hp.N_emb_dir + 3,
                      predict_normal=hp.predict_normal, predict_mirror_mask=hp.predict_mirror_mask)
            make = lambda: MirrorNeRF(**kw)  # noqa: E731
        self.embeddings = {"xyz": self.embedding_xyz, "dir": self.embedding_dir}
        self.nerf_coarse = make()
        self.models = {"coarse": self.nerf_coarse}
        if hp.N_importance > 0 and not hp.only_one_field:
            self.nerf_fine = make()
            self.models["fine"] = self.nerf_fine

    def forward(self, rays, extra=dict()):
        out = self._forward(rays, extra)
        # (training.train_step passes _guard=False: it reads the sticky flag once, after the backward, for both passes)
        if rays.shape[0] and extra.get("_guard", True) and check_guard(self):   # out of range: the models are on fp32 now
            try:
                out = self._forward(rays, extra)
            finally:
                release_transient(self)       # (a range-only trip: for this call only)
        return out

    def _forward(self, rays, extra):
        from .weights import validated
        with validated(self.models.values()):      # (the packed weight images are checked once per call, not per evaluation)
            return self._forward_chunks(rays, extra)

    def _forward_chunks(self, rays, extra):
        hp = self.hparams
        results = defaultdict(list)
        rays = _lib.f32_in(rays)             # once per call: the reflect launches of the no-grad route read (N,8) float32 rows
        for i in range(0, rays.shape[0], hp.chunk):
            ex = {k: (v[i:i + hp.chunk] if isinstance(v, torch.Tensor) else v) for k, v in extra.items() if k != "_guard"}
            rc = rays[i:i + hp.chunk].contiguous()
            # (train.py:115-119 hands an all-ones "previous mirror mask" to level 0, where nothing reads it: train.py:167-168 multiplies by it
            #  at recur_level > 0 only -- no tensor made for it)
            out = render_rays_chunk_recursively(self.models, self.embeddings, hp, rc, None, 0, ex,
                                                self.white_back, self.train_geometry_stage)
            for k, v in out.items():
                results[k] += [v]
        # (a single chunk -- every training batch -- needs no copy: torch.cat of one tensor is 27 copy kernels per step)
        return {k: (v[0] if len(v) == 1 else torch.cat(v, 0)) for k, v in results.items()}


# ----------------------------------------------------------------------------- eval semantics
_COPY_STREAMS, _PINNED = {}, {}


def _copy_stream(device):
    s = _COPY_STREAMS.get(device)
    if s is None:
        s = _COPY_STREAMS[device] = torch.cuda.Stream(device=device)
    return s


def _pinned(key, rows, tail, dtype):
    """Pinned host staging buffer for one per-ray map of a frame, kept between frames (pinning 51 MB costs more than copying
    them); grown when a larger frame arrives."""
    k = (key, tail, dtype)
    buf = _PINNED.get(k)
    if buf is None or buf.shape[0] < rows:
        buf = _PINNED[k] = torch.empty((rows,) + tail, dtype=dtype).pin_memory()
    return buf


def _resolve_call(models, rays, N_samples, N_importance, use_disp, chunk, kwargs):
    """One call of batched_inference, refused or resolved: a plain namespace that the stages below read.  Written after it is
    made: embeddings (batched_inference hands it on), noise_iter (_run_chunks starts it afresh per pass, _draw advances it) and
    the entries of mirror_fraction (the per-model evidence of _MIRROR_FRACTION).  _refuse_apps runs first; then every keyword is
    read once, here.  A single object (the single-object keywords) becomes a list of one record of the kind
    PlacedObject.resolve returns, rendered through the single-object launches (object_chain)."""
    args = kwargs.get("args")
    if isinstance(args, dict):
        args = SimpleNamespace(**args)
    _refuse_apps(args, models, dict(kwargs, _N_importance=N_importance))
    rays = _lib.f32_in(rays)             # once per call: every launch of every level reads the chunk as (N,8) float32 rows
    c = SimpleNamespace(models=models, rays=rays, N_samples=N_samples, N_importance=N_importance, use_disp=use_disp, chunk=chunk,
                        args=args)
    c.exclude, c.source_all = placed_mirrors.resolve_source(kwargs, rays)      # exclude_source_mirror=, source_mirror=
    c.objects = bool(getattr(args, "app_reflect_newly_placed_objects", False))
    listed, frame_time = kwargs.get("placed_objects"), kwargs.get("frame_time")
    # used: what the merges add into, element k for object k -- object_used itself for a single object; a list counts in a tensor
    # of its own, and used_out is then the caller's object_used, filled at the end of the call
    object_used = kwargs.get("object_used") if c.objects else None
    c.used, c.used_out = object_used, None
    c.placed, c.object_chain = None, bool(kwargs.get("_object_chain", False))
    if listed is None:                                                         # the single-object keywords, or no object at all
        kind = None if not c.objects else "d_nerf" if getattr(args, "obj_model_type", "d_nerf") == "d_nerf" else "nerf_pl"
        xform = resolve_new_object(args, kwargs.get("new_object")) if c.objects else None
        field = kwargs.get("render_kwargs_test_d_nerf" if kind == "d_nerf" else "system_obj") if c.objects else None
        time = float(frame_time) if kind == "d_nerf" else None
        bounds = resolve_object_bounds(kwargs.get("object_bounds"), kwargs.get("object_region"), kwargs.get("object_bounds_res", 64),
                                       kind, field, time, rays.device)
        if c.objects:
            c.placed, c.object_chain = [dict(kind=kind, field=field, xform=xform, bounds=bounds, time=time)], True
    else:
        c.placed = [o.resolve(args, None if frame_time is None else float(frame_time), rays.device) for o in listed]
        if object_used is not None:
            if object_used.numel() not in (1, len(c.placed)):
                raise ValueError(f"object_used holds {len(c.placed)} elements (one per placed object) or 1 (their total), not {object_used.numel()}")
            c.used, c.used_out = torch.empty(len(c.placed), dtype=torch.int32, device=rays.device), object_used
    if object_used is not None and object_used.dtype != torch.int32:      # the merge kernels add into it: a tensor the call writes is never converted
        raise ValueError(f"object_used must be an int32 tensor, not {object_used.dtype}")
    c.place, c.subst = bool(getattr(args, "app_place_new_mirror", False)), bool(getattr(args, "app_reflection_substitution", False))
    c.plane = resolve_new_mirror(args, kwargs.get("new_mirror")) if c.place else None
    mirrors = kwargs.get("new_mirrors")                                    # several mirrors on any plane (placed_mirrors.py)
    c.multi = mirrors is not None
    c.mirrors_packed = placed_mirrors.pack(mirrors) if c.multi else None
    c.xform = resolve_substitution(args) if c.subst else None
    c.system_sub = kwargs.get("system_substitution") if c.subst else None
    c.trace_flag = kwargs.get("trace_secondary_rays", False)
    c.test_time = kwargs.get("test_time", True)
    c.white_back = kwargs.get("white_back", False)
    c.noise_std = kwargs.get("normal_noise_std", 0)
    # injected draws are kept as a list so that a second pass after a range-guard trip replays the SAME draws
    draws = kwargs.get("_normal_noise")
    c.draws = None if draws is None else list(draws)
    c.to_cpu = kwargs.get("to_cpu", True)
    # per-ray maps only (the per-sample tensors are neither copied nor, in the final pass, produced at all: render_rays
    # `_maps_only`): what to_cpu="maps" returns anyway; with to_cpu=False it is opt-in (maps_only=True), the full dict stays
    # the default contract
    c.maps_only = bool(kwargs.get("maps_only", c.to_cpu == "maps"))
    c.rough = getattr(args, "app_control_mirror_roughness", False)
    # a roughness per mirror: its own keywords, its own branch of _stage_b; it takes every exclusion `rough` takes
    c.rough_times, c.scene_roughness = resolve_rough_rows(kwargs)
    c.rough_rows = c.rough_times is not None
    c.rough_row = placed_mirrors.roughness_row(mirrors) if c.rough_rows else None
    c.jitters_possible = c.rough_rows and (c.scene_roughness > 0 or any(v > 0 for v in c.rough_row[1][:c.rough_row[0]]))  # else J is empty, known here
    c.batch_jitter = kwargs.get("batch_jitter", c.draws is None)   # see _add_jitters
    c.one_field = getattr(args, "only_one_field", False)
    c.fine_epoch = getattr(args, "only_one_field_fine_epoch", 2)
    c.sel = "fine" if (N_importance > 0 and not c.one_field) else "coarse"
    c.blend_mode = kwargs.get("blended_level", "auto")      # True / False / "auto": see _stage_a
    if c.blend_mode not in (True, False, "auto"):
        raise ValueError(f"blended_level must be True, False or 'auto', not {c.blend_mode!r}")
    c.mirror_fraction = _MIRROR_FRACTION.setdefault(models.get(c.sel, models["coarse"]), {})      # level -> share of mirror rays in the chunk last counted
    # what several conditions of the stages ask, formed once
    c.jitters = bool(c.rough or c.rough_rows)                      # a roughness rule: further draws and renders per level
    c.implies_trace = bool(c.trace_flag or c.place or c.multi)     # a placed mirror makes every level below the last trace
    c.edits_level = bool(c.place or c.subst or c.objects or c.multi)      # an application reads or edits more of a level than the blend does
    c.renderers = [_renderer(c, o) for o in c.placed] if c.placed is not None else None
    # the models whose range guard the call reads (a D-NeRF object runs fp32 only: no guard)
    c.guarded = list(models.values()) + (list(c.system_sub.models.values()) if c.system_sub is not None else [])
    for o in c.placed or ():
        if o["kind"] == "nerf_pl":
            c.guarded += [m for m in _object_system(o["field"])[0].values() if not any(m is g for g in c.guarded)]
    return c


def _draw(c, n, dev):
    if c.noise_iter is not None:
        return next(c.noise_iter).to(dev).float().contiguous()
    return torch.randn(n, 3, device=dev)


def _render_field(c, obj_rays, dnerf, time, field_models, field_embeddings):
    if dnerf is not None:
        # eval.py:233-259: the time in column 8, the normalised directions behind it (a plain division); near and far are
        # the rays' own columns 6 and 7; samples, background and models come from the OBJECT's configuration
        d = obj_rays[:, 3:6]
        batch = torch.cat([obj_rays, torch.full_like(obj_rays[:, :1], time), d / torch.norm(d, dim=-1, keepdim=True)], -1)
        o = render_rays_dnerf(batch, **dict(dnerf, _frame_time=time))
        return {"rgb_fine": o["rgb_map"], "depth_fine": o["depth_map"], "opacity_fine": o["acc_map"]}
    # eval.py:221-232: only colour, depth and opacity of this render are read -- the maps-only path
    return render_rays(field_models, field_embeddings, obj_rays, c.N_samples, c.use_disp, 0, 0, c.N_importance, c.chunk, c.white_back,
                       test_time=True, compute_normal=False, _guard=False, _maps_only=True, _rgb_depth_only=True)


def _renderer(c, o):
    """rays -> the maps of the resolved object o (a record of c.placed) along them."""
    if o["kind"] == "d_nerf":
        return lambda obj_rays: _render_field(c, obj_rays, o["field"], o["time"], None, None)
    field_models, field_embeddings = _object_system(o["field"])
    return lambda obj_rays: _render_field(c, obj_rays, None, None, field_models, field_embeddings)


def _stage_a(c, rays_chunk, level, host=None, slot=0, source=None):
    """The primary pass of one chunk at one level, the objects and the placed mirrors merged into its maps, its mirror mask
    thresholded.  host: the pinned (flags, counts) of a pipelined pass (_run_chunks) -- the flag is then not waited for here."""
    args, sel = c.args, c.sel
    # The last level of a recursion traces nothing: its caller (_stage_b of the level above) reads rgb_* and depth_* of it
    # and nothing else (eval.py:676-697), so its final pass runs ray-fused without the mirror head (render_rays
    # `_rgb_depth_only`).  Not with the roughness jitters, whose groups add further keys of the render.
    rgb_depth = 1 <= level == args.max_recursive_level and not c.jitters
    # A level that traces has its colour replaced by m * reflected + (1 - m) * colour in _stage_b, m = 1 wherever the
    # composited mirror value is not below 0.5 (the threshold, then `!= 0`): the colour of such a ray reaches nothing --
    # no other key of the result carries it -- so the final pass may leave it out and write 0 (render_rays
    # `_blended_level`, mnrf_field_composite_fused MNRF_FUSED_BLENDED_LEVEL; 0 * colour and 0 * 0 are the same +0).  A chunk
    # whose "any mirror" flag comes back false is returned unblended -- and then holds no ray above the threshold, so no
    # row of it was left out.  Not with roughness jitters, a placed mirror, reflection substitution or placed objects:
    # those read or edit more of the level than the blend does.  (render_rays falls back to the launches of before when
    # the pass is not one the fused kernel covers: fp32 arithmetic, another sample count, density-gradient normals.)
    # Both routes give the same result, so the choice is one of speed alone, and it is made PER CHUNK from evidence: a chunk
    # with no ray above the threshold is about 3 % slower through the ray-fused form than through the two-kernel path, one
    # with every ray above it 5 % faster, and the two meet at BLENDED_BREAK_EVEN.  The evidence is the share of rays above
    # the threshold in the chunk of this level whose count was last known (neighbouring chunks of a frame, and the same
    # chunks of the frame before, see much the same scene); it is kept per model across calls (_MIRROR_FRACTION).  Without
    # evidence -- the first chunk ever rendered with a model -- the launches of before are used, so a scene with few mirror
    # pixels never takes the slower route for more than the chunks it takes to notice a change.
    # `blended_level=True` / `False` forces the choice (tests, measurements).
    can_blend = bool(level < args.max_recursive_level and c.trace_flag and c.test_time and c.blend_mode is not False
                     and not (c.jitters or c.edits_level))
    evidence = c.mirror_fraction.get(level)
    blended = can_blend and (c.blend_mode is True or (evidence is not None and evidence >= BLENDED_BREAK_EVEN))
    count_it = can_blend and c.blend_mode is not True
    r = render_rays(c.models, c.embeddings, rays_chunk, c.N_samples, c.use_disp, 0, 0, c.N_importance, c.chunk,
                    c.white_back, test_time=c.test_time,
                    compute_normal=c.trace_flag and (not args.predict_normal),
                    only_one_field=c.one_field, only_one_field_fine_epoch=c.fine_epoch,
                    current_epoch=c.fine_epoch + 1, _guard=False, _maps_only=c.maps_only or rgb_depth,
                    _rgb_depth_only=rgb_depth, _blended_level=blended)
    r[f"rgb_{sel}_reflect"] = torch.zeros_like(r[f"rgb_{sel}"])
    r[f"depth_{sel}_reflect"] = torch.zeros_like(r[f"depth_{sel}"])
    if c.placed is not None and not c.object_chain:                   # the K-object rule, ahead of the hard clip
        placed_objects._merge_placed(r, rays_chunk, c.placed, args.near, c.used, c.renderers)
    elif c.placed is not None:              # eval.py:173-291, ahead of the hard clip: the single-object launches, object after object
        for k, o in enumerate(c.placed):
            placed_objects._merge_object(r, rays_chunk, o["xform"], args.near, None if c.used is None else c.used.view(-1)[k:k + 1],
                                         c.renderers[k], o["bounds"])
    mask = next((r[key] for key in (f"mirror_mask_{sel}", "mirror_mask_fine", "mirror_mask_coarse") if key in r), None)
    # in place (eval.py:303-307); at the last level nothing branches on "any mirror pixel": no host read, so the next
    # chunk's launches queue behind this pass without a stream sync.  A new mirror (eval.py:311-320) makes every level
    # below the last one trace; it is merged into the mask right behind the threshold, and its flag is the one read.
    last = level >= args.max_recursive_level or not c.implies_trace
    edit = None
    if c.place and not last:
        edit = lambda flag: placed_mirrors._place_mirror_level(r, rays_chunk, sel, c.plane, args.near, flag)  # noqa: E731
    # (with a roughness per mirror every level that places mirrors keeps its index: the std of a ray follows the mirror it
    # took at THAT level; only level 0's is returned.  exclude_source_mirror keeps it too: it is the next level's `source`)
    if c.multi and (level == 0 or ((c.rough_rows or c.exclude) and not last)):      # the mirror each ray took; -1 where the list is not applied
        r["new_mirror_index"] = torch.full((rays_chunk.shape[0],), -1, dtype=torch.int32, device=rays_chunk.device)
    if c.multi and not last:
        edit = lambda flag: placed_mirrors._place_mirrors_level(r, rays_chunk, sel, c.mirrors_packed, args.near, flag,  # noqa: E731
                                                                r.get("new_mirror_index"), source, c.exclude)
    pending, any_mirror, counted = None, False, None
    if mask is not None:
        if host is not None and not last and rays_chunk.shape[0]:
            pending = _threshold_async(mask, host[0], slot, edit)
            if count_it:      # the count follows the flag to pinned memory; _stage_b reads it behind its own event
                host_count = host[1][slot:slot + 1]
                host_count.copy_(torch.count_nonzero(mask).view(1), non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
                counted = (host_count, ev)
        else:
            any_mirror = _threshold_(mask, want_any=not last, edit=edit)
            if count_it and rays_chunk.shape[0]:
                c.mirror_fraction[level] = (int(torch.count_nonzero(mask).item()) if any_mirror else 0) / rays_chunk.shape[0]
    return r, rays_chunk, level, mask, any_mirror, pending, counted


def _recurse(c, rays_chunk, level, source=None):
    return _stage_b(c, _stage_a(c, rays_chunk, level, source=source))


def _sources(c, r, index, m, n_rep=1):
    # the `source` of the rays reflected off this level (mnrf_mirror_sources): the mirror each took here, through the compaction
    return placed_mirrors.mirror_sources(r.get("new_mirror_index"), index, m, n_rep, r[f"rgb_{c.sel}"].device) if c.exclude else None


def _add_jitters(c, r, r2, rays_chunk, level, jit_index, row_map, fan, one, times):
    """`times` further samples added to rows of R = r2's colours, and the finish: both roughness rules end a level with it.
    jit_index: (mj,) int32, the compaction of the jitter set among the level's rays; row_map: the row of R that jittered ray p
    adds into (None: p itself); fan(noise (n, N, 3)) -> the (n * mj, 8) secondary rays of a group of n draws; one(draw (N, 3))
    -> the (mj, 8) rays of one draw (batch_jitter=False); `source` rows are handed on wherever the call keeps them (_sources).

    The reference renders the jittered reflections one after the other (run.sh:187: 64 of them, each a full secondary render).
    Rays are independent, so groups of them go through ONE recursion call and the colours are added in the reference's order.
    Groups are sized to JITTER_RAYS rays (~2.5 GB of per-sample tensors at 64+128 samples); a group is one buffer of draws (one
    (N,3) draw per jitter, in the reference's order), one fan launch, one recursion call and one mnrf_jitter_mean per colour
    key.  Not the default when a test injects the draws: their order interleaves with the nested levels' draws."""
    N, dev, mj = rays_chunk.shape[0], rays_chunk.device, jit_index.shape[0]
    keys = [f"rgb_{typ}" for typ in ("coarse", "fine") if f"rgb_{typ}" in r2]
    for k in keys:
        r2[k] = r2[k].contiguous()
    finish = float(np.float32(1) / np.float32(times + 1))   # torch's `/ (times + 1)` on the device: see ROUGH_FINISH
    g = 0
    while g < times:
        if c.batch_jitter:
            n_g = max(1, min(times - g, JITTER_RAYS // max(1, mj)))
            noise = torch.stack([_draw(c, N, dev) for _ in range(n_g)]) if c.noise_iter is not None \
                else torch.randn(n_g, N, 3, device=dev)
            s2 = fan(noise)
        else:
            n_g, s2 = 1, one(_draw(c, N, dev)).contiguous()
        r3 = _recurse(c, s2, level + 1, _sources(c, r, jit_index, mj, n_g))
        g += n_g
        for k in keys:
            _jitter_mean(r2[k], r3[k], row_map, mj, n_g, finish if g >= times else None)


def _stage_b(c, state):
    """The reflected pass of one chunk at one level: what _stage_a left is traced, where it holds a mirror ray, and blended."""
    r, rays_chunk, level, mask, any_mirror, pending, counted = state
    args, sel = c.args, c.sel
    if pending is not None:
        any_mirror = _flag_ready(pending)
    if counted is not None:
        counted[1].synchronize()
        c.mirror_fraction[level] = int(counted[0].item()) / rays_chunk.shape[0]
    N, dev = rays_chunk.shape[0], rays_chunk.device
    only_in = not (level < 1)                                         # eval.py:159
    trace = bool(mask is not None and any_mirror and c.implies_trace and level < args.max_recursive_level)     # eval.py:311-320, 503-504
    if not trace or N == 0:
        return r
    # `mirror_mask = mirror_mask.bool()` then `.float()` (eval.py:307, 689): an exact 0.5 blends as 1
    mask = (mask != 0).float()
    normal, x_surface = _pick_normal(r, sel), r[f"x_surface_{sel}"]
    nn0 = _draw(c, N, dev) if c.jitters else None                     # eval.py:506-511
    first_normal, first_std = normal, c.noise_std
    if c.rough_rows:
        # THE RULE of include/mnrf.h "A roughness per mirror" (DESIGN 4.4c): the std of a ray follows the mirror it took at
        # this level.  The first reflection is the existing launch on normals that carry draw_0 * std already (no addition
        # where the std is 0: the bits of the frame without roughness); with every std 0 there is nothing to add at all.
        if c.jitters_possible:
            std_rows, jitter_mask = _rough_rows(r.get("new_mirror_index"), mask, c.rough_row, c.scene_roughness)
            first_normal = _perturb_normals(normal, nn0, std_rows)
        nn0, first_std = None, 0.0                                    # (the draw is made either way: the order of draws)
    sec, index, rdir = _reflect(rays_chunk, x_surface, first_normal, mask, only_in, nn0, first_std)
    r["reflect_direction"] = rdir
    if sec.shape[0] == 0:
        return r
    if c.subst:                                                       # eval.py:550-613: no recursion below
        _transform_rays(sec, c.xform)
        # only rgb / depth of this render are read (eval.py:676-697): the maps-only path, without the density-gradient
        # normals the reference also computes for it
        r2 = render_rays(c.system_sub.models, c.system_sub.embeddings, sec.contiguous(), c.N_samples, c.use_disp, 0, 0,
                         c.N_importance, c.chunk, c.white_back, test_time=c.test_time, compute_normal=False,
                         only_one_field=c.one_field, only_one_field_fine_epoch=c.fine_epoch,
                         current_epoch=c.fine_epoch + 1, _guard=False, _maps_only=True, _rgb_depth_only=True)
    else:
        r2 = _recurse(c, sec.contiguous(), level + 1, _sources(c, r, index, sec.shape[0]))
    if c.rough and args.trace_ray_times > 0:                          # eval.py:622-674
        # THE RULE of include/mnrf.h "Mirror roughness" (DESIGN 4.4b).  The reference adds the (M,3) colours of each
        # jittered render, M = sum(mask), to the first secondary render, which at level 0 has N rows: that works only
        # where every ray of the chunk is a mirror ray.  Here the sums go through the compaction's index,
        # so a mirror ray gets the mean of its times + 1 samples and a ray of level 0 that is no mirror ray keeps the
        # one sample it has; where M == N it is the reference's arithmetic.
        # The ONE compaction of the level's mask, and the one host read of its count: every jitter compacts through
        # the same mask.  At levels >= 1 the first _reflect above made both; at level 0, which reflects every
        # ray, mnrf_reflect_compact runs once more with compact = 1 for its index alone
        jit_index = index if only_in else _reflect(rays_chunk, x_surface, normal, mask, True, want_dir=False)[1]
        _add_jitters(c, r, r2, rays_chunk, level, jit_index, None if only_in else jit_index,      # row of R: p at levels >= 1, index[p] at level 0
                     lambda noise: _reflect_fan(rays_chunk, x_surface, normal, noise, c.noise_std, jit_index),
                     lambda draw: _reflect(rays_chunk, x_surface, normal, mask, True, draw, c.noise_std, want_dir=False)[0],
                     args.trace_ray_times)
    elif c.rough:
        for k in [f"rgb_{typ}" for typ in ("coarse", "fine") if f"rgb_{typ}" in r2]:
            r2[k] = r2[k] / (args.trace_ray_times + 1)
    elif c.rough_rows and c.jitters_possible:
        # The branch above with J = {mask != 0 and std > 0} in the mask's place: ONE compaction of J and the read of its
        # count (the second and last of the level), the fan with the std per ray, the same groups, sums and finish.  A
        # mirror ray outside J keeps its one sample; an empty J takes no further draw.  One by one a jitter is
        # mnrf_perturb_normals, then mnrf_reflect_compact on J's mask.
        jit_index = _reflect(rays_chunk, x_surface, normal, jitter_mask, True, want_dir=False)[1]
        if jit_index.shape[0] > 0:
            row_map = jit_index
            if only_in:       # row of R: the ray's rank in the mask's compaction, from the two indices, on the device
                rank = torch.empty(N, dtype=torch.int32, device=dev)
                rank[index.long()] = torch.arange(index.shape[0], dtype=torch.int32, device=dev)
                row_map = rank[jit_index.long()]
            _add_jitters(c, r, r2, rays_chunk, level, jit_index, row_map,
                         lambda noise: _reflect_fan_rows(rays_chunk, x_surface, normal, noise, std_rows, jit_index),
                         lambda draw: _reflect(rays_chunk, x_surface, _perturb_normals(normal, draw, std_rows), jitter_mask, True,
                                               want_dir=False)[0],
                         c.rough_times)
    r[f"rgb_{sel}"], refl = _blend(r[f"rgb_{sel}"], r2[f"rgb_{sel}"], index, mask, True)
    r[f"rgb_{sel}_reflect"] = refl
    if only_in:
        d = torch.zeros_like(r[f"depth_{sel}"])
        d[index.long()] = r2[f"depth_{sel}"]
        r[f"depth_{sel}_reflect"] = d
    else:
        r[f"depth_{sel}_reflect"] = r2[f"depth_{sel}"]
    return r


def _collect(c, out, results, staging):
    """One chunk's result into `results` (key -> list of pieces).  staging (to_cpu="maps" on the GPU, else None): the per-ray
    maps of the chunk travel to PINNED staging buffers on a side stream while the next chunk renders (pageable destinations
    made every copy synchronous: 33 ms per 51 MB frame)."""
    if staging is not None:
        done = torch.cuda.Event()
        done.record()
        staging.stream.wait_event(done)
    maps = c.to_cpu == "maps" or c.maps_only                           # per-ray maps only
    for k, v in out.items():
        if maps and not (v.dim() <= 2 and (v.dim() == 1 or v.shape[1] <= 3)):
            continue
        if staging is None:
            results[k] += [v.to("cpu", non_blocking=True) if c.to_cpu == "maps" else (v.cpu() if c.to_cpu else v)]
            continue
        buf = staging.buffers.get(k)
        if buf is None:
            buf = staging.buffers[k] = _pinned(k, c.rays.shape[0], tuple(v.shape[1:]), v.dtype)
        r0 = staging.rows[k]
        with torch.cuda.stream(staging.stream):
            buf[r0:r0 + v.shape[0]].copy_(v, non_blocking=True)
        staging.rows[k] = r0 + v.shape[0]
        staging.hold.append(v)      # (alive until the copies have run)


def _run_chunks(c):
    """One pass over the chunks of the call -> key -> list of pieces.  A pass starts its own counts of object_used, its own
    iterator over injected draws and its own staging state, so a second pass after a range-guard trip repeats the first.
    Level 0 runs in two stages so that chunk k+1's primary pass can be queued BEFORE the host waits for chunk k's "any mirror
    pixel" flag (eval.py:303-312 branches on it): the GPU then never idles on that read.  Not used with the roughness jitters,
    whose random draws would change order against the primary passes.  MNRF_EVAL_PIPELINE (default on): the per-sample tensors
    of TWO chunks are then alive at once (~2 x 3 KB/ray x chunk: 200 MB at chunk 32768) -- set it to 0 on a memory-tight
    device.  With random roughness draws (no injection) a second pass draws afresh, as any re-render would."""
    rays, chunk = c.rays, c.chunk
    for counts in (c.used, c.used_out):
        if counts is not None:
            counts.zero_()
    c.noise_iter = iter(c.draws) if c.draws is not None else None
    results = defaultdict(list)
    staging = SimpleNamespace(stream=_copy_stream(rays.device), buffers={}, rows=defaultdict(int), hold=[]) \
        if c.to_cpu == "maps" and rays.is_cuda else None
    starts = list(range(0, rays.shape[0], chunk))
    pipelined = rays.is_cuda and not c.jitters and len(starts) > 1 and os.environ.get("MNRF_EVAL_PIPELINE", "1") != "0"
    host = (torch.zeros(2, dtype=torch.int32).pin_memory(), torch.zeros(2, dtype=torch.int64).pin_memory()) if pipelined else None
    source = lambda i: c.source_all[i:i + chunk] if c.source_all is not None else None  # noqa: E731
    primary = lambda n_c: _stage_a(c, rays[starts[n_c]:starts[n_c] + chunk].contiguous(), 0, host, n_c % 2, source(starts[n_c]))  # noqa: E731
    ahead = primary(0) if (pipelined and starts) else None
    for n_c, i in enumerate(starts):
        if pipelined:
            state = ahead
            ahead = primary(n_c + 1) if n_c + 1 < len(starts) else None
            out = _stage_b(c, state)
        else:
            out = _recurse(c, rays[i:i + chunk].contiguous(), 0, source(i))
        _collect(c, out, results, staging)
    if staging is not None:       # one host-side copy out of the (re-used) staging buffers hands back tensors the caller owns
        staging.stream.synchronize()
        staging.hold.clear()
        for k, buf in staging.buffers.items():
            results[k] = [buf[:staging.rows[k]].clone()]
    return results


@torch.no_grad()
def batched_inference(models, embeddings, rays, N_samples, N_importance, use_disp, chunk, **kwargs):
    """eval.batched_inference.  kwargs: args (namespace/dict with predict_normal, only_one_field,
    only_one_field_fine_epoch, max_recursive_level, app_control_mirror_roughness, trace_ray_times),
    trace_secondary_rays, normal_noise_std, test_time, white_back (the reference reads the module
    global `dataset.white_back`), to_cpu (True, the default: eval.py:735-736 moves every value to the CPU; False: keep
    everything on the device; "maps": return only the per-ray maps -- rgb, depth, opacity, mirror mask, normals,
    x_surface, ~100 B/ray instead of ~3 KB/ray of per-sample tensors nobody downstream of eval.py:743-894 reads -- on
    the CPU), batch_jitter (roughness: render the trace_ray_times jittered reflections of a level in groups through one
    recursion call each instead of one by one; default on unless draws are injected), blended_level (default "auto": a chunk
    of a level that traces renders its fine pass with the blended-level launch, which leaves out the colour of mirror rays,
    when the chunk last counted at that level held enough of them for it to pay -- same result either way; True / False force
    the choice, see _stage_a),
    _normal_noise (iterator of pre-drawn (n,3) standard-normal tensors, for tests).

    args.app_control_mirror_roughness with args.trace_ray_times and normal_noise_std= (eval.py:506-511, 622-674), on chunks with
    ANY share of mirror rays.  THE RULE (include/mnrf.h "Mirror roughness"), at a level that traces: R, the first
    secondary render, is as without roughness but reflected about l2n(normal + draw_0 * std) -- every ray of the chunk at level 0,
    the M mirror rays at levels >= 1; J_j, j = 1 .. trace_ray_times, renders the M compacted reflections of the mirror rays about
    l2n(normal + draw_j * std); a mirror ray's reflection colour is ((R + J_1) + J_2) + ... of its rows, single fp32 additions
    in that order, finished by trace_ray_times + 1 the way torch's `/` does it on the device: multiplied by the fp32 reciprocal.
    A ray of level 0 that is NOT a mirror ray keeps its row of R, the one sample it has (the blend gives it weight 0; rgb_*_reflect
    stays a consistent image).  One (N,3) draw per jitter, in the reference's order.  Where every ray of a chunk is a mirror ray
    this is the reference's arithmetic; where not, the reference's own addition of (M,3) to (N,3) raises or, with M == 1,
    broadcasts, so there is nothing of it to reproduce.  One order-preserving compaction of the mask and one host read of its
    count per chunk and level, whatever trace_ray_times is (mnrf_reflect_compact with compact = 1; then mnrf_reflect_jitter_fan
    and mnrf_jitter_mean per group of jitters; batch_jitter=False keeps one _reflect, with its count read, per jitter and adds
    through mnrf_jitter_mean too).

    Applications (the reference's flags, unchanged): args.app_place_new_mirror with args.plane_pos / args.root_dir (the
    preset, PLACE_MIRROR_PRESETS) and args.near -- every level below max_recursive_level traces, the new mirror is merged into
    the mirror mask right behind the threshold (mnrf_place_mirror), `new_mirror=dict(axis=, position=, normal=, rect=)`
    overrides the preset; args.app_reflection_substitution with system_substitution= (.models, .embeddings): the level-0
    reflections are moved by the args.root_dir preset (SUBSTITUTION_PRESETS, mnrf_transform_rays) and rendered once by
    that system.  Both may be combined, as in the reference.

    args.app_reflect_newly_placed_objects with args.obj_model_type="nerf_pl" and system_obj= (.models: the nerf_pl list
    [coarse, fine] or a dict; .embeddings: [xyz, dir] or a dict; load_object_system), or with args.obj_model_type="d_nerf" (the
    reference's default) and render_kwargs_test_d_nerf= (dnerf.load_dnerf_object) plus frame_time= (the object's time: it moves
    from frame to frame, and its reflection with it; args_d_nerf= is accepted and unused), and
    args.near: at EVERY recursion level, the last one included, the level's rays are moved into the object's frame by the
    args.root_dir preset (OBJECT_PRESETS; `new_object=dict(pose_align=None | 3x4 | 4x4, scale=, translation=)` overrides it),
    the object field is rendered for colour, depth and opacity, and where the object is opaque and not hidden by the scene it
    gives the level's colour and depth and clears the mirror flag (mnrf_object_rays, mnrf_object_merge) -- so the object is
    seen in the mirrors too.  Not combined with another application.  object_used= (a device int32 tensor of one element,
    zeroed here): receives the number of rays, over all levels, that took the object.
    object_bounds= (None, the default: every ray of a level renders the object; an object_bounds.ObjectBounds; or "auto" with
    object_region=(lo, hi) and optionally object_bounds_res=64, see resolve_object_bounds): the object is rendered only along
    the rays whose segment, in the object's frame, can touch the bounds (mnrf_object_cull, mnrf_object_merge_indexed).  Those
    rays get bit for bit what they get without bounds; the others stay as the scene rendered them.  Costs one more 4-byte
    device->host read per chunk and level.

    placed_objects=[PlacedObject(field, placement, bounds=, region=, bounds_res=, time=), ...] (placed_objects.py; 1..8
    objects, nerf_pl and D-NeRF mixed, each with its own placement, bounds and -- a D-NeRF object -- time, None meaning
    frame_time=) with args.app_reflect_newly_placed_objects: several objects, each seen in the mirrors.  It replaces the
    single-object keywords (system_obj=, render_kwargs_test_d_nerf=, new_object=, object_bounds=, object_region= are refused
    beside it) and args.obj_model_type is not consulted.  THE RULE, at every recursion level, the last included, ahead of the
    hard clip: per ray, for k = 0 .. K-1 in list order, the single-object merge above of object k is applied to the ray's
    current (rgb, depth, mask) -- current: as left by the scene and by the objects 0 .. k-1.  This is by definition the chain
    of K single-object applications.  The merge writes depth = d, so the nearest opaque object wins; an exact tie in depth
    goes to the LATER object of the list; a current depth <= near hides nothing, as in the reference's own rule
    (eval.py:275-281).  x_surface and the normals are not edited.  One mnrf_objects_cull, one read of the K counts, the
    renders of the objects with kept rays and one mnrf_objects_merge per chunk and level (_merge_placed).  object_used= is
    then a device int32 tensor of K elements -- element k: the number of rays, over all levels, that took object k when its
    turn came; a ray that a later, nearer object then takes counts for BOTH -- or of 1 element, which receives their sum.
    _object_chain=True (tests, measurements): the same list through K successive single-object passes (_merge_object), the
    launches of the single-object path; the result is the same bit for bit.

    new_mirrors=[PlacedMirror(center, normal, up, size, shape=) | PlacedMirror.axis_aligned(axis, position, normal, rect, shape=),
    ...] (placed_mirrors.py; 1..8 mirrors, on any plane, rectangular or elliptic) with args.near: like app_place_new_mirror it
    implies tracing and takes the un-blended route; at every level below the last, right behind the threshold (where the single
    mirror is merged), ONE mnrf_place_mirrors applies THE RULE of include/mnrf.h: every mirror is tested against the level's
    depth as it is before any mirror of the call, per ray the nearest hit wins (an exact tie goes to the later mirror) and writes
    x_surface, depth and normal; the normal of a ray inside a shape that takes no mirror is KEPT (the single mirror overwrites
    it, eval.py:458-460: that is why mirrors cannot be chained).  Allowed beside placed_objects= (the objects are merged first,
    the mirrors see the resulting depth) and beside app_reflection_substitution; refused beside app_place_new_mirror /
    new_mirror=, the single-object keywords and roughness.  The result gains new_mirror_index: int32 per ray of the call's own
    rays, the mirror the ray took at level 0, -1 for none.

    exclude_source_mirror=True (a bool; default False: nothing changes) with new_mirrors=: a ray never re-hits the placed mirror it
    has just left (include/mnrf.h mnrf_place_mirrors_from).  A ray reflected off a tilted frame mirror starts within
    an ulp of that mirror's plane, on either side; without the keyword THE RULE finds the same mirror again at a distance of 1e-9
    to 1e-7 and reflects the ray a second time off it.  With it every ray of a level carries `source`, the index in the list of
    the placed mirror it was reflected off at the level directly above (-1: the scene's own mirror, no mirror, a ray of the call),
    and mirror `source` is no hit: every level that applies the list keeps its index, _stage_b makes the next level's row from it
    through the compaction (mnrf_mirror_sources: the plain reflection, the rough_times fan and its one-by-one form), and the
    launch is mnrf_place_mirrors_from.  Only the mirror left directly above is excluded: a ray may return to it after another
    bounce.  source_mirror= ((N,) int32 on the rays' device, default all -1; another dtype, shape or device is refused): the
    `source` of the call's own rays, for a caller that traces level by level; sliced per chunk.  Allowed wherever new_mirrors=
    is; under substitution nothing recurses, so it changes nothing there.  new_mirror_index stays level 0's.

    rough_times=T (an int >= 1; None, the default: off) with scene_roughness=S (float32, >= 0, finite; default 0) and the
    `roughness` of each PlacedMirror: a roughness PER MIRROR (include/mnrf.h "A roughness per mirror").  At a level
    that traces, the std of ray i is the roughness of the placed mirror it took at THAT level (mnrf_place_mirrors' index) or S
    where it took none -- the scene's own mirrors.  The first reflection is the existing one, about l2n(normal + draw_0 * std_i)
    where std_i > 0 and about l2n(normal) with no addition where std_i == 0 (the bits of the frame without roughness); the rays
    of J = {mask != 0 and std > 0} get T further reflections about l2n(normal + draw_j * std_i) and the mean of their T + 1
    samples, added and finished as the roughness rule above does it; a mirror ray outside J (a polished mirror) and a ray of
    level 0 that is no mirror ray keep their single sample.  One (N,3) draw per tracing level, then T more iff J is not empty:
    where every std equals S > 0 the draws, the launches' inputs and the result are those of args.app_control_mirror_roughness
    with trace_ray_times = T and normal_noise_std = S.  At most two count reads per chunk and level (the mask's at levels >= 1,
    J's), whatever T is.  mnrf_rough_rows, mnrf_perturb_normals and mnrf_reflect_jitter_fan_rows; batch_jitter=False makes a
    jitter mnrf_perturb_normals followed by mnrf_reflect_compact on J's mask.  Allowed alone, beside new_mirrors=, beside
    placed_objects= (the objects are merged at every level of every render, the jittered ones included; object_used counts
    every render) and beside both; refused beside args.app_control_mirror_roughness (one roughness rule per call),
    app_place_new_mirror / new_mirror=, the single-object keywords and app_reflection_substitution.  normal_noise_std= and
    args.trace_ray_times are not read; _normal_noise= and batch_jitter= work as with the flag.  Without rough_times a mirror
    with roughness > 0, or a scene_roughness > 0, is refused.  The route takes the exclusions of the flag: no pipelined
    stage, no blended level, no colour/depth-only last level."""
    c = _resolve_call(models, rays, N_samples, N_importance, use_disp, chunk, kwargs)
    c.embeddings = embeddings
    results = _run_chunks(c)
    # range guard of the split arithmetic, once per call (= per frame): a tripped model is on the fp32 kernels now, and the
    # chunks are rendered once more, from the same resolved call
    if c.rays.shape[0] and check_guard(c.guarded):
        try:
            results = _run_chunks(c)
        finally:
            release_transient(c.guarded)      # (a range-only trip: this frame on fp32, the next one on split again)
    if c.used_out is not None:
        c.used_out.copy_(c.used if c.used_out.numel() == c.used.numel() else c.used.sum(dtype=torch.int32).view(1))
    return {k: torch.cat(v, 0) for k, v in results.items()}
