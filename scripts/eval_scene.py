#!/usr/bin/env python3
"""The counterpart of the reference's `python eval.py` for the Blender layout and for real captures (--dataset_name
real_arkit: datasets/real_arkit.py's layout, data.read_arkit): renders every frame of a split from a checkpoint and leaves the
reference's output directory behind.

    python scripts/eval_scene.py --root_dir data/scene --split test --img_wh 800 800 --ckpt_path ckpts/exp/last.ckpt \\
        --N_samples 64 --N_importance 128 --trace_secondary_rays --out_dir results/blender/exp

Per frame: RayBank.frame (rays made on the device), batched_inference(to_cpu=False, maps_only=True), frames.finish_frame (the
8-bit images, on the device), metrics.psnr against the ground truth (on the device), ONE device-to-host copy of the uint8
images into pinned staging, and PNGs written with PIL from a small thread pool.  The float depth maps stay resident; after the
last frame frames.colormap_depth re-colours them with the split-wide extremes (save_depth_unified_normalization) and the mean
PSNR line is printed.  Directory and file names are eval.py's (eval.py:1095-1116, 743-978):

    rgb_{typ}_{i:03d}.png                       depth/depth_{typ}_{i:03d}.png [.pfm] [raw bytes]
    mirror_mask/mirror_mask_{typ}_{i:03d}.png   depth_reflect/depth_reflect_{typ}_{i:03d}.png
    normal/surface_normal[_grad]_{typ}_{i:03d}.png      x_surface/x_surface_{typ}_{i:03d}.png
    depth_unified_normalization/depth_{typ}_{i:03d}.png
    depth_reflect_unified_normalization/depth_reflect_{typ}_{i:03d}.png

`pfm` and `bytes` in --depth_format copy the float depth map as well.

The fly-through splits of a real capture (--split test_rotate | test_interpolation) carry poses only: the rays of a frame come
from synthetic.generate_rays, there is no ground truth and so no PSNR line, the files keep the same names, and the frames'
GIF `{exp}_rgb_{typ}.gif` (eval.py:897-903; exp = --exp_name, by default the last component of --out_dir; 15 frames per
second) is written with PIL.  That GIF is NOT pinned against imageio's: the frames are the PNGs' bytes, the palette and the
container are PIL's.

A newly placed object (run.sh MODE 4): --app_reflect_newly_placed_objects --obj_ckpt_path PATH --obj_model_type nerf_pl loads
the object's nerf_pl checkpoint (recursion.load_object_system) and hands it to batched_inference, which shows the object in
the scene and in its mirrors; the preset of the ray move follows --root_dir as in the reference.  --obj_model_type d_nerf (the
reference's default) loads a D-NeRF `.tar` checkpoint with the `config.txt` beside it (dnerf.load_dnerf_object) and renders
frame i at frame_time = i / n_frames (eval.py:1130, 1154): the object moves from frame to frame, and in the mirrors with it.
--obj_bounds x0 y0 z0 x1 y1 z1 | auto renders the object only along the rays that can touch the given box of ITS frame, or
the cells `auto` finds occupied inside --obj_region at --obj_bounds_res cells per axis (object_bounds.py): the rays that are
kept get exactly what they get without the flag.

Several objects: --app_reflect_newly_placed_objects --objects_json FILE, a JSON list of entries

    {"ckpt_path": ..., "model_type": "nerf_pl" | "d_nerf", "pose_align": null | 3x4 | 4x4, "scale": 1.0, "translation": [0, 0, 0],
     "bounds": null | [x0, y0, z0, x1, y1, z1] | "auto", "region": [x0, y0, z0, x1, y1, z1], "bounds_res": 64,
     "time_offset": 0.0, "time_scale": 1.0}

(ckpt_path and model_type are required; a relative ckpt_path is taken from the file's directory) places up to 8 objects, each
with its own placement and bounds, through batched_inference(placed_objects=): per ray they are merged in list order by the
single-object rule, so the nearest opaque object wins and a tie in depth goes to the later entry.  Frame i of n renders D-NeRF
object j at time_offset + time_scale * i / n; a time outside [0, 1] is refused before the first frame.  The flag replaces
--obj_ckpt_path and the --obj_* flags and is refused beside them.

New mirrors: --app_place_new_mirror [--plane_pos plane_x | plane_y] places the reference's mirror (run.sh MODE 3; the preset
follows --root_dir).  --mirrors_json FILE, a JSON list of up to 8 entries

    {"center": [x, y, z], "normal": [x, y, z], "up": [x, y, z], "size": [width, height], "shape": "rect" | "ellipse"}
    {"axis": "x" | "y", "position": c, "normal": [x, y, z], "rect": [u0, u1, w0, w1], "shape": "rect" | "ellipse"}

(shape is optional) places several mirrors on any plane through batched_inference(new_mirrors=): per ray the nearest one that
the scene does not hide wins.  It implies tracing, may be combined with --objects_json (a placed object is then seen in the
placed mirrors) and is refused beside --app_place_new_mirror.  An entry of either kind may carry "roughness": s, the standard
deviation of the normal jitter of the rays that take that mirror (read with --rough_times, below).
--exclude_source_mirror, beside --mirrors_json and --max_recursive_level 2 or more: a reflected ray never re-hits the placed
mirror it has just left (batched_inference(exclude_source_mirror=True)) -- what two mirrors that face each other need unless
their normals are world axes.

Mirror roughness (run.sh "control_mirror_roughness"): --app_control_mirror_roughness --trace_ray_times T --normal_noise_std S
renders every mirror pixel as the mean of T + 1 reflections about jittered normals (batched_inference's roughness rule: a
frame may hold any share of mirror pixels; a pixel that is no mirror keeps its single reflection sample in rgb_*_reflect).
--normal_noise_std_changes lets S follow the reference's per-frame cycle (eval.py:1130-1136): frame i of n uses
S * c with p = i / n and c = 2 p below one half, 1 - 2 (p - 0.5) from there on.  The flag is refused beside the object and
new-mirror applications, with batched_inference's own messages.

A roughness per mirror: --rough_times T [--scene_roughness S] renders the pixels of every mirror whose roughness is not 0 as the
mean of T + 1 reflections about jittered normals (batched_inference(rough_times=, scene_roughness=)): a placed mirror has the
"roughness" of its --mirrors_json entry, the scene's own mirrors have S (default 0: polished), and a polished mirror is traced
once.  Allowed alone, beside --mirrors_json and beside --objects_json; refused beside --app_control_mirror_roughness (one
roughness rule per call) and --app_place_new_mirror.  --trace_ray_times and --normal_noise_std are not read, and the per-frame
cycle of --normal_noise_std_changes does not apply.

Out of scope: the other GIFs of save_gif_and_print_mean_psnr (imageio is not a dependency of this project), the COLMAP reader,
reflection substitution (batched_inference has it; this driver does not expose its flags) and --render_coarse_rgb (it sets
test_time=False and writes a second set of coarse images, eval.py:1148, 1178: the driver renders with test_time=True only).  The
depth colour table is frames.jet_table(), a restatement that is not pinned against cv2.COLORMAP_JET.  Needs a GPU: there is no
CPU path.
"""
import argparse
import os
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def get_opts(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root_dir", type=str, required=True, help="root directory of the dataset (transforms_{split}.json)")
    ap.add_argument("--dataset_name", type=str, default="blender", choices=("blender", "real_arkit"))
    ap.add_argument("--split", type=str, default="test",
                    help="test or test_train; with real_arkit also val, test_rotate and test_interpolation (poses only)")
    ap.add_argument("--scale_factor", type=float, default=1.0, help="real_arkit: translations, near and far are divided by it")
    ap.add_argument("--val_idx", type=int, default=0, help="real_arkit: the frame of val and the one test_rotate moves around")
    ap.add_argument("--exp_name", type=str, default=None, help="prefix of the GIF (default: the last component of --out_dir)")
    ap.add_argument("--img_wh", nargs=2, type=int, default=[800, 800], help="resolution (img_w, img_h) of the image")
    ap.add_argument("--ckpt_path", type=str, required=True, help="checkpoint holding nerf_coarse.* / nerf_fine.*")
    ap.add_argument("--trusted", action="store_true", help="unpickle the checkpoint fully (only for files you wrote)")
    ap.add_argument("--N_samples", type=int, default=64, help="number of coarse samples")
    ap.add_argument("--N_importance", type=int, default=128, help="number of additional fine samples")
    ap.add_argument("--chunk", type=int, default=32 * 1024, help="rays per pass")
    ap.add_argument("--depth_format", type=str, default="png", help="which of png, pfm, bytes to write (any substring)")
    ap.add_argument("--not_save_depth", action="store_true", help="write no depth maps")
    ap.add_argument("--out_dir", type=str, required=True, help="the reference's results/{dataset_name}/{exp_name}")
    # the model and the recursion, named as in the reference's opt.py; NeRFSystem builds whichever model_type asks for
    ap.add_argument("--model_type", type=str, default="nerf", choices=("nerf", "nerf_tcnn"))
    ap.add_argument("--bound", type=float, default=1.0, help="scene bound of the hash grid (nerf_tcnn)")
    ap.add_argument("--N_emb_xyz", type=int, default=10)
    ap.add_argument("--N_emb_dir", type=int, default=4)
    ap.add_argument("--no_predict_normal", dest="predict_normal", action="store_false")
    ap.add_argument("--no_predict_mirror_mask", dest="predict_mirror_mask", action="store_false")
    ap.add_argument("--only_one_field", action="store_true")
    ap.add_argument("--only_one_field_fine_epoch", type=int, default=2)
    ap.add_argument("--use_disp", action="store_true")
    ap.add_argument("--white_back", action="store_true")
    ap.add_argument("--trace_secondary_rays", action="store_true")
    ap.add_argument("--max_recursive_level", type=int, default=1)
    ap.add_argument("--near", type=float, default=2.0)
    ap.add_argument("--far", type=float, default=6.0)
    ap.add_argument("--workers", type=int, default=8, help="PNG-writing threads (at most 16)")
    # the new-object application, named as in the reference's eval.py
    ap.add_argument("--app_reflect_newly_placed_objects", action="store_true",
                    help="show a newly placed object in the scene and in its mirrors")
    ap.add_argument("--obj_ckpt_path", type=str, default=None, help="radiance field of the object (a nerf_pl .ckpt, or a D-NeRF .tar beside its config.txt)")
    ap.add_argument("--obj_model_type", type=str, default="d_nerf", choices=("nerf_pl", "d_nerf"))
    ap.add_argument("--obj_bounds", nargs="+", default=None, metavar="x0 y0 z0 x1 y1 z1 | auto",
                    help="render the object only along rays that can touch these bounds, in the OBJECT's frame: a box, or `auto` "
                         "(estimated from the object's density inside --obj_region)")
    ap.add_argument("--obj_region", nargs=6, type=float, default=[-1.5, -1.5, -1.5, 1.5, 1.5, 1.5], metavar="V",
                    help="x0 y0 z0 x1 y1 z1 of the region `--obj_bounds auto` looks for the object in.  The default is the extent of the "
                         "Blender-synthetic scenes such objects are trained in (cameras at radius 4, near 2, far 6): a guess, override it")
    ap.add_argument("--obj_bounds_res", type=int, default=64, help="cells per axis of the estimated bounds")
    ap.add_argument("--objects_json", type=str, default=None,
                    help="several placed objects: a JSON list of {ckpt_path, model_type, pose_align, scale, translation, bounds, region, "
                         "bounds_res, time_offset, time_scale}; replaces --obj_ckpt_path and the --obj_* flags")
    # new mirrors: the reference's single mirror, and several on any plane
    ap.add_argument("--app_place_new_mirror", action="store_true", help="place the reference's new mirror (the preset of --plane_pos and --root_dir)")
    ap.add_argument("--plane_pos", type=str, default="plane_x", choices=("plane_x", "plane_y"))
    ap.add_argument("--mirrors_json", type=str, default=None,
                    help="several new mirrors: a JSON list of {center, normal, up, size, shape} or {axis, position, normal, rect, shape}")
    ap.add_argument("--exclude_source_mirror", action="store_true",
                    help="with --mirrors_json: a reflected ray never re-hits the placed mirror it has just left (facing mirrors, two bounces or more)")
    # mirror roughness, named as in the reference's eval.py:60-70
    ap.add_argument("--app_control_mirror_roughness", action="store_true",
                    help="render mirror pixels as the mean of trace_ray_times + 1 reflections about jittered normals")
    ap.add_argument("--trace_ray_times", type=int, default=4, help="jittered reflections per mirror pixel beside the first")
    ap.add_argument("--normal_noise_std", type=float, default=0.01, help="standard deviation of the jitter added to the normal")
    ap.add_argument("--normal_noise_std_changes", action="store_true",
                    help="scale --normal_noise_std by the frame's place in the split: 0 -> 1 -> 0 (eval.py:1130-1136)")
    # a roughness per mirror: this project's own flags (batched_inference rough_times=, scene_roughness=)
    ap.add_argument("--rough_times", type=int, default=None,
                    help="jittered reflections beside the first for the rays of every mirror whose roughness is not 0")
    ap.add_argument("--scene_roughness", type=float, default=0.0,
                    help="with --rough_times: the jitter's standard deviation on the scene's own mirrors (placed ones: `roughness` in --mirrors_json)")
    args = ap.parse_args(argv)
    if args.rough_times is not None:           # batched_inference's own refusals (_refuse_rough_rows), before anything is loaded
        if args.rough_times < 1:
            ap.error("--rough_times counts the jittered reflections beside the first: at least 1")
        if not 0 <= args.scene_roughness < float("inf"):
            ap.error("--scene_roughness must be finite and not negative")
        if args.app_control_mirror_roughness:
            ap.error("rough_times= cannot be combined with app_control_mirror_roughness: one roughness rule per call")
        if args.app_place_new_mirror:
            ap.error("rough_times= cannot be combined with app_place_new_mirror (the single mirror carries no roughness; an entry "
                     "{axis, position, normal, rect, roughness} of --mirrors_json is that mirror)")
        if args.app_reflect_newly_placed_objects and args.objects_json is None:
            ap.error("rough_times= is combined with objects through --objects_json, not with --obj_ckpt_path")
    elif args.scene_roughness != 0:
        ap.error("--scene_roughness is read with --rough_times T alone")
    if args.app_control_mirror_roughness:      # batched_inference's own refusals (_refuse_apps), before anything is loaded
        if args.trace_ray_times < 0:
            ap.error("--trace_ray_times counts renders: it cannot be negative")
        if args.app_reflect_newly_placed_objects:
            ap.error("app_reflect_newly_placed_objects cannot be combined with app_control_mirror_roughness (one application at a time)")
        if args.app_place_new_mirror:
            ap.error("app_control_mirror_roughness cannot be combined with app_place_new_mirror (one application at a time, except "
                     "place-mirror with substitution)")
        if args.mirrors_json is not None:
            ap.error("app_control_mirror_roughness cannot be combined with new_mirrors= (one application at a time, except "
                     "placed mirrors with placed objects or substitution)")
    if args.exclude_source_mirror and args.mirrors_json is None:
        ap.error("--exclude_source_mirror keeps a ray from hitting the placed mirror it has just left: it needs --mirrors_json")
    if args.mirrors_json is not None and args.app_place_new_mirror:
        ap.error("--mirrors_json carries every new mirror: it cannot be combined with --app_place_new_mirror (an entry "
                 "{axis, position, normal, rect} is that mirror)")
    if args.objects_json is not None:
        given = sorted({a.split("=")[0] for a in (sys.argv[1:] if argv is None else argv) if str(a).startswith("--obj_")})
        if given:
            ap.error(f"--objects_json carries every object's checkpoint, kind and bounds: it cannot be combined with {', '.join(given)}")
        if not args.app_reflect_newly_placed_objects:
            ap.error("--objects_json lists the objects of --app_reflect_newly_placed_objects")
    if args.obj_bounds is not None:
        if not args.app_reflect_newly_placed_objects:
            ap.error("--obj_bounds bounds the object of --app_reflect_newly_placed_objects")
        if args.obj_bounds != ["auto"]:
            try:
                args.obj_bounds = [float(v) for v in args.obj_bounds]
            except ValueError:
                args.obj_bounds = []
            if len(args.obj_bounds) != 6:
                ap.error("--obj_bounds takes six numbers (x0 y0 z0 x1 y1 z1) or `auto`")
    return args


def load_system(args, device):
    """NeRFSystem for args.model_type with every model loaded from args.ckpt_path (eval.py:995-1001)."""
    import mirror_nerf_amd as M
    from mirror_nerf_amd import checkpoint
    system = M.NeRFSystem(args)
    for key, model in system.models.items():
        checkpoint.load_ckpt(model, args.ckpt_path, model_name="nerf_" + key if key in ("coarse", "fine") else key,
                             trusted=args.trusted)
        model.to(device).eval()
    return system


def load_object(args, device):
    """The object of --app_reflect_newly_placed_objects (eval.py:1035-1077) as the keyword of batched_inference that carries
    it: {"system_obj": ...} for a nerf_pl object, {"render_kwargs_test_d_nerf": ...} for a D-NeRF one; {} without the flag."""
    if not args.app_reflect_newly_placed_objects:
        return {}
    if args.obj_ckpt_path is None:
        raise SystemExit("[Error] obj_ckpt_path should be appointed in app_reflect_newly_placed_objects.")
    print("[info] Load object radiance field from ckpt:", args.obj_ckpt_path)
    if args.obj_model_type == "d_nerf":
        from mirror_nerf_amd.dnerf import load_dnerf_object
        return {"render_kwargs_test_d_nerf": load_dnerf_object(args.obj_ckpt_path, device, trusted=args.trusted)}
    from mirror_nerf_amd.recursion import load_object_system
    return {"system_obj": load_object_system(args.obj_ckpt_path, device, args.N_importance, trusted=args.trusted)}


OBJECT_KEYS = {"ckpt_path": None, "model_type": None, "pose_align": None, "scale": 1.0, "translation": (0.0, 0.0, 0.0), "bounds": None,
               "region": (-1.5, -1.5, -1.5, 1.5, 1.5, 1.5), "bounds_res": 64, "time_offset": 0.0, "time_scale": 1.0}


def read_objects_json(path):
    """--objects_json FILE -> the list of entries, every key present (OBJECT_KEYS holds the defaults), refused with the reason
    when the file is not what the flag describes."""
    import json
    with open(path) as f:
        entries = json.load(f)
    if not isinstance(entries, list) or not 1 <= len(entries) <= 8:
        raise SystemExit(f"[Error] {path}: --objects_json takes a list of 1..8 objects")
    out = []
    for j, e in enumerate(entries):
        if not isinstance(e, dict):
            raise SystemExit(f"[Error] {path}: object {j} is not a JSON object")
        unknown, missing = sorted(set(e) - set(OBJECT_KEYS)), [k for k in ("ckpt_path", "model_type") if e.get(k) is None]
        if unknown or missing:
            raise SystemExit(f"[Error] {path}: object {j}: unknown keys {unknown}, missing keys {missing} (known: {sorted(OBJECT_KEYS)})")
        e = dict(OBJECT_KEYS, **e)
        if e["model_type"] not in ("nerf_pl", "d_nerf"):
            raise SystemExit(f"[Error] {path}: object {j}: model_type must be 'nerf_pl' or 'd_nerf', not {e['model_type']!r}")
        b = e["bounds"]
        if not (b is None or b == "auto" or (isinstance(b, list) and len(b) == 6)):
            raise SystemExit(f"[Error] {path}: object {j}: bounds must be null, [x0, y0, z0, x1, y1, z1] or \"auto\", not {b!r}")
        if len(e["region"]) != 6:
            raise SystemExit(f"[Error] {path}: object {j}: region holds six numbers (x0 y0 z0 x1 y1 z1)")
        if not os.path.isabs(e["ckpt_path"]):
            e["ckpt_path"] = os.path.join(os.path.dirname(os.path.abspath(path)), e["ckpt_path"])
        out.append(e)
    return out


MIRROR_KEYS = {"frame": ("center", "normal", "up", "size"), "axis": ("axis", "position", "normal", "rect")}


def read_mirrors_json(path):
    """--mirrors_json FILE -> the list of PlacedMirror, refused with the file and the entry's index when the file is not what
    the flag describes.  An entry with the key `axis` is an axis-aligned mirror, any other a mirror on a frame."""
    import json
    from mirror_nerf_amd import PlacedMirror
    with open(path) as f:
        entries = json.load(f)
    if not isinstance(entries, list) or not 1 <= len(entries) <= 8:
        raise SystemExit(f"[Error] {path}: --mirrors_json takes a list of 1..8 mirrors")
    out = []
    for j, e in enumerate(entries):
        if not isinstance(e, dict):
            raise SystemExit(f"[Error] {path}: mirror {j} is not a JSON object")
        kind = "axis" if "axis" in e else "frame"
        known = MIRROR_KEYS[kind] + ("shape", "roughness")
        unknown, missing = sorted(set(e) - set(known)), [k for k in MIRROR_KEYS[kind] if e.get(k) is None]
        if unknown or missing:
            raise SystemExit(f"[Error] {path}: mirror {j}: unknown keys {unknown}, missing keys {missing} (known: {sorted(known)}; "
                             f"or those of the other kind, {sorted(MIRROR_KEYS['frame' if kind == 'axis' else 'axis'])})")
        try:
            e = dict(e, shape=e.get("shape") or "rect", roughness=0.0 if e.get("roughness") is None else e["roughness"])
            out.append(PlacedMirror.axis_aligned(**e) if kind == "axis" else PlacedMirror(**e))
        except (TypeError, ValueError) as err:
            raise SystemExit(f"[Error] {path}: mirror {j}: {err}") from None
    return out


def object_time(entry, i, n_frames):
    return float(entry["time_offset"]) + float(entry["time_scale"]) * i / n_frames


def check_object_times(entries, n_frames):
    """A D-NeRF object's time of every frame lies in [0, 1], or nothing is rendered."""
    for j, e in enumerate(entries):
        if e["model_type"] != "d_nerf":
            continue
        for i in range(n_frames):
            t = object_time(e, i, n_frames)
            if not 0.0 <= t <= 1.0:
                raise SystemExit(f"[Error] --objects_json: object {j} would be rendered at time {t:.4f} in frame {i} of {n_frames} "
                                 f"(time_offset {e['time_offset']} + time_scale {e['time_scale']} * i / n): outside [0, 1]")


def load_placed(entries, args, device):
    """The fields of --objects_json, loaded once: [(entry, field)]."""
    from mirror_nerf_amd.dnerf import load_dnerf_object
    from mirror_nerf_amd.recursion import load_object_system
    fields = []
    for j, e in enumerate(entries):
        print(f"[info] Load object {j} ({e['model_type']}) from ckpt:", e["ckpt_path"])
        if e["model_type"] == "d_nerf":
            fields.append((e, load_dnerf_object(e["ckpt_path"], device, trusted=args.trusted)))
        else:
            fields.append((e, load_object_system(e["ckpt_path"], device, args.N_importance, trusted=args.trusted)))
    return fields


def placed_objects(fields, i, n_frames):
    """The `placed_objects=` list of frame i: every object with its placement and bounds, a D-NeRF object at its time."""
    from mirror_nerf_amd import ObjectBounds, PlacedObject
    out = []
    for e, field in fields:
        b, region = e["bounds"], None
        if isinstance(b, list):
            b = ObjectBounds(b[:3], b[3:])
        elif b == "auto":
            region = (tuple(e["region"][:3]), tuple(e["region"][3:]))
        out.append(PlacedObject(field, dict(pose_align=e["pose_align"], scale=e["scale"], translation=e["translation"]), bounds=b, region=region,
                                bounds_res=e["bounds_res"], time=object_time(e, i, n_frames) if e["model_type"] == "d_nerf" else None))
    return out


_BOUNDS = {}      # id(the nerf_pl object) -> its bounds: estimated once; a D-NeRF object is estimated per frame


def object_bounds(args, obj, frame_time=None):
    """--obj_bounds as the ObjectBounds batched_inference takes (None without the flag).  `auto` estimates them from the
    object's density inside --obj_region and says what it found: the share of set cells, the tight box around them, and a
    warning when set cells touch the region's border (the object may continue outside: widen --obj_region)."""
    from mirror_nerf_amd import ObjectBounds, estimate_object_bounds
    spec = getattr(args, "obj_bounds", None)
    if spec is None or not obj:
        return None
    if spec != ["auto"]:
        return ObjectBounds(spec[:3], spec[3:])
    moving = "render_kwargs_test_d_nerf" in obj
    target = obj["render_kwargs_test_d_nerf"] if moving else obj["system_obj"]
    if not moving and id(target) in _BOUNDS:
        return _BOUNDS[id(target)]
    region = args.obj_region
    b = estimate_object_bounds(target, region[:3], region[3:], res=args.obj_bounds_res, frame_time=frame_time if moving else None)
    total = b.res[0] * b.res[1] * b.res[2]
    when = f" at frame_time {frame_time:.4f}" if moving else ""
    print(f"[info] object bounds{when}: {b.n_set} of {total} cells set ({100.0 * b.n_set / total:.1f} %), tight box {b.tight_box()}")
    if b.touches_region_border():
        print("[warning] object bounds: set cells touch the border of --obj_region; the object may continue outside it, where it "
              "would be culled: widen --obj_region")
    if not moving:
        _BOUNDS[id(target)] = b
    return b


def frame_noise_std(args, i, n_frames):
    """eval.py:1130-1136: the jitter of frame i of n -- --normal_noise_std, or with --normal_noise_std_changes that value
    times a cycle that rises from 0 to 1 over the first half of the split and falls back over the second."""
    progress = i / n_frames
    cycle = progress * 2 if progress < 0.5 else 1 - (progress - 0.5) * 2
    return args.normal_noise_std * cycle if args.normal_noise_std_changes else args.normal_noise_std


def render(system, rays, args, obj=None, frame_time=None, placed=None, mirrors=None, normal_noise_std=0):
    """The per-ray maps of one frame, on the device.  obj: load_object's dict; frame_time: the time of a D-NeRF object;
    placed: the frame's list of PlacedObject (--objects_json), in place of obj; mirrors: the list of PlacedMirror
    (--mirrors_json); normal_noise_std: the frame's jitter (--app_control_mirror_roughness).  --rough_times and --scene_roughness
    travel as batched_inference's keywords of the same names."""
    import torch
    import mirror_nerf_amd as M
    extra = dict(obj or {})
    if placed is not None:
        extra = {"placed_objects": placed}
    if mirrors is not None:
        extra["new_mirrors"] = mirrors
        if getattr(args, "exclude_source_mirror", False):
            extra["exclude_source_mirror"] = True
    if getattr(args, "rough_times", None) is not None:
        extra.update(rough_times=args.rough_times, scene_roughness=args.scene_roughness)
    if "render_kwargs_test_d_nerf" in extra:
        extra["frame_time"] = frame_time
    bounds = object_bounds(args, obj, frame_time)
    if bounds is not None:
        extra["object_bounds"] = bounds
    res = M.batched_inference(system.models, system.embeddings, rays, args.N_samples, args.N_importance, args.use_disp,
                              args.chunk, args=args, trace_secondary_rays=args.trace_secondary_rays,
                              white_back=args.white_back, to_cpu=False, maps_only=True, normal_noise_std=normal_noise_std, **extra)
    for k in ("mirror_mask_fine", "mirror_mask_coarse"):      # a new mirror returns the merged mask as torch.bool (eval.py:492-496)
        if k in res and res[k].dtype == torch.bool:
            res[k] = res[k].float()
    return res


def save_pfm(path, image):
    """utils.save_pfm: a little-endian single-channel PFM, rows bottom to top."""
    import numpy as np
    image = np.flipud(np.asarray(image, dtype="<f4"))
    with open(path, "wb") as f:
        f.write(b"Pf\n")
        f.write(f"{image.shape[1]} {image.shape[0]}\n".encode())
        f.write(b"-1.000000\n")
        image.tofile(f)


class Staging:
    """The images of a frame reach the host in ONE device-to-host copy: they are concatenated on the device and land in a
    pinned buffer that is re-used from frame to frame; the arrays handed out are copies the PNG threads own."""

    def __init__(self):
        self.buf = None

    def fetch(self, images):
        import torch
        names = list(images)
        flat = torch.cat([images[k].reshape(-1) for k in names])
        if self.buf is None or self.buf.numel() < flat.numel():
            self.buf = torch.empty(flat.numel(), dtype=torch.uint8).pin_memory()
        self.buf[:flat.numel()].copy_(flat, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        out, o = {}, 0
        for k in names:
            n = images[k].numel()
            out[k] = self.buf[o:o + n].numpy().reshape(tuple(images[k].shape)).copy()
            o += n
        return out


def main(argv=None):
    args = get_opts(argv)
    import torch
    from PIL import Image
    from mirror_nerf_amd import frames, metrics
    from mirror_nerf_amd.data import PATH_SPLITS, RayBank, read_arkit
    if not torch.cuda.is_available():
        raise SystemExit("eval_scene.py needs a GPU: there is no CPU path")
    dev = torch.device("cuda", 0)
    w, h = args.img_wh
    path_split = args.dataset_name == "real_arkit" and args.split in PATH_SPLITS
    if path_split:
        from mirror_nerf_amd import synthetic
        fly = read_arkit(args.root_dir, args.split, (w, h), args.near, args.far, args.scale_factor, args.val_idx)
        n_frames = len(fly["poses"])

        def frame_of(i):
            return {"rays": synthetic.generate_rays(h, w, fly["focal"], fly["poses"][i], fly["near"], fly["far"], dev)}
    else:
        if args.dataset_name == "real_arkit":
            bank = RayBank.from_arkit(args.root_dir, args.split, (w, h), args.near, args.far, args.scale_factor, args.val_idx,
                                      device=dev, workers=args.workers)
        else:
            bank = RayBank.from_blender(args.root_dir, args.split, (w, h), args.near, args.far, device=dev)
        n_frames, frame_of = bank.n_frames, bank.frame
    entries = read_objects_json(args.objects_json) if args.objects_json is not None else None
    mirrors = read_mirrors_json(args.mirrors_json) if args.mirrors_json is not None else None
    if entries is not None:
        check_object_times(entries, n_frames)
    system = load_system(args, dev)
    system_obj = load_object(args, dev) if entries is None else None
    fields = load_placed(entries, args, dev) if entries is not None else None

    out = args.out_dir
    dirs = {"rgb": out, "mirror_mask": os.path.join(out, "mirror_mask"), "depth": os.path.join(out, "depth"),
            "depth_reflect": os.path.join(out, "depth_reflect"), "surface_normal": os.path.join(out, "normal"),
            "surface_normal_grad": os.path.join(out, "normal"), "x_surface": os.path.join(out, "x_surface"),
            "depth_unified": os.path.join(out, "depth_unified_normalization"),
            "depth_reflect_unified": os.path.join(out, "depth_reflect_unified_normalization")}
    save_depth = not args.not_save_depth
    for k, d in dirs.items():
        if save_depth or k not in ("depth", "depth_unified"):
            os.makedirs(d, exist_ok=True)
    print(f"[info] Results saved to dir {out}.")
    depth_png = save_depth and "png" in args.depth_format

    def write_png(path, a):
        Image.fromarray(a.reshape(h, w, 3)).save(path)

    extrema = frames.SplitExtrema(dev)
    staging = Staging()
    depth_maps, reflect_maps, mask_maps, psnrs, gif_frames = [], [], [], [], []
    typ = "fine"
    pending = []
    with ThreadPoolExecutor(max_workers=max(1, min(16, args.workers))) as pool:
        for i in range(n_frames):
            sample = frame_of(i)
            results = render(system, sample["rays"], args, system_obj, frame_time=i / n_frames,      # eval.py:1130
                             placed=placed_objects(fields, i, n_frames) if fields is not None else None, mirrors=mirrors,
                             normal_noise_std=frame_noise_std(args, i, n_frames))
            typ = "fine" if "rgb_fine" in results else "coarse"
            want = [s for s in frames.STEMS if s != "depth" or depth_png]
            images = frames.finish_frame(results, typ, split_extrema=extrema, want=want)
            # eval.py:801-804: against the clipped prediction; the value stays on the device until the end
            if "rgbs" in sample:
                psnrs.append(metrics.psnr(results[f"rgb_{typ}"].clamp(0, 1), sample["rgbs"]))
            if save_depth:
                depth_maps.append(results[f"depth_{typ}"])
            if f"mirror_mask_{typ}" in results and f"depth_{typ}_reflect" in results:
                reflect_maps.append(results[f"depth_{typ}_reflect"])
                mask_maps.append(results[f"mirror_mask_{typ}"])
            for fut in pending:         # at most one frame of PNGs in flight; a failed write surfaces here
                fut.result()
            pending = []
            host = staging.fetch(images)
            if path_split:
                gif_frames.append(Image.fromarray(host[f"rgb_{typ}"].reshape(h, w, 3)))
            for name, a in host.items():
                stem = name[:-len(typ) - 1]
                pending.append(pool.submit(write_png, os.path.join(dirs[stem], f"{name}_{i:03d}.png"), a))
            if save_depth and ("pfm" in args.depth_format or "bytes" in args.depth_format):
                depth = results[f"depth_{typ}"].cpu().numpy().reshape(h, w)
                if "pfm" in args.depth_format:
                    save_pfm(os.path.join(dirs["depth"], f"depth_{typ}_{i:03d}.pfm"), depth)
                if "bytes" in args.depth_format:
                    with open(os.path.join(dirs["depth"], f"depth_{typ}_{i:03d}"), "wb") as f:
                        f.write(depth.tobytes())
        for fut in pending:
            fut.result()

        # save_depth_unified_normalization (eval.py:931-978): every map again, with the extremes of the whole split
        jobs = []
        if depth_png and depth_maps:
            jobs.append(("depth_unified", f"depth_{typ}", frames.colormap_depth(torch.stack(depth_maps), extrema.depth)))
        if reflect_maps:
            jobs.append(("depth_reflect_unified", f"depth_reflect_{typ}",
                         frames.colormap_depth(torch.stack(reflect_maps), extrema.depth_reflect, torch.stack(mask_maps))))
        for key, stem, stack in jobs:
            stack = stack.cpu().numpy()
            pending += [pool.submit(write_png, os.path.join(dirs[key], f"{stem}_{i:03d}.png"), stack[i])
                        for i in range(stack.shape[0])]
        for fut in pending:
            fut.result()

    if gif_frames:      # save_gif_and_print_mean_psnr's first GIF (eval.py:897-903), FPS = 15
        exp = args.exp_name or os.path.basename(os.path.normpath(out))
        gif_frames[0].save(os.path.join(out, f"{exp}_rgb_{typ}.gif"), save_all=True, append_images=gif_frames[1:],
                           duration=round(1000 / 15), loop=0)
    if psnrs:
        mean_psnr = float(torch.stack(psnrs).double().mean())
        print(f"Mean PSNR ({typ}): {mean_psnr:.2f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
