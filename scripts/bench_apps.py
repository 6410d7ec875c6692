#!/usr/bin/env python3
"""Cost of app_place_new_mirror (run.sh MODE 3) and app_reflect_newly_placed_objects (run.sh MODE 4) on the bench.py workload (BASELINE config 2: the synthetic 800x800 frame, 64 coarse
+ 192 fine samples per ray, chunk 32768, the all-mirror random-init pair) through mirror_nerf_amd.batched_inference.

Prints ONE JSON line: ms per frame with the application off (max_recursive_level 1, the bench.py call) and with the new mirror
(default plane_x preset, args.near = 0.05) at max_recursive_level 2 and 50; per run the rays rendered per recursion level (the
rows of every render_rays call of one frame, summed per level) and the rays whose level-0 depth the new mirror replaced (= hits
of the new mirror on the primary rays).  The object leg (--no_object skips it) renders the same frame at max_recursive_level 1
with and without a nerf_pl object -- the seeded random-init plain pair with the density tweaks of fixture g26_object_office_l2,
moved by the office preset -- and reports both times, the rows of the render_rays calls (scene and object renders alternate, so
two entries per level) and the rays, over all levels, that took the object.  The D-NeRF leg (--no_dnerf skips it) does the same with
the two-model D-NeRF object of fixture g27_dnerf_office_l2 (64 + 64 samples per ray of its own, frame_time 0.37): its render is
not a render_rays call, so the rows are per level.  By construction the object costs about one more field pass per level; nothing is asserted on the time.  One warm-up frame, then the median of --reps frames; result maps stay on the GPU
(to_cpu=False, as bench.py).

    python scripts/bench_apps.py [--reps 3] [--levels 2 50] [--no_object] [--no_dnerf]

--obj_bounds runs the object-bounds leg INSTEAD (batched_inference(object_bounds=), on the D-NeRF leg's workload and object): the
application off; then, alternating frame by frame after one warm-up each, the route without bounds and all-keeping bounds (a
+-1e6 box: every ray is kept, so the difference is the overhead of the cull, the count's read and the indexed merge); then
boxes of the object's frame that about 50 %, 10 % and 2 % of the PRIMARY rays hit (a cube around the point the central pixel
looks at, its size bisected with mnrf_object_cull), with the kept rays per level and the time the two parent figures predict,
app_off + kept_fraction x (unculled - app_off).  The random-init object is opaque everywhere, so a culled frame is NOT the
unculled frame: outside the box the object is simply absent.  Nothing is asserted on the times.

    python scripts/bench_apps.py --obj_bounds [--reps 3]

--objects K [K ...] runs the several-objects leg INSTEAD (batched_inference(placed_objects=), on the same workload at
max_recursive_level 1): for each K, K copies of the object (--objects_kind nerf_pl: the object leg's; d_nerf: the D-NeRF leg's)
under the office preset, each bounded by its own cube of the object's frame that about 10 % of the PRIMARY rays hit (cubes
around the points that K pixels spread over the middle row look at, sized by bisection with mnrf_object_cull).  Routes: `fused`
(one mnrf_objects_cull, one read of the K counts, one mnrf_objects_merge per chunk and level), `chain` (_object_chain=True: K
successive single-object passes, the launches of the single-object path) and, for K = 1, `legacy` (the single-object keywords).
One warm-up frame per route, then --reps rounds (default 7 for this leg) that alternate the routes frame by frame; the host
clock around a frame that ends in a synchronise; median and spread (max - min over the median) per route.  Also reported: the
kept rays per object and level, and the device->host reads of kept-ray counts per frame.  Nothing is asserted on the times.

    python scripts/bench_apps.py --objects 1 2 4 [--objects_kind nerf_pl] [--reps 7]

--mirrors K [K ...] runs the several-mirrors leg INSTEAD (batched_inference(new_mirrors=), on the same workload at
max_recursive_level 1; args.near = 1e9, so that the scene -- opaque right in front of the camera -- hides no mirror and every
ray inside the rectangle takes one): for each K, K copies of the default plane_x preset (the plane x = -1, its rectangle and
normal) as PlacedMirror.axis_aligned, copy k moved by 0.05 k along -normal, so the first one wins wherever it is hit and every
frame traces the same rays; beside them `legacy`, the unchanged single-mirror route (app_place_new_mirror with new_mirror= the
preset).  One warm-up frame per route, then --reps rounds (default 7) that alternate the routes frame by frame; the host clock
around a frame that ends in a synchronise; median and spread (max - min over the median) per route, and the rays that took each
mirror.  The edit is one elementwise launch per chunk and level in a frame of field passes: nothing is asserted on the times.

    python scripts/bench_apps.py --mirrors 1 2 4 8 [--reps 7] > profiles/mirrors_bench.json

--rough runs the mirror-roughness leg INSTEAD (app_control_mirror_roughness, batched_inference's roughness rule) and prints one
JSON line with two parts.  (a) the all-mirror BASELINE config 4 workload of benchlegs.roughness_leg's `one_bounce_64_jitters`
(480x360, 64 + 64 samples, chunk 16384, levels 0 and 1, trace_ray_times 64, std 0.0025): ms per frame as the median of --reps
(default 7) frames after one warm-up frame, the spread (max - min over the median), and the device->host reads of a compaction's
count per frame (the calls of recursion._reflect that compact, counted in a frame of their own).  With --parent_root DIR -- a
built checkout of the parent commit -- the same measurement is taken on that checkout's package too: each tree is measured in
child processes of its own (--rough_child; --package_root names the tree whose package the child imports), two rounds per tree,
alternating parent, this, parent, this.  (b) a partly mirrored frame, which the parent cannot render: the STRADDLE random-init
pair at 800x800, bench.py's sample counts and chunk, one bounce, trace_ray_times 4 and 64: ms per frame (median of 3), the share
of mirror rays, the count reads, and beside them the estimate t(roughness off) + times x (mirror rays) x c, with c = t(roughness
off) / (rays the roughness-off frame renders, all levels): the per-ray cost of a render in that frame.  Nothing is asserted.

    python scripts/bench_apps.py --rough [--parent_root DIR] [--reps 7] > profiles/rough_bench.json

--rough_mirrors runs the leg of a roughness per mirror INSTEAD (batched_inference rough_times=, scene_roughness=,
PlacedMirror(roughness=)) on part (b)'s frame -- STRADDLE, 800x800, one bounce -- and prints one JSON line.  Per part one warm-up
and one counting frame per route, then --reps rounds (default 7) alternating the routes frame by frame; median and spread.
(a) rough_times=4, scene_roughness=0.01 alone beside app_control_mirror_roughness with trace_ray_times 4 and std 0.01: the same
draws, launches and result, so the ratio is the route's overhead.  (b) one frosted placed mirror (roughness 0.03) taken by about
5 % and about 25 % of the primary rays, the scene's own mirror polished, T = 4 and 64: ms per frame, the rays in J, the count
reads, and the estimate t(off) + T x |J| x c with c = t(off) / (rays the roughness-off frame renders) and `off` the same frame
with the mirror polished and no rough_times.  (c) the same with scene_roughness=0.01.  Nothing is asserted.

    python scripts/bench_apps.py --rough_mirrors [--reps 7] > profiles/rough_mirrors_bench.json

--mirrors_facing runs the leg of exclude_source_mirror= INSTEAD, on the --mirrors leg's workload with near = 1e9: two parallel frame
mirrors tilted by 0.3 rad about z, one unit in front of the camera (3 x 3, facing it) and one unit behind it (8 x 8, facing it),
at max_recursive_level 1, 2 and 4, each with the keyword off and on.  One warm-up and one counting frame per route, then --reps
rounds (default 7) alternating the six routes frame by frame; median and spread per route, the rays each level renders (level 0:
the frame's; level L + 1: the rows the L-th reflection of a chunk hands on), and the smallest level-1 depth on the rows that
took the first mirror -- the self-hits of the route without the keyword.  At level 1 the keyword changes no ray: `on_over_off`
stands beside the two spreads.  At levels 2 and 4 the two routes trace different rays -- a self-hit row goes on bouncing off
one mirror, an excluded one crosses to the other -- so their times are not compared: nothing is asserted, no speed-up is claimed.

    python scripts/bench_apps.py --mirrors_facing [--reps 7] > profiles/mirrors_facing_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# --package_root DIR (the --rough leg's children): the tree whose mirror_nerf_amd is measured; by default this one
PACKAGE_ROOT = os.path.abspath(sys.argv[sys.argv.index("--package_root") + 1]) if "--package_root" in sys.argv[1:-1] else ROOT
sys.path.insert(0, PACKAGE_ROOT)

import torch  # noqa: E402

import mirror_nerf_amd as M  # noqa: E402
from mirror_nerf_amd import recursion as REC  # noqa: E402
from mirror_nerf_amd import synthetic as SY  # noqa: E402
from mirror_nerf_amd.benchlegs import ARGS, CHUNK, H, N_IMPORTANCE, N_SAMPLES, W  # noqa: E402


def dnerf_object(dev):
    """The object of fixture g27_dnerf_office_l2 as render_kwargs_test_d_nerf: seed 7, two models, density head x 1000 with the
    fixture's biases."""
    from mirror_nerf_amd.dnerf import DirectTemporalNeRF
    torch.manual_seed(7)
    nets = []
    for bias in (7.06, -5.08):
        m = DirectTemporalNeRF()
        with torch.no_grad():
            m._occ.alpha_linear.weight.mul_(1000.0)
            m._occ.alpha_linear.bias.fill_(bias)
        nets.append(m.to(dev).eval())
    return dict(network_fn=nets[0], network_fine=nets[1], N_samples=64, N_importance=64, white_bkgd=False, use_two_models_for_fine=True,
                lindisp=False, perturb=False, raw_noise_std=0.0)


def bounds_leg(a, models, emb, rays, dev, base_args):
    """The --obj_bounds leg (module docstring) -> the result dict."""
    from mirror_nerf_amd import ObjectBounds
    used = torch.zeros(1, dtype=torch.int32, device=dev)
    obj = dict(render_kwargs_test_d_nerf=dnerf_object(dev), frame_time=0.37, object_used=used)
    on_args = dict(base_args, app_reflect_newly_placed_objects=True, obj_model_type="d_nerf", root_dir="office", near=0.05)
    from types import SimpleNamespace
    xform = REC.resolve_new_object(SimpleNamespace(root_dir="office"))
    n_chunks = (rays.shape[0] + CHUNK - 1) // CHUNK

    def frame(args, **kw):
        out = M.batched_inference(models, emb, rays, N_SAMPLES, N_IMPORTANCE, False, CHUNK, args=args, trace_secondary_rays=True,
                                  to_cpu=False, **kw)
        torch.cuda.synchronize()
        return out

    def timed(args, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frame(args, **kw)
        return (time.perf_counter() - t0) * 1e3

    def rows_per_level(bounds):
        """(rows of the scene's renders, rows of the object's renders) of one unpipelined frame, by recursion level.  The scene's
        render of the last level is the one batched_inference asks for colour and depth only; the object's render follows the
        scene's render of its level (and is absent when no ray of the chunk was kept)."""
        scene_rows, object_rows, level = [0, 0], [0, 0], [0]
        scene, dn = REC.render_rays, REC.render_rays_dnerf

        def count_scene(m_, e_, r, *x, **k):
            level[0] = 1 if k.get("_rgb_depth_only") else 0
            scene_rows[level[0]] += int(r.shape[0])
            return scene(m_, e_, r, *x, **k)

        def count_object(b, **k):
            object_rows[level[0]] += int(b.shape[0])
            return dn(b, **k)
        REC.render_rays, REC.render_rays_dnerf = count_scene, count_object
        os.environ["MNRF_EVAL_PIPELINE"] = "0"
        try:
            frame(on_args, object_bounds=bounds, **obj)
        finally:
            REC.render_rays, REC.render_rays_dnerf = scene, dn
            os.environ.pop("MNRF_EVAL_PIPELINE")
        return scene_rows, object_rows

    res = {"workload": f"batched_inference {W}x{H}, {N_SAMPLES} coarse + {N_SAMPLES + N_IMPORTANCE} fine samples/ray, chunk {CHUNK}, "
                       "all-mirror random-init pair (bench.py config 2), max_recursive_level 1; D-NeRF object of the dnerf_object_l1 leg "
                       "(64 coarse + 128 fine samples per ray of its own, frame_time 0.37), office preset",
           "protocol": f"one warm-up frame per route, then the median of {a.reps} frames; the two overhead routes alternate frame by frame",
           "note": "the random-init object is opaque everywhere: a culled frame differs from the unculled one (outside the box the "
                   "object is absent); kept rays are those of the unculled frame"}
    frame(base_args)
    t_off = [timed(base_args) for _ in range(a.reps)]
    ms_off = statistics.median(t_off)
    res["app_off"] = {"ms_per_frame": round(ms_off, 2), "ms_reps": [round(t, 2) for t in t_off]}
    # overhead: no bounds against bounds that keep every ray
    keep_all = ObjectBounds((-1e6,) * 3, (1e6,) * 3)
    frame(on_args, **obj)
    frame(on_args, object_bounds=keep_all, **obj)
    t_none, t_all = [], []
    for _ in range(a.reps):
        t_none.append(timed(on_args, **obj))
        t_all.append(timed(on_args, object_bounds=keep_all, **obj))
    ms_none, ms_all = statistics.median(t_none), statistics.median(t_all)
    took_all = int(used.item())
    res["overhead"] = {"object_bounds_none": {"ms_per_frame": round(ms_none, 2), "ms_reps": [round(t, 2) for t in t_none]},
                       "all_keeping_bounds": {"ms_per_frame": round(ms_all, 2), "ms_reps": [round(t, 2) for t in t_all],
                                              "rays_that_took_the_object": took_all},
                       "ratio": round(ms_all / ms_none, 4),
                       "spread_of_reps": round(max(max(t) - min(t) for t in (t_none, t_all)) / ms_none, 4)}
    scene_none, object_none = rows_per_level(None)
    scene_all, object_all = rows_per_level(keep_all)
    res["overhead"]["object_bounds_none"].update(rays_per_level=scene_none, object_rays_per_level=object_none)
    res["overhead"]["all_keeping_bounds"].update(rays_per_level=scene_all, kept_rays_per_level=object_all)
    # the two parent figures as costs per row: the scene's from app_off (every primary ray reflects once), the object's from the rest
    # of the unculled frame
    us_scene = ms_off * 1e3 / (2.0 * rays.shape[0])
    us_object = (ms_none * 1e3 - us_scene * sum(scene_none)) / sum(object_none)
    res["per_row_us"] = {"scene": round(us_scene, 4), "object": round(us_object, 4)}
    # gain: cubes around the point the central pixel looks at (object frame, middle of its segment), bisected to the share
    centre_ray = rays[(H // 2) * W + W // 2].double().cpu()
    o = centre_ray[:3] * xform["scale"] + torch.tensor(xform["translation"], dtype=torch.float64)
    c = (o + centre_ray[3:6] * 0.5 * (centre_ray[6] + centre_ray[7])).tolist()
    n_primary = rays.shape[0]

    def cube(h):
        return ObjectBounds([v - h for v in c], [v + h for v in c])

    def share(h):
        return int(cube(h).cull(rays, xform)[2].item()) / n_primary

    res["gain"] = {}
    for target in (0.5, 0.1, 0.02):
        lo_h, hi_h = 1e-4, 64.0
        for _ in range(40):
            mid = (lo_h * hi_h) ** 0.5
            lo_h, hi_h = (mid, hi_h) if share(mid) < target else (lo_h, mid)
        bounds = cube(hi_h)
        frame(on_args, object_bounds=bounds, **obj)
        t = [timed(on_args, object_bounds=bounds, **obj) for _ in range(a.reps)]
        ms = statistics.median(t)
        scene_rows, rows = rows_per_level(bounds)
        # the issue's expectation, app_off + kept_fraction x (unculled - app_off), with the kept fraction over both levels of the
        # app_off frame; and the expectation by rows, which also knows that this frame traces other rays than the unculled one (a ray
        # that takes the object is no mirror any more: culling the object at level 0 leaves more rays to reflect)
        frac = sum(rows) / (2.0 * n_primary)
        expect = ms_off + frac * (ms_none - ms_off)
        by_rows = (us_scene * sum(scene_rows) + us_object * sum(rows)) * 1e-3
        res["gain"][f"primary_{target:g}"] = {
            "box_half_size": round(hi_h, 5), "primary_rays_hit": round(share(hi_h), 4), "rays_per_level": scene_rows,
            "kept_rays_per_level": rows, "kept_fraction_per_level": [round(k / max(n, 1), 4) for k, n in zip(rows, scene_rows)],
            "ms_per_frame": round(ms, 2), "ms_reps": [round(x, 2) for x in t],
            "kept_over_2x_primary": round(frac, 4), "expected_ms": round(expect, 2), "over_expectation_ms": round(ms - expect, 2),
            "expected_ms_by_rows": round(by_rows, 2), "over_expectation_by_rows_ms": round(ms - by_rows, 2),
            "rays_that_took_the_object": int(used.item()), "vs_unculled": round(ms / ms_none, 3)}
    return res


def nerf_pl_object(dev, emb):
    """The object of fixture g26_object_office_l2 as system_obj: seed 7, density head x 1000 with the fixture's biases."""
    from types import SimpleNamespace
    obj_models = {}
    for name, sd, bias in zip(("coarse", "fine"), SY.make_state_dict(7, 2, predict_normal=False, predict_mirror_mask=False), (6.18, 44.94)):
        SY.apply_tweaks(sd, [["sigma.weight", "mul", 1000.0], ["sigma.bias", "set", bias]])
        m = M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=False, predict_mirror_mask=False)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        obj_models[name] = m.to(dev).eval()
    return SimpleNamespace(models=obj_models, embeddings=emb)


def objects_leg(a, models, emb, rays, dev, base_args):
    """The --objects leg (module docstring) -> the result dict."""
    from types import SimpleNamespace
    from mirror_nerf_amd import ObjectBounds, PlacedObject
    from mirror_nerf_amd import placed_objects as PO
    reps = a.reps
    kind = a.objects_kind
    field = nerf_pl_object(dev, emb) if kind == "nerf_pl" else dnerf_object(dev)
    on_args = dict(base_args, app_reflect_newly_placed_objects=True, obj_model_type=kind, root_dir="office", near=0.05)
    xform = REC.resolve_new_object(SimpleNamespace(root_dir="office"))
    placement = dict(pose_align=None, scale=xform["scale"], translation=xform["translation"])
    n_primary = rays.shape[0]
    time_kw = dict(frame_time=0.37) if kind == "d_nerf" else {}

    def frame(**kw):
        out = M.batched_inference(models, emb, rays, N_SAMPLES, N_IMPORTANCE, False, CHUNK, args=on_args, trace_secondary_rays=True,
                                  to_cpu=False, **time_kw, **kw)
        torch.cuda.synchronize()
        return out

    def timed(**kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frame(**kw)
        return (time.perf_counter() - t0) * 1e3

    def cube_for(col, target=0.1):
        """A cube around the point the pixel (H / 2, col) looks at, in the object's frame, that `target` of the primary rays hit."""
        ray = rays[(H // 2) * W + col].double().cpu()
        o = ray[:3] * xform["scale"] + torch.tensor(xform["translation"], dtype=torch.float64)
        c = (o + ray[3:6] * 0.5 * (ray[6] + ray[7])).tolist()
        cube = lambda h: ObjectBounds([v - h for v in c], [v + h for v in c])  # noqa: E731
        share = lambda h: int(cube(h).cull(rays, xform)[2].item()) / n_primary  # noqa: E731
        lo_h, hi_h = 1e-4, 64.0
        for _ in range(40):
            mid = (lo_h * hi_h) ** 0.5
            lo_h, hi_h = (mid, hi_h) if share(mid) < target else (lo_h, mid)
        return cube(hi_h), round(share(hi_h), 4)

    def counted(K, **kw):
        """One unpipelined frame -> (kept rays [object][level], rays per level, reads of kept-ray counts)."""
        kept, level_rays, level, reads = [[0, 0] for _ in range(K)], [0, 0], [0], [0]
        scene, cull_k, cull_1 = REC.render_rays, PO.cull_objects, ObjectBounds.cull
        turn = [0]

        def count_scene(m_, e_, r, *x, **k):
            if m_ is models:
                level[0] = 1 if k.get("_rgb_depth_only") else 0
                level_rays[level[0]] += int(r.shape[0])
                turn[0] = 0
            return scene(m_, e_, r, *x, **k)

        def count_k(r, placed):
            out = cull_k(r, placed)
            reads[0] += 1
            for k, c in enumerate(out[3].tolist()):
                kept[k][level[0]] += c
            return out

        def count_1(self, r, xf):
            out = cull_1(self, r, xf)
            reads[0] += 1
            kept[turn[0] % K][level[0]] += int(out[2].item())
            turn[0] += 1
            return out
        REC.render_rays, PO.cull_objects, ObjectBounds.cull = count_scene, count_k, count_1
        os.environ["MNRF_EVAL_PIPELINE"] = "0"
        try:
            frame(**kw)
        finally:
            REC.render_rays, PO.cull_objects, ObjectBounds.cull = scene, cull_k, cull_1
            os.environ.pop("MNRF_EVAL_PIPELINE")
        return kept, level_rays, reads[0]

    res = {"workload": f"batched_inference {W}x{H}, {N_SAMPLES} coarse + {N_SAMPLES + N_IMPORTANCE} fine samples/ray, chunk {CHUNK}, "
                       f"all-mirror random-init pair (bench.py config 2), max_recursive_level 1; K copies of the {kind} object of the "
                       "object legs under the office preset, each in its own cube hit by about 10 % of the primary rays",
           "protocol": f"one warm-up frame per route, then {reps} rounds alternating the routes frame by frame; host clock around a frame "
                       "that ends in a synchronise; median, spread = (max - min) / median of a route's frames",
           "object_kind": kind}
    for K in a.objects:
        cols = [W * (j + 1) // (K + 1) for j in range(K)]
        cubes = [cube_for(c) for c in cols]
        placed = [PlacedObject(field, placement, bounds=b) for b, _ in cubes]
        used = torch.zeros(K, dtype=torch.int32, device=dev)
        routes = {"fused": dict(placed_objects=placed, object_used=used), "chain": dict(placed_objects=placed, object_used=used, _object_chain=True)}
        if K == 1:
            one = {"system_obj": field} if kind == "nerf_pl" else {"render_kwargs_test_d_nerf": field}
            routes["legacy"] = dict(one, object_bounds=cubes[0][0], object_used=used)
        times = {name: [] for name in routes}
        for kw in routes.values():
            frame(**kw)
        for _ in range(reps):
            for name, kw in routes.items():
                times[name].append(timed(**kw))
        entry = {"pixel_columns": cols, "primary_rays_hit": [s_ for _, s_ in cubes], "box_half_size": [round((b.hi[0] - b.lo[0]) / 2, 5) for b, _ in cubes]}
        for name, kw in routes.items():
            kept, level_rays, reads = counted(K, **kw)
            frame(**kw)
            ms = statistics.median(times[name])
            entry[name] = {"ms_per_frame": round(ms, 2), "ms_reps": [round(t, 2) for t in times[name]],
                           "spread": round((max(times[name]) - min(times[name])) / ms, 4), "rays_per_level": level_rays,
                           "kept_rays_per_object_and_level": kept,
                           "kept_share_per_level": [round(sum(k[lv] for k in kept) / max(K * level_rays[lv], 1), 4) for lv in range(2)],
                           "count_reads_per_frame": reads, "rays_that_took_each_object": used.tolist()}
        entry["fused_over_chain"] = round(entry["fused"]["ms_per_frame"] / entry["chain"]["ms_per_frame"], 4)
        if K == 1:
            entry["fused_over_legacy"] = round(entry["fused"]["ms_per_frame"] / entry["legacy"]["ms_per_frame"], 4)
        res[f"K{K}"] = entry
    return res


def mirrors_leg(a, models, emb, rays, dev, base_args):
    """The --mirrors leg (module docstring) -> the result dict."""
    from types import SimpleNamespace
    from mirror_nerf_amd import PlacedMirror
    reps = a.reps
    args = dict(base_args, max_recursive_level=1, plane_pos="plane_x", root_dir="synthetic", near=1e9)
    plane = REC.resolve_new_mirror(SimpleNamespace(**args))

    def frame(frame_args, **kw):
        out = M.batched_inference(models, emb, rays, N_SAMPLES, N_IMPORTANCE, False, CHUNK, args=frame_args, trace_secondary_rays=True,
                                  to_cpu=False, **kw)
        torch.cuda.synchronize()
        return out

    def timed(frame_args, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frame(frame_args, **kw)
        return (time.perf_counter() - t0) * 1e3

    routes = {"legacy": (dict(args, app_place_new_mirror=True), dict(new_mirror=plane))}
    for K in a.mirrors:
        copies = [PlacedMirror.axis_aligned(plane["axis"], plane["position"] - 0.05 * k * plane["normal"][0], plane["normal"], plane["rect"])
                  for k in range(K)]
        routes[f"K{K}"] = (args, dict(new_mirrors=copies))
    res = {"workload": f"batched_inference {W}x{H}, {N_SAMPLES} coarse + {N_SAMPLES + N_IMPORTANCE} fine samples/ray, chunk {CHUNK}, "
                       "all-mirror random-init pair (bench.py config 2), max_recursive_level 1, near 1e9 (nothing hides a mirror); K copies of the default plane_x "
                       "preset, copy k moved 0.05 k behind the first",
           "protocol": f"one warm-up frame per route, then {reps} rounds alternating the routes frame by frame; host clock around a frame "
                       "that ends in a synchronise; median, spread = (max - min) / median of a route's frames"}
    times = {name: [] for name in routes}
    outs = {name: frame(fa, **kw) for name, (fa, kw) in routes.items()}
    for _ in range(reps):
        for name, (fa, kw) in routes.items():
            times[name].append(timed(fa, **kw))
    for name in routes:
        ms = statistics.median(times[name])
        res[name] = {"ms_per_frame": round(ms, 2), "ms_reps": [round(t, 2) for t in times[name]],
                     "spread": round((max(times[name]) - min(times[name])) / ms, 4),
                     "merged_mirror_rays_level0": int(outs[name]["mirror_mask_fine"].sum().item())}
        if name != "legacy":
            idx = outs[name]["new_mirror_index"]
            res[name]["rays_that_took_each_mirror"] = torch.bincount(idx[idx >= 0].long(), minlength=int(name[1:])).tolist()
            res[name]["over_legacy"] = round(ms / statistics.median(times["legacy"]), 4)
            res[name]["depth_equals_legacy"] = bool(torch.equal(outs[name]["depth_fine"], outs["legacy"]["depth_fine"]))
    return res


def mirrors_facing_leg(a, models, emb, rays, dev, base_args):
    """The --mirrors_facing leg (module docstring) -> the result dict."""
    import math
    import numpy as np
    from mirror_nerf_amd import PlacedMirror
    reps = a.reps
    eye = np.array((0.0, -4.0, 1.5))                                        # synthetic.look_at_pose's defaults
    view = -eye / np.linalg.norm(eye)
    right = np.cross(view, (0.0, 0.0, 1.0))
    right /= np.linalg.norm(right)
    tilt = -math.cos(0.3) * view + math.sin(0.3) * right
    pair = [PlacedMirror(eye + view, tilt, (0, 0, 1), (3, 3)), PlacedMirror(eye - view, -tilt, (0, 0, 1), (8, 8))]

    def route(level, on):
        args = dict(base_args, max_recursive_level=level, near=1e9)
        kw = dict(exclude_source_mirror=True) if on else {}

        def frame():
            out = M.batched_inference(models, emb, rays, N_SAMPLES, N_IMPORTANCE, False, CHUNK, args=args, trace_secondary_rays=True,
                                      to_cpu=False, maps_only=True, new_mirrors=pair, **kw)
            torch.cuda.synchronize()
            return out

        frame()
        # the reflections of a chunk run depth first: the one that does not compact is level 0's, each further one a level deeper
        per_level, level_now, reflect = [int(rays.shape[0])] + [0] * level, [0], REC._reflect

        def counting_reflect(rays_, x, n, mask, compact, *a_, **k):
            got = reflect(rays_, x, n, mask, compact, *a_, **k)
            level_now[0] = level_now[0] + 1 if compact else 0
            per_level[level_now[0] + 1] += int(got[0].shape[0])
            return got

        REC._reflect = counting_reflect
        try:
            out = frame()
        finally:
            REC._reflect = reflect
        first = out["new_mirror_index"] == 0
        got = {"rays_per_level": per_level, "rays_that_took_each_mirror_level0": torch.bincount(out["new_mirror_index"].clamp(min=-1).long() + 1,
                                                                                                minlength=3)[1:].tolist()}
        if level >= 2 and bool(first.any()):
            depth = out["depth_fine_reflect"][first]
            got.update(min_level1_depth_on_first_mirror_rows=float(depth.min()), level1_depth_below_1e_6=int((depth < 1e-6).sum()))
        return got, frame

    routes = {f"l{level}_{'on' if on else 'off'}": route(level, on) for level in (1, 2, 4) for on in (False, True)}
    res = {"workload": f"batched_inference {W}x{H}, {N_SAMPLES} coarse + {N_SAMPLES + N_IMPORTANCE} fine samples/ray, chunk {CHUNK}, all-mirror "
                       "random-init pair (bench.py config 2), near 1e9 (nothing hides a mirror), maps_only; two parallel frame mirrors tilted by "
                       "0.3 rad about z, one unit in front of the camera (3 x 3) and one unit behind it (8 x 8), facing each other",
           "protocol": f"one warm-up and one counting frame per route, then {reps} rounds alternating the six routes frame by frame; host clock "
                       "around a frame that ends in a synchronise; median, spread = (max - min) / median of a route's frames"}
    res.update(_alternate(routes, reps))
    res["l1_on_over_off"] = round(res["l1_on"]["ms_per_frame"] / res["l1_off"]["ms_per_frame"], 4)
    return res


def _rough_frames(models, emb, rays, n_imp, chunk, args, reps, std):
    """One warm-up frame, one frame that counts the compacting _reflect calls (each reads its count on the host) and the rows
    of every render_rays call, then `reps` timed frames -> dict."""
    def frame():
        out = M.batched_inference(models, emb, rays, N_SAMPLES, n_imp, False, chunk, args=args, trace_secondary_rays=True,
                                  normal_noise_std=std, to_cpu=False)
        torch.cuda.synchronize()
        return out

    out = frame()
    reads, rows = [0], [0]
    reflect, render = REC._reflect, REC.render_rays

    def counting_reflect(rays_, x, n, mask, compact, *a, **k):
        reads[0] += 1 if compact else 0
        return reflect(rays_, x, n, mask, compact, *a, **k)

    def counting_render(models_, embeddings, r, *a, **k):
        rows[0] += int(r.shape[0])
        return render(models_, embeddings, r, *a, **k)

    REC._reflect, REC.render_rays = counting_reflect, counting_render
    try:
        frame()
    finally:
        REC._reflect, REC.render_rays = reflect, render
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        frame()
        times.append((time.perf_counter() - t0) * 1e3)
    ms = statistics.median(times)
    mask = out["mirror_mask_fine"] != 0
    return {"ms_per_frame": round(ms, 1), "ms_reps": [round(t, 1) for t in times], "spread": round((max(times) - min(times)) / ms, 4),
            "count_reads_per_frame": reads[0], "rays_rendered_per_frame": rows[0], "mirror_share_level0": round(float(mask.float().mean()), 4)}


def rough_all_mirror(dev, reps):
    """Part (a) of the --rough leg on the package this process imported."""
    models, _ = SY.build_models(dev, SY.ALL_MIRROR, seed=0)
    emb = {"xyz": M.Embedding(10), "dir": M.Embedding(4)}
    rays = SY.device_rays(360, 480, dev)
    args = dict(ARGS, max_recursive_level=1, app_control_mirror_roughness=True, trace_ray_times=64)
    return _rough_frames(models, emb, rays, 64, 16384, args, reps, 0.0025)


def rough_leg(a, dev):
    """The --rough leg (module docstring) -> the result dict."""
    import subprocess
    reps = a.reps
    res = {"workload_a": f"all-mirror random-init pair, 480x360, {N_SAMPLES} + 64 samples, chunk 16384, max_recursive_level 1 (levels 0 and "
                         "1), trace_ray_times 64, normal_noise_std 0.0025 (benchlegs.roughness_leg one_bounce_64_jitters)",
           "protocol_a": f"per round a fresh process: one warm-up frame, one counting frame, then {reps} timed frames; host clock around a "
                         "frame that ends in a synchronise; median, spread = (max - min) / median; rounds alternate parent, this"}
    if a.parent_root:
        rounds = {"parent": [], "this": []}
        for _ in range(2):
            for name, root in (("parent", os.path.abspath(a.parent_root)), ("this", ROOT)):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--rough_child", "--reps", str(reps), "--package_root", root],
                                   capture_output=True, text=True)
                if r.returncode != 0:
                    raise RuntimeError(f"the {name} round failed: {r.stderr[-2000:]}")
                rounds[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
        res.update(rounds)
        for name in rounds:
            frames = [t for r in rounds[name] for t in r["ms_reps"]]
            res[name + "_ms_per_frame"] = round(statistics.median(frames), 1)
            res[name + "_spread"] = round((max(frames) - min(frames)) / statistics.median(frames), 4)
        res["this_over_parent"] = round(res["this_ms_per_frame"] / res["parent_ms_per_frame"], 4)
    else:
        res["this"] = [rough_all_mirror(dev, reps)]
    # (b) a partly mirrored frame
    models, _ = SY.build_models(dev, SY.STRADDLE, seed=0)
    emb = {"xyz": M.Embedding(10), "dir": M.Embedding(4)}
    rays = SY.device_rays(H, W, dev)
    base = dict(ARGS, max_recursive_level=1)
    off = _rough_frames(models, emb, rays, N_IMPORTANCE, CHUNK, base, 3, 0)
    per_ray = off["ms_per_frame"] / off["rays_rendered_per_frame"]
    mirror_rays = round(off["mirror_share_level0"] * rays.shape[0])
    part = {"workload": f"STRADDLE random-init pair, {W}x{H}, {N_SAMPLES} + {N_IMPORTANCE} samples, chunk {CHUNK}, max_recursive_level 1, "
                        "normal_noise_std 0.01; the parent raises on this frame",
            "roughness_off": off, "ms_per_rendered_ray_of_the_roughness_off_frame": per_ray, "mirror_rays_level0": mirror_rays}
    for times in (4, 64):
        got = _rough_frames(models, emb, rays, N_IMPORTANCE, CHUNK, dict(base, app_control_mirror_roughness=True, trace_ray_times=times), 3, 0.01)
        got["estimate_ms"] = round(off["ms_per_frame"] + times * mirror_rays * per_ray, 1)
        got["measured_over_estimate"] = round(got["ms_per_frame"] / got["estimate_ms"], 4)
        part[f"trace_ray_times_{times}"] = got
    res["partly_mirrored"] = part
    return res


def _rough_mirrors_frames(models, emb, rays, args, **kw):
    """One warm-up frame and one frame that counts, per recursion level, the compacting _reflect calls (each reads its count on
    the host), the rays of J (the rows of every mnrf_jitter_mean) and the rows of every render_rays call -> (dict, frame); the
    caller times `frame` (the routes of a part alternate frame by frame)."""
    def frame():
        out = M.batched_inference(models, emb, rays, N_SAMPLES, N_IMPORTANCE, False, CHUNK, args=args, trace_secondary_rays=True,
                                  to_cpu=False, maps_only=True, **kw)
        torch.cuda.synchronize()
        return out

    out = frame()
    reads, rows, in_j = [0], [0], [0]
    reflect, render, mean = REC._reflect, REC.render_rays, REC._jitter_mean

    def counting_reflect(rays_, x, n, mask, compact, *a, **k):
        reads[0] += 1 if compact else 0
        return reflect(rays_, x, n, mask, compact, *a, **k)

    def counting_render(models_, embeddings, r, *a, **k):
        rows[0] += int(r.shape[0])
        return render(models_, embeddings, r, *a, **k)

    def counting_mean(acc, pieces, index, m, n_jit, finish=None):
        in_j[0] += m if finish is not None else 0      # (the finishing call of a chunk and level: once per J)
        return mean(acc, pieces, index, m, n_jit, finish)

    REC._reflect, REC.render_rays, REC._jitter_mean = counting_reflect, counting_render, counting_mean
    try:
        frame()
    finally:
        REC._reflect, REC.render_rays, REC._jitter_mean = reflect, render, mean
    print(f"counted: {sorted(kw)} {args.get('trace_ray_times', '')}", file=sys.stderr, flush=True)
    mask = out["mirror_mask_fine"] != 0
    keys = len([k for k in ("rgb_coarse", "rgb_fine") if k in out]) or 1
    got = {"count_reads_per_frame": reads[0], "rays_rendered_per_frame": rows[0], "rays_in_J_level0": in_j[0] // keys,
           "mirror_share_level0": round(float(mask.float().mean()), 4)}
    if "new_mirror_index" in out:
        got["placed_mirror_share_level0"] = round(float((out["new_mirror_index"] >= 0).float().mean()), 4)
    return got, frame


def _alternate(routes, reps):
    """routes: name -> (dict, frame).  `reps` rounds that alternate the routes frame by frame; median and spread into each dict."""
    times = {name: [] for name in routes}
    for _ in range(reps):
        for name, (_, frame) in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            frame()
            times[name].append((time.perf_counter() - t0) * 1e3)
    for name, (got, _) in routes.items():
        ms = statistics.median(times[name])
        got.update(ms_per_frame=round(ms, 1), ms_reps=[round(t, 1) for t in times[name]], spread=round((max(times[name]) - min(times[name])) / ms, 4))
    return {name: got for name, (got, _) in routes.items()}


def rough_mirrors_leg(a, dev):
    """The --rough_mirrors leg (module docstring) -> the result dict."""
    import math
    import numpy as np
    from mirror_nerf_amd import PlacedMirror
    reps = a.reps
    models, _ = SY.build_models(dev, SY.STRADDLE, seed=0)
    emb = {"xyz": M.Embedding(10), "dir": M.Embedding(4)}
    rays = SY.device_rays(H, W, dev)
    base = dict(ARGS, max_recursive_level=1, near=1e9)
    res = {"workload": f"STRADDLE random-init pair, {W}x{H}, {N_SAMPLES} + {N_IMPORTANCE} samples, chunk {CHUNK}, max_recursive_level 1, near 1e9 "
                       "(nothing hides a placed mirror), maps_only; the placed mirror is a square 0.5 down the central ray, tilted by 0.2 about z",
           "protocol": f"per part: one warm-up and one counting frame per route, then {reps} rounds alternating the routes frame by frame; host "
                       "clock around a frame that ends in a synchronise; median, spread = (max - min) / median of a route's frames"}
    # (a) the new route with one std everywhere beside the flag's route
    flag = dict(base, app_control_mirror_roughness=True, trace_ray_times=4)
    part = _alternate({"flag": _rough_mirrors_frames(models, emb, rays, flag, normal_noise_std=0.01),
                       "rough_times": _rough_mirrors_frames(models, emb, rays, base, rough_times=4, scene_roughness=0.01)}, reps)
    part["rough_times_over_flag"] = round(part["rough_times"]["ms_per_frame"] / part["flag"]["ms_per_frame"], 4)
    res["a_overhead_T4_std0.01"] = part
    # (b), (c) one frosted placed mirror taken by about 5 % and about 25 % of the primary rays
    eye = np.array((0.0, -4.0, 1.5))                                        # synthetic.look_at_pose's defaults
    view = -eye / np.linalg.norm(eye)
    right = np.cross(view, (0.0, 0.0, 1.0))
    right /= np.linalg.norm(right)
    for share in (0.05, 0.25):
        side = math.sqrt(share) * 2 * 0.5 * math.tan(SY.CAMERA_ANGLE_X / 2)
        mirror = dict(center=eye + 0.5 * view, normal=-view + 0.2 * right, up=(0, 0, 1), size=(side, side))
        polished, frosted = [PlacedMirror(**mirror)], [PlacedMirror(**mirror, roughness=0.03)]
        routes = {"off": _rough_mirrors_frames(models, emb, rays, base, new_mirrors=polished)}
        for times in (4, 64):
            routes[f"b_scene_polished_T{times}"] = _rough_mirrors_frames(models, emb, rays, base, new_mirrors=frosted, rough_times=times)
            routes[f"c_scene_frosted_T{times}"] = _rough_mirrors_frames(models, emb, rays, base, new_mirrors=frosted, rough_times=times,
                                                                      scene_roughness=0.01)
        part = _alternate(routes, reps)
        per_ray = part["off"]["ms_per_frame"] / part["off"]["rays_rendered_per_frame"]
        part["ms_per_rendered_ray_of_the_off_frame"] = per_ray
        for name, got in part.items():
            if name[:2] in ("b_", "c_"):
                times = int(name.rsplit("T", 1)[1])
                got["estimate_ms"] = round(part["off"]["ms_per_frame"] + times * got["rays_in_J_level0"] * per_ray, 1)
                got["measured_over_estimate"] = round(got["ms_per_frame"] / got["estimate_ms"], 4)
        res[f"placed_mirror_about_{round(share * 100)}_percent"] = part
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=None, help="timed frames per route (default 3; 7 for --objects)")
    ap.add_argument("--objects", type=int, nargs="+", default=None, metavar="K", help="run the several-objects leg instead, for each K (1..8)")
    ap.add_argument("--objects_kind", type=str, default="nerf_pl", choices=("nerf_pl", "d_nerf"))
    ap.add_argument("--mirrors", type=int, nargs="+", default=None, metavar="K", help="run the several-mirrors leg instead, for each K (1..8)")
    ap.add_argument("--levels", type=int, nargs="+", default=[2, 50])
    ap.add_argument("--no_object", action="store_true", help="skip the app_reflect_newly_placed_objects leg")
    ap.add_argument("--no_dnerf", action="store_true", help="skip the leg with a D-NeRF object")
    ap.add_argument("--obj_bounds", action="store_true", help="run the object-bounds leg instead of the others")
    ap.add_argument("--rough", action="store_true", help="run the mirror-roughness leg instead of the others")
    ap.add_argument("--parent_root", type=str, default=None, help="--rough: a built checkout of the parent commit to measure beside this tree")
    ap.add_argument("--rough_child", action="store_true", help="(--rough's child process) part (a) on the package of --package_root")
    ap.add_argument("--package_root", type=str, default=None, metavar="DIR", help="(--rough's child process) the tree whose package is imported")
    ap.add_argument("--rough_mirrors", action="store_true", help="run the leg of a roughness per mirror instead of the others")
    ap.add_argument("--mirrors_facing", action="store_true", help="run the leg of exclude_source_mirror= (two facing mirrors) instead of the others")
    a = ap.parse_args()
    a.reps = a.reps or (7 if (a.objects or a.mirrors or a.rough or a.rough_child or a.rough_mirrors or a.mirrors_facing) else 3)
    dev = "cuda:0"
    if a.rough_child:
        print(json.dumps(rough_all_mirror(dev, a.reps)))
        return
    if a.rough:
        print(json.dumps(rough_leg(a, dev)))
        return
    if a.rough_mirrors:
        print(json.dumps(rough_mirrors_leg(a, dev)))
        return
    models, _ = SY.build_models(dev, SY.ALL_MIRROR, seed=0)
    emb = {"xyz": M.Embedding(10), "dir": M.Embedding(4)}
    rays = SY.device_rays(H, W, dev)

    # rows per render_rays call, by recursion level: batched_inference recurses depth first, one call per level and chunk
    calls = []
    orig = REC.render_rays

    def counting(models_, embeddings, r, *args_, **kw):
        calls.append(int(r.shape[0]))
        return orig(models_, embeddings, r, *args_, **kw)

    extra = {}

    def frame(args):
        return M.batched_inference(models, emb, rays, N_SAMPLES, N_IMPORTANCE, False, CHUNK, args=args, trace_secondary_rays=True,
                                   to_cpu=False, **extra)

    n_chunks = (rays.shape[0] + CHUNK - 1) // CHUNK

    def run(args):
        out = frame(args)                                          # warm-up
        torch.cuda.synchronize()
        # one frame counted unpipelined (the counts do not depend on it): the calls are then n_chunks runs of (level 0,
        # level 1, ...) -- pipelined, chunk k+1's level 0 is queued in the middle of chunk k's run
        calls.clear()
        REC.render_rays = counting
        os.environ["MNRF_EVAL_PIPELINE"] = "0"
        try:
            out = frame(args)
            torch.cuda.synchronize()
        finally:
            REC.render_rays = orig
            os.environ.pop("MNRF_EVAL_PIPELINE")
        per_chunk = len(calls) // n_chunks if len(calls) % n_chunks == 0 else None
        traced = None
        if per_chunk:
            traced = [sum(calls[c * per_chunk + lv] for c in range(n_chunks)) for lv in range(per_chunk)]
        times = []
        for _ in range(a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = frame(args)
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        return out, statistics.median(times), times, traced

    base_args = dict(ARGS)
    if a.obj_bounds:
        print(json.dumps(bounds_leg(a, models, emb, rays, dev, base_args)))
        return
    if a.objects:
        print(json.dumps(objects_leg(a, models, emb, rays, dev, base_args)))
        return
    if a.mirrors:
        print(json.dumps(mirrors_leg(a, models, emb, rays, dev, base_args)))
        return
    if a.mirrors_facing:
        print(json.dumps(mirrors_facing_leg(a, models, emb, rays, dev, base_args)))
        return
    off, ms_off, t_off, traced_off = run(base_args)
    res = {"workload": f"batched_inference {W}x{H}, {N_SAMPLES} coarse + {N_SAMPLES + N_IMPORTANCE} fine samples/ray, chunk {CHUNK}, "
                       "all-mirror random-init pair (bench.py config 2)",
           "app_off": {"max_recursive_level": base_args["max_recursive_level"], "ms_per_frame": round(ms_off, 2),
                       "ms_reps": [round(t, 2) for t in t_off], "rays_per_level": traced_off}}
    for lv in a.levels:
        args = dict(base_args, max_recursive_level=lv, app_place_new_mirror=True, plane_pos="plane_x", root_dir="synthetic",
                    near=0.05)
        out, ms, t, traced = run(args)
        # level-0 depth replaced by the distance to the new mirror exactly where a primary ray hit it unoccluded
        hits = int((out["depth_fine"] != off["depth_fine"]).sum().item())
        res[f"place_mirror_l{lv}"] = {"ms_per_frame": round(ms, 2), "ms_reps": [round(x, 2) for x in t], "new_mirror_hits_level0": hits,
                                      "merged_mirror_rays_level0": int(out["mirror_mask_fine"].sum().item()),
                                      "rays_per_level": traced, "vs_app_off": round(ms / ms_off, 2)}
    if not a.no_object:
        # the object of fixture g26_object_office_l2: seed 7, density head x 1000 with the fixture's biases
        from types import SimpleNamespace
        obj_models = {}
        for name, sd, bias in zip(("coarse", "fine"), SY.make_state_dict(7, 2, predict_normal=False, predict_mirror_mask=False),
                                  (6.18, 44.94)):
            SY.apply_tweaks(sd, [["sigma.weight", "mul", 1000.0], ["sigma.bias", "set", bias]])
            m = M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=False, predict_mirror_mask=False)
            m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
            obj_models[name] = m.to(dev).eval()
        used = torch.zeros(1, dtype=torch.int32, device=dev)
        extra.update(system_obj=SimpleNamespace(models=obj_models, embeddings=emb), object_used=used)
        args = dict(base_args, app_reflect_newly_placed_objects=True, obj_model_type="nerf_pl", root_dir="office", near=0.05)
        out, ms, t, traced = run(args)
        extra.clear()
        res["object_l1"] = {"ms_per_frame": round(ms, 2), "ms_reps": [round(x, 2) for x in t], "rays_per_render_call": traced,
                            "rays_that_took_the_object": int(used.item()),
                            "changed_rays": int((out["rgb_fine"] != off["rgb_fine"]).any(-1).sum().item()),
                            "vs_app_off": round(ms / ms_off, 2)}
    if not a.no_dnerf:
        used = torch.zeros(1, dtype=torch.int32, device=dev)
        kw = dnerf_object(dev)
        extra.update(render_kwargs_test_d_nerf=kw, frame_time=0.37, object_used=used)
        args = dict(base_args, app_reflect_newly_placed_objects=True, obj_model_type="d_nerf", root_dir="office", near=0.05)
        out, ms, t, traced = run(args)
        extra.clear()
        res["dnerf_object_l1"] = {"ms_per_frame": round(ms, 2), "ms_reps": [round(x, 2) for x in t], "rays_per_level": traced,
                                  "object_samples_per_ray": "64 coarse (density only) + 128 fine", "frame_time": 0.37,
                                  "rays_that_took_the_object": int(used.item()),
                                  "changed_rays": int((out["rgb_fine"] != off["rgb_fine"]).any(-1).sum().item()),
                                  "vs_app_off": round(ms / ms_off, 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
