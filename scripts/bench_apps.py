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
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import mirror_nerf_amd as M  # noqa: E402
from mirror_nerf_amd import recursion as REC  # noqa: E402
from mirror_nerf_amd import synthetic as SY  # noqa: E402
from mirror_nerf_amd.benchlegs import ARGS, CHUNK, H, N_IMPORTANCE, N_SAMPLES, W  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--levels", type=int, nargs="+", default=[2, 50])
    ap.add_argument("--no_object", action="store_true", help="skip the app_reflect_newly_placed_objects leg")
    ap.add_argument("--no_dnerf", action="store_true", help="skip the leg with a D-NeRF object")
    a = ap.parse_args()
    dev = "cuda:0"
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
        # the object of fixture g27_dnerf_office_l2: seed 7, two models, density head x 1000 with the fixture's biases
        from mirror_nerf_amd.dnerf import DirectTemporalNeRF
        torch.manual_seed(7)
        nets = []
        for bias in (7.06, -5.08):
            m = DirectTemporalNeRF()
            with torch.no_grad():
                m._occ.alpha_linear.weight.mul_(1000.0)
                m._occ.alpha_linear.bias.fill_(bias)
            nets.append(m.to(dev).eval())
        used = torch.zeros(1, dtype=torch.int32, device=dev)
        kw = dict(network_fn=nets[0], network_fine=nets[1], N_samples=64, N_importance=64, white_bkgd=False, use_two_models_for_fine=True,
                  lindisp=False, perturb=False, raw_noise_std=0.0)
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
