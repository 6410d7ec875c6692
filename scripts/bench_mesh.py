#!/usr/bin/env python3
"""Times the stages of mesh extraction at N = 256 on the trained weights of fixture G11 (one JSON line):

    python scripts/bench_mesh.py [--N 256] [--repeats 5] [--warmup 2] [--out profiles/mesh_bench.json]

Milliseconds from torch.cuda.Event pairs on the launching stream, the median of `repeats` runs after `warmup` untimed
ones: the density grid (grid points + sigma-only field + clamp), marching cubes split into count, scan (torch.cumsum of
the per-block counts, with the host read of the totals) and emit, the connected components (labels, counts, compaction)
one view of the colour fusion (projection, the occlusion render and the accumulation), the vertex normals of the largest
component, and its colouring along those normals (rays, the 64 + 128-sample render with the coarse and the fine model, the
uint8 cast; `normal_colors_rays_per_s`: vertices over that time).  `mc_bytes_per_s`: the bytes
count + emit must move -- the volume once for each of the three launches, the vertex-base array written once, the
vertices and triangles written once -- over their time.  `mc_over_sigma`: (count + scan + emit) / grid sigma.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threshold", type=float, default=10.0)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import numpy as np
    import torch
    import mirror_nerf_amd as M
    from mirror_nerf_amd import mesh, mirror_nerf as MN, synthetic as SY
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh.py measures on the GPU only")
    dev = "cuda:0"
    z = np.load(os.path.join(ROOT, "tests", "golden", "g11_trained_weights.npz"))
    model = M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=True)
    model.load_state_dict({k[len("fine__"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("fine__")})
    model = model.to(dev)
    coarse = M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=True)
    coarse.load_state_dict({k[len("coarse__"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("coarse__")})
    coarse = coarse.to(dev)
    emb = {"xyz": M.Embedding(10), "dir": M.Embedding(4)}
    N, box = args.N, ((-1.5, 1.5), (-1.5, 1.5), (-0.3, 1.7))
    H = W = 400
    image = torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, device=dev)
    pose = SY.look_at_pose(eye=(2.6 * np.sin(0.2), -2.6 * np.cos(0.2) + 0.2, 1.4), target=(0.1, 0.6, 0.6))[None]
    focal = 0.5 * W / np.tan(0.45)

    def ev():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    rows, sizes = [], {}
    for it in range(args.warmup + args.repeats):
        e0 = ev()
        vol = mesh.density_grid(model, emb["xyz"], *box, N)
        e1 = ev()
        tm = {}
        v, t = mesh.marching_cubes(vol, args.threshold, timings=tm)
        e2 = ev()
        lv, lt = mesh.largest_component(v, t)
        e3 = ev()
        world = mesh.index_to_world(lv, *box, N)
        e4 = ev()
        mesh.fuse_vertex_colors(world, model, emb, image, pose, focal, 0.05)
        e5 = ev()
        normals = mesh.vertex_normals(world, lt)
        e6 = ev()
        mesh.normal_vertex_colors(world, lt, {"coarse": coarse, "fine": model}, emb, 0.05, 8.0, normals=normals)
        e7 = ev()
        torch.cuda.synchronize()
        marks = dict(tm["events"])
        row = dict(grid_sigma_ms=e0.elapsed_time(e1), count_ms=marks["start"].elapsed_time(marks["count"]),
                   scan_ms=marks["count"].elapsed_time(marks["scan"]), emit_ms=marks["scan"].elapsed_time(marks["emit"]),
                   components_ms=e2.elapsed_time(e3), color_view_ms=e4.elapsed_time(e5),
                   vertex_normals_ms=e5.elapsed_time(e6), normal_colors_ms=e6.elapsed_time(e7))
        sizes = dict(vertices=int(v.shape[0]), triangles=int(t.shape[0]), largest_vertices=int(lv.shape[0]),
                     largest_triangles=int(lt.shape[0]))
        if it >= args.warmup:
            rows.append(row)
    med = {k: statistics.median(r[k] for r in rows) for k in rows[0]}
    spread = {k.replace("_ms", "_minmax_ms"): [min(r[k] for r in rows), max(r[k] for r in rows)] for k in rows[0]}
    mc_bytes = 3 * 4 * N ** 3 + 4 * N ** 3 + 12 * sizes["vertices"] + 12 * sizes["triangles"]
    line = dict(metric="mesh_extraction_stages", N=N, threshold=args.threshold, precision=MN.PRECISION, repeats=args.repeats,
                warmup=args.warmup, **{k: round(x, 4) for k, x in med.items()}, **spread, **sizes, mc_bytes=mc_bytes,
                mc_bytes_per_s=mc_bytes / ((med["count_ms"] + med["emit_ms"]) * 1e-3),
                mc_over_sigma=(med["count_ms"] + med["scan_ms"] + med["emit_ms"]) / med["grid_sigma_ms"],
                sigma_evals_per_s=N ** 3 / (med["grid_sigma_ms"] * 1e-3), color_view_image=[H, W],
                normal_colors_rays_per_s=sizes["largest_vertices"] / (med["normal_colors_ms"] * 1e-3), normal_colors_samples=[64, 128])
    text = json.dumps(line)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
