#!/usr/bin/env python3
"""Command line of mesh extraction (the reference's extract_color_mesh.py without its dataset and colour stage):

    python scripts/extract_mesh.py --ckpt_path ckpts/exp/last.ckpt --N_grid 256 --x_range -1 1 --y_range -1 1 \\
        --z_range -1 1 --sigma_threshold 20 --out mesh.ply
    python scripts/extract_mesh.py --g11 --N_grid 48 --x_range -1.5 1.5 --y_range -1.5 1.5 --z_range -0.3 1.7 \\
        --sigma_threshold 10 --out g11.ply

The density of `nerf_fine` is sampled on the grid, meshed and (unless --keep_all) reduced to its largest connected
component, all on the GPU; the PLY holds world coordinates.  Argument names follow extract_color_mesh.py:26-87 where
they apply.  Vertex colours need images and poses, which come from a dataset: mirror_nerf_amd.mesh.fuse_vertex_colors.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def get_opts(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--ckpt_path", type=str, help="checkpoint holding nerf_fine.* (Lightning .ckpt or a plain dict)")
    src.add_argument("--g11", action="store_true", help="the trained weights of fixture G11 (tests/golden)")
    ap.add_argument("--trusted", action="store_true", help="unpickle the checkpoint fully (only for files you wrote)")
    ap.add_argument("--N_grid", type=int, default=256, help="size of the grid on 1 side, larger=higher resolution")
    ap.add_argument("--x_range", nargs=2, type=float, default=[-1.0, 1.0], help="x range of the object")
    ap.add_argument("--y_range", nargs=2, type=float, default=[-1.0, 1.0], help="y range of the object")
    ap.add_argument("--z_range", nargs=2, type=float, default=[-1.0, 1.0], help="z range of the object")
    ap.add_argument("--sigma_threshold", type=float, default=20.0, help="threshold to consider a location is occupied")
    ap.add_argument("--chunk", type=int, default=1 << 20, help="grid points per field launch")
    ap.add_argument("--keep_all", action="store_true", help="keep every connected component (the reference's first file)")
    ap.add_argument("--exact_spacing", action="store_true",
                    help="divide the index by N - 1 and scale every axis with its own range (the reference divides by N)")
    ap.add_argument("--precision", choices=("split", "fp32"), default=None, help="arithmetic of the field kernel")
    ap.add_argument("--out", type=str, required=True, help="output .ply")
    return ap.parse_args(argv)


def main(argv=None):
    args = get_opts(argv)
    import numpy as np
    import torch
    import mirror_nerf_amd as M
    from mirror_nerf_amd import checkpoint, mesh
    if not torch.cuda.is_available():
        raise SystemExit("extract_mesh.py needs a GPU: there is no CPU path")
    if args.precision:
        M.set_precision(args.precision)
    dev = "cuda:0"
    model = M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=True)
    if args.g11:
        z = np.load(os.path.join(ROOT, "tests", "golden", "g11_trained_weights.npz"))
        model.load_state_dict({k[len("fine__"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("fine__")})
    else:
        checkpoint.load_ckpt(model, args.ckpt_path, model_name="nerf_fine", trusted=args.trusted)
    model = model.to(dev)
    t0 = time.time()
    vertices, triangles = mesh.extract_mesh(model, M.Embedding(10), args.x_range, args.y_range, args.z_range, args.N_grid,
                                            args.sigma_threshold, keep_largest=not args.keep_all,
                                            exact_spacing=args.exact_spacing, chunk=args.chunk)
    torch.cuda.synchronize()
    print(f"Mesh has {vertices.shape[0] / 1e6:.2f} M vertices and {triangles.shape[0] / 1e6:.2f} M faces "
          f"({time.time() - t0:.2f} s).")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    mesh.write_ply(args.out, vertices, triangles)
    print(f"wrote {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
