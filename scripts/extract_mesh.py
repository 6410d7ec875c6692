#!/usr/bin/env python3
"""Command line of mesh extraction (the reference's extract_color_mesh.py without its dataset):

    python scripts/extract_mesh.py --ckpt_path ckpts/exp/last.ckpt --N_grid 256 --x_range -1 1 --y_range -1 1 \\
        --z_range -1 1 --sigma_threshold 20 --out mesh.ply
    python scripts/extract_mesh.py --g11 --N_grid 48 --x_range -1.5 1.5 --y_range -1.5 1.5 --z_range -0.3 1.7 \\
        --sigma_threshold 10 --out g11.ply
    python scripts/extract_mesh.py --g11 ... --use_vertex_normal --near 0.05 --far 8 --write_normals --out g11_color.ply

The density of `nerf_fine` is sampled on the grid, meshed and (unless --keep_all) reduced to its largest connected
component, all on the GPU; the PLY holds world coordinates.  Argument names follow extract_color_mesh.py:26-87 where
they apply.  --use_vertex_normal colours the vertices from the checkpoint alone (one ray per vertex along its normal,
rendered with nerf_coarse and nerf_fine; --near / --far stand in for the reference's dataset.bounds); --write_normals adds
the vertex normals to the PLY.  The reference's other colouring, from images and poses, is
mirror_nerf_amd.mesh.fuse_vertex_colors.
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
    ap.add_argument("--use_vertex_normal", action="store_true",
                    help="colour the vertices by rendering one ray per vertex along its normal (needs --near and --far)")
    ap.add_argument("--near", type=float, default=None, help="near bound of the colouring rays (dataset.bounds.min())")
    ap.add_argument("--far", type=float, default=None, help="far bound of the colouring rays (dataset.bounds.max())")
    ap.add_argument("--near_t", type=float, default=1.0, help="the ray starts near * near_t in front of the vertex")
    ap.add_argument("--N_samples", type=int, default=64, help="number of coarse samples of the colouring rays")
    ap.add_argument("--N_importance", type=int, default=128, help="number of additional fine samples of the colouring rays")
    ap.add_argument("--white_back", action="store_true", help="composite the colouring rays on a white background")
    ap.add_argument("--render_chunk", type=int, default=32 * 1024, help="colouring rays per render_rays call")
    ap.add_argument("--write_normals", action="store_true", help="write the vertex normals (nx, ny, nz) into the PLY")
    ap.add_argument("--out", type=str, required=True, help="output .ply")
    args = ap.parse_args(argv)
    if args.use_vertex_normal and (args.near is None or args.far is None):
        ap.error("--use_vertex_normal requires --near and --far")
    return args


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

    z = np.load(os.path.join(ROOT, "tests", "golden", "g11_trained_weights.npz")) if args.g11 else None

    def load(which):
        m = M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=True)
        if args.g11:
            m.load_state_dict({k[len(which) + 2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(which + "__")})
        else:
            checkpoint.load_ckpt(m, args.ckpt_path, model_name="nerf_" + which, trusted=args.trusted)
        return m.to(dev)

    model = load("fine")
    t0 = time.time()
    vertices, triangles = mesh.extract_mesh(model, M.Embedding(10), args.x_range, args.y_range, args.z_range, args.N_grid,
                                            args.sigma_threshold, keep_largest=not args.keep_all,
                                            exact_spacing=args.exact_spacing, chunk=args.chunk)
    torch.cuda.synchronize()
    print(f"Mesh has {vertices.shape[0] / 1e6:.2f} M vertices and {triangles.shape[0] / 1e6:.2f} M faces "
          f"({time.time() - t0:.2f} s).")
    colors = normals = None
    if args.use_vertex_normal or args.write_normals:
        normals = mesh.vertex_normals(vertices, triangles)
    if args.use_vertex_normal:
        t0 = time.time()
        colors = mesh.normal_vertex_colors(vertices, triangles, {"coarse": load("coarse"), "fine": model},
                                           {"xyz": M.Embedding(10), "dir": M.Embedding(4)}, args.near, args.far, args.near_t,
                                           args.N_samples, args.N_importance, args.white_back, args.render_chunk, normals=normals)
        torch.cuda.synchronize()
        print(f"Coloured {vertices.shape[0]} vertices along their normals ({time.time() - t0:.2f} s).")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    mesh.write_ply(args.out, vertices, triangles, colors, normals if args.write_normals else None)
    print(f"wrote {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
