#!/usr/bin/env python3
"""Fixture G21: the colouring of a mesh along its vertex normals (extract_color_mesh.py --use_vertex_normal, lines 247-267
and 358-359), from the REFERENCE's render_rays on the trained weights of G11.

Build-container only (imports the reference read-only through `_ref_import`):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mesh_normals.py

The mesh is G20's: its stored float32 volume, max(sigma, 0), at threshold 10 through the restatement of tests/mesh_ref.py,
the largest component, world coordinates.  Its vertex normals come from the numpy float64 restatement of the project's
definition (tests/mesh_normals_ref.py; open3d is not available).  4096 vertices are picked with a fixed seed, their rays
built with the reference's own torch expression (lines 250-253: d = n, o = v - d * near * near_t) and rendered by the
reference's `render_rays` with the coarse and the fine model, N_samples = 64, N_importance = 128, test_time=True, in float32
and once more in float64 (stored as its float32 difference from the float32 run).  near = 0.05, far = 8.0: the bounds of
G11's training rays.

The reference is NOT stable on these rays: they start 0.05 in front of a surface, put their weight into the first coarse
bins, and a share of them flips a bin of sample_pdf between float32 and float64.  `meta.stats` records that
distribution -- per ray the largest difference over the channels: median, 95th percentile, share above 1e-4 -- and the
tests compare error distributions against the float64 run, not a max norm.  The bounds asserted below keep a regenerated
fixture from going ill-conditioned unnoticed.
"""
import copy
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.dont_write_bytecode = True

import make_golden as MG  # noqa: E402  (installs the reference import shim)
import make_golden_trained_capture as TC  # noqa: E402
import torch  # noqa: E402
import weights as W  # noqa: E402
from tests import mesh_normals_ref as NR  # noqa: E402
from tests import mesh_ref as MR  # noqa: E402
from tests.golden import fixtures as FX  # noqa: E402

N_VERTICES, N_SAMPLES, N_IMPORTANCE, NEAR, FAR, NEAR_T, CHUNK, PICK_SEED = 4096, 64, 128, 0.05, 8.0, 1.0, 32 * 1024, 21
PROBE = 0.02


def sigma64(model64, pts):
    """float64 sigma of the reference's field at (n, 3) points (the full forward with an all-zero direction)."""
    emb_xyz, emb_dir = MG.EMB["xyz"], MG.EMB["dir"]
    xyz = torch.from_numpy(np.asarray(pts, dtype=np.float64))
    with torch.no_grad():
        x = torch.cat([xyz, emb_dir(torch.zeros_like(xyz))], 1)
        return model64(x, compute_normal=False, sigma_only=False, embedding_xyz=emb_xyz)["sigma"].numpy().reshape(-1)


def main():
    from mirror_nerf_amd import mesh
    g20 = FX.Fixture("g20_mesh_trained")
    m = g20.meta
    mods, sds = TC.trained_models(0, 2, [])
    assert [W.checksum(s) for s in sds] == m["checksum"]
    volume = np.maximum(g20.outputs["sigma"], 0)
    v, t = MR.marching_cubes(volume, m["threshold"], mesh.mc_table())
    lv, lt, _, _ = MR.largest_component(v, t)
    assert (len(v), len(t), len(lv)) == (m["mesh"]["V"], m["mesh"]["T"], m["mesh"]["largest_vertices"])
    world = MR.index_to_world(lv, m["x_range"], m["y_range"], m["z_range"], m["N"])
    normals_all = NR.vertex_normals(world, lt)
    pick = np.sort(np.random.RandomState(PICK_SEED).choice(len(world), N_VERTICES, replace=False))
    verts, normals = world[pick], normals_all[pick]
    assert np.abs(np.linalg.norm(normals.astype(np.float64), axis=1) - 1).max() < 1e-6

    rays = NR.normal_rays_torch(verts, normals, NEAR, FAR, NEAR_T)
    assert rays.dtype == np.float32 and rays.shape == (N_VERTICES, 8)
    models = {"coarse": mods[0], "fine": mods[1]}
    models64 = {k: copy.deepcopy(mod).double() for k, mod in models.items()}
    with torch.no_grad():
        out = MG.ref_render_rays(models, MG.EMB, torch.from_numpy(rays), N_SAMPLES, False, 0, 0, N_IMPORTANCE, CHUNK, False,
                                 test_time=True)
        out64 = MG.ref_render_rays(models64, MG.EMB, torch.from_numpy(rays).double(), N_SAMPLES, False, 0, 0, N_IMPORTANCE,
                                   CHUNK, False, test_time=True)
    rgb32 = out["rgb_fine"].detach().numpy().astype(np.float32)
    rgb64 = out64["rgb_fine"].detach().numpy().astype(np.float64)
    assert out["rgb_fine"].dtype == torch.float32 and out64["rgb_fine"].dtype == torch.float64
    med, p95, share, d = NR.ray_error_stats(rgb32, rgb64)
    p, n = verts.astype(np.float64), normals.astype(np.float64)
    inward = float((sigma64(models64["fine"], p + PROBE * n) > sigma64(models64["fine"], p - PROBE * n)).mean())
    stats = dict(ref_median=med, ref_p95=p95, ref_share_1e4=share, ref_share_1e5=float((d > 1e-5).mean()), ref_max=float(d.max()),
                 agree_1e5=int((d <= 1e-5).sum()), normals_towards_higher_density=inward,
                 opacity_coarse_at_least_half=float((out["opacity_coarse"].numpy() >= 0.5).mean()),
                 rgb_min=float(rgb32.min()), rgb_max=float(rgb32.max()))
    print(json.dumps(stats, indent=1))
    assert med <= 1e-6 and p95 <= 4e-5 and share <= 0.02
    assert inward > 2.0 / 3.0      # a clear (two to one) majority: G11's trained surface is rough, the number itself is not pinned

    meta = dict(seed=0, n_models=2, tweaks=[], checksum=[W.checksum(s) for s in sds], weights_file=TC.WEIGHTS,
                mesh_of="g20_mesh_trained", threshold=m["threshold"], n_vertices=N_VERTICES, pick_seed=PICK_SEED,
                N_samples=N_SAMPLES, N_importance=N_IMPORTANCE, near=NEAR, far=FAR, near_t=NEAR_T, chunk=CHUNK, probe=PROBE,
                largest_vertices=int(len(world)), largest_triangles=int(len(lt)), stats=stats)
    MG.save("g21_mesh_normal_colors", meta, dict(vertices=verts, normals=normals, rays=rays, pick=pick.astype(np.int32)),
            dict(rgb_fine=rgb32, rgb_fine_fp64_minus_fp32=(rgb64 - rgb32).astype(np.float32)))


if __name__ == "__main__":
    main()
