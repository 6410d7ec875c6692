#!/usr/bin/env python3
"""Fixture G20: the density volume of mesh extraction, from the REFERENCE's field on the trained weights of G11.

Build-container only (imports the reference read-only through `_ref_import`):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mesh.py

What extract_color_mesh.py:146-185 computes before it hands over to mcubes, for a 48^3 grid over the box of the analytic
mirror scene (x, y in [-1.5, 1.5], z in [-0.3, 1.7]; the sphere of make_golden_trained.py lies inside): the query points
from three float64 linspaces and numpy's "xy" meshgrid, the reference's `nerf_fine` run on them in chunks with the FULL
forward and an all-zero direction, in float32 and once more in float64.  The volume is stored raw (before max(sigma, 0));
the float64 volume is stored as its difference from the float32 one (in float32: the difference is ~5e-5, so the sum
restores it to ~1e-11), which keeps the file below 1 MiB.
Then, for the colour fusion: the mesh of that volume at threshold 10 (restated by tests/mesh_ref.py with this
repository's table -- the reference's own mesher, mcubes, is not available), its largest component mapped to world
coordinates, 2048 of its vertices, their occlusion rays for the first training pose of G11, and the reference's
`render_rays({"coarse": nerf_fine}, ..., N_samples=64, N_importance=0, test_time=True)["opacity_coarse"]` on those rays.
`meta` records the properties of the volume the tests lean on; they are asserted here so that a regenerated fixture
cannot silently become ill-conditioned.
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
from oracle import mirror_nerf_oracle as O  # noqa: E402
from tests import mesh_ref as MR  # noqa: E402

N = 48
X_RANGE, Y_RANGE, Z_RANGE = (-1.5, 1.5), (-1.5, 1.5), (-0.3, 1.7)
THRESHOLD = 10.0
CHUNK = 32 * 1024
N_VERTICES, N_SAMPLES, RES, NEAR = 2048, 64, 64, 0.05


def query_points():
    x = np.linspace(X_RANGE[0], X_RANGE[1], N)
    y = np.linspace(Y_RANGE[0], Y_RANGE[1], N)
    z = np.linspace(Z_RANGE[0], Z_RANGE[1], N)
    return np.stack(np.meshgrid(x, y, z), -1).reshape(-1, 3)


def sigma_volume(model, emb_xyz, emb_dir, pts, dtype):
    xyz = torch.from_numpy(pts).to(dtype)
    dirs = torch.zeros_like(xyz)
    out = []
    with torch.no_grad():
        for i in range(0, xyz.shape[0], CHUNK):
            x = torch.cat([xyz[i:i + CHUNK], emb_dir(dirs[i:i + CHUNK])], 1)
            out.append(model(x, compute_normal=False, sigma_only=False, embedding_xyz=emb_xyz)["sigma"])
    return torch.cat(out, 0).numpy().reshape(N, N, N)


def first_training_pose():
    """View 0 of make_golden_trained.scene_views(24, ...): the pose and the focal length of its 64 x 64 images."""
    a = -0.9
    eye = (2.6 * np.sin(a), -2.6 * np.cos(a) + 0.2, 0.9 + 0.5 * np.cos(0.0))
    return O.look_at_pose(eye=eye, target=(0.1, 0.6, 0.6)), 0.5 * RES / np.tan(0.5 * 0.9)


def main():
    from mirror_nerf_amd import mesh
    mods, sds = TC.trained_models(0, 2, [])
    fine = mods[1]
    emb_xyz, emb_dir = MG.EMB["xyz"], MG.EMB["dir"]
    pts = query_points()
    s32 = sigma_volume(fine, emb_xyz, emb_dir, pts.astype(np.float32), torch.float32).astype(np.float32)
    s64 = sigma_volume(copy.deepcopy(fine).double(), emb_xyz, emb_dir, pts.astype(np.float32).astype(np.float64), torch.float64)
    assert s32.dtype == np.float32 and s64.dtype == np.float64

    floor = float(np.abs(s64 - s32).max())
    scale = float(np.abs(s64).max())
    near_thr = int((np.abs(s64 - THRESHOLD) <= 1e-4 * scale).sum())
    in32, in64 = s32 >= np.float32(THRESHOLD), s64 >= THRESHOLD
    centre = np.array([0.45, 0.1, 0.55])
    core = np.linalg.norm(pts - centre, axis=1).reshape(N, N, N) < 0.45
    clamped = np.maximum(s32, 0)
    z_cross = in32[:, :, 1:] != in32[:, :, :-1]
    min_z_diff = float(np.abs(clamped[:, :, 1:] - clamped[:, :, :-1])[z_cross].min())
    stats = dict(sigma_min=float(s32.min()), sigma_max=float(s32.max()), inside_fraction=float(in32.mean()),
                 crossed_edges=MR.crossed_edges(clamped, THRESHOLD), floor_sigma=floor, near_threshold_points=near_thr,
                 decisions_differ=int((in32 != in64).sum()), min_crossed_z_difference=min_z_diff,
                 core_points=int(core.sum()), core_fraction_above_10=float((s32[core] > 10).mean()))
    print(json.dumps(stats, indent=1))
    assert stats["core_fraction_above_10"] == 1.0 and stats["decisions_differ"] == 0
    assert 0.05 < stats["inside_fraction"] < 0.3 and stats["floor_sigma"] < 1e-3
    assert stats["near_threshold_points"] <= 11 and stats["min_crossed_z_difference"] > 0.1

    table = mesh.mc_table()
    v, t = MR.marching_cubes(clamped, THRESHOLD, table)
    assert len(v) == stats["crossed_edges"]
    lv, lt, n_comp, largest = MR.largest_component(v, t)
    world = MR.index_to_world(lv, X_RANGE, Y_RANGE, Z_RANGE, N)
    pick = np.sort(np.random.RandomState(20).choice(len(world), N_VERTICES, replace=False))
    verts = world[pick]
    pose, focal = first_training_pose()
    image = np.zeros((RES, RES, 3), np.uint8)
    _, depth, _, rays64 = MR.project_view(verts, image, pose, focal, NEAR)
    rays = rays64.astype(np.float32)
    with torch.no_grad():
        out = MG.ref_render_rays({"coarse": fine}, MG.EMB, torch.from_numpy(rays), N_SAMPLES, False, 0, 0, 0, CHUNK, False,
                                 test_time=True)
        out64 = MG.ref_render_rays({"coarse": copy.deepcopy(fine).double()}, MG.EMB, torch.from_numpy(rays).double(), N_SAMPLES,
                                   False, 0, 0, 0, CHUNK, False, test_time=True)
    opacity = out["opacity_coarse"].numpy().astype(np.float32)
    floor_op = float(np.abs(out64["opacity_coarse"].numpy() - opacity).max())
    print(f"mesh: V={len(v)} T={len(t)} components={n_comp} largest={largest} ({len(lv)} vertices); opacity in "
          f"[{opacity.min():.3f}, {opacity.max():.3f}], {float((opacity < 0.2).mean()):.3f} below 0.2, fp32-vs-fp64 {floor_op:.1e}")
    meta = dict(seed=0, n_models=2, tweaks=[], checksum=[W.checksum(s) for s in sds], weights_file=TC.WEIGHTS,
                N=N, x_range=X_RANGE, y_range=Y_RANGE, z_range=Z_RANGE, threshold=THRESHOLD, chunk=CHUNK,
                floor={"sigma": floor, "opacity_coarse": floor_op}, stats=stats,
                mesh=dict(V=int(len(v)), T=int(len(t)), n_components=n_comp, largest_triangles=largest, largest_vertices=int(len(lv))),
                fusion=dict(n_vertices=N_VERTICES, N_samples=N_SAMPLES, near=NEAR, res=RES, focal=float(focal), pick_seed=20))
    MG.save("g20_mesh_trained", meta, dict(vertices=verts, pose=pose.astype(np.float32), rays=rays),
            dict(sigma=s32, sigma_fp64_minus_fp32=(s64 - s32).astype(np.float32), opacity_coarse=opacity, depth=depth))


if __name__ == "__main__":
    main()
