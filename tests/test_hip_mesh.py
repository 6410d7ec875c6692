"""GPU tests of mesh extraction (mirror_nerf_amd/mesh.py over csrc/mnrf_mesh.hip): grid points bit-equal to numpy's
construction, the density grid against the reference's volume (fixture G20, tests/golden/make_golden_mesh.py), marching
cubes against the cell-loop restatement of tests/mesh_ref.py, manifold properties of closed surfaces, the largest
component against a numpy union-find, the colour fusion against a float64 restatement and the reference's opacities,
and the whole chain down to a PLY file.  Sections 8 to 10 take the kernels to the edges of their launch geometry: blocks
filled to the 768 vertices the count kernel packs, more than 65 535 blocks, strides of 70 001 points, non-finite
densities; components of renumbered meshes, of strips a million triangles long and of triangle arrays with indices out
of range; the projection on images one pixel wide or high.  Every one of those cases asserts that it reaches its edge.

Bars.  sigma: the project's 1e-4 * max(1, max|sigma_ref|) (tests/test_hip_parity.py), raised to 4 x the fixture's own
fp32-vs-fp64 difference if that is larger (FX.tolerance's rule); the inside mask must agree wherever the reference is
farther than that from the threshold, and at most 0.01 % of the grid (11 points; the reference alone leaves out 3) may be
that close.  Marching cubes: identical topology after canonicalisation, vertices within 2 ulp of the grid extent (the
restatement evaluates the same float32 expression, so only the rounding of the division may differ).  Colours: 1e-5
(relative; absolute below 1) on the interpolated floats, 1 unit on the uint8 output (truncation next to an integer); opacity at the
project's 1e-4 (raised by the floor rule)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mesh_ref as MR
from tests.golden import fixtures as FX

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(params=["split", "fp32"])
def precision(request):
    from mirror_nerf_amd import mirror_nerf as MN
    old = MN.PRECISION
    MN.set_precision(request.param)
    yield request.param
    MN.set_precision(old)


@pytest.fixture(scope="module")
def g20():
    return FX.Fixture("g20_mesh_trained")


@pytest.fixture(scope="module")
def table():
    from mirror_nerf_amd import mesh
    return mesh.mc_table()


def _fine(fx):
    import mirror_nerf_amd as M
    sd = fx.state_dicts()[1]
    m = M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV)


def _emb():
    import mirror_nerf_amd as M
    return {"xyz": M.Embedding(10), "dir": M.Embedding(4)}


def _mc(volume, thr):
    from mirror_nerf_amd import mesh
    v, t = mesh.marching_cubes(torch.from_numpy(np.ascontiguousarray(volume, dtype=np.float32)).to(DEV), thr)
    assert v.is_cuda and t.is_cuda and v.dtype == torch.float32 and t.dtype == torch.int32
    return v, t


# ----------------------------------------------------------------------------------------------- 1. grid points
@pytest.mark.parametrize("N,xr,yr,zr,chunk", [
    (2, (-1.0, 1.0), (-1.0, 1.0), (-1.0, 1.0), 8),
    (5, (-1.0, 1.0), (-1.0, 1.0), (-1.0, 1.0), 7),                     # a chunk that does not divide N^3
    (17, (-1.5, 1.5), (-0.37, 2.2), (0.11, 0.93), 1000),                # a non-cubic box
    (48, (-1.5, 1.5), (-1.5, 1.5), (-0.3, 1.7), 32768),                 # the G20 grid
    (33, (0.1, 0.1), (-2.0, 3.0), (1e-3, 1e-3 + 1e-9), 4097),           # a degenerate range and a nearly degenerate one
    (64, (-1.0 / 3.0, 2.0 / 3.0), (1e6, 1e6 + 1.0), (-1e-20, 1e-20), 100000),
])
def test_grid_points_bit_equal_numpy(N, xr, yr, zr, chunk):
    from mirror_nerf_amd import mesh
    x, y, z = np.linspace(xr[0], xr[1], N), np.linspace(yr[0], yr[1], N), np.linspace(zr[0], zr[1], N)
    want = np.stack(np.meshgrid(x, y, z), -1).reshape(-1, 3).astype(np.float32)
    got = np.empty_like(want)
    buf = torch.empty(chunk, 3, device=DEV)
    for s in range(0, N ** 3, chunk):
        n = min(chunk, N ** 3 - s)
        got[s:s + n] = mesh.grid_points(xr, yr, zr, N, s, n, out=buf).cpu().numpy()
    assert got.tobytes() == want.tobytes()


# ----------------------------------------------------------------------------------------------- 2. density grid vs G20
def test_density_grid_matches_reference(g20, precision):
    from mirror_nerf_amd import mesh
    m = g20.meta
    ref = g20.outputs["sigma"].astype(np.float64)
    ref64 = ref + g20.outputs["sigma_fp64_minus_fp32"].astype(np.float64)
    tol = max(1e-4 * max(1.0, float(np.abs(ref).max())), 4.0 * m["floor"]["sigma"])
    model = _fine(g20)
    vol = mesh.density_grid(model, _emb()["xyz"], m["x_range"], m["y_range"], m["z_range"], m["N"], chunk=50000)
    assert vol.shape == (m["N"],) * 3 and vol.is_cuda and vol.dtype == torch.float32
    got = vol.cpu().numpy().astype(np.float64)
    assert got.min() >= 0.0
    err = float(np.abs(got - np.maximum(ref, 0)).max())
    thr = m["threshold"]
    far = np.abs(ref - thr) > tol
    left_out = int((~far).sum())
    wrong = int(((got >= thr) != (ref >= thr))[far].sum())
    print(f"[{precision}] max |sigma - sigma_ref| = {err:.3e} (tol {tol:.3e}, max|sigma_ref| {np.abs(ref).max():.1f}); "
          f"{left_out} points within tol of the threshold; {wrong} decisions differ elsewhere; "
          f"vs the fp64 reference {np.abs(got - np.maximum(ref64, 0)).max():.3e}")
    assert err <= tol
    assert left_out <= int(1e-4 * ref.size)
    assert wrong == 0
    # another chunking writes the same volume
    vol2 = mesh.density_grid(model, _emb()["xyz"], m["x_range"], m["y_range"], m["z_range"], m["N"], chunk=1 << 20)
    assert torch.equal(vol, vol2)


def test_density_grid_hash_grid_model():
    import mirror_nerf_amd as M
    from mirror_nerf_amd import mesh
    torch.manual_seed(0)
    model = M.MirrorNeRFTcnn(encoding="hashgrid", bound=1.0, predict_normal=True, predict_mirror_mask=True).to(DEV)
    N, rng = 12, (-0.9, 0.9)
    vol = mesh.density_grid(model, M.Embedding(0), rng, rng, rng, N, chunk=1000)
    pts = mesh.grid_points(rng, rng, rng, N, 0, N ** 3, device=DEV)
    want = model(pts.contiguous(), compute_normal=False, sigma_only=True)["sigma"].clamp_min(0).view(N, N, N)
    assert torch.equal(vol, want) and float(vol.abs().max()) > 0


# ----------------------------------------------------------------------------------------------- 3. marching cubes
def _axes(shape, pad=0.0):
    return np.meshgrid(*[np.linspace(-1 - pad, 1 + pad, n) for n in shape], indexing="ij")


def _sphere(shape=(24, 24, 24), r=0.6, c=(0.05, -0.1, 0.02)):
    X, Y, Z = _axes(shape, 0.2)
    return (r - np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2)).astype(np.float32)


def _torus(shape=(28, 28, 20), R=0.65, r=0.25):
    X, Y, Z = _axes(shape, 0.2)
    return (r - np.sqrt((np.sqrt(X ** 2 + Y ** 2) - R) ** 2 + (1.3 * Z) ** 2)).astype(np.float32)


def _two_spheres(shape=(30, 22, 22)):
    X, Y, Z = _axes(shape, 0.2)
    a = 0.42 - np.sqrt((X + 0.55) ** 2 + Y ** 2 + Z ** 2)
    b = 0.27 - np.sqrt((X - 0.6) ** 2 + (Y - 0.1) ** 2 + Z ** 2)
    return np.maximum(a, b).astype(np.float32)


def _smooth_random(shape=(22, 23, 24), seed=1, border=True):
    rs = np.random.RandomState(seed)
    X, Y, Z = _axes(shape)
    f = np.zeros(shape)
    for _ in range(6):
        k = rs.uniform(3, 9, 3)
        f += rs.uniform(0.5, 1) * np.sin(k[0] * X + k[1] * Y + k[2] * Z + rs.uniform(0, 6.28))
    f = f.astype(np.float32)
    if border:
        f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = (-3.0,) * 6
    return f


VOLUMES = {
    "sphere": (_sphere, 0.0), "torus": (_torus, 0.0), "two_spheres": (_two_spheres, 0.0),
    "smooth_random": (_smooth_random, 0.1),
    "cut_by_boundary": (lambda: _smooth_random((19, 21, 17), seed=2, border=False), -0.2),
    "sphere_cut": (lambda: _sphere((16, 20, 12), r=1.3), 0.0),
    "non_cubic": (lambda: _sphere((9, 31, 14), r=0.7), 0.0),
    "long_z": (lambda: _smooth_random((3, 4, 300), seed=3, border=False), 0.0),      # rows longer than a block
    "all_inside": (lambda: np.full((7, 8, 9), 5.0, np.float32), 1.0),
    "all_outside": (lambda: np.full((7, 8, 9), -5.0, np.float32), 1.0),
    "n2_one_corner": (lambda: np.array([[[1, 0], [0, 0]], [[0, 0], [0, 0]]], np.float32), 0.5),
    "n2_checker": (lambda: np.array([[[1, 0], [0, 1]], [[0, 1], [1, 0]]], np.float32), 0.5),
    "ties": (lambda: np.round(_smooth_random((14, 14, 14), seed=4) * 2) / 2, 0.5),     # many values equal to the threshold
}


def _compare_with_restatement(vol, thr, table):
    v, t = _mc(vol, thr)
    rv, rt = MR.marching_cubes(vol, thr, table)
    assert v.shape[0] == rv.shape[0] == MR.crossed_edges(vol, thr) and t.shape[0] == rt.shape[0]
    gv, gt = MR.canonical(v.cpu().numpy(), t.cpu().numpy())
    wv, wt = MR.canonical(rv, rt)
    if len(gv):
        ulp = np.spacing(np.float32(max(vol.shape) - 1))
        err = float(np.abs(gv.astype(np.float64) - wv).max())
        assert err <= 2 * ulp, (err, ulp)
    assert np.array_equal(gt, wt)
    return v, t


@pytest.mark.parametrize("name", sorted(VOLUMES))
def test_marching_cubes_matches_restatement(name, table):
    make, thr = VOLUMES[name]
    vol = make()
    v, t = _compare_with_restatement(vol, thr, table)
    if name in ("all_inside", "all_outside"):
        assert v.shape == (0, 3) and t.shape == (0, 3)
    if name == "n2_one_corner":
        assert v.shape[0] == 3 and t.shape[0] == 1
    if name == "n2_checker":
        assert v.shape[0] == 12 and t.shape[0] == 4
    if name == "smooth_random":      # the ambiguous faces are there
        ins = vol >= thr
        amb = (ins[:-1, :-1] & ins[1:, 1:] & ~ins[1:, :-1] & ~ins[:-1, 1:]).sum()
        assert amb > 0


def test_marching_cubes_g20(g20, table):
    from mirror_nerf_amd import mesh
    m = g20.meta
    vol = np.maximum(g20.outputs["sigma"], 0)
    v, t = _compare_with_restatement(vol, m["threshold"], table)
    assert (v.shape[0], t.shape[0]) == (m["mesh"]["V"], m["mesh"]["T"]) and v.shape[0] == m["stats"]["crossed_edges"]
    lv, lt, info = mesh.largest_component(v, t, return_info=True)
    assert info == {"n_components": m["mesh"]["n_components"], "largest_triangles": m["mesh"]["largest_triangles"]}
    assert lt.shape[0] == m["mesh"]["largest_triangles"] and lv.shape[0] == m["mesh"]["largest_vertices"]


# ----------------------------------------------------------------------------------------------- 4. manifold properties
@pytest.mark.parametrize("name,euler", [("sphere", 2), ("torus", 0), ("two_spheres", 4)])
def test_closed_surfaces_are_oriented_manifolds(name, euler):
    make, thr = VOLUMES[name]
    vol = make()
    v, t = _mc(vol, thr)
    vn, tn = v.cpu().numpy(), t.cpu().numpy()
    assert MR.is_closed_oriented(tn)
    assert MR.euler_characteristic(len(vn), tn) == euler
    assert MR.signed_volume(vn, tn) > 0
    assert MR.on_grid_edges(vn) and vn.min() >= 0 and (vn.max(0) <= np.array(vol.shape) - 1).all()
    assert tn.min() >= 0 and tn.max() < len(vn) and len(np.unique(tn)) == len(vn)
    v2, t2 = _mc(vol, thr)
    assert torch.equal(v, v2) and torch.equal(t, t2)
    if name == "sphere":      # the volume of the sphere, in cells
        cell = (2.4 / (vol.shape[0] - 1)) ** 3
        assert abs(MR.signed_volume(vn, tn) * cell / (4 / 3 * np.pi * 0.6 ** 3) - 1) < 0.05


# ----------------------------------------------------------------------------------------------- 5. largest component
@pytest.mark.parametrize("name", ["two_spheres", "smooth_random", "g20", "ties"])
def test_largest_component_matches_union_find(name, g20):
    from mirror_nerf_amd import mesh
    if name == "g20":
        vol, thr = np.maximum(g20.outputs["sigma"], 0), g20.meta["threshold"]
    else:
        make, thr = VOLUMES[name]
        vol = make()
    v, t = _mc(vol, thr)
    labels = mesh.component_labels(int(v.shape[0]), t).cpu().numpy()
    assert np.array_equal(labels, MR.union_find_labels(int(v.shape[0]), t.cpu().numpy()))
    lv, lt, info = mesh.largest_component(v, t, return_info=True)
    wv, wt, n_comp, largest = MR.largest_component(v.cpu().numpy(), t.cpu().numpy())
    assert info == {"n_components": n_comp, "largest_triangles": largest}
    assert lt.dtype == torch.int32 and np.array_equal(lt.cpu().numpy(), wt)          # compacted indices, triangle order kept
    assert np.array_equal(lv.cpu().numpy(), wv)
    assert len(np.unique(wt)) == len(wv) == lv.shape[0]                               # no unreferenced vertex is left
    if name == "two_spheres":      # the bigger sphere survives: it sits at x < 0 (low first index)
        assert n_comp == 2 and float(lv[:, 0].max()) < (vol.shape[0] - 1) / 2
        assert MR.is_closed_oriented(wt) and MR.euler_characteristic(len(wv), wt) == 2


def test_largest_component_ties_and_empty():
    from mirror_nerf_amd import mesh
    # two components of two triangles each: the smallest label (the one holding vertex 0) wins; vertex 4 is unreferenced
    v = torch.arange(27, dtype=torch.float32, device=DEV).view(9, 3)
    t = torch.tensor([[5, 6, 7], [0, 1, 2], [6, 7, 8], [2, 1, 3]], dtype=torch.int32, device=DEV)
    lv, lt = mesh.largest_component(v, t)
    assert lt.cpu().tolist() == [[0, 1, 2], [2, 1, 3]] and torch.equal(lv, v[:4])
    ev, et = mesh.largest_component(v[:0], t[:0])
    assert ev.shape == (0, 3) and et.shape == (0, 3)


# ----------------------------------------------------------------------------------------------- 6. colour fusion
def _poses():
    from mirror_nerf_amd import synthetic as SY
    return np.stack([SY.look_at_pose(eye=e, target=(0.1, 0.4, 0.5)) for e in
                     ((2.2, -2.4, 1.3), (-2.0, -2.2, 0.9), (0.3, -3.0, 1.6))]).astype(np.float32)


def test_projection_and_sampling_match_float64(g20):
    from mirror_nerf_amd import mesh
    rs = np.random.RandomState(7)
    H, W, focal, near = 37, 53, 61.7, 0.05
    verts = g20.inputs["vertices"].copy()
    poses = _poses()
    # one vertex behind the first camera and one far outside its image: clipped to the border, not dropped
    eye, fwd = poses[0][:, 3], -poses[0][:, 2]
    verts[0] = eye - 1.5 * fwd + 0.2 * poses[0][:, 0]
    verts[1] = eye + 1.0 * fwd + 40.0 * poses[0][:, 0] - 30.0 * poses[0][:, 1]
    images = rs.randint(0, 256, (3, H, W, 3)).astype(np.uint8)
    opac = rs.uniform(0, 0.4, (3, len(verts))).astype(np.float32)
    opac[1, 5], opac[2, 6], opac[0, 7] = np.nan, np.inf, -np.inf
    dv = torch.from_numpy(verts).to(DEV)
    cs, ds, per_view = [], [], []
    for k in range(3):
        colors, depth, rays = mesh.project_view(dv, torch.from_numpy(images[k]).to(DEV), poses[k], focal, near)
        wc, wd, pix, wr = MR.project_view(verts, images[k], poses[k], focal, near)
        # 1e-5 relative (absolute below 1): the kernel interpolates in float32 -- three roundings of 2^-24 relative on
        # terms that are all positive -- from the same float32 pixel coordinate the restatement uses
        assert (np.abs(colors.cpu().numpy() - wc) <= 1e-5 * np.maximum(1.0, np.abs(wc))).all()
        np.testing.assert_allclose(depth.cpu().numpy(), wd, rtol=1e-12, atol=1e-12)
        r = rays.cpu().numpy()
        np.testing.assert_allclose(r[:, :7], wr[:, :7], rtol=0, atol=2e-6)
        np.testing.assert_allclose(r[:, 7], wd, rtol=1e-7)
        cs.append(wc), ds.append(wd), per_view.append((colors, depth))
        if k == 0:
            assert wd[0] < 0 and (pix[1, 0] in (0, W - 1)) and (pix[1, 1] in (0, H - 1))
            assert np.isfinite(colors.cpu().numpy()[:2]).all()
    # the accumulation with given opacities (NaN -> 0 = unoccluded, as numpy.nan_to_num(opacity, 1) really does)
    from mirror_nerf_amd import _lib
    V = len(verts)
    csum = torch.zeros(V, 3, dtype=torch.float64, device=DEV)
    wsum = torch.zeros(V, dtype=torch.float64, device=DEV)
    for k, (colors, depth) in enumerate(per_view):
        _lib.check(_lib.lib().mnrf_accumulate_colors(_lib.ptr(colors), _lib.ptr(depth), _lib.ptr(torch.from_numpy(opac[k]).to(DEV)),
                                                     0.2, V, _lib.ptr(csum), _lib.ptr(wsum), _lib.stream()), "accumulate")
    want8, wcs, wws = MR.fuse(cs, ds, opac, 0.2)
    np.testing.assert_allclose(wsum.cpu().numpy(), wws, rtol=1e-12)
    np.testing.assert_allclose(csum.cpu().numpy(), wcs, rtol=1e-5, atol=1e-5)
    got8 = (csum / wsum[:, None]).to(torch.uint8).cpu().numpy()
    ok = wws > 0.5      # (a vertex behind a camera has a negative weight there; the ratio is still the reference's)
    assert np.abs(got8[ok].astype(int) - want8[ok].astype(int)).max() <= 1


def test_occlusion_opacity_matches_reference(g20, precision):
    from mirror_nerf_amd import mesh
    f = g20.meta["fusion"]
    rays = torch.from_numpy(g20.inputs["rays"]).to(DEV)
    got = mesh.occlusion_opacity(_fine(g20), _emb(), rays, f["N_samples"], False, 700).cpu().numpy()
    want = g20.outputs["opacity_coarse"]
    tol = FX.tolerance("opacity_coarse", g20.meta)
    err = float(np.abs(got - want).max())
    print(f"[{precision}] max |opacity - ref| = {err:.3e} (tol {tol:.1e})")
    assert err <= tol
    # and the rays the kernel builds for those vertices are the fixture's rays
    img = torch.zeros(f["res"], f["res"], 3, dtype=torch.uint8, device=DEV)
    _, depth, r = mesh.project_view(torch.from_numpy(g20.inputs["vertices"]).to(DEV), img, g20.inputs["pose"], f["focal"], f["near"])
    np.testing.assert_allclose(r.cpu().numpy(), g20.inputs["rays"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(depth.cpu().numpy(), g20.outputs["depth"], rtol=1e-12)


def test_fuse_vertex_colors_end_to_end(g20, precision):
    from mirror_nerf_amd import mesh
    rs = np.random.RandomState(11)
    H = W = 32
    focal, near = 0.5 * W / np.tan(0.45), 0.05
    verts = g20.inputs["vertices"][:600]
    poses = _poses()
    images = rs.randint(0, 256, (3, H, W, 3)).astype(np.uint8)
    model = _fine(g20)
    dv = torch.from_numpy(verts).to(DEV)
    got, csum, wsum = mesh.fuse_vertex_colors(dv, model, _emb(), torch.from_numpy(images).to(DEV), poses, focal, near,
                                              N_samples=64, occ_threshold=0.2, chunk=256, return_sums=True)
    assert got.dtype == torch.uint8 and got.shape == (600, 3)
    cs, ds, ops = [], [], []
    for k in range(3):
        wc, wd, _, _ = MR.project_view(verts, images[k], poses[k], focal, near)
        _, _, rays = mesh.project_view(dv, torch.from_numpy(images[k]).to(DEV), poses[k], focal, near)
        cs.append(wc), ds.append(wd), ops.append(mesh.occlusion_opacity(model, _emb(), rays, 64, False, 256).cpu().numpy())
    want8, wcs, wws = MR.fuse(cs, ds, ops, 0.2)
    np.testing.assert_allclose(wsum.cpu().numpy(), wws, rtol=1e-12)
    assert np.abs(got.cpu().numpy().astype(int) - want8.astype(int)).max() <= 1


# ----------------------------------------------------------------------------------------------- 7. end to end
def test_extract_mesh_end_to_end(g20, precision, tmp_path):
    from mirror_nerf_amd import mesh
    m = g20.meta
    model = _fine(g20)
    v, t = mesh.extract_mesh(model, _emb()["xyz"], m["x_range"], m["y_range"], m["z_range"], m["N"], m["threshold"])
    assert v.dtype == torch.float32 and t.dtype == torch.int32 and t.shape[0] > 20000
    # the mesh of the volume the kernels computed, through the restatements
    vol = mesh.density_grid(model, _emb()["xyz"], m["x_range"], m["y_range"], m["z_range"], m["N"]).cpu().numpy()
    rv, rt = MR.marching_cubes(vol, m["threshold"], mesh.mc_table())
    wv, wt, _, _ = MR.largest_component(rv, rt)
    a, b = MR.canonical(v.cpu().numpy(), t.cpu().numpy()), MR.canonical(MR.index_to_world(wv, m["x_range"], m["y_range"], m["z_range"], m["N"]), wt)
    assert np.array_equal(a[1], b[1]) and float(np.abs(a[0] - b[0]).max()) <= 1e-5
    # the trained sphere (centre (0.45, 0.1, 0.55), radius 0.55) is in it
    c = v.cpu().numpy()
    d = np.linalg.norm(c * m["N"] / (m["N"] - 1.0) - np.array([0.45, 0.1, 0.55]) * 1.0, axis=1)
    assert (np.abs(d - 0.55) < 0.12).sum() > 500
    path = str(tmp_path / "mesh.ply")
    mesh.write_ply(path, v, t)
    pv, pt, pc = mesh.read_ply(path)
    assert pc is None and pv.tobytes() == v.cpu().numpy().tobytes() and np.array_equal(pt, t.cpu().numpy())
    ve, te = mesh.extract_mesh(model, _emb()["xyz"], m["x_range"], m["y_range"], m["z_range"], m["N"], m["threshold"],
                               keep_largest=False, exact_spacing=True)
    assert (ve.shape[0], te.shape[0]) == (rv.shape[0], rt.shape[0])


def test_extract_mesh_script(tmp_path):
    out = str(tmp_path / "g11.ply")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "extract_mesh.py"), "--g11", "--N_grid", "48",
                        "--x_range", "-1.5", "1.5", "--y_range", "-1.5", "1.5", "--z_range", "-0.3", "1.7",
                        "--sigma_threshold", "10", "--out", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    from mirror_nerf_amd import mesh
    v, t, c = mesh.read_ply(out)
    assert len(t) > 20000 and t.max() < len(v) and c is None


# ----------------------------------------------------------------------------------------------- 8. marching cubes at its edges
MC_BLOCK = 256        # points per block of the marching-cubes kernels
GUARD = 16


def _mc_block_counts(vol, thr):
    """mnrf_mc_count alone: the (blocks, 2) int32 [vertices, triangles] per block, written inside a buffer of sentinels."""
    from mirror_nerf_amd import _lib
    L = _lib.lib()
    dv = torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32)).to(DEV)
    nx, ny, nz = vol.shape
    blocks = int(L.mnrf_mc_blocks(nx, ny, nz))
    assert blocks == (vol.size + MC_BLOCK - 1) // MC_BLOCK
    buf = torch.full((GUARD + blocks + GUARD, 2), -7, dtype=torch.int32, device=DEV)
    with torch.cuda.device(DEV):
        _lib.check(L.mnrf_mc_count(_lib.ptr(dv), nx, ny, nz, float(thr), _lib.ptr(buf[GUARD:GUARD + blocks]), _lib.stream()), "mnrf_mc_count")
    got = buf.cpu().numpy()
    assert (got[:GUARD] == -7).all() and (got[GUARD + blocks:] == -7).all()
    return got[GUARD:GUARD + blocks]


def _checker(shape):
    I, J, K = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    return ((I + J + K) % 2).astype(np.float32)


def _profile_volume(shape, seed):
    """A seeded smooth profile along the long axis plus a small dependence on the two short ones: crossings of all three
    edge kinds, a few thousand of them."""
    rs = np.random.RandomState(seed)
    axis = int(np.argmax(shape))
    s = np.arange(shape[axis], dtype=np.float64)
    f = sum(rs.uniform(0.5, 1) * np.sin(s * 2 * np.pi / rs.uniform(40, 90) + rs.uniform(0, 6.28)) for _ in range(3))
    grid = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    a, b = [g for i, g in enumerate(grid) if i != axis]
    return (f[tuple(slice(None) if i == axis else None for i in range(3))] + 0.21 * a - 0.13 * b).astype(np.float32)


@pytest.mark.parametrize("name", sorted(VOLUMES) + ["checker_rows", "checker_planes"])
def test_block_counts_match_restatement(name, table):
    """What mc_count_kernel leaves per block -- vertices in the low half of one scanned word, triangles in the high half --
    against numpy, block by block.  The checkerboards cross every grid edge: (3, 3, 600) keeps whole blocks inside one z-row,
    where a block reaches the 768 vertices (3 a point) the packing is sized for; (9, 10, 31) has rows of 31 and planes of 310
    points, so every block holds eight rows or more and most hold parts of two planes."""
    if name.startswith("checker"):
        shape = (3, 3, 600) if name == "checker_rows" else (9, 10, 31)
        vol, thr = _checker(shape), 0.5
    else:
        make, thr = VOLUMES[name]
        vol = make()
    got = _mc_block_counts(vol, thr)
    want = MR.block_counts(vol, thr, table, MC_BLOCK)
    assert got.shape == want.shape and np.array_equal(got, want)
    if name == "checker_rows":
        assert got[:, 0].max() == 3 * MC_BLOCK == 768 and (got[:, 0] == 768).sum() >= 2 and got[:, 1].max() >= 2 * MC_BLOCK
    if name == "checker_planes":
        first, last = np.arange(len(got)) * MC_BLOCK, np.minimum(np.arange(len(got)) * MC_BLOCK + MC_BLOCK, vol.size) - 1
        rows = last // 31 - first // 31 + 1
        assert len(got) == 11 and rows[:-1].min() >= 8 and (last // 310 != first // 310).sum() >= 6
        assert got[:, 0].sum() == MR.crossed_edges(vol, thr) == 8 * 10 * 31 + 9 * 9 * 31 + 9 * 10 * 30
    if name.startswith("checker"):      # and the whole mesh
        _compare_with_restatement(vol, thr, table)


def _far_corner_volume():
    """257^3, negative everywhere but in a lens in the plane i = 255: 12 cells of radius along j and k, less than one along
    i.  Only the planes i >= 254 lie past block 65 535 (65 536 * 256 points are 254.01 planes), so a closed surface that
    keeps all its work there is one point thick."""
    N = 257
    vol = np.full((N, N, N), -1.0, dtype=np.float32)
    i, J, K = np.meshgrid(np.arange(250, N), np.arange(N), np.arange(N), indexing="ij")
    vol[250:] = 1.0 - np.sqrt(((i - 255.1) / 0.8) ** 2 + ((J - 236.3) / 12.0) ** 2 + ((K - 229.6) / 12.0) ** 2)
    return vol


def test_marching_cubes_past_65535_blocks(table):
    """66 308 blocks (257^3 = 66 307 * 256 + 1 points); every active point lies in a block with an index above 65 535.
    Against the cropped restatement (tests/test_mesh_cpu.py shows it equal to the uncropped one).  Measured next to an
    MI355X: the whole test 0.43 s, most of it numpy over the 17 M points."""
    from mirror_nerf_amd import _lib
    vol, thr = _far_corner_volume(), 0.0
    assert int(_lib.lib().mnrf_mc_blocks(*vol.shape)) == 66308 > 65535
    # the reach: the lowest flat index of a point that owns a crossed edge or an active cell
    ins = vol >= thr
    owner = np.zeros(vol.shape, dtype=bool)
    owner[:-1] |= ins[1:] != ins[:-1]
    owner[:, :-1] |= ins[:, 1:] != ins[:, :-1]
    owner[:, :, :-1] |= ins[:, :, 1:] != ins[:, :, :-1]
    cases = MR.cell_cases(vol, thr)
    owner[:-1, :-1, :-1] |= (cases != 0) & (cases != 255)
    lowest = int(np.flatnonzero(owner.reshape(-1))[0])
    assert lowest >= 65536 * MC_BLOCK and owner.sum() > 900
    v, t = _mc(vol, thr)
    rv, rt = MR.marching_cubes_cropped(vol, thr, table)
    assert v.shape[0] == rv.shape[0] == MR.crossed_edges(vol, thr) and t.shape[0] == rt.shape[0] > 1000
    vn, tn = v.cpu().numpy(), t.cpu().numpy()
    gv, gt = MR.canonical(vn, tn)
    wv, wt = MR.canonical(rv, rt)
    ulp = np.spacing(np.float32(256.0))
    assert float(np.abs(gv.astype(np.float64) - wv).max()) <= 2 * ulp and np.array_equal(gt, wt)
    assert MR.is_closed_oriented(tn) and MR.euler_characteristic(len(vn), tn) == 2 and MR.signed_volume(vn, tn) > 0
    assert vn[:, 0].min() > 254 and tn.min() == 0 and tn.max() == len(vn) - 1
    v2, t2 = _mc(vol, thr)
    assert torch.equal(v, v2) and torch.equal(t, t2)
    bc = _mc_block_counts(vol, thr)
    assert not bc[:65536].any() and bc[65536:, 0].sum() == len(vn) and bc[65536:, 1].sum() == len(tn)


@pytest.mark.parametrize("shape", [(2, 2, 70001), (70001, 2, 2)])
def test_marching_cubes_long_strides(shape, table):
    """One long axis: along z the row stride nz and the plane stride ny * nz are 70 001 and 140 002 points, far beyond a
    block and beyond 65 535; along x the volume is 70 001 planes of four points, 64 planes a block."""
    vol, thr = _profile_volume(shape, seed=sum(shape)), 0.0
    if shape[2] > 2:
        assert shape[2] > 65535 and shape[1] * shape[2] > 65535
    else:
        assert shape[0] > 65535 and shape[1] * shape[2] == 4
    ins = vol >= thr
    kinds = [(ins[1:] != ins[:-1]).sum(), (ins[:, 1:] != ins[:, :-1]).sum(), (ins[:, :, 1:] != ins[:, :, :-1]).sum()]
    assert min(kinds) > 500, kinds
    v, t = _compare_with_restatement(vol, thr, table)
    assert t.shape[0] > 2000
    assert np.array_equal(_mc_block_counts(vol, thr), MR.block_counts(vol, thr, table, MC_BLOCK))


def test_marching_cubes_non_finite_densities(table):
    """A handful of NaN (outside, as under >=) and +inf (inside) values next to the surface.  Positions next to them may be
    NaN, so the topology is compared: the vertex count, every index in range, and the triangle array under the vertex
    numbering the kernels document (crossed edges in the flat order of their lower end, +x, +y, +z within a point)."""
    vol, thr = _smooth_random().copy(), 0.1
    rs = np.random.RandomState(8)
    ins = vol >= thr
    edge = np.zeros(vol.shape, dtype=bool)       # interior points with a neighbour on the other side
    edge[1:-1, 1:-1, 1:-1] = ((ins[1:-1, 1:-1, 1:-1] != ins[2:, 1:-1, 1:-1]) | (ins[1:-1, 1:-1, 1:-1] != ins[1:-1, 2:, 1:-1])
                              | (ins[1:-1, 1:-1, 1:-1] != ins[1:-1, 1:-1, 2:]))
    inside, outside = np.argwhere(edge & ins), np.argwhere(edge & ~ins)
    for p in inside[rs.choice(len(inside), 4, replace=False)]:
        vol[tuple(p)] = np.nan
    for p in outside[rs.choice(len(outside), 4, replace=False)]:
        vol[tuple(p)] = np.inf
    assert np.isnan(vol).sum() == 4 and np.isposinf(vol).sum() == 4
    v, t = _mc(vol, thr)
    V = v.shape[0]
    vn, tn = v.cpu().numpy(), t.cpu().numpy()
    assert V == MR.crossed_edges(vol, thr) != MR.crossed_edges(_smooth_random(), thr)
    assert tn.min() >= 0 and tn.max() < V and len(np.unique(tn)) == V
    rv, rt, edges = MR.marching_cubes(vol, thr, table, return_edges=True)
    rank = MR.flat_edge_rank(edges, vol.shape)
    assert len(rv) == V and len(rt) == len(tn)
    assert np.array_equal(MR.canonical_triangles(tn), MR.canonical_triangles(rank[rt]))
    # the positions: NaN at the same vertices (there are some), elsewhere the usual 2 ulp
    want = np.empty_like(rv)
    want[rank] = rv
    assert np.isnan(want).any() and np.array_equal(np.isnan(vn), np.isnan(want))
    ok = ~np.isnan(want)
    assert float(np.abs(vn[ok].astype(np.float64) - want[ok]).max()) <= 2 * np.spacing(np.float32(max(vol.shape) - 1))
    v2, t2 = _mc(vol, thr)
    assert v.cpu().numpy().tobytes() == v2.cpu().numpy().tobytes() and torch.equal(t, t2)


# ----------------------------------------------------------------------------------------------- 9. components at their edges
def _mean_edge_span(t):
    t = np.asarray(t, dtype=np.int64)
    return float(np.abs(t - np.roll(t, 1, 1)).mean())


@pytest.mark.parametrize("name", ["torus", "two_spheres", "smooth_random", "g20"])
def test_components_of_renumbered_meshes(name, g20):
    """The hook rounds have only seen marching cubes' flat order, where neighbours have neighbouring numbers.  Here the same
    meshes under a seeded random renumbering of the vertices, a shuffled triangle array and rotated corners."""
    from mirror_nerf_amd import mesh
    if name == "g20":
        vol, thr = np.maximum(g20.outputs["sigma"], 0), g20.meta["threshold"]
    else:
        make, thr = VOLUMES[name]
        vol = make()
    v, t = _mc(vol, thr)
    vn, tn = v.cpu().numpy(), t.cpu().numpy()
    V = len(vn)
    perm, rt = MR.renumber(V, tn, seed=len(name))
    nv = np.empty_like(vn)
    nv[perm] = vn
    assert _mean_edge_span(rt) > V / 5 > 4 * _mean_edge_span(tn)      # neighbours are far apart now
    dt, dv = torch.from_numpy(rt).to(DEV), torch.from_numpy(nv).to(DEV)
    want = MR.union_find_labels(V, rt)
    labels = mesh.component_labels(V, dt).cpu().numpy()
    assert np.array_equal(labels, want)
    assert len(np.unique(want)) == len(np.unique(MR.union_find_labels(V, tn)))
    lv, lt, info = mesh.largest_component(dv, dt, return_info=True)
    wv, wt, n_comp, largest = MR.largest_component(nv, rt)
    assert info == {"n_components": n_comp, "largest_triangles": largest}
    assert np.array_equal(lt.cpu().numpy(), wt) and np.array_equal(lv.cpu().numpy(), wv)


STRIP = 1000000


@pytest.mark.parametrize("numbering", ["ascending", "descending", "shuffled"])
def test_components_of_a_long_strip(numbering):
    """One strip of 1 000 000 triangles (V = 1 000 002 > 65 535): a chain as long as the mesh, under three numberings; the
    one component carries label 0.  Every round costs a host synchronisation.  Measured on an MI355X for component_labels:
    ascending 0.017 s (the first launch of the process), descending 0.002 s, shuffled 0.005 s; a tenth of the length took
    0.005 / 0.001 / 0.001 s, so the strip is a million long and not the 70 000 that would do."""
    import time
    from mirror_nerf_amd import mesh
    strip = MR.triangle_strip(STRIP)
    V = STRIP + 2
    assert V > 65535
    tri = {"ascending": strip, "descending": (V - 1 - strip).astype(np.int32), "shuffled": MR.renumber(V, strip, 3)[1]}[numbering]
    dt = torch.from_numpy(np.ascontiguousarray(tri)).to(DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    labels = mesh.component_labels(V, dt)
    torch.cuda.synchronize()
    print(f"component_labels, strip of {STRIP} triangles, {numbering}: {time.perf_counter() - t0:.3f} s")
    assert labels.shape == (V,) and not bool(labels.any())
    v = torch.arange(V, dtype=torch.float32, device=DEV)[:, None].repeat(1, 3).contiguous()
    lv, lt, info = mesh.largest_component(v, dt, return_info=True)
    assert info == {"n_components": 1, "largest_triangles": STRIP} and torch.equal(lv, v) and torch.equal(lt, dt)


def test_components_of_two_interleaved_strips():
    """Two strips of 35 001 triangles over the even and the odd vertices (V = 70 006): two labels, 0 and 1, and between the
    two equal components the documented tie rule: the lowest label wins."""
    from mirror_nerf_amd import mesh
    T = 35001
    V = 2 * (T + 2)
    rs = np.random.RandomState(4)
    tri = np.concatenate([MR.triangle_strip(T, 0, 2), MR.triangle_strip(T, 1, 2)])[rs.permutation(2 * T)]
    assert V > 65535 and tri.max() == V - 1
    dt = torch.from_numpy(np.ascontiguousarray(tri)).to(DEV)
    labels = mesh.component_labels(V, dt).cpu().numpy()
    assert np.array_equal(labels, np.arange(V) % 2) and np.array_equal(labels, MR.union_find_labels(V, tri))
    v = torch.arange(V, dtype=torch.float32, device=DEV)[:, None].repeat(1, 3).contiguous()
    lv, lt, info = mesh.largest_component(v, dt, return_info=True)
    wv, wt, n_comp, largest = MR.largest_component(v.cpu().numpy(), tri)
    assert info == {"n_components": 2, "largest_triangles": T} == {"n_components": n_comp, "largest_triangles": largest}
    assert np.array_equal(lv.cpu().numpy()[:, 0], np.arange(0, V, 2)) and np.array_equal(lt.cpu().numpy(), wt)


def test_component_kernels_refuse_indices_out_of_range():
    """mnrf_cc_step and mnrf_cc_count on a triangle array in which rows hold -1, V, V + 5, 2^31 - 1 and -2^31 in every
    column, at the start, across a block edge and at the end: those rows are skipped by both kernels, the other rows give
    the labels and counts of the restatement on the valid rows alone, and nothing is written outside labels[0, V) and
    counts[0, V).  The rows whose first index is good and whose second or third is not are what caught cc_count_kernel
    looking at the first index only: it counted triangles the hook kernel had refused (167 for 165 under label 0)."""
    from mirror_nerf_amd import _lib
    L = _lib.lib()
    rs = np.random.RandomState(6)
    V, T = 300, 700
    # four groups of vertices that never mix, so that there are several components
    group = rs.randint(0, 4, T)
    tri = (group[:, None] * 75 + rs.randint(0, 75, (T, 3))).astype(np.int64)
    bad_values = [-1, V, V + 5, 2 ** 31 - 1, -2 ** 31]
    bad_rows = [0, 1, 2, 254, 255, 256, 257, 258, 400, 401, 402, 403, T - 3, T - 2, T - 1]
    for k, r in enumerate(bad_rows):
        tri[r, k % 3] = bad_values[k % 5]
    tri = tri.astype(np.int32)
    valid = ((tri >= 0) & (tri < V)).all(1)
    assert (~valid).sum() == len(bad_rows) and all(((tri[~valid] == b).any()) for b in bad_values)
    assert all((~((tri[~valid][:, c] >= 0) & (tri[~valid][:, c] < V))).any() for c in range(3))      # every column holds a bad index
    assert (((tri[~valid][:, 0] >= 0) & (tri[~valid][:, 0] < V))).any()      # and some bad rows start with a good one
    want = MR.union_find_labels(V, tri[valid])
    want_counts = np.bincount(want[tri[valid][:, 0]], minlength=V)
    dt = torch.from_numpy(tri).to(DEV)
    labels = torch.full((GUARD + V + GUARD,), -99, dtype=torch.int32, device=DEV)
    counts = torch.full((GUARD + V + GUARD,), -99, dtype=torch.int32, device=DEV)
    counts[GUARD:GUARD + V] = 0
    changed = torch.zeros(1, dtype=torch.int32, device=DEV)
    with torch.cuda.device(DEV):
        lab, cnt = labels[GUARD:GUARD + V], counts[GUARD:GUARD + V]
        _lib.check(L.mnrf_cc_init(_lib.ptr(lab), V, _lib.stream()), "mnrf_cc_init")
        for _ in range(V + 2):
            changed.zero_()
            _lib.check(L.mnrf_cc_step(_lib.ptr(dt), T, _lib.ptr(lab), V, _lib.ptr(changed), _lib.stream()), "mnrf_cc_step")
            if int(changed.item()) == 0:
                break
        else:
            raise AssertionError("no fixed point")
        _lib.check(L.mnrf_cc_count(_lib.ptr(dt), T, _lib.ptr(lab), V, _lib.ptr(cnt), _lib.stream()), "mnrf_cc_count")
    got, got_counts = labels.cpu().numpy(), counts.cpu().numpy()
    assert (got[:GUARD] == -99).all() and (got[GUARD + V:] == -99).all()
    assert (got_counts[:GUARD] == -99).all() and (got_counts[GUARD + V:] == -99).all()
    assert np.array_equal(got[GUARD:GUARD + V], want) and len(np.unique(want[tri[valid].reshape(-1)])) == 4
    assert np.array_equal(got_counts[GUARD:GUARD + V], want_counts) and want_counts.sum() == valid.sum()


# ----------------------------------------------------------------------------------------------- 10. colour projection at its edges
@pytest.mark.parametrize("H,W,V", [(1, 53, 257), (37, 1, 257), (1, 1, 257), (37, 53, 65537)])
def test_projection_on_one_pixel_axes_and_the_last_pixel(H, W, V):
    """Images of one row, one column and one pixel; 257 and 65 537 vertices (one past a block, one past 65 536); vertex 0
    reaches the last column and the last row by a few float32 steps and is clamped onto them (x1 = W, y1 = H are clamped
    too), vertex 1 lies far outside the same corner, vertex 2 stops a few steps short of it.  The bars are those of
    test_projection_and_sampling_match_float64."""
    from mirror_nerf_amd import mesh
    rs = np.random.RandomState(H * 1000 + W)
    focal, near, z = 41.3, 0.05, -2.0
    pose = np.concatenate([np.eye(3), np.zeros((3, 1))], 1).astype(np.float32)
    f32 = float(np.float32(focal))
    depth = -z + 1e-5
    edge_x = ((W - 1) * depth + 0.5 * W * z) / f32             # projects onto column W - 1
    edge_y = -((H - 1) * depth + 0.5 * H * z) / f32            # projects onto row H - 1
    span = 1.4 * max(abs(edge_x), abs(edge_y), 0.1)
    verts = np.stack([rs.uniform(-span, span, V), rs.uniform(-span, span, V), rs.uniform(-3.0, -1.0, V)], 1).astype(np.float32)

    up = lambda x: np.nextafter(np.float32(x), np.float32(np.inf))      # noqa: E731
    down = lambda x: np.nextafter(np.float32(x), np.float32(-np.inf))   # noqa: E731
    xa, xb, ya, yb = np.float32(edge_x), np.float32(edge_x), np.float32(edge_y), np.float32(edge_y)
    for _ in range(8):      # column grows with x, row grows as y falls
        xa, xb, ya, yb = up(xa), down(xb), down(ya), up(yb)
    verts[0] = [xa, ya, z]
    verts[1] = [edge_x + 50.0, edge_y - 50.0, z]
    verts[2] = [xb, yb, z]
    image = rs.randint(0, 256, (H, W, 3)).astype(np.uint8)
    wc, wd, pix, wr = MR.project_view(verts, image, pose, focal, near)
    assert pix[0].tolist() == [W - 1, H - 1] and pix[1].tolist() == [W - 1, H - 1]
    if W > 1:
        assert W - 1 - 1e-3 < pix[2, 0] < W - 1
    if H > 1:
        assert H - 1 - 1e-3 < pix[2, 1] < H - 1
    assert (pix[:, 0] == 0).sum() > V // 20 and (pix[:, 1] == 0).sum() > V // 20      # clipped on the other side too
    colors, depth_, rays = mesh.project_view(torch.from_numpy(verts).to(DEV), torch.from_numpy(image).to(DEV), pose, focal, near)
    assert colors.shape == (V, 3) and depth_.shape == (V,) and rays.shape == (V, 8)
    got = colors.cpu().numpy()
    assert (np.abs(got - wc) <= 1e-5 * np.maximum(1.0, np.abs(wc))).all()
    assert np.array_equal(got[:2], np.tile(image[H - 1, W - 1].astype(np.float32), (2, 1)))
    if H == 1 and W == 1:
        assert np.array_equal(got, np.tile(image[0, 0].astype(np.float32), (V, 1)))
    np.testing.assert_allclose(depth_.cpu().numpy(), wd, rtol=1e-12, atol=1e-12)
    r = rays.cpu().numpy()
    np.testing.assert_allclose(r[:, :7], wr[:, :7], rtol=0, atol=2e-6)
    np.testing.assert_allclose(r[:, 7], wd, rtol=1e-7)
