"""GPU tests of mesh extraction (mirror_nerf_amd/mesh.py over csrc/mnrf_mesh.hip): grid points bit-equal to numpy's
construction, the density grid against the reference's volume (fixture G20, tests/golden/make_golden_mesh.py), marching
cubes against the cell-loop restatement of tests/mesh_ref.py, manifold properties of closed surfaces, the largest
component against a numpy union-find, the colour fusion against a float64 restatement and the reference's opacities,
and the whole chain down to a PLY file.

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
