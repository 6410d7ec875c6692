"""GPU tests of the colouring along the vertex normals (mirror_nerf_amd/mesh.py: vertex_normals, normal_rays,
normal_vertex_colors, rgb_to_uint8 over csrc/mnrf_mesh.hip; extract_color_mesh.py --use_vertex_normal).

Bars.  Vertex normals: every component within 2e-7 of the float64 restatement of tests/mesh_normals_ref.py -- one float32
rounding at 1 (6e-8; the restatement and the kernel may round a value next to a tie differently) plus the kernel's
fixed-point step, which is below 2^-38 of the mesh's largest cross product; bit-identical between runs and under any order
of the triangle array.  Rays: bit-equal to the reference's torch expression on the CPU.  Colours against the reference
(fixture G21): the reference itself is not stable on these rays (bin flips of sample_pdf between its float32 and float64
runs), so error DISTRIBUTIONS are compared against its float64 run over all 4096 rays: 95th percentile <= 1e-4 (the
project's bar for rgb), share above 1e-4 <= 2 x the reference's own share + 4 / 4096, and on the rays where the
reference's two runs agree to 1e-5 the share of rays more than 1e-4 from its float32 run <= the same cap.
Measured on an MI355X (V = 4096; the reference's own share is 14 rays, the cap 32), against the float64 run:
    split: median 4.65e-7, 95th percentile 3.58e-6, 10 rays above 1e-4 (max 2.97e-3), 0 of the 4009 agreeing rays off;
    fp32:  median 2.57e-7, 95th percentile 3.19e-6,  9 rays above 1e-4 (max 2.86e-3), 0 of the 4009 agreeing rays off."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mesh_normals_ref as NR
from tests.golden import fixtures as FX

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 2e-7


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
def g21():
    return FX.Fixture("g21_mesh_normal_colors")


def _models(fx):
    import mirror_nerf_amd as M
    out = {}
    for name, sd in zip(("coarse", "fine"), fx.state_dicts()):
        m = M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=True)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        out[name] = m.to(DEV)
    return out


def _emb():
    import mirror_nerf_amd as M
    return {"xyz": M.Embedding(10), "dir": M.Embedding(4)}


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


# ----------------------------------------------------------------------------------------------- volumes (as tests/test_hip_mesh.py)
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


def _smooth_random(shape=(22, 23, 24), seed=1):
    rs = np.random.RandomState(seed)
    X, Y, Z = _axes(shape)
    f = np.zeros(shape)
    for _ in range(6):
        k = rs.uniform(3, 9, 3)
        f += rs.uniform(0.5, 1) * np.sin(k[0] * X + k[1] * Y + k[2] * Z + rs.uniform(0, 6.28))
    f = f.astype(np.float32)
    f[0], f[-1], f[:, 0], f[:, -1], f[:, :, 0], f[:, :, -1] = (-3.0,) * 6
    return f


VOLUMES = {"sphere": (_sphere, 0.0), "torus": (_torus, 0.0), "two_spheres": (_two_spheres, 0.0), "smooth_random": (_smooth_random, 0.1)}


def _mesh_of(name, g20):
    """(vertices, triangles) on the device: marching cubes of a synthetic volume in index coordinates, or G20's mesh
    (largest component, world coordinates)."""
    from mirror_nerf_amd import mesh
    if name == "g20":
        m = g20.meta
        v, t = mesh.marching_cubes(_dev(np.maximum(g20.outputs["sigma"], 0), np.float32), m["threshold"])
        v, t = mesh.largest_component(v, t)
        return mesh.index_to_world(v, m["x_range"], m["y_range"], m["z_range"], m["N"]), t
    make, thr = VOLUMES[name]
    return mesh.marching_cubes(_dev(make(), np.float32), thr)


# ----------------------------------------------------------------------------------------------- 1. vertex normals
@pytest.mark.parametrize("name", sorted(VOLUMES) + ["g20"])
def test_vertex_normals_match_restatement(name, g20):
    from mirror_nerf_amd import mesh
    v, t = _mesh_of(name, g20)
    n = mesh.vertex_normals(v, t)
    assert n.is_cuda and n.dtype == torch.float32 and n.shape == v.shape
    want = NR.vertex_normals(v.cpu().numpy(), t.cpu().numpy(), dtype=np.float64)
    got = n.cpu().numpy().astype(np.float64)
    err = float(np.abs(got - want).max())
    unit = float(np.abs(np.linalg.norm(got, axis=1) - 1).max())
    print(f"[{name}] V = {len(got)}, T = {t.shape[0]}: max |n - n_ref| = {err:.3e} (bar {BAR:.0e}), max | |n| - 1 | = {unit:.1e}")
    assert err <= BAR and unit <= 2e-7
    # two runs agree to the bit, and so does any order of the triangle array
    assert torch.equal(n, mesh.vertex_normals(v, t))
    rs = np.random.RandomState(5)
    perm = torch.from_numpy(rs.permutation(t.shape[0])).to(DEV)
    assert torch.equal(n, mesh.vertex_normals(v, t[perm].contiguous()))
    # rotating a triangle's indices moves the corner the two edges start from: other roundings, the same bar
    rot = mesh.vertex_normals(v, torch.roll(t, 1, 1).contiguous()).cpu().numpy().astype(np.float64)
    assert float(np.abs(rot - want).max()) <= BAR
    # the reversed winding (a, c, b) gives the opposite normals, to the bit
    flipped = mesh.vertex_normals(v, t[:, [0, 2, 1]].contiguous())
    summed = ~((n == torch.tensor([0.0, 0.0, 1.0], device=DEV)).all(1) & (flipped == n).all(1))      # (not the (0, 0, 1) default)
    assert bool(summed.any()) and torch.equal(-n[summed], flipped[summed])


def test_vertex_normals_hand_made_and_degenerate():
    from mirror_nerf_amd import mesh
    tv = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], dtype=np.float32)
    tt = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], dtype=np.int32)
    n = mesh.vertex_normals(_dev(tv, np.float32), _dev(tt, np.int32)).cpu().numpy()
    assert np.abs(n - tv / np.sqrt(3.0)).max() <= BAR
    # a single triangle; an isolated vertex; a zero-area triangle; a vertex that has only the degenerate one
    v = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [5, 5, 5], [0, 1, 0]], dtype=np.float32)
    for tris in ([[0, 4, 1]], [[0, 1, 2]], [[0, 1, 2], [0, 4, 1]], [[0, 1, 4], [1, 1, 4], [3, 3, 3]]):
        got = mesh.vertex_normals(_dev(v, np.float32), _dev(np.array(tris), np.int32)).cpu().numpy()
        assert np.array_equal(got, NR.vertex_normals(v, tris)), tris
    assert np.array_equal(mesh.vertex_normals(_dev(v, np.float32), _dev(np.array([[0, 1, 2]]), np.int32)).cpu().numpy(),
                          np.tile(np.float32([0, 0, 1]), (5, 1)))
    # no triangle at all, no vertex at all, and triangles that index outside the vertices (skipped, never dereferenced)
    none = torch.zeros(0, 3, dtype=torch.int32, device=DEV)
    assert np.array_equal(mesh.vertex_normals(_dev(v, np.float32), none).cpu().numpy(), np.tile(np.float32([0, 0, 1]), (5, 1)))
    assert mesh.vertex_normals(torch.zeros(0, 3, device=DEV), none).shape == (0, 3)
    got = mesh.vertex_normals(_dev(v, np.float32), _dev(np.array([[0, 1, 4], [0, 1, 7], [-1, 0, 1]]), np.int32)).cpu().numpy()
    assert np.array_equal(got, NR.vertex_normals(v, [[0, 1, 4]]))
    # a non-finite vertex: its triangles' vertices get (0, 0, 1), as under the restatement; the others are untouched
    w = v.copy()
    w[3] = [np.nan, 0, np.inf]
    tris = [[0, 1, 4], [1, 3, 4], [0, 4, 2]]
    got = mesh.vertex_normals(_dev(w, np.float32), _dev(np.array(tris), np.int32)).cpu().numpy()
    assert np.array_equal(got, NR.vertex_normals(w, tris)) and np.array_equal(got[0], np.float32([0, 0, -1]))
    # scales far from 1: tiny and huge triangles keep their precision (the fixed-point step follows the mesh)
    rs = np.random.RandomState(9)
    p = rs.normal(size=(300, 3))
    t = rs.randint(0, 300, (900, 3)).astype(np.int32)
    for scale in (1e-12, 1.0, 1e12):
        vv = (p * scale).astype(np.float32)
        got = mesh.vertex_normals(_dev(vv, np.float32), _dev(t, np.int32)).cpu().numpy()
        assert np.abs(got.astype(np.float64) - NR.vertex_normals(vv, t, dtype=np.float64)).max() <= BAR, scale


# ----------------------------------------------------------------------------------------------- 1b. past one sweep of the maximum
SWEEP = 1024 * 256      # triangles per pass of vn_max_kernel's grid-stride loop


@pytest.fixture(scope="module")
def field():
    """The 400 x 400 height field (318 402 triangles), flat around its last corner: built once, copied by the tests."""
    v, t = NR.height_field_mesh(400)
    corner = len(v) - 1
    v[[corner, corner - 1, corner - 400, corner - 401], 2] = 0.0
    return v, t


def _normals(v, t):
    from mirror_nerf_amd import mesh
    return mesh.vertex_normals(_dev(v, np.float32), _dev(t, np.int32))


def _count_bits(T):
    return int(3 * T).bit_length()      # 3 T < 2^count_bits, as mnrf_vertex_normals counts them


def test_vertex_normals_maximum_in_the_second_sweep(field):
    """The corner vertex of the last but one triangle (index 318 400 >= 262 144) is pulled out by 0.9 * 2^20 grid steps: that
    triangle's cross product is 0.9 * 2^20 times the largest of all the others, and only the second pass of vn_max_kernel's
    loop sees it.  With M < 2^20 and 3 T < 2^20 the fixed-point step is 2^-22, so a vertex with m triangles is at most
    m * 2^-23 off on a sum of length >= m: 1.2e-7 and one float32 rounding, inside BAR at every vertex.
    A maximum lost in the later pass would make the step 2^20 times finer; at this ratio the sums still fit 64 bits, so the
    same mesh is run again with the corner 2^23 steps out, where a step taken from the first pass alone saturates the
    conversion of that triangle: its three vertices are then checked (the others are 2^-18 coarse there, by design).
    Measured on an MI355X: max |n - n_ref| 1.19e-7 over the 160 000 vertices."""
    v, t = field[0].copy(), field[1]
    T, corner = len(t), len(v) - 1
    v[corner, 0] += np.float32(0.9 * 2 ** 20)
    big = np.abs(NR.cross_products(v, t)).max(1)
    k = int(np.argmax(big))
    ratio = big[k] / np.delete(big, k).max()
    assert k == T - 2 >= SWEEP and 0.85 * 2 ** 20 < ratio < 2 ** 20 and _count_bits(T) == 20 and big[k] < 2 ** 20
    n = _normals(v, t)
    want = NR.vertex_normals(v, t, dtype=np.float64)
    err = float(np.abs(n.cpu().numpy().astype(np.float64) - want).max())
    print(f"[second sweep] V = {len(v)}, T = {T}: max |n - n_ref| = {err:.3e} (bar {BAR:.0e})")
    assert err <= BAR
    # any order of the triangle array gives the same bits ...
    rs = np.random.RandomState(5)
    assert torch.equal(n, _normals(v, t[rs.permutation(T)]))
    # ... also the one with the large triangle at index 0, in the first sweep: the later sweep was seen, not luck
    first = np.concatenate([t[k:k + 1], t[:k], t[k + 1:]])
    assert int(np.argmax(np.abs(NR.cross_products(v, first)).max(1))) == 0
    assert torch.equal(n, _normals(v, first))
    # the corner 2^23 steps out: the large triangle's vertices
    v[corner, 0] = np.float32(399 + 2 ** 23)
    big = np.abs(NR.cross_products(v, t)).max(1)
    assert int(np.argmax(big)) == k and big[k] / np.delete(big, k).max() > 2 ** 23 > 2 ** (_count_bits(T) + 2)
    far = _normals(v, t)
    want = NR.vertex_normals(v, t, dtype=np.float64)
    assert float(np.abs(far.cpu().numpy().astype(np.float64) - want)[t[k]].max()) <= BAR and want[t[k], 2].min() > 0.999999
    assert torch.equal(far, _normals(v, first))


def test_vertex_normals_fan_on_one_vertex():
    """100 000 congruent triangles around one hub: every one of them adds a cross product close to the mesh's largest to the
    hub's three accumulators -- the largest sum the bound |sum| < 2^62 has to hold (here 2^58.7), all of it on one address.
    Measured on an MI355X: the hub is (0, 0, 1) exactly, the rim within 1.9e-8."""
    T = 100000
    v, t = NR.fan_mesh(T)
    c = NR.cross_products(v, t)
    big = np.abs(c).max(1)
    assert np.bincount(t.reshape(-1))[0] == T and big.min() > 0.99 * big.max() and (c[:, 2] == big).all()
    _, e = np.frexp(big.max())
    steps = c[:, 2].sum() * 2.0 ** (62 - int(e) - _count_bits(T))      # the hub's z accumulator, in fixed-point steps
    assert 2.0 ** 58 < steps < 2.0 ** 62
    n = _normals(v, t)
    want = NR.vertex_normals(v, t, dtype=np.float64)
    got = n.cpu().numpy().astype(np.float64)
    err_hub, err_rim = float(np.abs(got[0] - want[0]).max()), float(np.abs(got[1:] - want[1:]).max())
    print(f"[fan] T = {T}: hub {got[0].tolist()}, |n - n_ref| hub {err_hub:.3e}, rim {err_rim:.3e} (bar {BAR:.0e})")
    assert err_hub <= BAR and err_rim <= BAR and got[0, 2] > 0.999999
    rs = np.random.RandomState(6)
    assert torch.equal(n, _normals(v, t[rs.permutation(T)]))


def test_vertex_normals_non_finite_corner_in_the_second_sweep(field):
    """One more triangle at index 318 402 (second sweep) with a vertex at infinity: its three vertices get (0, 0, 1), every
    other vertex is what the mesh without that triangle gives."""
    v, t = field
    V, T = len(v), len(t)
    a = 200 * 400 + 200
    v2 = np.concatenate([v, np.float32([[np.inf, 0.0, 0.0]])])
    t2 = np.concatenate([t, np.int32([[a, a + 1, V]])])
    assert len(t2) - 1 >= SWEEP and not np.isfinite(NR.cross_products(v2, t2)[-1]).all()
    got = _normals(v2, t2).cpu().numpy()
    assert np.array_equal(got[[a, a + 1, V]], np.tile(np.float32([0, 0, 1]), (3, 1)))
    without = NR.vertex_normals(v2, t, dtype=np.float64)
    others = np.ones(V + 1, dtype=bool)
    others[[a, a + 1, V]] = False
    assert float(np.abs(got.astype(np.float64) - without)[others].max()) <= BAR
    assert np.abs(without[[a, a + 1]] - [0, 0, 1]).max() > 1e-3      # they had normals of their own
    assert np.array_equal(NR.vertex_normals(v2, t2)[[a, a + 1, V]], np.tile(np.float32([0, 0, 1]), (3, 1)))      # as the restatement


# ----------------------------------------------------------------------------------------------- 2. direction
@pytest.mark.parametrize("exact_spacing", [False, True])
@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_normals_point_towards_higher_density(name, exact_spacing):
    """extract_mesh's own steps (marching cubes, largest component, index_to_world) on an analytic volume: the volume is
    sampled on the grid that index_to_world(exact_spacing=True) maps back onto; exact_spacing=False shrinks the mesh by
    (N - 1) / N around the box minimum, so the gradient is taken at the vertex scaled back."""
    from mirror_nerf_amd import mesh
    N, rng = 32, (-1.2, 1.2)
    x = np.linspace(rng[0], rng[1], N)
    X, Y, Z = np.meshgrid(x, x, x)      # "xy" order, as density_grid: volume[a, b, c] is the density at (x[b], y[a], z[c])
    c = np.array([0.05, -0.1, 0.02])
    if name == "sphere":
        vol = 0.6 - np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2)
    else:
        vol = 0.25 - np.sqrt((np.sqrt(X ** 2 + Y ** 2) - 0.65) ** 2 + Z ** 2)
    v, t = mesh.marching_cubes(_dev(vol, np.float32), 0.0)
    v, t = mesh.largest_component(v, t)
    world = mesh.index_to_world(v, rng, rng, rng, N, exact_spacing=exact_spacing)
    n = mesh.vertex_normals(world, t).cpu().numpy().astype(np.float64)
    p = world.cpu().numpy().astype(np.float64)
    if not exact_spacing:
        p = (p - rng[0]) * (N / (N - 1.0)) + rng[0]
    if name == "sphere":
        assert np.abs(np.linalg.norm(p - c, axis=1) - 0.6).max() < 0.02      # the vertices are where the surface is
        grad = -(p - c) / np.linalg.norm(p - c, axis=1, keepdims=True)
    else:
        rho = np.sqrt(p[:, 0] ** 2 + p[:, 1] ** 2)
        q = np.sqrt((rho - 0.65) ** 2 + p[:, 2] ** 2)
        assert np.abs(q - 0.25).max() < 0.02
        grad = -np.stack([(rho - 0.65) / q * p[:, 0] / rho, (rho - 0.65) / q * p[:, 1] / rho, p[:, 2] / q], 1)
    dots = (n * grad).sum(1)
    print(f"[{name}, exact_spacing={exact_spacing}] V = {len(p)}: min n . grad(sigma) = {dots.min():.3f}")
    assert (dots > 0).all()


# ----------------------------------------------------------------------------------------------- 3. rays
@pytest.mark.parametrize("near,far,near_t", [(0.05, 8.0, 1.0), (0.05, 8.0, 0.37), (2.0 / 3.0, 6.1, 1.7)])
def test_normal_rays_bit_equal_torch(g21, near, far, near_t):
    from mirror_nerf_amd import mesh
    v, n = g21.inputs["vertices"], g21.inputs["normals"]
    got = mesh.normal_rays(_dev(v, np.float32), _dev(n, np.float32), near, far, near_t).cpu().numpy()
    want = NR.normal_rays_torch(v, n, near, far, near_t)
    assert got.dtype == np.float32 and got.shape == (len(v), 8) and got.tobytes() == want.tobytes()
    if (near, far, near_t) == (g21.meta["near"], g21.meta["far"], g21.meta["near_t"]):
        assert got.tobytes() == g21.inputs["rays"].tobytes()


# ----------------------------------------------------------------------------------------------- 4. colours
def test_rgb_to_uint8_truncates():
    from mirror_nerf_amd import mesh
    k = np.arange(1, 256, dtype=np.float64)
    below = np.nextafter((k / 255.0).astype(np.float32), np.float32(0))
    rs = np.random.RandomState(3)
    x = np.concatenate([np.float32([0.0, 1.0, 0.5, 1e-30, -0.0]), (k / 255.0).astype(np.float32), below, np.nextafter(below, np.float32(0)),
                        rs.uniform(0, 1, 5000).astype(np.float32)])
    x = x[:len(x) // 3 * 3].reshape(-1, 3)
    got = mesh.rgb_to_uint8(_dev(x, np.float32))
    assert got.dtype == torch.uint8 and got.shape == x.shape
    want = np.trunc(x * np.float32(255.0)).astype(np.int64)
    assert want.min() == 0 and want.max() == 255
    assert np.array_equal(got.cpu().numpy().astype(np.int64), want) and np.array_equal(got.cpu().numpy(), NR.rgb_to_uint8(x))
    assert mesh.rgb_to_uint8(_dev([1.0, 0.0], np.float32)).cpu().tolist() == [255, 0]
    # outside [0, 1]: saturated; a NaN is 0
    odd = mesh.rgb_to_uint8(_dev([1.01, 300.0, -0.2, np.nan, np.inf, -np.inf], np.float32)).cpu().tolist()
    assert odd == [255, 255, 0, 0, 255, 0]


def _plain_rgb(models, rays, m, chunk, **kw):
    """The reference's f(...) (extract_color_mesh.py:90-115, under torch.no_grad()) with this project's plain render_rays."""
    import mirror_nerf_amd as M
    with torch.no_grad():
        return torch.cat([M.render_rays(models, _emb(), rays[i:i + chunk], m["N_samples"], False, 0, 0, m["N_importance"], chunk,
                                        False, test_time=True, **kw)["rgb_fine"] for i in range(0, rays.shape[0], chunk)], 0)


def test_colors_match_reference(g21, precision):
    """Parity with the reference's render under the distribution rule of the module docstring; all 4096 rays."""
    from mirror_nerf_amd import mesh
    m = g21.meta
    models = _models(g21)
    v, n = _dev(g21.inputs["vertices"], np.float32), _dev(g21.inputs["normals"], np.float32)
    none = torch.zeros(0, 3, dtype=torch.int32, device=DEV)      # (the normals are the fixture's: no triangle is read)
    colors, rgb = mesh.normal_vertex_colors(v, none, models, _emb(), m["near"], m["far"], m["near_t"], m["N_samples"],
                                            m["N_importance"], False, 1000, normals=n, return_rgb=True)
    assert colors.dtype == torch.uint8 and colors.shape == (len(v), 3) and rgb.dtype == torch.float32 and rgb.shape == (len(v), 3)
    got = rgb.cpu().numpy()
    ref32 = g21.outputs["rgb_fine"].astype(np.float64)
    ref64 = ref32 + g21.outputs["rgb_fine_fp64_minus_fp32"].astype(np.float64)
    _, _, ref_share, d_ref = NR.ray_error_stats(ref32, ref64)
    med, p95, share, d = NR.ray_error_stats(got, ref64)
    agree = d_ref <= 1e-5
    _, _, _, d32 = NR.ray_error_stats(got, ref32)
    share_agree = float((d32[agree] > 1e-4).mean())
    cap = 2.0 * m["stats"]["ref_share_1e4"] + 4.0 / len(got)
    print(f"[{precision}] vs the reference's fp64 run over {len(got)} rays: median {med:.2e}, p95 {p95:.2e}, share > 1e-4 "
          f"{share:.5f} ({int((d > 1e-4).sum())} rays; the reference's own {ref_share:.5f} = {int((d_ref > 1e-4).sum())} rays; cap "
          f"{cap:.5f}), max {d.max():.2e}; on the {int(agree.sum())} rays where the reference agrees with itself to 1e-5: "
          f"{int((d32[agree] > 1e-4).sum())} rays more than 1e-4 from its fp32 run (share {share_agree:.5f})")
    assert abs(ref_share - m["stats"]["ref_share_1e4"]) <= 1.5 / len(got)
    assert p95 <= 1e-4
    assert share <= cap
    assert share_agree <= cap
    # the uint8 colours are the truncation of that very map, at every vertex
    assert np.array_equal(colors.cpu().numpy().astype(np.int64), np.trunc(got * np.float32(255.0)).astype(np.int64))


def test_fused_route_equals_plain_render_rays(g21, precision):
    """normal_vertex_colors renders through the ray-fused colour / depth pass (split arithmetic), and the fused kernel is what
    ran; its rgb_fine is, bit for bit, that of the plain two-kernel render_rays route (no `_maps_only`, per-sample tensors in
    memory) with the same field kernel, i.e. compute_normal=False.  The reference's literal call leaves compute_normal at
    True: the fine pass then runs the field kernel that also carries the density gradient (a normal map nobody reads), which
    rounds rgb differently -- measured 1.2e-6 (split) / 3.0e-7 (fp32) at most over G21's rays.  Bar for that comparison:
    1e-5, a tenth of the project's bar for rgb (the same network in another accumulation order: a few float32 roundings on
    a sum of 192 weighted colours in [0, 1]), the figure printed."""
    from mirror_nerf_amd import mesh
    from mirror_nerf_amd import mirror_nerf as MN
    m = g21.meta
    models = _models(g21)
    v, n = _dev(g21.inputs["vertices"], np.float32), _dev(g21.inputs["normals"], np.float32)
    rays = _dev(g21.inputs["rays"], np.float32)
    none = torch.zeros(0, 3, dtype=torch.int32, device=DEV)
    MN.LAUNCH_LOG = []
    try:
        _, rgb = mesh.normal_vertex_colors(v, none, models, _emb(), m["near"], m["far"], m["near_t"], m["N_samples"],
                                           m["N_importance"], False, 1500, normals=n, return_rgb=True)
        torch.cuda.synchronize()
        log = list(MN.LAUNCH_LOG)
    finally:
        MN.LAUNCH_LOG = None
    fused = [e for e in log if e[0] & 0x2000]
    if precision == "split" and all(MN.precision_of(mod) == "split" for mod in models.values()):
        assert len(fused) == 3 and all(e[0] & 0x4000 for e in fused)      # 4096 rays in chunks of 1500, colour / depth variant
        assert sum(e[1] for e in fused) == len(v) * (m["N_samples"] + m["N_importance"])
    else:
        assert not fused
    assert torch.equal(rgb, _plain_rgb(models, rays, m, 1500, compute_normal=False))
    assert torch.equal(rgb, _plain_rgb(models, rays, m, 4096, compute_normal=False))      # and the chunking is immaterial
    literal = float((rgb - _plain_rgb(models, rays, m, 4096)).abs().max())
    print(f"[{precision}] rgb_fine against the call with the density-gradient normals (compute_normal=True): max {literal:.2e}")
    assert literal <= 1e-5


def test_hash_grid_models_take_the_plain_route():
    import mirror_nerf_amd as M
    from mirror_nerf_amd import mesh
    models = {}
    for i, name in enumerate(("coarse", "fine")):
        torch.manual_seed(i)
        mod = M.MirrorNeRFTcnn(encoding="hashgrid", bound=1.0, predict_normal=True, predict_mirror_mask=True)
        with torch.no_grad():
            mod.encoder.embeddings.uniform_(-0.5, 0.5)
        models[name] = mod.to(DEV)
    emb = {"xyz": M.Embedding(0), "dir": M.Embedding(0)}
    v, t = mesh.marching_cubes(_dev(_sphere((16, 16, 16)), np.float32), 0.0)
    v = (v / 15.0 * 1.6 - 0.8).contiguous()
    colors, rgb = mesh.normal_vertex_colors(v, t, models, emb, 0.05, 2.0, N_samples=32, N_importance=32, chunk=300, return_rgb=True)
    rays = mesh.normal_rays(v, mesh.vertex_normals(v, t), 0.05, 2.0)
    with torch.no_grad():
        want = torch.cat([M.render_rays(models, emb, rays[i:i + 300], 32, False, 0, 0, 32, 300, False, test_time=True)["rgb_fine"]
                          for i in range(0, rays.shape[0], 300)], 0)
    assert torch.equal(rgb, want) and float(rgb.abs().max()) > 0
    assert torch.equal(colors, mesh.rgb_to_uint8(want))


# ----------------------------------------------------------------------------------------------- 5. end to end
G20_ARGS = ["--g11", "--N_grid", "48", "--x_range", "-1.5", "1.5", "--y_range", "-1.5", "1.5", "--z_range", "-0.3", "1.7",
            "--sigma_threshold", "10"]


def _script(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "extract_mesh.py")] + args, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


def test_extract_mesh_script_with_vertex_normal_colours(g20, g21, tmp_path):
    from mirror_nerf_amd import mesh
    out = str(tmp_path / "colour.ply")
    _script(G20_ARGS + ["--use_vertex_normal", "--near", "0.05", "--far", "8", "--write_normals", "--out", out])
    pv, pt, pc, pn = mesh.read_ply(out, return_normals=True)
    # the same through the Python interface
    m = g20.meta
    models = _models(g21)
    v, t = mesh.extract_mesh(models["fine"], _emb()["xyz"], m["x_range"], m["y_range"], m["z_range"], m["N"], m["threshold"])
    n = mesh.vertex_normals(v, t)
    c = mesh.normal_vertex_colors(v, t, models, _emb(), 0.05, 8.0)
    V = v.shape[0]
    assert len(pt) > 20000 and pv.shape == (V, 3) and pn.shape == (V, 3) and pc.shape == (V, 3) and pc.dtype == np.uint8
    assert np.abs(np.linalg.norm(pn.astype(np.float64), axis=1) - 1).max() <= 2e-7
    assert pv.tobytes() == v.cpu().numpy().tobytes() and np.array_equal(pt, t.cpu().numpy())
    assert pn.tobytes() == n.cpu().numpy().tobytes()
    assert np.array_equal(pc, c.cpu().numpy())
    assert len(np.unique(pc.reshape(-1))) > 50      # a picture, not a constant
    # normals without colours; and without the new flags the file the script always wrote
    out_n, out_plain = str(tmp_path / "normals.ply"), str(tmp_path / "plain.ply")
    _script(G20_ARGS + ["--write_normals", "--out", out_n])
    qv, qt, qc, qn = mesh.read_ply(out_n, return_normals=True)
    assert qc is None and qn.tobytes() == pn.tobytes() and qv.tobytes() == pv.tobytes()
    _script(G20_ARGS + ["--out", out_plain])
    rv, rt, rc = mesh.read_ply(out_plain)
    assert len(rt) > 20000 and rt.max() < len(rv) and rc is None
    expected = str(tmp_path / "expected.ply")
    mesh.write_ply(expected, v, t)
    assert open(out_plain, "rb").read() == open(expected, "rb").read()
