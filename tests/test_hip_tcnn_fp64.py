"""The hash-grid field kernels (csrc/mnrf_tcnn.hip) against a float64 reference (tests/torch_ref.py: tcnn_field64 and its pieces, run
through torch on the device) at the sample counts, table configurations and positions where the launchers change what they do:
the 512-thread block of the VALU kernel, the 16-sample groups and 256-sample tiles of the matrix-pipe kernel, the 64-lane run
aggregation and the 256-sample tiles of the backward, a second tile per workgroup of every persistent grid, every level kind
(dense, mask, modulo) and every accumulation kind (32 copies, 8 copies, none), box faces, cell faces, a tile outside the box, waves
that are one run.  The C entry points are called directly (mirror_nerf_amd._lib): the module fixes the table configuration.
Cases and clouds: tests/tcnn_cases.py (checked on their own, with the reference, by tests/test_tcnn_ref_cpu.py)."""
import numpy as np
import pytest
import torch

from tests import tcnn_cases as C
from tests import torch_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -777.25                    # sentinel of rows and planes a launch must not write
HEADS = ("sigma", "rgb", "pred_normal", "is_mirror")
EPS32 = 2.0 ** -23
# a ReLU pre-activation this close to zero, relative to the magnitudes of its dot product's terms, may fall on either side in fp32
# (four 64-term sums deep: 4 * 64 roundings); gradients of such a sample are compared through the tensor-wide sums only
FLIP = 4 * 64 * EPS32

_MODELS, _REFS = {}, {}      # models and the references of the SMALL cases (<= 4096 samples), shared between tests of this module
CACHE_MAX = 4096


@pytest.fixture(scope="module", autouse=True)
def _drop_caches():
    yield
    _MODELS.clear()
    _REFS.clear()
    torch.cuda.empty_cache()


def _field(name, bound, seed=0, table_scale=0.5):
    """A MirrorNeRFTcnn on the device holding the table configuration `name` (cached: nothing below changes a model)."""
    key = (name, bound, seed, table_scale)
    if key not in _MODELS:
        import mirror_nerf_amd as M
        from mirror_nerf_amd.mirror_nerf_tcnn import _Encoder
        torch.manual_seed(seed)
        m = M.MirrorNeRFTcnn(encoding="hashgrid", bound=bound, predict_normal=True, predict_mirror_mask=True)
        cfg = C.table_config(name, bound)
        if name == "std":
            assert np.array_equal(cfg["offsets"], m.cfg["offsets"]) and cfg["S"] == m.cfg["S"]
        else:
            m.cfg = cfg
            m.encoder = _Encoder(int(cfg["offsets"][-1]))
        with torch.no_grad():      # the default 1e-4 table makes every output ~constant: a livelier one
            m.encoder.embeddings.copy_((torch.rand(m.encoder.embeddings.shape, generator=C.gen("table", *key)) * 2 - 1) * table_scale)
        _MODELS[key] = m.to(DEV)
    return _MODELS[key]


def _w64(m, half=False):
    w = {k: v.detach().double() for k, v in m.state_dict().items()}
    if half:
        w["encoder.embeddings"] = m.encoder.embeddings.detach().half().double()
    return w


def _half_table(m):
    from mirror_nerf_amd import _lib
    table = m.encoder.embeddings.detach().contiguous()
    half = torch.empty(table.shape[0], 2, dtype=torch.float16, device=DEV)
    _lib.check(_lib.lib().mnrf_tcnn_table_half(_lib.ptr(table), table.shape[0], half.data_ptr(), _lib.stream()), "table_half")
    assert torch.equal(half, table.half())
    return half


def _common(m):
    from mirror_nerf_amd.mirror_nerf_tcnn import _offsets17
    return _offsets17(m.cfg), m.cfg["S"], m.cfg["H"], float(m.bound)


FWD_FLAGS = {"valu": 8, "pipe": 0, "planes": 0, "sigma_only": 1, "grad_normal": 2}      # include/mnrf.h


def _forward(m, B, mode, *, xyz=None, stride=6, rays=None, z=None, spr=1, n_live=None):
    """mnrf_tcnn_forward_n over sentinel-filled outputs.  mode: the VALU flag, the matrix pipe (default launch), the matrix pipe
    behind level-major planes, sigma only, full + density-gradient normal."""
    from mirror_nerf_amd import _lib
    assert _lib.MNRF_TCNN_VALU == 8 and _lib.MNRF_SIGMA_ONLY == 1 and _lib.MNRF_GRAD_NORMAL == 2
    offs, S, H, bound = _common(m)
    f = lambda *s: torch.full(s, SENT, dtype=torch.float32, device=DEV)  # noqa: E731
    out = dict(sigma=f(B), pred_normal=f(B, 3), geo_feat=f(B, 15))
    if mode != "sigma_only":
        out.update(rgb=f(B, 3), is_mirror=f(B))
    if mode == "grad_normal":
        out["normal"] = f(B, 3)
    if mode == "planes":
        out["enc"] = f(32 * B)
    p = _lib.ptr
    for t in (xyz, rays, z):
        assert t is None or (t.is_contiguous() and t.dtype == torch.float32)
    assert (xyz is None or tuple(xyz.shape) == (B, stride)) and (rays is None or rays.shape[0] * spr == B == z.numel())
    table = m.encoder.embeddings.detach()
    _lib.check(_lib.lib().mnrf_tcnn_forward_n(
        table.data_ptr(), offs, S, H, bound, p(m._weights()), FWD_FLAGS[mode], B, p(xyz), stride, p(rays), p(z), spr, None, 3,
        p(out["sigma"]), p(out.get("rgb")), p(out["pred_normal"]), p(out.get("is_mirror")), p(out.get("normal")), p(out["geo_feat"]),
        p(out.get("enc")), p(n_live), _lib.stream()), "mnrf_tcnn_forward_n")
    return out


def _backward(m, B, cot, *, xyz6=None, rays=None, z=None, spr=1, g_normal=None, kind="fixed", n_live=None):
    """mnrf_tcnn_backward_n.  kind: "atomics" (no workspace: fp32 atomics straight into d_table), "copies" (private copies of the
    coarse levels, fp32 atomics elsewhere), "f16" (packed half2 atomics on the levels without copies), "fixed" (the default of the
    Python shim: packed 64-bit fixed point there).  cot: dict head -> cotangent, absent heads are null pointers.
    Returns dict: the named weight gradients, "encoder.embeddings", "x", "d", and the workspace."""
    from mirror_nerf_amd import _lib
    from mirror_nerf_amd.mirror_nerf_tcnn import _BLOB
    L = _lib.lib()
    offs, S, H, bound = _common(m)
    table = m.encoder.embeddings.detach()
    d_table = torch.zeros_like(table)
    d_blob = torch.zeros(L.mnrf_tcnn_weight_floats(), dtype=torch.float32, device=DEV)
    d_xyz = torch.full((B, 3), SENT, dtype=torch.float32, device=DEV)
    d_dir = torch.full((B, 3), SENT, dtype=torch.float32, device=DEV)
    flags = 0
    if kind == "atomics":
        ws = None
    elif kind in ("copies", "f16"):
        flags = _lib.MNRF_TCNN_GRAD_F16 if kind == "f16" else 0
        ws = torch.zeros(max(1, L.mnrf_tcnn_backward_workspace_floats2(offs, flags)), dtype=torch.float32, device=DEV)
    else:
        assert kind == "fixed"
        flags = _lib.MNRF_TCNN_GRAD_FIXED
        ws = torch.empty(max(1, L.mnrf_tcnn_backward_workspace_floats3(offs, flags, B)), dtype=torch.float32, device=DEV)
        ws[:L.mnrf_tcnn_backward_workspace_floats(offs)].zero_()
    g = {k: (cot[k].to(DEV).float().contiguous() if k in cot else None) for k in HEADS}
    for k, t in g.items():
        assert t is None or t.shape[0] == B
    assert g_normal is None or tuple(g_normal.shape) == (B, 3)
    assert (xyz6 is None or tuple(xyz6.shape) == (B, 6)) and (rays is None or rays.shape[0] * spr == B == z.numel())
    p = _lib.ptr
    _lib.check(L.mnrf_tcnn_backward_n(
        table.data_ptr(), offs, S, H, bound, p(m._weights()), B, p(xyz6), 6, p(rays), p(z), spr, None, 3, p(g["sigma"]), p(g["rgb"]),
        p(g["pred_normal"]), p(g["is_mirror"]), p(g_normal), p(ws), p(d_table), p(d_blob), p(d_xyz), p(d_dir), None, flags,
        p(n_live), _lib.stream()), "mnrf_tcnn_backward_n")
    out, off = {"encoder.embeddings": d_table, "x": d_xyz, "d": d_dir, "ws": ws}, 0
    for name, rows, used, padded in _BLOB:
        if padded:
            out[name] = d_blob[off:off + rows * padded].view(rows, padded)[:, :used]
            off += rows * padded
        else:
            out[name] = d_blob[off:off + rows]
            off += rows
    return out


def _cloud(cloud, B, name, bound):
    """(x (B, 3), parts or keep or None) on the CPU."""
    cfg = C.table_config(name, bound)
    if cloud == "random":
        return C.random_cloud(B, bound), None
    if cloud == "edges":
        return C.edges_cloud(bound, cfg)
    if cloud == "one_cell":
        return C.one_cell_cloud(bound, cfg), None
    if cloud == "runs":
        return C.runs_cloud(bound, cfg), None
    assert cloud == "all_out"
    return C.all_out_cloud(bound)


def _inputs(cloud, B, name, bound):
    x, extra = _cloud(cloud, B, name, bound)
    d = C.directions(x.shape[0], cloud)
    return torch.cat([x, d], 1).contiguous().to(DEV), extra


# ----------------------------------------------------------------------------------------------------------- the references
def _ref_forward(name, bound, cloud, B):
    """Float64 outputs (incl. the density-gradient normal), the near-face mask and the ReLU margin of a case: computed once."""
    key = ("fwd", name, bound, cloud, B)
    if key not in _REFS:
        m = _field(name, bound)
        x6, _ = _inputs(cloud, B, name, bound)
        acts = {}
        w = _w64(m)
        o = R.tcnn_field64(w, x6[:, :3], x6[:, 3:], m.cfg, with_normal=True, acts=acts)
        ref = {k: o[k].detach() for k in HEADS + ("geo_feat", "normal")}
        ref["near"] = R.tcnn_near_face(x6[:, :3], m.cfg)
        ref["margin"] = R.tcnn_relu_margin(w, acts, o["enc"].detach(), o["dd"].detach())
        if x6.shape[0] > CACHE_MAX:
            return ref
        _REFS[key] = ref
    return _REFS[key]


def _ref_backward(name, bound, cloud, B, heads, second, x6=None, cot=None, g_normal=None, tag=""):
    """Float64 gradients of sum_k <cot_k, out_k> (+ <g_normal, normal>): dict of the named tensors, "x", "d", "e" = dL/d encoding,
    "n_e", "near", "margin" and the bound sums of dL/dx.  Computed once per case and shared by the scatter kinds."""
    key = ("bwd", name, bound, cloud, B, heads, second, tag)
    if key not in _REFS:
        m = _field(name, bound)
        if x6 is None:
            x6, _ = _inputs(cloud, B, name, bound)
        n = x6.shape[0]
        if cot is None:
            cot = C.cotangents(n, cloud)
        if second and g_normal is None:
            g_normal = torch.randn(n, 3, generator=C.gen("g_normal", n, cloud))
        w = {k: v.clone().requires_grad_(True) for k, v in _w64(m).items()}
        acts = {}
        o = R.tcnn_field64(w, x6[:, :3], x6[:, 3:], m.cfg, with_normal=second, acts=acts)
        loss = sum((o[k] * cot[k].to(DEV).double()).sum() for k in heads)
        if second:
            loss = loss + (o["normal"] * g_normal.to(DEV).double()).sum()
        loss.backward(retain_graph=n <= CACHE_MAX)
        ref = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in w.items()}
        wd = {k: v.detach() for k, v in w.items()}
        table = wd["encoder.embeddings"]
        if n <= CACHE_MAX and o["enc"].grad is not None:      # per entry: the sum of the MAGNITUDES of its contributions
            (ref["abs"],) = torch.autograd.grad((o["enc"] * o["enc"].grad.abs()).sum(), w["encoder.embeddings"])
            if second:
                ref["abs"] = ref["abs"] + R.tcnn_second_order_table_abs(x6[:, :3], table, m.cfg, wd, acts, o["grad_sigma"],
                                                                        g_normal.to(DEV))
        ref["x"] = o["xd"].grad if o["xd"].grad is not None else torch.zeros_like(o["xd"])
        ref["d"] = o["dd"].grad if o["dd"].grad is not None else torch.zeros_like(o["dd"])
        ref["e"] = o["enc"].grad if o["enc"].grad is not None else torch.zeros_like(o["enc"])
        ref["n_e"] = R.tcnn_entry_counts(x6[:, :3], m.cfg)
        ref["near"] = R.tcnn_near_face(x6[:, :3], m.cfg)
        ref["n_in"] = ~R.tcnn_unit(x6[:, :3], m.cfg["bound"])[2]
        ref["margin"] = R.tcnn_relu_margin({k: v.detach() for k, v in w.items()}, acts, o["enc"].detach(), o["dd"].detach())
        # per-sample, per-axis tolerance of dL/dx: the 128-term sum of six-factor products (136 roundings of the sum of its terms'
        # magnitudes) plus the same sum taken with the rounding bound of the sample's own e (torch_ref.tcnn_enc_grad_bound)
        g16 = acts["h16"].grad if acts["h16"].grad is not None else torch.zeros_like(acts["h16"])
        de = R.tcnn_enc_grad_bound(wd, acts, g16)
        ref["x_tol"] = 136 * EPS32 * R.tcnn_dx_sums(x6[:, :3], table, m.cfg, ref["e"])[0] + R.tcnn_dx_sums(x6[:, :3], table, m.cfg, de)[0]
        if second:
            ref["x_tol"] = ref["x_tol"] + R.tcnn_second_order_dx_bound(x6[:, :3], table, m.cfg, wd, acts, o["grad_sigma"], g_normal.to(DEV))
        ref["cot"], ref["g_normal"] = cot, g_normal
        ref = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in ref.items()}
        if n > CACHE_MAX:
            return ref
        _REFS[key] = ref
    return _REFS[key]


# --------------------------------------------------------------------------------------------------------------- the checks
def _check_forward(got, ref, mode, what, cap=True):
    """The absolute tolerances of test_tcnn_field_matches_oracle (same table scale): 2e-5 on sigma, geo_feat, rgb, is_mirror; the
    l2-normalised heads in the median and the worst case; the density-gradient normal off the near-face mask only."""
    B = ref["sigma"].shape[0]
    for k in ("sigma", "geo_feat") + (() if mode == "sigma_only" else ("rgb", "is_mirror")):
        assert got[k].shape == ref[k].shape, (what, k)
        err = float((got[k].double() - ref[k]).abs().max())
        print(f"{what} {mode} {k}: err {err:.3e}")
        assert err <= 2e-5, (what, mode, k, err)
    dp = (got["pred_normal"].double() - ref["pred_normal"]).abs().amax(-1)
    print(f"{what} {mode} pred_normal: median {float(dp.median()):.3e} max {float(dp.max()):.3e}")
    assert float(dp.median()) <= 1e-4 and float(dp.max()) <= 2e-2, (what, mode)
    if mode == "grad_normal":
        ok = ~ref["near"]
        assert not cap or int(ok.sum()) >= 0.8 * B, (what, "the near-face mask hides too much")
        dn = (got["normal"].double() - ref["normal"]).abs().amax(-1)[ok]
        if dn.numel():
            print(f"{what} normal: median {float(dn.median()):.3e} max {float(dn.max()):.3e} masked {B - int(ok.sum())}")
            assert float(dn.median()) <= 1e-5 and float((dn < 1e-3).double().mean()) >= 0.95, (what, float(dn.median()))


def _level_slices(m):
    return [(f, slice(f["off0"], f["off0"] + f["hsize"])) for f in C.level_facts(m.cfg)]


def _check_backward(m, got, ref, kind, second, what):
    B = ref["x"].shape[0]
    # ---- MLP weights: 2e-5 of the tensor's largest entry (test_tcnn_backward_matches_torch_autograd); through the second-order
    # kernel sigma_net carries the 1 / |grad sigma| of the normalisation: 2e-3 (test_tcnn_second_order_backward_matches_double_backward)
    for k, wv in ref.items():
        if "." not in k or k == "encoder.embeddings":
            continue
        scale = float(wv.abs().max()) + 1e-12
        err = float((got[k].double() - wv).abs().max())
        tol = 2e-3 if (second and k.startswith("sigma_net")) else 2e-5
        print(f"{what} {kind} {k}: err/scale {err / scale:.3e}")
        assert err <= tol * scale + 1e-7, (what, kind, k, err, scale)
    # ---- table
    gt, wt = got["encoder.embeddings"].double(), ref["encoder.embeddings"]
    scale = float(wt.abs().max()) + 1e-12
    err = (gt - wt).abs()
    print(f"{what} {kind} table: err/scale {float(err.max()) / scale:.3e}")
    if kind == "f16":
        # half2 sums on the levels without copies: test_tcnn_backward_packed_f16_table_gradient's 2e-3 of the largest entry, and where
        # many samples pile into one entry what the format allows: each of the n_e adds rounds its operand and the running sum,
        # both at most the entry's sum of magnitudes, to 11 bits
        for f, sl in _level_slices(m):
            if f["copies"]:
                assert float(err[sl].max()) <= (2e-3 if second else 6e-5) * scale + 1e-7, (what, kind, f, float(err[sl].max()), scale)
                continue
            adds = (2 if second else 1) * ref["n_e"][sl, None]          # (the second-order kernel scatters once more)
            tol = torch.maximum(torch.full_like(err[sl], 2e-3 * scale + 1e-7), (2 * adds + 2) * 2.0 ** -11 * ref["abs"][sl] + 1e-9)
            assert bool((err[sl] <= tol).all()), (what, kind, f, float((err[sl] / tol).max()))
    else:
        assert float(err.max()) <= (2e-3 if second else 6e-5) * scale + 1e-7, (what, kind, float(err.max()), scale)
    untouched = ref["n_e"] == 0
    assert bool((got["encoder.embeddings"][untouched] == 0).all()), (what, kind, "an entry no sample touches is not zero")
    assert bool((wt[untouched] == 0).all())
    # ---- directions and positions, sample by sample
    steady = ref["margin"] > FLIP
    inside = ref["n_in"]
    hidden = int((~steady & inside).sum())      # (outside the box every pre-activation of sigma_net.0 is exactly 0: checked as zeros)
    assert hidden <= max(0.1 * int(inside.sum()), 1), (what, "the ReLU margin hides too much", hidden)
    assert bool((got["x"][~inside] == 0).all()), (what, kind, "dL/dx outside the box")
    gd, wd = got["d"].double(), ref["d"]
    assert bool((got["d"] != SENT).all()) and bool((got["x"] != SENT).all())
    errd = (gd - wd).abs()[steady]
    if errd.numel():
        print(f"{what} {kind} d_dir: err/scale {float(errd.max()) / (float(wd.abs().max()) + 1e-12):.3e}")
        assert float(errd.max()) <= 2e-5 * float(wd.abs().max()) + 1e-7, (what, kind)
    ok = steady & ~ref["near"]
    gx, wx = got["x"].double(), ref["x"]
    # every sample off the masks, every axis, first and second order: err <= x_tol (_ref_backward; outside the box 0 <= 0)
    ratio = ((gx - wx).abs() / (ref["x_tol"] + 1e-30))[ok]
    if ratio.numel():
        print(f"{what} {kind} d_xyz: worst err/tol {float(ratio.max()):.3e} over {int(ok.sum())} of {B} samples")
        assert float(ratio.max()) <= 1.0, (what, kind, float(ratio.max()))


# ================================================================================================ 1. encoding planes
def _encode(m, B, *, xyz=None, stride=0, rays=None, z=None, spr=1, half=False, tail=64):
    from mirror_nerf_amd import _lib
    offs, S, H, bound = _common(m)
    planes = torch.full((32 * B + tail,), SENT, dtype=torch.float32, device=DEV)
    p = _lib.ptr
    if half:
        th = _half_table(m)
        code = _lib.lib().mnrf_tcnn_encode_flags(th.data_ptr(), offs, S, H, bound, B, p(xyz), stride, p(rays), p(z), spr, p(planes),
                                                 _lib.MNRF_TCNN_TABLE_F16, _lib.stream())
    else:
        table = m.encoder.embeddings.detach().contiguous()
        code = _lib.lib().mnrf_tcnn_encode(_lib.ptr(table), offs, S, H, bound, B, p(xyz), stride, p(rays), p(z), spr, p(planes), _lib.stream())
    return code, planes


def _check_planes(m, planes, x, B, half, what):
    assert bool((planes[32 * B:] == SENT).all()), (what, "wrote past the planes")
    got = planes[:32 * B].view(16, B, 2).permute(1, 0, 2).reshape(B, 32).double()
    table = _w64(m, half)["encoder.embeddings"]
    ref = R.tcnn_encode(x, table, m.cfg, pos="f64")
    bnd = R.tcnn_plane_bound(x, table, m.cfg)
    err = (got - ref).abs()
    worst = float((err / bnd.clamp_min(1e-300)).max())
    print(f"{what}: worst err/bound {worst:.3f}, err {float(err.max()):.3e}")
    assert bool((err <= bnd).all()), (what, worst)
    assert float(ref.abs().max()) > 0.01


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("shape", C.ENCODE_SHAPES)
@pytest.mark.parametrize("name,bound", [("std", 1.0), ("std", 6.0), ("small", 1.0)])
def test_encode_planes_ray_mode(name, bound, shape, half):
    """mnrf_tcnn_encode / mnrf_tcnn_encode_flags (half2 table) in ray mode over every thread map of tcnn_encode_kernel -- one patch,
    patches with and without the XCD permutation, both flat fallbacks -- element by element within the derived rounding bound
    (torch_ref.tcnn_plane_bound) of the float64 encoding; nothing is written behind the planes."""
    n, spr = shape
    m = _field(name, bound)
    rays, z = C.ray_cloud(n, spr, bound, name)
    x = (rays[:, None, :3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3)       # fp32, product then sum, like the kernels
    B = n * spr
    code, planes = _encode(m, B, rays=rays.to(DEV), z=z.to(DEV), spr=spr, half=half)
    assert code == 0
    oob = R.tcnn_unit(x, bound)[2]
    assert 0.02 * B <= int(oob.sum()) <= 0.7 * B          # (the rays enter and leave the box)
    _check_planes(m, planes, x.to(DEV), B, half, f"encode {name} b{bound} {shape} half={half}")


@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("stride", [6, 9])
@pytest.mark.parametrize("B", C.FWD_B)
def test_encode_planes_xyz_mode(B, stride, half):
    m = _field("std", 1.0)
    x = C.random_cloud(B, 1.0)
    if B >= 255:      # the faces, corners and cell faces ride along at the end of the larger clouds
        e = C.edges_cloud(1.0, m.cfg)[0]
        x[B - e.shape[0]:] = e
    xyz = torch.full((B, stride), 1e30)
    xyz[:, :3] = x
    code, planes = _encode(m, B, xyz=xyz.contiguous().to(DEV), stride=stride, half=half)
    assert code == 0
    _check_planes(m, planes, x.to(DEV), B, half, f"encode xyz B={B} stride={stride} half={half}")


def test_encode_planes_on_the_faces_and_cell_faces():
    m = _field("std", 6.0)
    x, _parts = C.edges_cloud(6.0, m.cfg)
    B = x.shape[0]
    xyz = torch.cat([x, torch.zeros(B, 3)], 1).contiguous().to(DEV)
    for half in (False, True):
        code, planes = _encode(m, B, xyz=xyz, stride=6, half=half)
        assert code == 0
        _check_planes(m, planes, x.to(DEV), B, half, f"encode edges half={half}")


def test_encode_refuses_a_modulo_level_on_the_host():
    """A hashed level whose size is no power of two: MNRF_ERR_UNSUPPORTED from the host-side checks, nothing launched."""
    from mirror_nerf_amd import _lib
    m = _field("odd", 1.0)
    assert any(f["mode"] == 2 for f in C.level_facts(m.cfg))
    xyz = torch.cat([C.random_cloud(64, 1.0), torch.zeros(64, 3)], 1).contiguous().to(DEV)
    for half in (False, True):
        code, planes = _encode(m, 64, xyz=xyz, stride=6, half=half)
        torch.cuda.synchronize()
        assert code == -3, code                                    # MNRF_ERR_UNSUPPORTED (include/mnrf.h)
        assert b"power-of-two" in _lib.lib().mnrf_last_error()
        assert bool((planes == SENT).all())


# ======================================================================================================== 2. forward
FWD_MODES = ("valu", "pipe", "planes", "sigma_only", "grad_normal")


def _run_forward(name, bound, cloud, B, mode):
    m = _field(name, bound)
    x6, _ = _inputs(cloud, B, name, bound)
    n = x6.shape[0]
    got = _forward(m, n, mode, xyz=x6, stride=6)
    for k, v in got.items():
        if k != "enc":
            assert bool((v != SENT).all()), (k, "a live row was not written")
    return got, _ref_forward(name, bound, cloud, B)


@pytest.mark.parametrize("mode", FWD_MODES)
@pytest.mark.parametrize("B", C.FWD_B)
def test_forward_sample_count_ladder(B, mode):
    got, ref = _run_forward("std", 1.0, "random", B, mode)
    _check_forward(got, ref, mode, f"fwd std B={B}")


@pytest.mark.parametrize("name,bound", [("std", 6.0), ("small", 1.0), ("mid", 1.0), ("odd", 1.0)])
def test_forward_every_table_configuration(name, bound):
    """Dense / mask / modulo levels at B = 257.  `odd` (a modulo level) cannot run on the matrix pipe: the default launch must give the
    VALU kernel's result, bit for bit, and both agree with float64."""
    outs = {}
    for mode in FWD_MODES:
        got, ref = _run_forward(name, bound, "random", 257, mode)
        _check_forward(got, ref, mode, f"fwd {name} b{bound}")
        outs[mode] = got
    if name == "odd":
        for mode in ("pipe", "planes"):
            for k in HEADS + ("geo_feat",):
                assert torch.equal(outs[mode][k], outs["valu"][k]), (mode, k)
        assert bool((outs["planes"]["enc"] == SENT).all())          # (the VALU kernel does not touch the planes)


@pytest.mark.parametrize("cloud", ["edges", "all_out", "one_cell"])
@pytest.mark.parametrize("bound", [1.0, 6.0])
def test_forward_clouds(cloud, bound):
    for mode in FWD_MODES:
        got, ref = _run_forward("std", bound, cloud, 0, mode)
        _check_forward(got, ref, mode, f"fwd {cloud} b{bound}", cap=False)       # (edges: most points sit ON cell faces)
        if cloud == "all_out":      # the tile outside the box: the features are exact zeros, so every sample gives the same outputs
            assert bool((got["sigma"][256:512] == got["sigma"][256]).all()) and bool((ref["geo_feat"][256:512] == 0).all())


@pytest.mark.parametrize("mode", ["pipe", "planes"])
def test_forward_second_tile_per_workgroup(mode):
    """WRAP_FWD samples: 513 tiles for the 512 workgroups of tcnn_mfma_kernel."""
    got, ref = _run_forward("std", 1.0, "random", C.WRAP_FWD, mode)
    _check_forward(got, ref, mode, f"fwd wrap B={C.WRAP_FWD}")


# ======================================================================================================= 3. backward
KINDS = ("atomics", "copies", "f16", "fixed")


def _run_backward(name, bound, cloud, B, kind, second, heads=HEADS):
    m = _field(name, bound)
    x6, _ = _inputs(cloud, B, name, bound)
    ref = _ref_backward(name, bound, cloud, B, heads, second)
    got = _backward(m, x6.shape[0], {k: ref["cot"][k] for k in heads}, xyz6=x6, kind=kind,
                    g_normal=ref["g_normal"].to(DEV).float().contiguous() if second else None)
    _check_backward(m, got, ref, kind, second, f"bwd {name} b{bound} {cloud} B={x6.shape[0]} 2nd={second} heads={len(heads)}")
    return got, ref


@pytest.mark.parametrize("second", [False, True])
@pytest.mark.parametrize("B", C.BWD_B)
def test_backward_sample_count_ladder(B, second):
    for kind in ("fixed", "atomics"):
        _run_backward("std", 1.0, "random", B, kind, second)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,bound", [("std", 1.0), ("std", 6.0), ("small", 1.0), ("mid", 1.0), ("odd", 1.0)])
def test_backward_every_table_configuration_and_scatter_kind(name, bound, kind):
    for second in (False, True):
        _run_backward(name, bound, "random", 257, kind, second)


@pytest.mark.parametrize("absent", HEADS)
def test_backward_one_absent_head(absent):
    heads = tuple(k for k in HEADS if k != absent)
    got, ref = _run_backward("std", 1.0, "random", 257, "fixed", False, heads)
    if absent == "rgb":
        assert float(got["color_net.2.weight"].abs().max()) == 0.0 and float(got["d"].abs().max()) == 0.0
    if absent == "is_mirror":
        assert float(got["is_mirror_net.2.weight"].abs().max()) == 0.0
    if absent == "pred_normal":
        assert float(got["normal_net.1.weight"].abs().max()) == 0.0


@pytest.mark.parametrize("second", [False, True])
@pytest.mark.parametrize("cloud", ["runs", "one_cell", "edges", "all_out"])
def test_backward_clouds(cloud, second):
    for kind in KINDS:
        _run_backward("std", 1.0, cloud, 0, kind, second)


def test_backward_tile_outside_the_box_adds_nothing():
    """all_out: three tiles, the middle one outside the box.  Its samples must add nothing: on the fixed-point levels -- exact
    integer sums under a scale that only depends on the level's S -- the table gradient equals, bit for bit, the run over the two
    inside tiles alone; the levels with private copies are sums of fp32 atomics (order-dependent in the last bits)."""
    m = _field("std", 1.0)
    x6, keep = _inputs("all_out", 0, "std", 1.0)
    cot = C.cotangents(768, "all_out")
    full = _backward(m, 768, cot, xyz6=x6, kind="fixed")
    keep = keep.to(DEV)
    part = _backward(m, 512, {k: v[keep.cpu()] for k, v in cot.items()}, xyz6=x6[keep].contiguous(), kind="fixed")
    assert bool((full["x"][256:512] == 0).all()) and torch.equal(full["x"][keep], part["x"]) and torch.equal(full["d"][keep], part["d"])
    a, b = full["encoder.embeddings"], part["encoder.embeddings"]
    n_fixed = 0
    for f, sl in _level_slices(m):
        if f["copies"]:
            assert float((a[sl] - b[sl]).abs().max()) <= 1e-5 * float(b[sl].abs().max()), f
        else:
            n_fixed += 1
            assert torch.equal(a[sl], b[sl]), f
    assert n_fixed >= 8


@pytest.mark.parametrize("second", [False, True])
def test_backward_second_tile_per_workgroup(second):
    """WRAP_BWD samples: 257 tiles for the 256 workgroups of tcnn_bwd_kernel / tcnn_bwd2_kernel, whose weight-gradient register tiles
    live across the tiles of a workgroup."""
    _run_backward("std", 1.0, "random", C.WRAP_BWD, "fixed", second)


# ================================================================================================= 4. live row counts
@pytest.mark.parametrize("n_live", [0, 1, 63, 64])
def test_live_row_counts(n_live):
    """mnrf_tcnn_forward_n / mnrf_tcnn_backward_n in ray mode, capacity 64 rays x 8: the live rows equal the plain call over the first
    n_live rays bit for bit, rows and planes past the count keep their sentinel, the gradients are those of the plain call."""
    m = _field("std", 1.0)
    spr, cap = 8, 64
    rays, z = C.ray_cloud(cap, spr, 1.0, "live")
    rays, z = rays.to(DEV), z.to(DEV)
    nl = torch.tensor([n_live], dtype=torch.int32, device=DEV)
    n = n_live * spr
    for mode in FWD_MODES:
        got = _forward(m, cap * spr, mode, rays=rays, z=z, spr=spr, n_live=nl)
        plain = _forward(m, n, mode, rays=rays[:n_live].contiguous(), z=z[:n_live].contiguous(), spr=spr) if n else None
        for k, v in got.items():
            if k == "enc":
                planes = v.view(16, cap * spr, 2)
                assert bool((planes[:, n:] == SENT).all()), (mode, "planes past the count")
                if n:
                    assert torch.equal(planes[:, :n], plain["enc"].view(16, n, 2)), mode
                continue
            assert bool((v[n:] == SENT).all()), (mode, k, "rows past the count")
            if n:
                assert torch.equal(v[:n], plain[k]), (mode, k)
    cot = C.cotangents(cap * spr, "live")
    g_normal = torch.randn(cap * spr, 3, generator=C.gen("g_normal", "live")).to(DEV)
    for kind in ("fixed", "copies"):
        for second in (False, True):
            got = _backward(m, cap * spr, cot, rays=rays, z=z, spr=spr, kind=kind, n_live=nl, g_normal=g_normal if second else None)
            assert bool((got["x"][n:] == SENT).all()) and bool((got["d"][n:] == SENT).all())
            if not n:
                assert all(float(v.abs().max()) == 0.0 for k, v in got.items() if "." in k)
                continue
            plain = _backward(m, n, {k: v[:n] for k, v in cot.items()}, rays=rays[:n_live].contiguous(), z=z[:n_live].contiguous(),
                              spr=spr, kind=kind, g_normal=g_normal[:n].contiguous() if second else None)
            assert torch.equal(got["x"][:n], plain["x"]) and torch.equal(got["d"][:n], plain["d"])
            for k, v in plain.items():
                if "." in k:      # sums of atomics: equal to the order of the adds
                    assert float((got[k] - v).abs().max()) <= 1e-5 * float(v.abs().max()) + 1e-30, (kind, second, k)


# ================================================================================ 5. fixed-point scatter at training sizes
def _shim_table_grad(m, x6, cot):
    """The table gradient as training gets it: through TcnnFieldFn, which picks the scatter."""
    from mirror_nerf_amd.mirror_nerf_tcnn import TcnnFieldFn
    m.zero_grad()
    outs = TcnnFieldFn.apply(m, 1, x6.clone().requires_grad_(True), None, None, None, False, m.encoder.embeddings, *m.mlp_params())
    sum((o_ * cot[k].to(DEV)).sum() for o_, k in zip(outs[:4], HEADS)).backward()
    g = m.encoder.embeddings.grad.clone()
    m.zero_grad()
    return g


def _scatter_errors(B, kinds=("fixed", "copies")):
    """Table gradients of B uniform samples in the bound-6 box against float64, per level without private copies: worst error
    relative to the level's largest entry for the fixed-point and the fp32-atomic path, and the hard checks of the fixed-point
    path.  Entries that a sample with a ReLU pre-activation within rounding of zero adds to are left out (FLIP above: its whole
    dL/d encoding may differ between two correct fp32 evaluations -- both paths then miss float64 by that sample's contribution,
    a few 1e-3 of the level's largest entry); at most 3 % of the samples are of that kind."""
    m = _field("std", 6.0)
    ref = _ref_backward("std", 6.0, "random", B, HEADS, False)
    x6, _ = _inputs("random", B, "std", 6.0)
    S = R.tcnn_level_sums(ref["e"], x6[:, :3], m.cfg)
    want = ref["encoder.embeddings"]
    unsteady = ref["margin"] <= FLIP
    print(f"samples with a ReLU pre-activation within rounding of zero: {int(unsteady.sum())} of {B}")
    assert int(unsteady.sum()) <= 0.03 * B
    shaky = R.tcnn_entry_counts(x6[:, :3][unsteady].contiguous(), m.cfg) > 0
    rows = []
    got = {kind: (_shim_table_grad(m, x6, ref["cot"]) if kind == "shim" else
                  _backward(m, B, ref["cot"], xyz6=x6, kind=kind)["encoder.embeddings"]).double() for kind in kinds}
    for lv, (f, sl) in enumerate(_level_slices(m)):
        if f["copies"]:
            continue
        ok = ~shaky[sl]
        touched = ref["n_e"][sl] > 0
        hidden = float(shaky[sl].sum()) / max(1, int(touched.sum()))
        # an entry is left out when any of its n_e contributors is unsteady: with a share p of such samples that is
        # 1 - (1 - p)^n_e of the entries with n_e contributors -- asserted per level, with 2 % on top for the scatter of a count
        p_un = float(unsteady.double().mean())
        expect = float((1 - (1 - p_un) ** ref["n_e"][sl][touched].double()).mean()) if int(touched.sum()) else 0.0
        assert hidden <= expect + 0.02, (lv, hidden, expect)
        top = float(want[sl].abs().max())
        err = {kind: ((g[sl] - want[sl]).abs() * ok[:, None]) for kind, g in got.items()}
        # the power of two k of a level puts k S below 2^31: half a step is below S 2^-30 per add.  (The kernel takes S from its
        # own fp32 dL/d encoding, good to 2e-5 of its largest entry: 1e-4 of slack on S.)
        bnd = ref["n_e"][sl, None].double() * float(S[lv]) * 2.0 ** -30 * (1 + 1e-4) + 2 * EPS32 * want[sl].abs()
        row = dict(level=lv, step=float(S[lv]) * 2.0 ** -30 / top, n_max=int(ref["n_e"][sl].max()), hidden=hidden)
        for kind in kinds:
            row[kind] = float(err[kind].max()) / top
        if "fixed" in kinds:
            row["ratio"] = float((err["fixed"] / bnd.clamp_min(1e-300)).max())
            big = (want[sl].abs() > bnd) & ok[:, None]
            row["signs_ok"] = bool((torch.sign(got["fixed"][sl][big]) == torch.sign(want[sl][big])).all())
        rows.append(row)
    print(f"table-gradient scatter against float64, B = {B}: level | " + " | ".join(f"{k} err/top" for k in kinds)
          + " | S 2^-30/top | max n_e | fixed err/bound | entries left out")
    for r in rows:
        print(f"  {r['level']:2d} | " + " | ".join(f"{r[k]:.2e}" for k in kinds)
              + f" | {r['step']:.2e} | {r['n_max']:4d} | {r.get('ratio', float('nan')):.3f} | {r['hidden']:.4f}")
    return rows


YARDSTICK = 4e-5      # of each level's largest entry: what test_tcnn_fixed_point_table_gradient holds the default scatter to


def test_fixed_point_scatter_small_batch_against_float64():
    """The size the suite already runs (7968 samples), now against float64 instead of against the fp32-atomic path: both paths
    within the yardstick.  (At this size the fixed-point step is below 1e-6 of a level's largest entry and the error of BOTH paths
    is the fp32 rounding of dL/d encoding and of the interpolation weights, about 4e-6: the per-entry bound of the training sizes
    -- which knows the fixed-point rounding only -- is not asserted here.)"""
    rows = _scatter_errors(C.FX_SMALL_B)
    assert len(rows) >= 8
    for r in rows:
        assert r["fixed"] <= YARDSTICK and r["copies"] <= YARDSTICK, r
        assert r["signs_ok"], r


def test_fixed_point_scatter_at_the_training_size():
    """TRAIN_B = 196 608 samples (1024 rays x 192), bound 6: every entry of a fixed-point level within n_e S 2^-30 + 2 eps32 |entry|
    of float64, no half overflowed, and the yardstick of the default scatter -- 4e-5 of each level's largest entry -- holds.
    Measured: worst level 2.1e-5 in fixed point (fp32 atomics 6.1e-6), a factor 1.9 inside the yardstick; worst
    error / bound 0.56.  With the scale at 2^30 instead of 2^31 it was 4.7e-5: over the yardstick, which is what moved the scale."""
    from mirror_nerf_amd.mirror_nerf_tcnn import FIXED_MAX_SAMPLES
    assert C.TRAIN_B <= FIXED_MAX_SAMPLES
    rows = _scatter_errors(C.TRAIN_B)
    assert len(rows) >= 8
    for r in rows:
        assert r["ratio"] <= 1.0, r
        assert r["signs_ok"], r
        assert r["fixed"] <= YARDSTICK, r


def test_fixed_point_scatter_at_the_edge_of_the_rule():
    """B = FIXED_MAX_SAMPLES, the largest call TcnnFieldFn still scatters in fixed point: what training gets there (through the
    shim) is the fixed-point gradient bit for bit, and it meets the yardstick.  Measured: worst level 2.4e-5."""
    from mirror_nerf_amd.mirror_nerf_tcnn import FIXED_MAX_SAMPLES
    rows = _scatter_errors(FIXED_MAX_SAMPLES, kinds=("fixed", "shim"))
    assert len(rows) >= 8
    for r in rows:
        assert r["ratio"] <= 1.0 and r["signs_ok"], r
        assert r["shim"] == r["fixed"] <= YARDSTICK, r


def test_fixed_point_scatter_past_the_rule():
    """WRAP_FX = 2048 * 256 + 77 samples: some workgroup of tcnn_scatter_fx_kernel takes a second tile, and the per-entry bound and
    the no-overflow check hold as at TRAIN_B.  The step has grown with the sample count, though.
    Measured: worst level 6.4e-5 of its largest entry in fixed point (1.4e-4 before the scale moved to 2^31) against
    9.5e-6 with fp32 atomics; worst error / bound 0.49.  Fixed point misses the 4e-5 yardstick here.
    So the Python shim leaves fixed point above FIXED_MAX_SAMPLES samples per call: what training gets at this size
    -- through TcnnFieldFn -- is the fp32-atomic gradient, and it meets the yardstick."""
    from mirror_nerf_amd.mirror_nerf_tcnn import FIXED_MAX_SAMPLES
    assert FIXED_MAX_SAMPLES < C.WRAP_FX
    rows = _scatter_errors(C.WRAP_FX, kinds=("fixed", "copies", "shim"))
    assert len(rows) >= 8
    for r in rows:
        assert r["ratio"] <= 1.0, r
        assert r["signs_ok"], r
        assert r["shim"] <= YARDSTICK and r["copies"] <= YARDSTICK, r
    assert max(r["fixed"] for r in rows) > max(r["shim"] for r in rows)
