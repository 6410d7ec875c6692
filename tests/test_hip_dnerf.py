"""GPU tests of the D-NeRF object field (csrc/mnrf_dnerf.hip, mirror_nerf_amd/dnerf.py).

The kernel against the float64 restatement (tests/dnerf_ref.py, pinned to the reference by tests/test_dnerf_ref_cpu.py) on the
points of fixture G27-model.  Bar per output group: 4 x the reference's own fp32 deviation from float64 on these points
(meta.floor, which is relative to max(1, max |value|) over the fixture's points, times that same scale) -- the factor
FX.tolerance uses; it leaves room for the MFMA's accumulation order and the time columns folded into the first bias.  t = 1.0
is not in the fixture and takes the floor of t = 0.37 (the same chain of operations).  Measured on an MI355X (max over the
sizes, times and modes of test_kernel_matches_float64, test_ray_generated_positions and test_module_forward; bar in brackets):
    t = 0.37 / 1.0:  dx 1.5e-7 (6.2e-7), raw rgb 1.7e-7 (4.3e-7), alpha 5.5e-4 (1.8e-3) on values up to 36
    t = 0:           dx 0 (0), raw rgb 5.7e-8 (2.5e-7), alpha 3.3e-5 (9.1e-5)

DirectTemporalNeRF.forward and render_rays_dnerf against the restatement: the module on the same bar; the renderer on the bars
of the fixture comparisons (1e-4, depth-like keys 8e-4, or 4 x the floor if that is larger), where the floor is the
restatement's own fp32 run against its float64 run on the same rays, and the share of rays beyond the base bar is at most
that run's share plus one ray.

batched_inference against G27-scene on the bars of test_hip_objects.test_objects_golden, on both arithmetics of the scene
field, and one scripts/eval_scene.py run with a moving object."""
import importlib.util
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import dnerf_ref as DR
from tests.golden import fixtures as FX
from tests.golden import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WG = 128                        # samples of one workgroup (csrc/mnrf_dnerf.hip WG_SAMPLES)
SIZES = [1, WG - 1, WG, WG + 1, 3 * WG + 17]
KEYS = ("rgb_", "depth_", "opacity_", "mirror_mask_", "surface_normal_", "x_surface_")
GUARD = 7.5


@pytest.fixture(params=["split", "fp32"])
def precision(request):
    from mirror_nerf_amd import mirror_nerf as MN
    old = MN.PRECISION
    MN.set_precision(request.param)
    yield request.param
    MN.set_precision(old)


class _Model:
    """Fixture G27-model: its weights on the device and, per time, the float64 restatement on its first points, computed once."""

    def __init__(self):
        self.fx = FX.Fixture("g27_dnerf_model")
        self.sd = DR.make_state_dicts(self.fx.meta["seed"], 1)[0]
        W.apply_tweaks(self.sd, self.fx.meta["tweaks"])
        c = self.fx.meta["checksum"][0]
        assert abs(W.checksum(self.sd) - c) <= 1e-9 * max(1.0, abs(c))
        self.module = DR.module_of(self.sd, DEV)
        self.n = SIZES[-1]
        self.xyz, self.view = self.fx.inputs["xyz"][:self.n], self.fx.inputs["viewdirs"][:self.n]
        self.want = {}

    def ref(self, t):
        if t not in self.want:
            raw, dx = DR.field(self.sd, torch.from_numpy(self.xyz).double(), torch.from_numpy(self.view).double(), t)
            self.want[t] = (raw.numpy(), dx.numpy())
        return self.want[t]

    def bars(self, t):
        """Absolute bar per output group: 4 x meta.floor x max(1, max |value|) over the fixture's points."""
        tag = "t0" if t == 0.0 else "t037"
        out = {}
        for key, vals in (("dx", self.fx.outputs[f"dx64_{tag}"]), ("rgb", self.fx.outputs[f"raw64_{tag}"][:, :3]),
                          ("alpha", self.fx.outputs[f"raw64_{tag}"][:, 3])):
            out[key] = 4.0 * self.fx.meta["floor"][f"{key}_{tag}"] * max(1.0, float(np.abs(vals).max()))
        return out


@pytest.fixture(scope="module")
def model():
    return _Model()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _dir_emb(view):
    from mirror_nerf_amd.rendering import _embed
    return _embed(_dev(view), 4)


def _launch(module, t, B, *, xyz=None, rays=None, z=None, spr=1, dir_emb=None, sigma_only=False, raw=True):
    """mnrf_dnerf_forward through dnerf_field's own packing, into buffers with guard rows behind row B."""
    from mirror_nerf_amd import _lib, dnerf as DN
    pad = 5
    f = lambda *s: torch.full(s, GUARD, dtype=torch.float32, device=DEV)  # noqa: E731
    sigma, rgb, dx = f(B + pad), f(B + pad, 3), f(B + pad, 3)
    flags = (_lib.MNRF_DNERF_SIGMA_ONLY if sigma_only else 0) | (_lib.MNRF_DNERF_RAW_RGB if raw else 0)
    if t == 0.0 and module.zero_canonical:
        flags |= _lib.MNRF_DNERF_CANONICAL
    p = _lib.ptr
    _lib.check(_lib.lib().mnrf_dnerf_forward(p(DN.packed_of(module)), flags, B, p(xyz), 3, p(rays), p(z), spr, p(dir_emb), 27, float(t),
                                             p(sigma), p(rgb), p(dx), _lib.stream()), "mnrf_dnerf_forward")
    out = {k: v.cpu().numpy() for k, v in (("sigma", sigma), ("rgb", rgb), ("dx", dx))}
    for k, v in out.items():                                  # rows past B are not written
        assert (v[B:] == GUARD).all(), f"{k}: a row behind B = {B} was written"
        if sigma_only and k == "rgb":
            assert (v == GUARD).all(), "sigma only: rgb was written"
    return {k: v[:B] for k, v in out.items()}


def _check(tag, got, raw64, dx64, bars, sigma_only=False):
    errs = {"alpha": np.abs(got["sigma"].astype(np.float64) - raw64[:, 3]).max(),
            "dx": np.abs(got["dx"].astype(np.float64) - dx64).max()}
    if not sigma_only:
        errs["rgb"] = np.abs(got["rgb"].astype(np.float64) - raw64[:, :3]).max()
    print(f"dnerf {tag}: " + ", ".join(f"{k} {v:.3e} (bar {bars[k]:.1e})" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= bars[k], f"{tag}: {k} deviates by {v:.3e} from float64, bar {bars[k]:.3e}"


@pytest.mark.parametrize("t", [0.0, 0.37, 1.0])
@pytest.mark.parametrize("B", SIZES)
def test_kernel_matches_float64(model, B, t):
    """Explicit positions; the full launch and the sigma-only launch."""
    raw64, dx64 = model.ref(t)
    xyz, de = _dev(model.xyz[:B]), _dir_emb(model.view[:B])
    got = _launch(model.module, t, B, xyz=xyz, dir_emb=de)
    _check(f"B={B} t={t}", got, raw64[:B], dx64[:B], model.bars(t))
    only = _launch(model.module, t, B, xyz=xyz, sigma_only=True)
    _check(f"B={B} t={t} sigma only", only, raw64[:B], dx64[:B], model.bars(t), sigma_only=True)
    # stopping in front of the colour branch changes nothing in front of it
    assert np.array_equal(only["sigma"], got["sigma"]) and np.array_equal(only["dx"], got["dx"])
    if t == 0.0:
        assert not got["dx"].any()


def test_sigmoid_flag(model):
    """Without the raw flag the colour is the sigmoid of the raw colour, as raw2outputs applies it."""
    B = WG + 1
    xyz, de = _dev(model.xyz[:B]), _dir_emb(model.view[:B])
    raw = _launch(model.module, 0.37, B, xyz=xyz, dir_emb=de, raw=True)
    rgb = _launch(model.module, 0.37, B, xyz=xyz, dir_emb=de, raw=False)
    assert np.array_equal(raw["sigma"], rgb["sigma"]) and np.array_equal(raw["dx"], rgb["dx"])
    want = 1.0 / (1.0 + np.exp(-raw["rgb"].astype(np.float64)))
    assert np.abs(rgb["rgb"] - want).max() <= 2e-7          # an fp32 exp, an add and a division on values in (0, 1)


@pytest.mark.parametrize("t", [0.0, 0.37])
@pytest.mark.parametrize("spr", [5, 7])
def test_ray_generated_positions(model, spr, t):
    """o + d z from rays and depths, the view encoding per ray: with 5 and 7 samples per ray a ray's samples straddle the
    16-sample groups of a wave and the workgroup seams.  The restatement sees the fp32 positions the kernel forms (a multiply,
    then an add), so the bar of the explicit positions holds."""
    n_rays = (3 * WG + 17) // spr + 1
    B = n_rays * spr
    rs = np.random.RandomState(spr)
    rays = np.zeros((n_rays, 8), np.float32)
    rays[:, :3] = model.fx.inputs["xyz"][-n_rays:] * np.float32(0.8)
    rays[:, 3:6] = model.fx.inputs["viewdirs"][-n_rays:]
    z = np.sort(rs.uniform(0.0, 0.3, (n_rays, spr)).astype(np.float32), axis=1)
    pts = (rays[:, None, :3] + rays[:, None, 3:6] * z[:, :, None]).astype(np.float32).reshape(-1, 3)
    assert np.abs(pts).max() <= 1.5
    view = np.repeat(rays[:, 3:6], spr, axis=0)
    raw64, dx64 = DR.field(model.sd, torch.from_numpy(pts).double(), torch.from_numpy(view).double(), t)
    got = _launch(model.module, t, B, rays=_dev(rays), z=_dev(z), spr=spr, dir_emb=_dir_emb(rays[:, 3:6]))
    _check(f"rays spr={spr} t={t}", got, raw64.numpy(), dx64.numpy(), model.bars(t))
    same = _launch(model.module, t, B, xyz=_dev(pts), spr=spr, dir_emb=_dir_emb(rays[:, 3:6]))
    for k in got:
        assert np.array_equal(got[k], same[k]), f"{k}: ray-generated and explicit positions differ"


def test_canonical_flag_is_a_zero_deformation(model):
    """t = 0: dx is exactly zero, and the outputs are bit for bit those of a launch at t != 0 of the same model with a
    _time_out of zeros (whose deformation net runs and yields dx = 0)."""
    B = 3 * WG + 17
    xyz, de = _dev(model.xyz[:B]), _dir_emb(model.view[:B])
    canon = _launch(model.module, 0.0, B, xyz=xyz, dir_emb=de)
    assert not canon["dx"].any() and not np.signbit(canon["dx"]).any()
    sd = {k: v.copy() for k, v in model.sd.items()}
    sd["_time_out.weight"][...] = 0
    sd["_time_out.bias"][...] = 0
    still = _launch(DR.module_of(sd, DEV), 0.37, B, xyz=xyz, dir_emb=de)
    assert not still["dx"].any()
    for k in ("sigma", "rgb"):
        assert np.array_equal(canon[k], still[k]), k
    # not_zero_canonical: t = 0 runs the deformation net like any other time
    moved = _launch(DR.module_of(model.sd, DEV, zero_canonical=False), 0.0, B, xyz=xyz, dir_emb=de)
    assert np.abs(moved["dx"]).max() > 0.01


def test_module_forward(model):
    """DirectTemporalNeRF.forward(x, ts) with the reference's inputs: cat[embed(xyz), embed(viewdir)] and the time encoding."""
    from mirror_nerf_amd.rendering import _embed
    B = 3 * WG + 17
    x = torch.cat([_embed(_dev(model.xyz[:B]), 10), _dir_emb(model.view[:B])], 1)
    for t in (0.37, 0.0):
        ts = _embed(torch.full((B, 1), t, device=DEV), 10)
        out, dx = model.module(x, [ts, ts])
        assert tuple(out.shape) == (B, 4) and tuple(dx.shape) == (B, 3)
        raw64, dx64 = model.ref(t)
        _check(f"forward t={t}", {"sigma": out[:, 3].cpu().numpy(), "rgb": out[:, :3].cpu().numpy(), "dx": dx.cpu().numpy()},
               raw64[:B], dx64[:B], model.bars(t))
    ts2 = ts.clone()
    ts2[3, 0] = 0.5
    with pytest.raises(AssertionError, match="same time"):
        model.module(x, [ts2, ts2])


# ------------------------------------------------------------------------------------------------------ render_rays_dnerf
RENDER_TWEAKS = [["_occ.alpha_linear.weight", "mul", 1000.0]]      # the deformation gain stays at 1, as in G27-scene


@pytest.fixture(scope="module")
def render_models():
    sds = DR.make_state_dicts(DR.MODEL_SEED, 2)
    for sd in sds:
        W.apply_tweaks(sd, RENDER_TWEAKS)
    return sds, [DR.module_of(sd, DEV) for sd in sds]


def _ray_batch(n, seed):
    rs = np.random.RandomState(seed)
    b = np.zeros((n, 12), np.float32)
    b[:, :3] = rs.uniform(-1.0, 1.0, (n, 3))
    d = rs.normal(size=(n, 3))
    b[:, 3:6] = d / np.linalg.norm(d, axis=1, keepdims=True)
    b[:, 6], b[:, 7], b[:, 8] = 0.1, rs.uniform(0.5, 3.0, n), 0.37
    b[:, 9:] = b[:, 3:6] / np.linalg.norm(b[:, 3:6], axis=1, keepdims=True)
    return b


@pytest.mark.parametrize("two", [True, False], ids=["two_models", "single_model"])
@pytest.mark.parametrize("n,ns,ni", [(37, 5, 7), (64, 64, 64)])
def test_render_rays_dnerf(render_models, n, ns, ni, two):
    from mirror_nerf_amd.dnerf import render_rays_dnerf
    sds, mods = render_models
    batch = _ray_batch(n, 100 + n)
    kw = dict(network_fn=mods[0], network_fine=mods[1] if two else None, N_samples=ns, N_importance=ni, white_bkgd=True,
              use_two_models_for_fine=two, perturb=False, raw_noise_std=0.0, network_query_fn=None, near=2.0, far=6.0, ndc=False)
    got = render_rays_dnerf(_dev(batch), **kw)
    assert set(got) == {"rgb_map", "disp_map", "acc_map", "depth_map", "z_vals", "position_delta"}
    assert tuple(got["z_vals"].shape) == (n, ns + ni) and tuple(got["position_delta"].shape) == (n, ns + ni, 3)
    args = (sds[0], sds[1] if two else None)
    want = DR.render(*args, torch.from_numpy(batch).double(), ns, ni, True)
    own32 = DR.render(*args, torch.from_numpy(batch), ns, ni, True)          # the restatement's own fp32 noise on these rays
    for k in ("rgb_map", "depth_map", "acc_map"):
        w = want[k].numpy().reshape(n, -1)
        d = np.abs(got[k].double().cpu().numpy().reshape(n, -1) - w).max(1)
        d32 = np.abs(own32[k].double().numpy().reshape(n, -1) - w).max(1)
        base = 8e-4 if k == "depth_map" else 1e-4
        tol = max(base, 4.0 * float(d32.max()))
        allowed = float((d32 > base).mean()) + 1.0 / n
        print(f"render_rays_dnerf n={n} {ns}+{ni} two={two} {k}: max |err| {d.max():.3e} (tolerance {tol:.1e}), share beyond {base:.0e}: "
              f"{(d > base).mean():.4f} (allowed {allowed:.4f})")
        assert d.max() <= tol, f"{k}: {d.max():.3e} > {tol:.1e}"
        assert (d > base).mean() <= allowed, k
    # (N, 9) rows: the view direction is d / |d|, the plain division of eval.py:242-243
    b9 = _dev(batch[:, :9])
    short = render_rays_dnerf(b9, **kw)
    full = render_rays_dnerf(torch.cat([b9, b9[:, 3:6] / torch.norm(b9[:, 3:6], dim=-1, keepdim=True)], -1), **kw)
    for k in full:      # (disp_map of a ray that met no density is 0 / 0, there as here)
        assert np.array_equal(short[k].cpu().numpy(), full[k].cpu().numpy(), equal_nan=True), k


# ------------------------------------------------------------------------------------- batched_inference against G27-scene
def _scene_module(sd):
    import mirror_nerf_amd as M
    m = M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV)


def _object_kwargs(meta):
    sds = DR.make_state_dicts(meta["obj_seed"], len(meta["obj_tweaks"]))
    for sd, tw, c in zip(sds, meta["obj_tweaks"], meta["obj_checksum"]):
        W.apply_tweaks(sd, tw)
        assert abs(W.checksum(sd) - c) <= 1e-9 * max(1.0, abs(c)), "object weights differ from the fixture's"
    mods = [DR.module_of(sd, DEV) for sd in sds]
    cfg = meta["obj_config"]
    return dict(network_fn=mods[0], network_fine=mods[1] if len(mods) > 1 else None, N_samples=cfg["N_samples"],
                N_importance=cfg["N_importance"], white_bkgd=cfg["white_bkgd"], use_two_models_for_fine=cfg["use_two_models_for_fine"],
                lindisp=cfg["lindisp"], perturb=False, raw_noise_std=0.0, network_query_fn=None, near=2.0, far=6.0)


def _run(fx, **extra):
    import mirror_nerf_amd as M
    m = fx.meta
    sds = fx.state_dicts()
    models = {"coarse": _scene_module(sds[0]), "fine": _scene_module(sds[1])}
    emb = {"xyz": M.Embedding(10), "dir": M.Embedding(4)}
    out = M.batched_inference(models, emb, _dev(fx.inputs["rays"]), m["N_samples"], m["N_importance"], False, m["chunk"], args=m["args"],
                              trace_secondary_rays=True, new_object=m["new_object"], render_kwargs_test_d_nerf=_object_kwargs(m),
                              args_d_nerf=SimpleNamespace(use_viewdirs=True), frame_time=m["frame_time"], **extra)
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name", ["g27_dnerf_office_canonical_l2", "g27_dnerf_office_l2", "g27_dnerf_single_posed_l1"])
def test_dnerf_scene_golden(name, precision):
    fx = FX.Fixture(name)
    used = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = _run(fx, object_used=used)
    keys = [k for k in fx.outputs if k.startswith(KEYS) or k == "reflect_direction"]
    assert {"rgb_fine", "depth_fine", "mirror_mask_fine", "surface_normal_fine", "x_surface_fine", "rgb_fine_reflect",
            "depth_fine_reflect"} <= set(keys), keys
    assert int(used.item()) > 0
    fails = []
    for k in keys:
        want = fx.outputs[k]
        assert k in got, f"{name}: missing {k}"
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, (name, k, got[k].dtype, want.dtype, got[k].shape, want.shape)
        g, w = got[k].astype(np.float64), want.astype(np.float64)
        d = np.abs(g - w).reshape(w.shape[0], -1).max(1) if w.size else np.zeros(0)
        bar = 8e-4 if k.startswith(("depth", "x_surface")) else 1e-4
        frac = float((d > bar).mean()) if d.size else 0.0
        tol, allowed = FX.tolerance(k, fx.meta), fx.meta["floor_frac"].get(k, 0.0)
        print(f"G27 {name} [{precision}] {k}: max |err| {d.max(initial=0.0):.3e}, share beyond {bar:.0e}: {frac:.4f} "
              f"(allowed {allowed:.4f}), tolerance {tol:.1e}")
        if d.max(initial=0.0) > tol:
            fails.append(f"{name}:{k} max-abs {d.max():.3e} > {tol:.1e}")
        if frac > allowed:
            fails.append(f"{name}:{k} {frac:.4f} of the rays off by more than {bar:.0e} (reference fp32 vs fp64: {allowed:.4f})")
    assert not fails, "\n".join(fails)


def test_the_object_does_not_depend_on_the_scene_precision():
    """set_precision reaches the scene's field only: the object's own maps are bit for bit the same under both."""
    from mirror_nerf_amd import mirror_nerf as MN
    from mirror_nerf_amd.dnerf import render_rays_dnerf
    fx = FX.Fixture("g27_dnerf_office_l2")
    kw = _object_kwargs(fx.meta)
    batch = _dev(fx.inputs["object_batch"][:64])
    old, res = MN.PRECISION, []
    try:
        for mode in ("split", "fp32"):
            MN.set_precision(mode)
            res.append(render_rays_dnerf(batch, **kw))
    finally:
        MN.set_precision(old)
    for k in res[0]:
        assert torch.equal(res[0][k], res[1][k]), k
    # ... and they are the reference's own maps of the object alone, on the bars of the scene comparison
    for k, base in (("rgb_map", 1e-4), ("acc_map", 1e-4), ("depth_map", 8e-4)):
        want64, want32 = fx.outputs[f"object_{k}64"][:64], fx.outputs[f"object_{k}"][:64]
        floor = np.abs(want32.astype(np.float64) - want64).reshape(64, -1).max(1)
        d = np.abs(res[0][k].double().cpu().numpy() - want64).reshape(64, -1).max(1)
        assert d.max() <= max(base, 4.0 * floor.max()), (k, d.max(), floor.max())


# ----------------------------------------------------------------------------------------------------- scripts/eval_scene.py
def _load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_eval_scene_with_a_moving_object(tmp_path):
    """scripts/eval_scene.py end to end on a Blender-layout directory of 2 frames of 8 x 8 under an `office` root with a D-NeRF
    checkpoint (a `.tar` beside its config.txt): frame i is the direct batched_inference call at frame_time = i / 2, the object
    is in the frames, and it is not the same object in frame 1 as it would be at frame 0's time."""
    from PIL import Image
    import mirror_nerf_amd as M
    from mirror_nerf_amd import checkpoint
    from mirror_nerf_amd import synthetic as SY
    from mirror_nerf_amd.data import RayBank
    from mirror_nerf_amd.dnerf import load_dnerf_object
    root = tmp_path / "office"
    (root / "test").mkdir(parents=True)
    rng = np.random.default_rng(0)
    frames_meta = []
    for i, eye in enumerate(((0.0, -4.0, 1.5), (1.0, -3.5, 2.0))):
        Image.fromarray(rng.integers(0, 256, size=(8, 8, 3), dtype=np.uint8)).save(root / "test" / f"r_{i}.png")
        pose = np.eye(4)
        pose[:3, :4] = SY.look_at_pose(eye=eye)
        frames_meta.append({"file_path": f"./test/r_{i}", "transform_matrix": pose.tolist()})
    with open(root / "transforms_test.json", "w") as f:
        json.dump({"camera_angle_x": SY.CAMERA_ANGLE_X, "frames": frames_meta}, f)
    models = SY.build_models(DEV, SY.STRADDLE, seed=0)[0]
    ckpt = tmp_path / "last.ckpt"
    checkpoint.save_ckpt(str(ckpt), SimpleNamespace(nerf_coarse=models["coarse"], nerf_fine=models["fine"]))
    meta = FX.Fixture("g27_dnerf_office_l2").meta
    okw = _object_kwargs(meta)
    obj_dir = tmp_path / "logs" / "object"
    obj_dir.mkdir(parents=True)
    torch.save({"global_step": 1, "network_fn_state_dict": {k: v.cpu() for k, v in okw["network_fn"].state_dict().items()},
                "network_fine_state_dict": {k: v.cpu() for k, v in okw["network_fine"].state_dict().items()}}, str(obj_dir / "000001.tar"))
    (obj_dir / "config.txt").write_text("expname = object\nnerf_type = direct_temporal\nuse_viewdirs = True\nN_samples = 64\n"
                                        "N_importance = 64\nuse_two_models_for_fine = True\n")
    out = tmp_path / "results"
    argv = ["--root_dir", str(root), "--split", "test", "--img_wh", "8", "8", "--ckpt_path", str(ckpt), "--N_samples", "64",
            "--N_importance", "64", "--chunk", "32768", "--trace_secondary_rays", "--near", str(SY.NEAR), "--far", str(SY.FAR),
            "--out_dir", str(out)]
    app = ["--app_reflect_newly_placed_objects", "--obj_ckpt_path", str(obj_dir / "000001.tar"), "--obj_model_type", "d_nerf"]
    ES = _load_script("eval_scene")
    assert ES.main(argv + app) == 0
    args = ES.get_opts(argv + app)
    system = ES.load_system(args, torch.device(DEV))
    obj = load_dnerf_object(str(obj_dir / "000001.tar"), torch.device(DEV))
    bank = RayBank.from_blender(str(root), "test", (8, 8), SY.NEAR, SY.FAR, device=torch.device(DEV))
    changed, moved = 0, 0
    for i in range(2):
        rays = bank.frame(i)["rays"]
        used = torch.zeros(1, dtype=torch.int32, device=DEV)
        call = lambda t, **kw: M.batched_inference(system.models, system.embeddings, rays, 64, 64, False, 32768, args=args,  # noqa: E731
                                                   trace_secondary_rays=True, white_back=False, to_cpu=False, maps_only=True,
                                                   render_kwargs_test_d_nerf=obj, frame_time=t, **kw)
        res = call(i / 2, object_used=used)
        images = M.finish_frame(res, "fine")
        png = np.asarray(Image.open(out / f"rgb_fine_{i:03d}.png"))
        assert png.shape == (8, 8, 3) and (png.reshape(64, 3) == images["rgb_fine"].cpu().numpy()).all()
        assert int(used.item()) > 0
        plain = ES.render(system, rays, ES.get_opts(argv))
        changed += int((plain["rgb_fine"] != res["rgb_fine"]).any(-1).sum().item())
        if i == 1:      # the same camera at frame 0's time: the object's pixels differ
            moved = int((call(0.0)["rgb_fine"] != res["rgb_fine"]).any(-1).sum().item())
    assert changed > 0, "the object is nowhere in the frames"
    assert moved > 0, "the object looks the same at both times"
