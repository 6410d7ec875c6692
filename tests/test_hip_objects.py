"""GPU tests of app_reflect_newly_placed_objects (eval.py:173-291) with a nerf_pl object: the two per-ray kernels
(mnrf_object_rays, mnrf_object_merge) against numpy, and batched_inference against the fixtures G26 captured from the reference's
own branch (tests/golden/make_golden_objects.py), on both arithmetics of the field kernel.

Bars of the fixture comparison: those of test_hip_apps.test_apps_golden -- FX.tolerance per key, and the share of rays beyond
1e-4 (depth-like keys 8e-4) at most the reference's own fp32-vs-fp64 share (meta.floor_frac).  The kernels are compared with
tolerance zero, except the posed ray move: torch's 3x3 product order is not specified, so that one is held to 2e-6 x max(1, |o|)
of a float64 evaluation (a few fp32 roundings of values of that size)."""
import ctypes
import importlib.util
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.golden import fixtures as FX
from tests.golden import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("rgb_", "depth_", "opacity_", "mirror_mask_", "surface_normal_", "x_surface_")
F32 = np.float32


@pytest.fixture(params=["split", "fp32"])
def precision(request):
    from mirror_nerf_amd import mirror_nerf as MN
    old = MN.PRECISION
    MN.set_precision(request.param)
    yield request.param
    MN.set_precision(old)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ----------------------------------------------------------------------------- mnrf_object_merge
def _merge_inputs(n, scale, ps0, near, seed=0):
    """Rows of every branch, the equalities of every comparison, negative depths and a NaN in each input."""
    rs = np.random.RandomState(seed)
    obj_rgb = rs.uniform(0, 1, (n, 3)).astype(F32)
    obj_depth = rs.uniform(-0.5, 4.0, n).astype(F32)
    obj_opacity = rs.uniform(0.5, 1.0, n).astype(F32)
    rgb = rs.uniform(0, 1, (n, 3)).astype(F32)
    depth = rs.uniform(-0.2, 2.0, n).astype(F32)
    mask = rs.uniform(0, 1, n).astype(F32)
    if n >= 64:
        obj_depth[0:24] = rs.uniform(0.5, 2.0, 24).astype(F32)        # rows 0..15: in front of the scene, the opacity decides
        depth[0:16] = 3.0
        d = (obj_depth / F32(scale)) / F32(ps0)
        obj_opacity[0:8] = F32(0.8)                          # exactly the threshold: not opaque
        obj_opacity[8:16] = np.nextafter(F32(0.8), F32(1))   # one ulp above: opaque
        depth[16:24] = d[16:24]                              # d == depth: not behind the scene
        obj_opacity[16:24] = 0.9
        depth[24:32] = F32(near)                             # depth == near: the scene's depth is not valid, nothing blocks
        obj_depth[24:32] = 3.0
        obj_opacity[24:32] = 0.95
        obj_depth[32:36] = 0.0                               # d == 0: no object
        obj_opacity[32:36] = 1.0
        obj_depth[36:40] = -1.0                              # negative object depth
        obj_opacity[36:40] = 1.0
        depth[40:44] = -0.5                                  # negative scene depth: below near, nothing blocks
        obj_depth[40:44] = 1.0
        obj_opacity[40:44] = 1.0
        obj_depth[44] = np.nan
        obj_opacity[45] = np.nan
        depth[46] = np.nan                                   # NaN scene depth: both comparisons false, the object is taken
        obj_depth[46], obj_opacity[46] = 1.0, 1.0
        obj_rgb[47, 1] = np.nan                              # copied as it is
        obj_depth[47], obj_opacity[47], depth[47] = 0.5, 1.0, 3.0
        rgb[48, 0] = np.nan
        mask[49] = np.nan
    elif n == 1:
        obj_depth[0], obj_opacity[0], depth[0] = 0.5, 0.9, 3.0
    return obj_rgb, obj_depth, obj_opacity, rgb, depth, mask


def _merge_numpy(obj_rgb, obj_depth, obj_opacity, rgb, depth, mask, scale, ps0, near):
    with np.errstate(invalid="ignore"):
        d = (obj_depth / F32(scale)) / F32(ps0)
        use = ((d > 0) & (obj_opacity > F32(0.8))) & ~((d > depth) & (depth > F32(near)))
    rgb, depth = rgb.copy(), depth.copy()
    rgb[use], depth[use] = obj_rgb[use], d[use]
    if mask is not None:
        mask = mask.copy()
        mask[use] = 0
    return rgb, depth, mask, use


@pytest.mark.parametrize("with_mask", [True, False], ids=["mask", "null_mask"])
@pytest.mark.parametrize("scale,ps0", [(2.0, 1.25), (3.0, 0.7), (1.0, 1.0)])
@pytest.mark.parametrize("n", [1000, 1, 0])
def test_object_merge_equals_numpy(n, scale, ps0, with_mask):
    from mirror_nerf_amd import _lib
    near = 0.05
    inp = _merge_inputs(n, scale, ps0, near)
    obj_rgb, obj_depth, obj_opacity, rgb, depth, mask = inp
    w_rgb, w_depth, w_mask, use = _merge_numpy(obj_rgb, obj_depth, obj_opacity, rgb, depth, mask if with_mask else None, scale, ps0, near)
    if n == 1000:
        with np.errstate(invalid="ignore"):
            d = (obj_depth / F32(scale)) / F32(ps0)
            obj = (d > 0) & (obj_opacity > F32(0.8))
            blocked = (d > depth) & (depth > F32(near))
        assert (~obj).sum() > 50 and (obj & blocked).sum() > 50 and use.sum() > 50          # every branch
        assert not use[0:8].any() and use[8:16].all() and use[16:24].all() and use[24:32].all()
        assert not use[32:40].any() and use[40:44].all() and not use[44] and not use[45] and use[46] and use[47]
        if (scale, ps0) == (3.0, 0.7):      # the two divisions are not one division by the product
            assert (d != obj_depth / (F32(scale) * F32(ps0))).any()
    t = [_dev(a) for a in (obj_rgb, obj_depth, obj_opacity, rgb, depth, mask)]
    n_used = torch.zeros(1, dtype=torch.int32, device=DEV)
    p = _lib.ptr
    _lib.check(_lib.lib().mnrf_object_merge(p(t[0]), p(t[1]), p(t[2]), n, scale, ps0, near, p(t[3]), p(t[4]),
                                            p(t[5]) if with_mask else None, p(n_used), _lib.stream()), "mnrf_object_merge")
    torch.cuda.synchronize()
    assert int(n_used.item()) == int(use.sum())
    assert np.array_equal(_bits(t[3].cpu().numpy()), _bits(w_rgb))                 # unused rows bit-untouched, used rows copied
    assert np.array_equal(_bits(t[4].cpu().numpy()), _bits(w_depth))
    assert np.array_equal(_bits(t[5].cpu().numpy()), _bits(w_mask if with_mask else mask))
    for a, src in zip(t[:3], inp[:3]):                                             # the object's maps are read only
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(src))
    # without the counter
    t2 = [_dev(a) for a in (rgb, depth)]
    _lib.check(_lib.lib().mnrf_object_merge(p(t[0]), p(t[1]), p(t[2]), n, scale, ps0, near, p(t2[0]), p(t2[1]), None, None,
                                            _lib.stream()), "mnrf_object_merge")
    assert np.array_equal(_bits(t2[1].cpu().numpy()), _bits(w_depth))


# ----------------------------------------------------------------------------- mnrf_object_rays
def _rays(n, seed=1):
    rs = np.random.RandomState(seed)
    d = rs.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.concatenate([rs.uniform(-4, 4, (n, 3)), d, rs.uniform(0.05, 0.2, (n, 1)), rs.uniform(0.25, 8, (n, 1))], 1)
    return r.astype(F32)


def _object_rays(rays, pose, scale, t):
    from mirror_nerf_amd import _lib
    src = _dev(rays)
    out = torch.full_like(src, -7.0)
    pose_c = (ctypes.c_float * 12)(*np.asarray(pose, F32)[:3, :4].reshape(-1).tolist()) if pose is not None else None
    _lib.check(_lib.lib().mnrf_object_rays(_lib.ptr(src), rays.shape[0], pose_c, scale, t[0], t[1], t[2], _lib.ptr(out),
                                           _lib.stream()), "mnrf_object_rays")
    torch.cuda.synchronize()
    assert np.array_equal(_bits(src.cpu().numpy()), _bits(rays)), "the source rays were written"
    return out.cpu().numpy()


@pytest.mark.parametrize("pose", [None, np.eye(4), np.eye(3, 4)], ids=["no_pose", "identity4x4", "identity3x4"])
def test_object_rays_without_rotation(pose):
    rays = _rays(257)
    scale, t = 2.0, (0.1, 3.0, 0.5)
    got = _object_rays(rays, pose, scale, t)
    want_o = (rays[:, :3] * F32(scale)) + np.asarray(t, F32)          # two roundings
    assert np.array_equal(_bits(got[:, :3]), _bits(want_o))
    assert np.array_equal(_bits(got[:, 6:]), _bits(rays[:, 6:]))
    if pose is None:
        assert np.array_equal(_bits(got[:, 3:6]), _bits(rays[:, 3:6]))
    else:       # l2_normalize of a unit vector: within an fp32 rounding or two of it
        assert np.abs(got[:, 3:6] - rays[:, 3:6]).max() <= 2e-7
    assert np.abs(np.linalg.norm(got[:, 3:6].astype(np.float64), axis=1) - 1).max() <= 1e-6


def test_object_rays_with_a_similarity():
    pose = np.asarray(FX.Fixture("g26_object_posed_l1").meta["new_object"]["pose_align"], F32)
    rays = _rays(257, seed=2)
    scale, t = 2.0, (-0.5, -0.5, 0.0)
    got = _object_rays(rays, pose, scale, t)
    A, p = pose[:3, :3].astype(np.float64), pose[:3, 3].astype(np.float64)
    o = (rays[:, :3].astype(np.float64) @ A.T + p) * scale + np.asarray(t)
    d = rays[:, 3:6].astype(np.float64) @ A.T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    assert (np.abs(got[:, :3] - o) <= 2e-6 * np.maximum(1.0, np.abs(o))).all(), np.abs(got[:, :3] - o).max()
    assert np.abs(got[:, 3:6] - d).max() <= 2e-6
    assert np.abs(np.linalg.norm(got[:, 3:6].astype(np.float64), axis=1) - 1).max() <= 1e-6
    assert np.array_equal(_bits(got[:, 6:]), _bits(rays[:, 6:]))


def test_object_rays_zero_rays_is_a_no_op():
    from mirror_nerf_amd import _lib
    assert _lib.lib().mnrf_object_rays(None, 0, None, 1.0, 0.0, 0.0, 0.0, None, None) == 0
    assert _lib.lib().mnrf_object_merge(None, None, None, 0, 1.0, 1.0, 0.05, None, None, None, None, None) == 0


# ----------------------------------------------------------------------------- batched_inference against the reference
def _module(sd, heads=True):
    import mirror_nerf_amd as M
    m = M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=heads, predict_mirror_mask=heads)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV)


def _emb():
    import mirror_nerf_amd as M
    return {"xyz": M.Embedding(10), "dir": M.Embedding(4)}


def _object_sds(meta, tweaks=None):
    sds = W.make_state_dict(meta["obj_seed"], 2, predict_normal=False, predict_mirror_mask=False)
    for sd, tw, c in zip(sds, tweaks or meta["obj_tweaks"], meta["obj_checksum"]):
        W.apply_tweaks(sd, tw)
        if tweaks is None:
            assert abs(W.checksum(sd) - c) <= 1e-9 * max(1.0, abs(c)), "object weights differ from the fixture's"
    return sds


def _object_system(meta, as_lists=False, tweaks=None):
    mods = [_module(sd, heads=False) for sd in _object_sds(meta, tweaks)]
    if as_lists:      # nerf_pl's own containers
        return SimpleNamespace(models=mods, embeddings=[_emb()["xyz"], _emb()["dir"]])
    return SimpleNamespace(models={"coarse": mods[0], "fine": mods[1]}, embeddings=_emb())


def _run(fx, system_obj="fixture", args=None, chunk=None, **extra):
    import mirror_nerf_amd as M
    m = fx.meta
    sds = fx.state_dicts()
    models = {"coarse": _module(sds[0]), "fine": _module(sds[1])}
    kw = dict(args=args or m["args"], trace_secondary_rays=True)
    if (args or m["args"]).get("app_reflect_newly_placed_objects"):
        kw["system_obj"] = _object_system(m) if isinstance(system_obj, str) else system_obj
        kw["new_object"] = m["new_object"]
    rays = torch.from_numpy(fx.inputs["rays"]).to(DEV)
    out = M.batched_inference(models, _emb(), rays, m["N_samples"], m["N_importance"], False, chunk or m["chunk"], **kw, **extra)
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def _compared(fx):
    return [k for k in fx.outputs if k.startswith(KEYS) or k == "reflect_direction"]


def test_fixtures_exist():
    assert FX.names("g26_object_") == ["g26_object_default_chunk96", "g26_object_office_l2", "g26_object_posed_l1"]


@pytest.mark.parametrize("name", FX.names("g26_object_"))
def test_objects_golden(name, precision):
    fx = FX.Fixture(name)
    got = _run(fx)
    keys = _compared(fx)
    assert {"rgb_fine", "depth_fine", "mirror_mask_fine", "surface_normal_fine", "x_surface_fine", "rgb_fine_reflect",
            "depth_fine_reflect"} <= set(keys), keys
    worst = {}
    for k in keys:
        want = fx.outputs[k]
        assert k in got, f"{name}: missing {k}"
        assert got[k].dtype == want.dtype and got[k].shape == want.shape, (name, k, got[k].dtype, want.dtype, got[k].shape, want.shape)
        g, w = got[k].astype(np.float64), want.astype(np.float64)
        d = np.abs(g - w).reshape(w.shape[0], -1).max(1) if w.size else np.zeros(0)
        worst[k] = float(d.max(initial=0.0))
        bar = 8e-4 if k.startswith(("depth", "x_surface")) else 1e-4
        frac = float((d > bar).mean()) if d.size else 0.0
        print(f"G26 {name} [{precision}] {k}: max |err| {worst[k]:.3e}, share beyond {bar:.0e}: {frac:.4f} "
              f"(allowed {fx.meta['floor_frac'].get(k, 0.0):.4f}), tolerance {FX.tolerance(k, fx.meta):.1e}")
    for k in keys:
        want = fx.outputs[k]
        g, w = got[k].astype(np.float64), want.astype(np.float64)
        d = np.abs(g - w).reshape(w.shape[0], -1).max(1) if w.size else np.zeros(0)
        tol = FX.tolerance(k, fx.meta)
        assert d.max(initial=0.0) <= tol, f"{name}:{k} max-abs {d.max():.3e} > {tol:.1e}"
        bar = 8e-4 if k.startswith(("depth", "x_surface")) else 1e-4
        frac = float((d > bar).mean()) if d.size else 0.0
        allowed = fx.meta["floor_frac"].get(k, 0.0)
        assert frac <= allowed, f"{name}:{k} {frac:.4f} of the rays off by more than {bar:.0e} (reference fp32 vs fp64: {allowed:.4f})"


def test_an_empty_object_changes_nothing(precision):
    """sigma.bias = -1e3: the object is transparent everywhere, so every key equals the call without the application."""
    fx = FX.Fixture("g26_object_office_l2")
    empty = [[["sigma.bias", "set", -1e3]], [["sigma.bias", "set", -1e3]]]
    used = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    on = _run(fx, system_obj=_object_system(fx.meta, tweaks=empty), object_used=used)
    off = _run(fx, args={k: v for k, v in fx.meta["args"].items() if k not in ("app_reflect_newly_placed_objects", "obj_model_type")})
    assert int(used.item()) == 0
    assert set(on) == set(off)
    for k in off:
        assert on[k].dtype == off[k].dtype and np.array_equal(on[k], off[k], equal_nan=True), k


def test_variants_are_bit_identical(precision):
    import mirror_nerf_amd as M
    fx = FX.Fixture("g26_object_office_l2")
    used = torch.zeros(1, dtype=torch.int32, device=DEV)
    base = _run(fx, object_used=used)
    per_level = fx.meta["conditions"]["per_level"]
    print("rays that took the object:", int(used.item()), "reference:", sum(v["used"] for v in per_level.values()))
    assert int(used.item()) > 0
    variants = {
        "to_cpu=False": _run(fx, to_cpu=False),
        "maps_only": _run(fx, maps_only=True),
        'to_cpu="maps"': _run(fx, to_cpu="maps"),
        "chunk<N": _run(fx, chunk=96),
        "lists": _run(fx, system_obj=_object_system(fx.meta, as_lists=True)),
    }
    maps = [k for k in _compared(fx)]
    for what, got in variants.items():
        for k in maps:
            assert k in got, (what, k)
            assert np.array_equal(base[k], got[k], equal_nan=True), (what, k)
    assert M.recursion.resolve_new_object(SimpleNamespace(root_dir="data/office"))["scale"] == fx.meta["new_object"]["scale"]


# ----------------------------------------------------------------------------- scripts/eval_scene.py
def _load_script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_eval_scene_with_an_object(tmp_path):
    """scripts/eval_scene.py end to end on a Blender-layout directory of 2 frames of 8 x 8 under an `office` root, with the
    object's checkpoint in nerf_pl's layout: the frames are those of the direct batched_inference call, and the object is in
    them."""
    from PIL import Image
    import mirror_nerf_amd as M
    from mirror_nerf_amd import checkpoint
    from mirror_nerf_amd import synthetic as SY
    from mirror_nerf_amd.data import RayBank
    from mirror_nerf_amd.recursion import load_object_system
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
    meta = FX.Fixture("g26_object_office_l2").meta
    obj_ckpt = tmp_path / "object.ckpt"
    torch.save({"state_dict": {f"nerf_{n}.{k}": torch.from_numpy(v) for n, sd in zip(("coarse", "fine"), _object_sds(meta))
                               for k, v in sd.items()}}, str(obj_ckpt))
    out = tmp_path / "results"
    argv = ["--root_dir", str(root), "--split", "test", "--img_wh", "8", "8", "--ckpt_path", str(ckpt), "--N_samples", "64",
            "--N_importance", "64", "--chunk", "32768", "--trace_secondary_rays", "--near", str(SY.NEAR), "--far", str(SY.FAR),
            "--out_dir", str(out)]
    app = ["--app_reflect_newly_placed_objects", "--obj_ckpt_path", str(obj_ckpt), "--obj_model_type", "nerf_pl"]
    ES = _load_script("eval_scene")
    assert ES.main(argv + app) == 0
    # the same frames by hand
    args = ES.get_opts(argv + app)
    system = ES.load_system(args, torch.device(DEV))
    system_obj = load_object_system(str(obj_ckpt), torch.device(DEV), 64)
    bank = RayBank.from_blender(str(root), "test", (8, 8), SY.NEAR, SY.FAR, device=torch.device(DEV))
    changed = 0
    for i in range(2):
        rays = bank.frame(i)["rays"]
        used = torch.zeros(1, dtype=torch.int32, device=DEV)
        res = M.batched_inference(system.models, system.embeddings, rays, 64, 64, False, 32768, args=args, trace_secondary_rays=True,
                                  white_back=False, to_cpu=False, maps_only=True, system_obj=system_obj, object_used=used)
        images = M.finish_frame(res, "fine")
        png = np.asarray(Image.open(out / f"rgb_fine_{i:03d}.png"))
        assert png.shape == (8, 8, 3) and (png.reshape(64, 3) == images["rgb_fine"].cpu().numpy()).all()
        png = np.asarray(Image.open(out / "depth" / f"depth_fine_{i:03d}.png"))
        assert (png.reshape(64, 3) == images["depth_fine"].cpu().numpy()).all()
        plain = ES.render(system, rays, ES.get_opts(argv))
        changed += int((plain["rgb_fine"] != res["rgb_fine"]).any(-1).sum().item())
        assert int(used.item()) > 0
    assert changed > 0, "the object is nowhere in the frames"
