"""A roughness per placed mirror end to end (batched_inference rough_times=, scene_roughness=, PlacedMirror(roughness=); include/mnrf.h
"A roughness per mirror"), with injected draws and T = 2: the mean is over three samples and does not end in a
power of two.

The anchor carries the pin of tests/test_hip_rough.py over: with one std on every mirror ray the new route gives the result of
args.app_control_mirror_roughness, every key torch.equal.  The other tests run on the trained G11 pair with a tilted rectangle
and an ellipse placed in front of a camera that also sees the scene's own mirror; checked with the CPU oracle and
tests/mirrors_ref.py at near = 0.05, of its 256 rays 60 take the rectangle, 34 the ellipse, 85 only the scene's mirror and 77
none, and no soft mask value lies within 0.18 of the threshold.  Every comparison is bit for bit."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import rough_ref as RR
from tests import rough_rows_ref as RW

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
T = 2
NEAR2 = 0.1               # recursion.RAY_FORWARD_OFFSET
EYE, TARGET = np.array((-0.6, -1.2, 1.0)), np.array((-0.3, 1.2, 0.9))
ROUGH_RECT, ROUGH_SCENE = 0.03, 0.01


def _M():
    import mirror_nerf_amd as M
    return M


def _TM():
    from tests import test_hip_mirrors as TM
    return TM


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32}[a.dtype.itemsize])


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, f"{what}: {len(bad)} entries differ, the first at {bad[0].tolist()}: got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}"


def _same_results(a, b, what, skip=()):
    assert set(a) == set(b), (what, set(a) ^ set(b))
    for k in a:
        if k not in skip:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True), (what, k)


# ------------------------------------------------------------------------------------------------ 1: the anchor
@pytest.mark.parametrize("precision", ["split", "fp32"])
@pytest.mark.parametrize("chunk", [96, 32])
def test_anchor_one_std_everywhere_is_the_uniform_route(chunk, precision):
    """Fixture g7_eval_l1 (STRADDLE, 39 of 96 mirror rays): rough_times=2, scene_roughness=0.01 alone against
    args.app_control_mirror_roughness with trace_ray_times=2, normal_noise_std=0.01, on both routes of the driver."""
    from mirror_nerf_amd import mirror_nerf as MN
    from tests import test_hip_rough as TR
    old = MN.PRECISION
    MN.set_precision(precision)
    try:
        g = TR._g7()
        models = {"coarse": TR._module(g["sds"][0]), "fine": TR._module(g["sds"][1])}
        rays = torch.from_numpy(g["rays"]).to(DEV)
        draws = TR._draws(96, chunk, T + 1)
        off = {k: v for k, v in g["args"].items() if k not in ("app_control_mirror_roughness", "trace_ray_times", "normal_noise_std")}
        for batch in (True, False):
            want = TR._run(models, rays, chunk, dict(g["args"], trace_ray_times=T, normal_noise_std=0.01), draws, batch_jitter=batch)
            got = TR._run(models, rays, chunk, off, draws, batch_jitter=batch, rough_times=T, scene_roughness=0.01)
            assert int((got["mirror_mask_fine"] != 0).sum()) == 39 and set(got) == set(want)
            for k in want:
                assert torch.equal(got[k], want[k]), (k, batch)
    finally:
        MN.set_precision(old)


# ------------------------------------------------------------------------------------------------ 2: the camera
def _frame():
    """The view's unit direction f and r = normalize(cross(f, z))."""
    f = (TARGET - EYE) / np.linalg.norm(TARGET - EYE)
    r = np.cross(f, (0.0, 0.0, 1.0))
    return f, r / np.linalg.norm(r)


def _mirrors(rect=ROUGH_RECT, ellipse=0.0, sign=1.0):
    """The tilted rectangle (index 0) and the ellipse (index 1) in front of the camera, or (sign = -1) mirrored through the eye:
    behind it."""
    M = _M()
    f, r = _frame()
    a = M.PlacedMirror(EYE + sign * (0.6 * f - 0.22 * r + np.array((0, 0, 0.05))), sign * (-f + 0.3 * r + np.array((0, 0, 0.17))), (0, 0, 1),
                       (0.22, 0.4), roughness=rect)
    b = M.PlacedMirror(EYE + sign * (0.5 * f + 0.2 * r - np.array((0, 0, 0.05))), sign * (-f - 0.3 * r + np.array((0, 0, 0.1))), (0, 0.2, 1),
                       (0.2, 0.3), shape="ellipse", roughness=ellipse)
    return [a, b]


_CACHE = {}


def _rays():
    if "rays" not in _CACHE:
        _CACHE["rays"] = _TM().camera_rays(tuple(EYE), tuple(TARGET))
    return _CACHE["rays"]


def _draws(n=256, count=T + 1, seed=11):
    rs = np.random.RandomState(seed)
    return [rs.normal(size=(n, 3)).astype(F) for _ in range(count)]


def _run(key, rays=None, args=None, draws=None, chunk=256, **kw):
    """batched_inference on the G11 pair -> numpy maps (to_cpu=False, maps_only=True); cached under `key` (None: not cached)."""
    P = _TM()._pipe()
    if key is None or key not in _CACHE:
        noise = None if draws is None else [torch.from_numpy(d) for d in draws]
        out = _M().batched_inference(P.models, P.emb, torch.from_numpy(np.ascontiguousarray(_rays() if rays is None else rays)).to(DEV), 64, 64,
                                     False, chunk, args=dict(P.args, **(args or {})), trace_secondary_rays=True, to_cpu=False, maps_only=True,
                                     _normal_noise=noise, **kw)
        out = {k: v.detach().cpu().numpy() for k, v in out.items()}
        if key is None:
            return out
        _CACHE[key] = out
    return _CACHE[key]


def _main(batch=True):
    """The frame of tests 4, 5 and 7: rectangle 0.03, ellipse polished, the scene's own mirror 0.01, one bounce."""
    return _run(("main", batch), draws=_draws(), new_mirrors=_mirrors(), rough_times=T, scene_roughness=ROUGH_SCENE, batch_jitter=batch)


def _populations(res):
    index, mask = res["new_mirror_index"], res["mirror_mask_fine"] != 0
    return dict(rect=index == 0, ellipse=index == 1, scene=(index == -1) & mask, none=(index == -1) & ~mask)


def test_the_camera_sees_all_four_populations():
    got = _main()
    pops = {k: int(v.sum()) for k, v in _populations(got).items()}
    print("rays that take the rectangle, the ellipse, only the scene's own mirror, no mirror:", pops)
    assert min(pops.values()) >= 16 and sum(pops.values()) == 256, pops
    assert got["mirror_mask_fine"].dtype == np.bool_ and got["new_mirror_index"].dtype == np.int32


# ------------------------------------------------------------------------------------------------ 3: mirrors behind the camera
def test_mirrors_behind_the_camera_change_nothing():
    alone = _run("alone", draws=_draws(), rough_times=T, scene_roughness=ROUGH_SCENE, batch_jitter=True)
    behind = dict(_run("behind", draws=_draws(), new_mirrors=_mirrors(0.03, 0.02, sign=-1.0), rough_times=T, scene_roughness=ROUGH_SCENE,
                       batch_jitter=True))
    assert (behind.pop("new_mirror_index") == -1).all()
    mask = behind["mirror_mask_fine"]
    assert mask.dtype == np.bool_ and np.array_equal(mask, alone["mirror_mask_fine"] != 0) and 16 <= int(mask.sum()) <= 240
    _same_results(behind, alone, "mirrors behind the camera", skip=("mirror_mask_fine",))     # (the merged mask is returned as torch.bool)
    # and the scene's own mirror is frosted: its rows are not those of the polished frame
    off = _run("off")
    assert not np.array_equal(alone["rgb_fine_reflect"][mask], off["rgb_fine_reflect"][mask])


# ------------------------------------------------------------------------------------------------ 4: the std per mirror
def _std_rows(res, rough=(ROUGH_RECT, 0.0), scene=ROUGH_SCENE):
    return RW.rough_rows_ref(res["new_mirror_index"], (res["mirror_mask_fine"] != 0).astype(F), rough, scene)


def test_std_per_mirror_at_level_0():
    got, rays, draw0 = _main(), _rays(), _draws()[0]
    rows = _std_rows(got)
    pops = _populations(got)
    assert (rows["std_rows"][pops["rect"]] == F(ROUGH_RECT)).all() and (rows["std_rows"][pops["ellipse"]] == 0).all()
    assert (rows["std_rows"][pops["scene"] | pops["none"]] == F(ROUGH_SCENE)).all()
    want = RW.first_reflection_ref(got["surface_normal_fine"], draw0, rows["std_rows"], rays[:, 3:6])
    _same(got["reflect_direction"], want, "reflect_direction on all 256 rows")
    # the ellipse's rows: the polished frame's bits; the others moved
    off = _run("off_mirrors", new_mirrors=_mirrors(0.0, 0.0))
    _same(got["reflect_direction"][pops["ellipse"]], off["reflect_direction"][pops["ellipse"]], "the ellipse is polished")
    assert (got["reflect_direction"][pops["rect"]] != off["reflect_direction"][pops["rect"]]).any(axis=1).all()


# ------------------------------------------------------------------------------------------------ 5, 9: the mean, no oracle in between
def _check_mean(got, draws, **objects):
    """rgb_fine_reflect against mnrf_jitter_mean's restatement over the colours batched_inference itself gives for the restated
    secondary rays of draws 0..T (roughness off, max_recursive_level = 0, the same placed objects)."""
    rays = _rays()
    rows = _std_rows(got)
    J = np.nonzero(rows["jitter_mask"])[0].astype(np.int32)
    pops = _populations(got)
    assert np.array_equal(rows["jitter_mask"] != 0, pops["rect"] | pops["scene"]) and J.size >= 32
    normal, xs = got["surface_normal_fine"], got["x_surface_fine"]
    sec0 = np.concatenate([xs, RW.first_reflection_ref(normal, draws[0], rows["std_rows"], rays[:, 3:6]), np.full((256, 1), NEAR2, F), rays[:, 7:8]], 1).astype(F)
    fan = RW.reflect_jitter_fan_rows_ref(rays, xs, normal, np.stack(draws[1:]), rows["std_rows"], J, NEAR2)
    colours = _run(None, rays=np.concatenate([sec0, fan]), args=dict(max_recursive_level=0, **objects.pop("args", {})), chunk=256 + T * J.size,
                   **objects)["rgb_fine"]
    want = RR.jitter_mean_ref(colours[:256], colours[256:].reshape(T, J.size, 3), J, RR.DEVICE_FINISH, RR.finish_value(T))
    _same(got["rgb_fine_reflect"], want, "rgb_fine_reflect")
    single = pops["ellipse"] | pops["none"]
    _same(got["rgb_fine_reflect"][single], colours[:256][single], "a polished mirror and a ray that is no mirror keep the sample of draw 0")
    assert (got["rgb_fine_reflect"][J] != colours[:256][J]).any(axis=1).sum() >= J.size // 2


def test_the_mean_over_the_rows_of_J():
    _check_mean(_main(), _draws())


# ------------------------------------------------------------------------------------------------ 6: all polished
def test_all_polished_is_the_call_without_rough_times():
    plain = _run("off_mirrors", new_mirrors=_mirrors(0.0, 0.0))
    got = _run(None, draws=_draws(), new_mirrors=_mirrors(0.0, 0.0), rough_times=T, scene_roughness=0.0)
    _same_results(got, plain, "every roughness 0")
    assert {"rgb_fine", "rgb_fine_reflect", "depth_fine_reflect", "reflect_direction", "new_mirror_index"} <= set(got)
    off = _run("off")
    _same_results(_run(None, draws=_draws(), rough_times=T), off, "no mirror placed, scene_roughness 0")


# ------------------------------------------------------------------------------------------------ 7: both routes
def test_both_routes_are_equal_on_every_key():
    _same_results(_main(True), _main(False), "batch_jitter=True against False")


# ------------------------------------------------------------------------------------------------ 8: two levels
def test_two_levels_take_the_std_of_the_mirror_met_at_that_level():
    """The two facing mirrors of test_two_facing_mirrors_over_two_levels: on the rows that take the first (polished) mirror at
    level 0 every reflected ray meets the second at level 1, so its roughness -- not scene_roughness -- is the std there."""
    M, TM = _M(), _TM()
    rays = TM.camera_rays((0.0, 0.0, 0.6), (0.1, 1.0, 0.65))
    first = dict(center=(0.0, 1.0, 0.6), normal=(0.0, -1.0, 0.0), up=(0, 0, 1), size=(3.0, 3.0))
    second = dict(center=(0.0, -1.0, 0.6), normal=(0.0, 1.0, 0.0), up=(0, 0, 1), size=(8.0, 8.0))
    runs = {}
    for name, rough2, scene in (("X", 0.02, 0.005), ("Y", 0.02, 0.02), ("Z", 0.0, 0.005)):
        torch.manual_seed(3)                               # the draws of X and Y have the same shapes in the same order: the same values
        runs[name] = _run(None, rays=rays, args=dict(near=1e9, max_recursive_level=2), rough_times=T, scene_roughness=scene,
                          new_mirrors=[M.PlacedMirror(**first), M.PlacedMirror(**second, roughness=rough2)])
    X, Y, Z = runs["X"], runs["Y"], runs["Z"]
    rows = X["new_mirror_index"] == 0
    assert rows.sum() >= 200 and np.array_equal(X["new_mirror_index"], Y["new_mirror_index"])
    for k in ("rgb_fine", "rgb_fine_reflect", "depth_fine_reflect", "reflect_direction"):
        _same(X[k][rows], Y[k][rows], f"{k} on the rows that took the first mirror")
    _same(X["reflect_direction"][rows], Z["reflect_direction"][rows], "level 0 is polished on those rows")
    assert (X["rgb_fine"][rows] != Z["rgb_fine"][rows]).any(axis=1).sum() >= rows.sum() // 2
    assert (Y["rgb_fine"][rows] != Z["rgb_fine"][rows]).any(axis=1).sum() >= rows.sum() // 2


# ------------------------------------------------------------------------------------------------ 9: objects
def test_objects_are_in_every_render():
    P = _TM()._pipe()
    obj = _TM()._object(P)
    on = dict(app_reflect_newly_placed_objects=True)
    used = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = _run(None, args=on, draws=_draws(), placed_objects=[obj], object_used=used, new_mirrors=_mirrors(), rough_times=T,
               scene_roughness=ROUGH_SCENE, batch_jitter=True)
    n_used = int(used.item())
    without = _main()
    print(f"rays that took the object, over all renders: {n_used}")
    assert n_used > 0 and (got["rgb_fine"] != without["rgb_fine"]).any()
    _check_mean(got, _draws(), args=on, placed_objects=[obj])


# ------------------------------------------------------------------------------------------------ 10: count reads
def test_at_most_two_compactions_per_chunk_and_level_whatever_T_is(monkeypatch):
    from mirror_nerf_amd import recursion as R
    calls = []
    reflect = R._reflect

    def counting(rays_, x, n, mask, compact, *a, **k):
        calls.append(bool(compact))
        return reflect(rays_, x, n, mask, compact, *a, **k)

    monkeypatch.setattr(R, "_reflect", counting)
    seen = {}
    for times in (2, 5):
        # one bounce, three chunks of level 0: per chunk that traces, its first reflection (not compacted) and J's compaction
        calls.clear()
        torch.manual_seed(0)
        _run(None, chunk=96, new_mirrors=_mirrors(), rough_times=times, scene_roughness=ROUGH_SCENE)
        traced = len(calls) - sum(calls)
        assert 2 <= traced <= 3 and 1 <= sum(calls) <= 2 * traced, (times, calls)
        seen[times, "chunks"] = list(calls)
        # two bounces, one chunk: level 0 as above; level 1 is entered twice (R and one group of jitters), each with the mask's
        # compaction and J's
        calls.clear()
        torch.manual_seed(0)
        _run(None, args=dict(max_recursive_level=2), new_mirrors=_mirrors(), rough_times=times, scene_roughness=ROUGH_SCENE)
        assert len(calls) - sum(calls) == 1 and sum(calls) <= 2 + 2 * 2, (times, calls)
        seen[times, "levels"] = list(calls)
    assert seen[2, "chunks"] == seen[5, "chunks"] and seen[2, "levels"] == seen[5, "levels"], seen


# ------------------------------------------------------------------------------------------------ 11: scripts/eval_scene.py
def test_eval_scene_with_a_frosted_mirror(tmp_path):
    """scripts/eval_scene.py --mirrors_json (an entry with "roughness") --rough_times 2 --scene_roughness on a Blender-layout
    directory of one 8 x 8 frame writes its frames; the direct call with the file's mirrors has rays on the frosted mirror."""
    import json
    from PIL import Image
    from mirror_nerf_amd import checkpoint
    from mirror_nerf_amd import synthetic as SY
    from mirror_nerf_amd.data import RayBank
    from tests import test_hip_objects as TO
    root = tmp_path / "office"
    (root / "test").mkdir(parents=True)
    rng = np.random.default_rng(0)
    Image.fromarray(rng.integers(0, 256, size=(8, 8, 3), dtype=np.uint8)).save(root / "test" / "r_0.png")
    eye = np.array((0.0, -4.0, 1.5))
    pose = np.eye(4)
    pose[:3, :4] = SY.look_at_pose(eye=tuple(eye))
    (root / "transforms_test.json").write_text(json.dumps({"camera_angle_x": SY.CAMERA_ANGLE_X,
                                                           "frames": [{"file_path": "./test/r_0", "transform_matrix": pose.tolist()}]}))
    models = SY.build_models(DEV, SY.STRADDLE, seed=0)[0]
    ckpt = tmp_path / "last.ckpt"
    checkpoint.save_ckpt(str(ckpt), SimpleNamespace(nerf_coarse=models["coarse"], nerf_fine=models["fine"]))
    view = -eye / np.linalg.norm(eye)
    right = np.cross(view, (0, 0, 1.0))
    right /= np.linalg.norm(right)
    mirrors = [dict(center=(eye + 0.045 * view).tolist(), normal=(-view).tolist(), up=[0, 0, 1], size=[0.2, 0.2], roughness=0.05),
               dict(center=(eye + 0.03 * view + 0.02 * right).tolist(), normal=(-view + 0.2 * right).tolist(), up=[0, 0, 1], size=[0.04, 0.2], shape="ellipse")]
    (tmp_path / "mirrors.json").write_text(json.dumps(mirrors))
    out = tmp_path / "results"
    argv = ["--root_dir", str(root), "--split", "test", "--img_wh", "8", "8", "--ckpt_path", str(ckpt), "--N_samples", "64",
            "--N_importance", "64", "--chunk", "32768", "--trace_secondary_rays", "--near", str(SY.NEAR), "--far", str(SY.FAR),
            "--out_dir", str(out), "--mirrors_json", str(tmp_path / "mirrors.json"), "--rough_times", "2", "--scene_roughness", "0.01"]
    ES = TO._load_script("eval_scene")
    assert ES.main(argv) == 0
    for path in (out / "rgb_fine_000.png", out / "mirror_mask" / "mirror_mask_fine_000.png"):
        assert np.asarray(Image.open(path)).shape == (8, 8, 3), path
    args = ES.get_opts(argv)
    placed = ES.read_mirrors_json(args.mirrors_json)
    assert [m.roughness for m in placed] == [float(F(0.05)), 0.0]
    system = ES.load_system(args, torch.device(DEV))
    rays = RayBank.from_blender(str(root), "test", (8, 8), SY.NEAR, SY.FAR, device=torch.device(DEV)).frame(0)["rays"]
    res = ES.render(system, rays, args, mirrors=placed)
    polished = ES.render(system, rays, ES.get_opts(argv[:-4]), mirrors=[_M().PlacedMirror(**{k: v for k, v in mirrors[0].items() if k != "roughness"}), placed[1]])
    index = res["new_mirror_index"].cpu().numpy()
    print("winners (none, first, second):", np.bincount(index + 1, minlength=3).tolist())
    assert {0, 1} <= set(index.tolist())
    assert not torch.equal(res["rgb_fine"], polished["rgb_fine"])
