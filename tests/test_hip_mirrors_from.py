"""mnrf_place_mirrors_from, mnrf_mirror_sources (csrc/mnrf_mirrors.hip) and batched_inference(exclude_source_mirror=) on the GPU.

The kernels against the float32 numpy restatement (tests/mirrors_from_ref.py; include/mnrf.h), bit for bit: the
tolerance is zero for the reasons tests/test_hip_mirrors.py gives, whose cases, sentinels and G11 pipeline are used here.
End to end: two parallel frame mirrors tilted by 0.3 rad about z that face each other across the camera (the "facing pair").
Without the keyword 94 of the 256 rays reflected off the first re-hit it at a distance of about 4e-9 (tests/test_mirrors_from_cpu.py
counts them); with it every one of them reaches the second mirror, 1.91 or more away."""
import json
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import mirrors_from_ref as MF
from tests import mirrors_ref as MR
from tests import test_hip_mirrors as TM
from tests.test_hip_mirrors import DEV, GUARD_WORD, PAD, SENT_BYTE, SENT_INT, _dev, _padded, _same

pytestmark = pytest.mark.gpu
F = np.float32
NEAR = TM.NEAR
NEAR2 = 0.1


def hip_place_from(c, mirrors, source, near=NEAR, any_in=0, shift=0, entry="from"):
    """One launch on copies of c's arrays with sentinel rows behind.  entry "from": mnrf_place_mirrors_from with `source` (numpy
    int32 or None: the null pointer); "old": mnrf_place_mirrors.  shift: as test_hip_mirrors.hip_place."""
    from mirror_nerf_amd import placed_mirrors as PM
    n = c["rays"].shape[0]
    rays = torch.cat([torch.zeros(shift, device=DEV), _dev(c["rays"]).reshape(-1)])[shift:].view(n, 8)
    t = {k: _dev(_padded(c[k])) for k in ("depth", "mask", "normal", "x_surface")}
    mb = torch.full((n + PAD,), SENT_BYTE, dtype=torch.uint8, device=DEV)
    index = torch.full((n + PAD,), SENT_INT, dtype=torch.int32, device=DEV)
    flag = torch.tensor([GUARD_WORD, any_in, GUARD_WORD], dtype=torch.int32, device=DEV)
    src = None if source is None else _dev(np.asarray(source, np.int32))
    PM._place_mirrors(rays, PM.pack([TM._mirror(m) for m in mirrors]), near, t["depth"], t["mask"], t["normal"], t["x_surface"], mb, flag[1:2], index,
                      src, entry == "from")
    out = {k: v.cpu().numpy() for k, v in t.items()}
    out.update(rays=rays.cpu().numpy(), mask_bool=mb.cpu().numpy(), any=flag.cpu().numpy(), index=index.cpu().numpy())
    return out


def check_from(c, mirrors, source, near=NEAR, any_in=0, tag="", shift=0):
    want = MF.place_mirrors(mirrors=mirrors, near=near, any_in=any_in, source=source, **c)
    got = hip_place_from(c, mirrors, source, near, any_in, shift)
    _same(got["rays"], c["rays"], f"{tag} rays (an input)")
    for k in ("depth", "mask", "normal", "x_surface"):
        _same(got[k], _padded(want[k]), f"{tag} {k}")
    _same(got["mask_bool"], _padded(want["mask_bool"], SENT_BYTE), f"{tag} mask_bool")
    _same(got["index"], _padded(want["index"], SENT_INT), f"{tag} index")
    assert got["any"].tolist() == [GUARD_WORD, want["any"], GUARD_WORD], f"{tag} any: {got['any'].tolist()}"
    if source is not None:
        named = source >= 0
        assert not (got["index"][:len(source)][named] == source[named]).any(), f"{tag}: a ray took the mirror it left"
    return got, want


def draw_source(n, K, seed):
    """-2, -1, every mirror of the list, K and 127: half of the rays name a mirror of the list."""
    rs = np.random.RandomState(seed)
    return np.where(rs.uniform(size=n) < 0.5, rs.randint(0, K, n), rs.choice([-2, -1, K, 127], n)).astype(np.int32)


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("K", TM.COUNTS)
@pytest.mark.parametrize("n", TM.SIZES)
def test_place_mirrors_from_bit_exact(n, K):
    mirrors = TM.mirrors_for(K)
    c = TM.seeded_case(n, mirrors, 7000 + 10 * n + K)
    source = draw_source(n, K, 31 * n + K)
    _, want = check_from(c, mirrors, source, tag=f"n={n} K={K}")
    if n >= 255:
        old = MR.place_mirrors(mirrors=mirrors, near=NEAR, **c)
        lost = (old["index"] == source)
        print(f"n={n} K={K}: {int(lost.sum())} rays name the mirror they would have taken; {int((want['index'][lost] >= 0).sum())} of them take another")
        assert lost.sum() >= 0.03 * n, "the exclusion decides some rays"
        if K == 8:
            assert (want["index"][lost] >= 0).any(), "an excluded winner gives way to the next mirror"


def test_rays_aligned_to_four_bytes_only():
    mirrors = TM.mirrors_for(8)
    c = TM.seeded_case(321, mirrors, 4242)
    source = draw_source(321, 8, 9)
    for shift in (1, 2):
        check_from(c, mirrors, source, shift=shift, tag=f"rays {4 * shift} bytes into a 16-byte line")


def test_an_exact_tie_whose_later_mirror_is_excluded():
    """test_hip_mirrors' edge rows behind seeded ones (the last is the only thread of the second block).  On tie_later_wins mirrors
    1 and 2 lie in one plane: the later one wins; with source = 2 the earlier one does, at the same depth with its own normal."""
    e = TM.edge_rows()
    E = len(TM.EDGE_NAMES)
    s = TM.seeded_case(257 - E, TM.EDGE_MIRRORS, 99)
    c = {k: np.concatenate([s[k], e[k]]) for k in s}
    i = 257 - E + TM.EDGE_NAMES.index("tie_later_wins")
    source = draw_source(257, 4, 17)
    source[i] = 2
    got, want = check_from(c, TM.EDGE_MIRRORS, source, tag="edges")
    old = MR.place_mirrors(mirrors=TM.EDGE_MIRRORS, near=NEAR, **c)
    assert old["index"][i] == 2 and got["index"][i] == 1 and got["depth"][i] == old["depth"][i] == 1.0
    assert got["normal"][i].tolist() == [0.0, 0.0, 1.0] and old["normal"][i].tolist() == [0.0, 0.0, 2.0]
    source[i] = 1                                               # the earlier one excluded: the later one wins as before
    got, _ = check_from(c, TM.EDGE_MIRRORS, source, tag="edges, the earlier excluded")
    assert got["index"][i] == 2 and got["normal"][i].tolist() == [0.0, 0.0, 2.0]


@pytest.mark.parametrize("n,K", [(1, 1), (65, 2), (257, 3), (321, 8)])
def test_a_null_source_is_mnrf_place_mirrors(n, K):
    mirrors = TM.mirrors_for(K)
    c = TM.seeded_case(n, mirrors, 50 + n)
    old = hip_place_from(c, mirrors, None, any_in=4, entry="old")
    got = hip_place_from(c, mirrors, None, any_in=4)
    minus = hip_place_from(c, mirrors, np.full(n, -1, np.int32), any_in=4)
    for k in old:
        _same(got[k], old[k], f"null source, {k}")
        _same(minus[k], old[k], f"source -1 everywhere, {k}")


@pytest.mark.parametrize("n", [257, 321])
def test_the_only_hit_excluded_leaves_the_ray_alone(n):
    """One mirror, named by every ray: no index, no write, the mask as it was, the flag the old mask's alone."""
    mirrors = TM.mirrors_for(1)
    c = TM.seeded_case(n, mirrors, 3)
    for mask in (np.zeros(n, F), c["mask"]):
        case = dict(c, mask=mask)
        got, _ = check_from(case, mirrors, np.zeros(n, np.int32), tag="every ray names the only mirror")
        assert (got["index"][:n] == -1).all() and got["any"][1] == int(mask.any())
        for k in ("depth", "normal", "x_surface"):
            _same(got[k][:n], case[k], k)
        _same(got["mask"][:n], (mask != 0).astype(F), "mask")


# ------------------------------------------------------------------------------------------------ mnrf_mirror_sources
@pytest.mark.parametrize("n_rep", [1, 3])
@pytest.mark.parametrize("m", [0, 1, 64, 65, 257])
def test_mirror_sources(m, n_rep):
    from mirror_nerf_amd import _lib
    rs = np.random.RandomState(m + n_rep)
    N = 2 * m + 3
    level = rs.randint(-1, 8, N).astype(np.int32)
    comp = np.sort(rs.choice(N, m, replace=False)).astype(np.int32)
    for li, ci in ((level, comp), (level, None), (None, comp), (None, None)):
        out = torch.full((n_rep * m + PAD,), SENT_INT, dtype=torch.int32, device=DEV)
        a, b = (None if li is None else _dev(li)), (None if ci is None else _dev(ci))
        _lib.check(_lib.lib().mnrf_mirror_sources(_lib.ptr(a), _lib.ptr(b), m, n_rep, _lib.ptr(out), _lib.stream()), "mnrf_mirror_sources")
        want = MF.mirror_sources(li, ci, m, n_rep)
        _same(out.cpu().numpy(), _padded(want, SENT_INT), f"m={m} n_rep={n_rep} level {'given' if li is not None else 'null'}, compaction "
              f"{'given' if ci is not None else 'null'}")


def test_mirror_sources_wrapper():
    from mirror_nerf_amd import placed_mirrors as PM
    level, comp = np.array([3, -1, 0, 7, -1], np.int32), np.array([4, 0, 3], np.int32)
    got = PM.mirror_sources(_dev(level), _dev(comp), 3, 2)
    assert got.dtype == torch.int32 and got.cpu().tolist() == [-1, 3, 7, -1, 3, 7]
    assert PM.mirror_sources(None, None, 4, 1, torch.device(DEV)).cpu().tolist() == [-1] * 4
    assert PM.mirror_sources(None, None, 0, 1, torch.device(DEV)).shape == (0,)


# ------------------------------------------------------------------------------------------------ batched_inference
def facing_pair(rough2=0.0):
    import mirror_nerf_amd as M
    s, c = np.sin(0.3), np.cos(0.3)
    return [M.PlacedMirror((0, 1, 0.6), (s, -c, 0), (0, 0, 1), (3, 3)), M.PlacedMirror((0, -1, 0.6), (-s, c, 0), (0, 0, 1), (8, 8), roughness=rough2)]


def facing_rays():
    return TM.camera_rays((0.0, 0.0, 0.6), (0.1, 1.0, 0.65))


def _facing(level, on, **kw):
    key = ("from_facing", level, on) + tuple(sorted(kw))
    extra = dict(exclude_source_mirror=True) if on else {}
    return TM._run(key, facing_rays(), args=dict(near=1e9, max_recursive_level=level), chunk=256, new_mirrors=facing_pair(), to_cpu=False,
                   maps_only=True, **extra, **kw)


def _secondary(res, rays, near=0.0):
    return np.concatenate([res["x_surface_fine"], res["reflect_direction"], np.full((len(rays), 1), near, F), rays[:, 7:8]], 1).astype(F)


def test_the_facing_pair_over_two_levels():
    """max_recursive_level = 2, near = 1e9, keyword on.  On the rows that take the first mirror at level 0, depth_fine_reflect -- the
    level-1 depth -- is the restatement's distance of the traced rays [x_surface_fine, reflect_direction] to the SECOND mirror,
    1.9 or more: no ray is reflected off the first mirror twice.  (Without the keyword the self-hit rows return about 4e-9.)"""
    rays = facing_rays()
    got = _facing(2, True)
    rows = got["new_mirror_index"] == 0
    assert rows.sum() >= 200, int(rows.sum())
    first, second = (m.as_dict() for m in facing_pair())
    sec = _secondary(got, rays)
    far, own = MR.intersect(sec, second), MR.intersect(sec, first)
    again = own["inside"] & (own["s"] > 0)
    print(f"{int(rows.sum())} rows take the first mirror; {int(again[rows].sum())} of their reflections meet its plane again, at up to "
          f"{float(own['dist'][rows & again].max()) if (rows & again).any() else 0.0}; smallest depth_fine_reflect {float(got['depth_fine_reflect'][rows].min())}")
    assert again[rows].sum() >= 32, "a condition on the inputs: the old rule would take the first mirror again on these rows"
    assert far["inside"][rows].all() and (far["s"][rows] > 0).all()
    _same(got["depth_fine_reflect"][rows], far["dist"][rows], "depth_fine_reflect on the rows that took the first mirror")
    assert (far["dist"][rows] > 1.9).all()


def test_the_recursion_identity():
    """Run A: the facing pair over three levels.  Run B: two levels on A's restated secondary rays with source_mirror = A's level-0
    index.  B's level 0 is A's level 1: a ray's render does not depend on its batch."""
    rays = facing_rays()
    A = _facing(3, True)
    sec = _secondary(A, rays, NEAR2)
    B = TM._run("from_identity_B", sec, args=dict(near=1e9, max_recursive_level=2), chunk=256, new_mirrors=facing_pair(), to_cpu=False,
                maps_only=True, exclude_source_mirror=True, source_mirror=_dev(A["new_mirror_index"]))
    rows = A["mirror_mask_fine"] != 0
    assert rows.sum() >= 200 and (A["new_mirror_index"][rows] == 0).sum() >= 200
    assert not (B["new_mirror_index"][rows] == A["new_mirror_index"][rows]).any()
    _same(B["rgb_fine"][rows], A["rgb_fine_reflect"][rows], "B's rgb_fine against A's rgb_fine_reflect")
    _same(B["depth_fine"][rows], A["depth_fine_reflect"][rows], "B's depth_fine against A's depth_fine_reflect")
    # ... and without the source the same call is another frame: B's rays start on the first mirror
    plain = TM._run("from_identity_plain", sec, args=dict(near=1e9, max_recursive_level=2), chunk=256, new_mirrors=facing_pair(), to_cpu=False,
                    maps_only=True, exclude_source_mirror=True)
    assert (plain["new_mirror_index"][rows] == 0).sum() >= 32 and (plain["depth_fine"][plain["new_mirror_index"] == 0] < 1e-6).all()


def _same_results(a, b, what):
    assert set(a) == set(b), (what, set(a) ^ set(b))
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def test_anchor_one_level_changes_nothing():
    """max_recursive_level = 1: the list is applied at level 0 alone, where no ray has a source."""
    _same_results(_facing(1, True), _facing(1, False), "the facing pair")
    rays = TM.camera_rays(TM.EYE, TM.TARGET)
    kw = dict(args=dict(max_recursive_level=1), new_mirrors=TM._two_mirrors())
    off = TM._run("from_two_off", rays, **kw)
    on = TM._run("from_two_on", rays, exclude_source_mirror=True, **kw)
    assert {0, 1} <= set(off["new_mirror_index"].tolist()) and "weights_fine" in off
    _same_results(on, off, "two mirrors in front of the camera, the full dict, three chunks")


def test_anchor_world_axis_planes_change_nothing():
    """Two facing axis-aligned mirrors, x = 0.5 and x = -0.5, three levels: the intersection's x is the plane's exactly, so a ray
    that leaves one meets it again at t = 0 with s = 0 -- no hit under either rule."""
    import mirror_nerf_amd as M
    rays = TM.camera_rays((0.0, 0.0, 0.6), (1.0, 0.1, 0.65))
    pair = [M.PlacedMirror.axis_aligned("x", 0.5, (-1, 0, 0), (-1.5, 1.5, -0.9, 2.1)), M.PlacedMirror.axis_aligned("x", -0.5, (1, 0, 0), (-4, 4, -3.4, 4.6))]
    kw = dict(args=dict(near=1e9, max_recursive_level=3), chunk=256, new_mirrors=pair, to_cpu=False, maps_only=True)
    off = TM._run("from_axis_off", rays, **kw)
    on = TM._run("from_axis_on", rays, exclude_source_mirror=True, **kw)
    assert (off["new_mirror_index"] == 0).sum() >= 200 and (off["depth_fine_reflect"][off["new_mirror_index"] == 0] >= 0.999).all()
    _same_results(on, off, "world-axis planes")


def test_anchor_pipelined_and_flat_agree(monkeypatch):
    """Three chunks of 96, 96 and 64 rays with a source_mirror that names the first mirror on every third ray: the rows are sliced
    with the chunks on both routes."""
    rays = facing_rays()
    src = np.where(np.arange(256) % 3 == 0, 0, -1).astype(np.int32)
    kw = dict(args=dict(near=1e9, max_recursive_level=2), chunk=TM.CHUNK, new_mirrors=facing_pair(), exclude_source_mirror=True, source_mirror=_dev(src))
    full = TM._run("from_pipe", rays, **kw)
    monkeypatch.setenv("MNRF_EVAL_PIPELINE", "0")
    flat = TM._run("from_flat", rays, **kw)
    _same_results(flat, full, "MNRF_EVAL_PIPELINE=0")
    assert (full["new_mirror_index"][src == -1] == 0).all() and (full["new_mirror_index"][src == 0] != 0).all()
    rows = full["new_mirror_index"] == 0
    assert (full["depth_fine_reflect"][rows] > 1.9).all()


def test_with_rough_times():
    """The second mirror frosted, T = 2, injected draws, two levels: the routes agree, and the rows that take the first mirror see
    the second one in it."""
    from tests import test_hip_rough_mirrors as TR
    runs = {}
    for batch in (True, False):
        runs[batch] = TR._run(None, rays=facing_rays(), args=dict(near=1e9, max_recursive_level=2), draws=TR._draws(count=6), new_mirrors=facing_pair(0.02),
                              rough_times=2, scene_roughness=0.0, batch_jitter=batch, exclude_source_mirror=True)
    _same_results(runs[True], runs[False], "batch_jitter=True against False")
    rows = runs[True]["new_mirror_index"] == 0
    assert rows.sum() >= 200 and not (runs[True]["depth_fine_reflect"][rows] < 1.9).any()
    polished = _facing(2, True)
    assert (runs[True]["rgb_fine"][rows] != polished["rgb_fine"][rows]).any(), "the frosted mirror is seen at level 1"


# ------------------------------------------------------------------------------------------------ scripts/eval_scene.py
def test_eval_scene_with_the_flag(tmp_path):
    """scripts/eval_scene.py --mirrors_json --exclude_source_mirror --max_recursive_level 2 end to end on a Blender-layout directory of
    one 8 x 8 frame: the frame written is that of the direct batched_inference(new_mirrors=, exclude_source_mirror=True) call."""
    from PIL import Image
    import mirror_nerf_amd as M
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
    tilt = -view + 0.3 * right           # closer to the eye than the scene's first sample: nothing hides the pair
    mirrors = [dict(center=(eye + 0.045 * view).tolist(), normal=tilt.tolist(), up=[0, 0, 1], size=[0.2, 0.2]),
               dict(center=(eye - 0.045 * view).tolist(), normal=(-tilt).tolist(), up=[0, 0, 1], size=[0.6, 0.6])]
    (tmp_path / "mirrors.json").write_text(json.dumps(mirrors))
    out = tmp_path / "results"
    argv = ["--root_dir", str(root), "--split", "test", "--img_wh", "8", "8", "--ckpt_path", str(ckpt), "--N_samples", "64",
            "--N_importance", "64", "--chunk", "32768", "--trace_secondary_rays", "--near", str(SY.NEAR), "--far", str(SY.FAR),
            "--out_dir", str(out), "--mirrors_json", str(tmp_path / "mirrors.json"), "--exclude_source_mirror", "--max_recursive_level", "2"]
    ES = TO._load_script("eval_scene")
    assert ES.main(argv) == 0
    args = ES.get_opts(argv)
    assert args.exclude_source_mirror and args.max_recursive_level == 2
    system = ES.load_system(args, torch.device(DEV))
    rays = RayBank.from_blender(str(root), "test", (8, 8), SY.NEAR, SY.FAR, device=torch.device(DEV)).frame(0)["rays"]
    res = M.batched_inference(system.models, system.embeddings, rays, 64, 64, False, 32768, args=args, trace_secondary_rays=True, white_back=False,
                              to_cpu=False, maps_only=True, new_mirrors=ES.read_mirrors_json(str(tmp_path / "mirrors.json")),
                              exclude_source_mirror=True)
    index = res["new_mirror_index"].cpu().numpy()
    print("winners (none, first, second):", np.bincount(index + 1, minlength=3).tolist())
    assert (index == 0).sum() >= 16
    images = M.finish_frame(dict(res, mirror_mask_fine=res["mirror_mask_fine"].float()), "fine")
    png = np.asarray(Image.open(out / "rgb_fine_000.png"))
    assert png.shape == (8, 8, 3) and (png.reshape(64, 3) == images["rgb_fine"].cpu().numpy()).all()
    with pytest.raises(SystemExit):
        ES.get_opts([a for a in argv if a not in ("--mirrors_json", str(tmp_path / "mirrors.json"))])
