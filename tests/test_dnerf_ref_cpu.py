"""CPU-side checks of the D-NeRF object (mirror_nerf_amd/dnerf.py): the float64 restatement the GPU tests hold the kernel to
(tests/dnerf_ref.py) against values captured from the reference itself (fixtures G27: the module's forward, and the object's
maps on the level-0 rays of every scene case), the module's names and seeded weights, the new refusals of batched_inference,
the `config.txt` reader, a checkpoint round trip in D-NeRF's layout, argument validation of the new C entry points without a
GPU, and a round trip of one fixture through its generator (skipped where the reference tree is absent)."""
import json
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import dnerf_ref as DR
from tests.golden import fixtures as FX
from tests.golden import weights as W

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
SCENES = ["g27_dnerf_office_canonical_l2", "g27_dnerf_office_l2", "g27_dnerf_single_posed_l1"]


def test_fixture_files_exist_and_are_small():
    assert FX.names("g27_dnerf_") == sorted(SCENES + ["g27_dnerf_model"])
    src = open(os.path.join(GOLDEN, "make_golden_dnerf.py")).read()
    for name in FX.names("g27_dnerf_"):
        assert name in src and os.path.getsize(os.path.join(GOLDEN, name + ".npz")) < 400 * 1024


def test_fixture_conditions():
    """What the generator asserted, as stored (the conditions of G26), and what the three cases are about."""
    for name in SCENES:
        m = FX.Fixture(name).meta
        c = m["conditions"]
        n = c["per_level"]["0"]["rays"]
        assert n == c["candidates"] - c["dropped"] and c["dropped"] <= 0.05 * c["candidates"]
        for k in ("transparent", "blocked", "used"):
            assert c["per_level"]["0"][k] >= 0.15 * n, (name, k)
        assert c["per_level"]["1"]["used"] > 0
        assert m["args"]["obj_model_type"] == "d_nerf"
        two = m["obj_config"]["use_two_models_for_fine"]
        assert len(m["obj_tweaks"]) == len(m["obj_checksum"]) == (2 if two else 1)
        # the deformation gain stays at 1: only the density head is touched
        assert all(t[0].startswith("_occ.alpha_linear.") for tw in m["obj_tweaks"] for t in tw)
    a, b, c = (FX.Fixture(n).meta for n in SCENES)
    assert a["frame_time"] == 0.0 and b["frame_time"] == 0.37 and c["frame_time"] == 0.37
    assert a["args"]["max_recursive_level"] == b["args"]["max_recursive_level"] == 2 and c["args"]["max_recursive_level"] == 1
    assert a["obj_config"]["use_two_models_for_fine"] and b["obj_config"]["use_two_models_for_fine"]
    assert not c["obj_config"]["use_two_models_for_fine"]
    pose = np.asarray(c["new_object"]["pose_align"])
    assert abs(np.linalg.norm(pose[:3, 0]) - 1.25) < 1e-5 and abs(pose[0, 1]) > 0.1


def test_module_mirrors_reference_names_and_seeded_weights():
    from mirror_nerf_amd import dnerf as DN
    fx = FX.Fixture("g27_dnerf_model")
    sd = DR.make_state_dicts(fx.meta["seed"], 1)[0]
    assert list(sd) == DN.PARAM_NAMES and len(sd) == 42
    for k, v in sd.items():
        assert tuple(v.shape) == DN.PARAM_SHAPES[k], k
    assert sd["_time.0.weight"].shape == (256, 84) and sd["_time.5.weight"].shape == (256, 319)
    assert sd["_occ.pts_linears.5.weight"].shape == (256, 319) and sd["_occ.pts_linears.4.weight"].shape == (256, 256)
    # the generator checked that the reference's class under this seed gives these very arrays, and stored their digest
    W.apply_tweaks(sd, fx.meta["tweaks"])
    assert abs(W.checksum(sd) - fx.meta["checksum"][0]) <= 1e-9 * max(1.0, abs(fx.meta["checksum"][0]))
    for bad in (dict(D=6), dict(W=128), dict(input_ch=39), dict(input_ch_views=15), dict(input_ch_time=13), dict(skips=[3]),
                dict(use_viewdirs=False)):
        with pytest.raises(NotImplementedError, match="D=8, W=256"):
            DN.DirectTemporalNeRF(**bad)
    m = DN.DirectTemporalNeRF(zero_canonical=False)
    assert m.zero_canonical is False and [n for n, _ in m.named_children()] == ["_occ", "_time", "_time_out"]


@pytest.mark.parametrize("tag", ["t037", "t0"])
def test_restatement_matches_the_reference_module(tag):
    """float64 against float64: the same operations, so only the order of the sums inside the matrix products may differ."""
    fx = FX.Fixture("g27_dnerf_model")
    sd = DR.make_state_dicts(fx.meta["seed"], 1)[0]
    W.apply_tweaks(sd, fx.meta["tweaks"])
    t = fx.meta["times"][tag]
    raw, dx = DR.field(sd, torch.from_numpy(fx.inputs["xyz"]).double(), torch.from_numpy(fx.inputs["viewdirs"]).double(), t)
    want_raw, want_dx = fx.outputs[f"raw64_{tag}"], fx.outputs[f"dx64_{tag}"]
    assert np.abs(raw.numpy() - want_raw).max() <= 1e-10 * max(1.0, np.abs(want_raw).max())
    assert np.abs(dx.numpy() - want_dx).max() <= 1e-12
    if t == 0.0:
        assert not want_dx.any() and not fx.outputs["dx_t0"].any()
    else:
        assert 0.05 < np.abs(want_dx).max() < 0.5          # the deformation is neither absent nor wild
    # ... and the stored floors are what the stored captures say
    for key, a, b in (("dx", fx.outputs[f"dx_{tag}"], want_dx), ("rgb", fx.outputs[f"raw_{tag}"][:, :3], want_raw[:, :3]),
                      ("alpha", fx.outputs[f"raw_{tag}"][:, 3], want_raw[:, 3])):
        scale = max(1.0, float(np.abs(b).max()))
        assert fx.meta["floor"][f"{key}_{tag}"] == pytest.approx(float(np.abs(a.astype(np.float64) - b).max()) / scale, rel=1e-12, abs=1e-300)


@pytest.mark.parametrize("tag", ["t037", "t0"])
def test_field_is_the_composition_of_its_two_networks(tag):
    """field() = canonical() at x + deformation(): the two halves that the GPU tests hold the kernel's two stages to, composed by
    hand, give the bits field() gives and with them the committed G27 values on the bars of the test above."""
    fx = FX.Fixture("g27_dnerf_model")
    sd = DR.make_state_dicts(fx.meta["seed"], 1)[0]
    W.apply_tweaks(sd, fx.meta["tweaks"])
    t = fx.meta["times"][tag]
    xyz, view = torch.from_numpy(fx.inputs["xyz"]).double(), torch.from_numpy(fx.inputs["viewdirs"]).double()
    dx = DR.deformation(sd, xyz, t)
    assert dx.shape == xyz.shape and dx.dtype == torch.float64
    if t == 0.0:
        # the canonical frame: the deformation net is not asked, though it would answer
        raw, want_dx = DR.canonical(sd, xyz, view), torch.zeros_like(xyz)
        assert float(dx.abs().max()) > 0.01
        moved, moved_dx = DR.field(sd, xyz, view, t, zero_canonical=False)
        assert torch.equal(moved_dx, dx) and torch.equal(moved, DR.canonical(sd, xyz + dx, view))
    else:
        raw, want_dx = DR.canonical(sd, xyz + dx, view), dx
    got_raw, got_dx = DR.field(sd, xyz, view, t)
    assert torch.equal(got_raw, raw) and torch.equal(got_dx, want_dx)
    want_raw = fx.outputs[f"raw64_{tag}"]
    assert np.abs(raw.numpy() - want_raw).max() <= 1e-10 * max(1.0, np.abs(want_raw).max())
    assert np.abs(want_dx.numpy() - fx.outputs[f"dx64_{tag}"]).max() <= 1e-12
    # float32 in, float32 out: the restatement's own fp32 run is what the kernel's bars are taken from
    raw32, dx32 = DR.field(sd, xyz.float(), view.float(), t)
    assert raw32.dtype == torch.float32 and dx32.dtype == torch.float32
    floor = fx.meta["floor"]
    scale = max(1.0, float(np.abs(want_raw[:, 3]).max()))
    assert np.abs(raw32.numpy()[:, 3] - want_raw[:, 3]).max() <= 4.0 * floor[f"alpha_{tag}"] * scale


def object_state_dicts(meta):
    sds = DR.make_state_dicts(meta["obj_seed"], len(meta["obj_tweaks"]))
    for sd, tw, c in zip(sds, meta["obj_tweaks"], meta["obj_checksum"]):
        W.apply_tweaks(sd, tw)
        assert abs(W.checksum(sd) - c) <= 1e-9 * max(1.0, abs(c))
    return sds


@pytest.mark.parametrize("name", SCENES)
def test_restatement_matches_the_reference_renderer(name):
    """The object alone on the first rays of a scene case, float64 against the reference's float64 render_rays."""
    fx = FX.Fixture(name)
    sds = object_state_dicts(fx.meta)
    cfg = fx.meta["obj_config"]
    n = 48
    batch = torch.from_numpy(fx.inputs["object_batch"][:n]).double()
    got = DR.render(sds[0], sds[1] if cfg["use_two_models_for_fine"] else None, batch, cfg["N_samples"], cfg["N_importance"],
                    cfg["white_bkgd"], cfg["lindisp"])
    for k in ("rgb_map", "depth_map", "acc_map", "disp_map"):
        want = fx.outputs[f"object_{k}64"][:n]
        scale = max(1.0, float(np.abs(want).max()))
        assert np.abs(got[k].numpy() - want).max() <= 1e-8 * scale, k
    assert got["position_delta"].shape == (n, cfg["N_samples"] + cfg["N_importance"], 3)
    assert bool(got["position_delta"].any()) == (fx.meta["frame_time"] != 0.0)


# ----------------------------------------------------------------------------------------------------------- refusals
def _models():
    import mirror_nerf_amd as M
    make = lambda: M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=True)  # noqa: E731
    return {"coarse": make(), "fine": make()}


def _args(**over):
    a = dict(predict_normal=True, only_one_field=False, only_one_field_fine_epoch=2, max_recursive_level=1, near=0.05,
             root_dir="office", app_reflect_newly_placed_objects=True, obj_model_type="d_nerf")
    a.update(over)
    return a


KW = {"render_kwargs_test_d_nerf": {"network_fn": None}}


@pytest.mark.parametrize("args,kw,n_imp,exc,msg", [
    (_args(), KW, 64, ValueError, "needs frame_time="),
    (_args(), dict(KW, frame_time=None, args_d_nerf=object()), 64, ValueError, "needs frame_time="),
    ({k: v for k, v in _args().items() if k != "obj_model_type"}, KW, 64, ValueError, "needs frame_time="),
    (_args(), {"frame_time": 0.5}, 64, NotImplementedError, "render_kwargs_test_d_nerf="),
    (_args(), {"frame_time": 0.5}, 64, NotImplementedError, "load_dnerf_object"),
    (_args(app_place_new_mirror=True), dict(KW, frame_time=0.5), 64, ValueError, "cannot be combined with app_place_new_mirror"),
    (_args(), dict(KW, frame_time=0.5), 0, ValueError, "needs a fine mirror mask"),
    (_args(near=None), dict(KW, frame_time=0.5), 64, ValueError, "needs args.near"),
], ids=["without_frame_time", "frame_time_none", "default_type_without_frame_time", "says_how_to_pass_it", "names_the_loader",
        "with_place", "no_importance", "without_near"])
def test_refusals(args, kw, n_imp, exc, msg):
    import mirror_nerf_amd as M
    with pytest.raises(exc, match=msg):
        M.batched_inference(_models(), {}, torch.zeros(4, 8), 64, n_imp, False, 32, args=args, trace_secondary_rays=True, **kw)


def test_render_rays_dnerf_refuses_what_it_does_not_do():
    from mirror_nerf_amd.dnerf import DirectTemporalNeRF, render_rays_dnerf
    net = DirectTemporalNeRF()
    ok = dict(network_fn=net, N_samples=8, N_importance=0)
    with pytest.raises(NotImplementedError, match="perturb"):
        render_rays_dnerf(torch.zeros(4, 12), perturb=1.0, **ok)
    with pytest.raises(NotImplementedError, match="raw_noise_std"):
        render_rays_dnerf(torch.zeros(4, 12), raw_noise_std=1.0, **ok)
    with pytest.raises(NotImplementedError, match="DirectTemporalNeRF"):
        render_rays_dnerf(torch.zeros(4, 12), network_fn=torch.nn.Linear(3, 4), N_samples=8)
    with pytest.raises(ValueError, match=r"\(N, 9\) or \(N, 12\)"):
        render_rays_dnerf(torch.zeros(4, 8), **ok)
    with pytest.raises(RuntimeError, match="no CPU path"):
        render_rays_dnerf(torch.zeros(4, 12), network_query_fn=None, near=2.0, far=6.0, some_unknown_key=1, **ok)


# ----------------------------------------------------------------------------------------------- config.txt, checkpoints
CONFIG = """expname = mutant
basedir = ./logs
datadir = ./data/mutant
dataset_type = blender

nerf_type = direct_temporal
no_batching = True
not_zero_canonical = False   # the canonical frame is t = 0

use_viewdirs = True
white_bkgd = True
lrate_decay = 500

N_iter = 800000
N_samples = 64
N_importance = 128
N_rand = 500
"""


def test_read_config(tmp_path):
    from mirror_nerf_amd.dnerf import read_config
    p = tmp_path / "config.txt"
    p.write_text(CONFIG)
    cfg = read_config(str(p))
    assert cfg == dict(netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, multires=10, multires_views=4, i_embed=0,
                       N_samples=64, N_importance=128, use_viewdirs=True, use_two_models_for_fine=False, white_bkgd=True,
                       nerf_type="direct_temporal", not_zero_canonical=False, lindisp=False)
    p.write_text("N_samples = many\n")
    with pytest.raises(ValueError, match="N_samples"):
        read_config(str(p))
    p.write_text("use_viewdirs = maybe\n")
    with pytest.raises(ValueError, match="use_viewdirs"):
        read_config(str(p))
    p.write_text("")
    assert read_config(str(p))["nerf_type"] == "original" and read_config(str(p))["N_importance"] == 0     # the parser's defaults


@pytest.mark.parametrize("line,what", [
    ("netwidth = 128", "netwidth"), ("netdepth = 6", "netdepth"), ("multires = 6", "multires"), ("multires_views = 2", "multires_views"),
    ("i_embed = -1", "i_embed"), ("use_viewdirs = False", "use_viewdirs"), ("nerf_type = original", "nerf_type"),
    ("use_two_models_for_fine = True\nnetwidth_fine = 128", "netwidth_fine"), ("N_samples = 2", "N_samples"),
])
def test_configurations_the_kernel_does_not_cover_are_refused(tmp_path, line, what):
    from mirror_nerf_amd.dnerf import load_dnerf_object
    (tmp_path / "config.txt").write_text("nerf_type = direct_temporal\nuse_viewdirs = True\n" + line + "\n")
    torch.save({"network_fn_state_dict": {}}, str(tmp_path / "800000.tar"))
    with pytest.raises(NotImplementedError, match=what):
        load_dnerf_object(str(tmp_path / "800000.tar"), "cpu")


def test_checkpoint_round_trip(tmp_path):
    """A `.tar` in D-NeRF's layout (run_dnerf.py:342-350, its train loop's torch.save) written from this package's module."""
    from mirror_nerf_amd.dnerf import DirectTemporalNeRF, load_dnerf_object
    torch.manual_seed(3)
    nets = [DirectTemporalNeRF(), DirectTemporalNeRF()]
    d = tmp_path / "logs" / "mutant"
    d.mkdir(parents=True)
    ckpt = {"global_step": 800000, "network_fn_state_dict": nets[0].state_dict(), "network_fine_state_dict": nets[1].state_dict(),
            "optimizer_state_dict": {"state": {}, "param_groups": []}}
    torch.save(ckpt, str(d / "800000.tar"))
    with pytest.raises(FileNotFoundError, match="config.txt"):
        load_dnerf_object(str(d / "800000.tar"), "cpu")
    (d / "config.txt").write_text(CONFIG + "use_two_models_for_fine = True\n")
    kw = load_dnerf_object(str(d / "800000.tar"), "cpu")
    assert (kw["N_samples"], kw["N_importance"], kw["white_bkgd"], kw["use_two_models_for_fine"], kw["lindisp"]) == (64, 128, True, True, False)
    assert kw["perturb"] is False and kw["raw_noise_std"] == 0.0 and (kw["near"], kw["far"]) == (2.0, 6.0)
    for key, net in zip(("network_fn", "network_fine"), nets):
        assert isinstance(kw[key], DirectTemporalNeRF) and not kw[key].training and kw[key].zero_canonical
        for (k, a), (k2, b) in zip(kw[key].state_dict().items(), net.state_dict().items()):
            assert k == k2 and torch.equal(a, b), k
    # one model for both passes: the fine state dict of the file is not read
    (d / "config.txt").write_text(CONFIG + "not_zero_canonical = True\n")
    kw = load_dnerf_object(str(d / "800000.tar"), "cpu")
    assert kw["network_fine"] is None and not kw["use_two_models_for_fine"] and kw["network_fn"].zero_canonical is False
    torch.save({"network_fine_state_dict": nets[1].state_dict()}, str(d / "1.tar"))
    with pytest.raises(KeyError, match="network_fn_state_dict"):
        load_dnerf_object(str(d / "1.tar"), "cpu")


# ------------------------------------------------------------------------------------------------------------- C ABI
@pytest.fixture(scope="module")
def L():
    from mirror_nerf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_dnerf_entry_points_validate_their_arguments(L):
    null = None
    # tiles of both streams, the two bias blocks, 21 time columns of 256 rows (csrc/mnrf_dnerf.hip)
    assert L.mnrf_dnerf_packed_floats() == (1936 + 2352) * 256 + 2064 + 2464 + 21 * 256
    assert L.mnrf_dnerf_pack_weights(null, null, null) < 0 and b"mnrf_dnerf_pack_weights" in L.mnrf_last_error()
    import ctypes
    arr = (ctypes.c_void_p * 42)()
    assert L.mnrf_dnerf_pack_weights(arr, 64, null) < 0 and b"null parameter pointer" in L.mnrf_last_error()
    fwd = lambda packed=64, flags=0, B=4, xyz=64, stride=3, rays=null, z=null, spr=1, de=64, ds=27, t=0.5: L.mnrf_dnerf_forward(  # noqa: E731
        packed, flags, B, xyz, stride, rays, z, spr, de, ds, t, null, null, null, null)
    for kw, msg in ((dict(packed=null), b"packed"), (dict(flags=8), b"unknown flag"), (dict(B=-1), b"negative"),
                    (dict(xyz=null), b"need xyz or rays"), (dict(xyz=null, rays=64), b"need xyz or rays"), (dict(stride=2), b"xyz_stride"),
                    (dict(spr=0), b"samples per ray"), (dict(xyz=null, rays=64, z=64, spr=3), b"multiple of spr"),
                    (dict(de=null), b"dir_emb required"), (dict(ds=26), b"dir_stride"), (dict(t=float("nan")), b"finite"),
                    (dict(t=float("inf")), b"finite")):
        assert fwd(**kw) < 0 and msg in L.mnrf_last_error(), kw
    assert fwd(B=0) == 0                                       # zero samples: a no-op behind the checks
    assert fwd(B=0, flags=1, de=null) == 0                     # sigma only: no view encoding needed


@pytest.mark.skipif(not os.path.isdir("/root/reference/models"), reason="the reference tree is not on this machine (GPU box)")
def test_g27_generator_reproduces_committed_fixture(tmp_path):
    name = "g27_dnerf_model"
    code = f"import sys; sys.path.insert(0, {GOLDEN!r}); import make_golden_dnerf as G; sys.argv[1:] = [{name!r}]; G.main()"
    env = dict(os.environ, MNRF_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", code], cwd=GOLDEN, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    new, old = np.load(tmp_path / f"{name}.npz"), np.load(os.path.join(GOLDEN, f"{name}.npz"))
    assert sorted(new.files) == sorted(old.files), sorted(set(new.files) ^ set(old.files))
    for k in old.files:
        if k == "meta":
            assert json.loads(str(new[k])) == json.loads(str(old[k]))
        else:
            assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape, k
            assert np.array_equal(new[k], old[k], equal_nan=True), k
