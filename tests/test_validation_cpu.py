"""The validation loop without a GPU: tests/val_panel_ref.py (the numpy restatement the GPU tests compare frames.val_panel
with) against the panel captured from the reference (tests/golden/validation/val_panel_6x8.npz) and against cases worked out by
hand, the argument validation of the two panel entry points (it happens before any launch), the resumable training state of
checkpoint.py on CPU tensors, and the fixture generator's round trip (build container only)."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import val_panel_ref as VR

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
VAL = os.path.join(GOLDEN, "validation")

REFERENCE_NAMES = ["gt_img", "img_fine", "img_coarse", "img_reflect_fine", "img_reflect_coarse", "img_direct_fine",
                   "img_direct_coarse", "depth_fine", "depth_coarse", "depth_reflect_fine", "depth_reflect_coarse",
                   "gt_mirror_mask", "mirror_mask_pred_fine", "mirror_mask_pred_coarse", "normal_pred_fine", "normal_grad_fine",
                   "normal_pred_coarse", "normal_grad_coarse", "secondary_rays_o", "secondary_rays_o_vis", "reflect_direction",
                   "reflect_direction_vis", "x_surface_fine", "x_surface_coarse"]      # visualization.py:32-179, read off the file


def _load(name):
    z = np.load(os.path.join(VAL, name + ".npz"))
    return z, json.loads(str(z["meta"]))


@pytest.fixture(scope="module")
def L():
    from mirror_nerf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_numpy_panel_reproduces_the_reference_capture():
    from mirror_nerf_amd.frames import jet_table
    z, meta = _load("val_panel_6x8")
    assert "NOT pinned" in meta["table"]
    batch = {k[7:]: z[k] for k in z.files if k.startswith("batch__")}
    results = {k[4:]: z[k] for k in z.files if k.startswith("in__")}
    stack, names = VR.val_panel((meta["W"], meta["H"]), batch, results, jet_table())
    assert names == meta["names"] == REFERENCE_NAMES
    assert stack.dtype == F32 and stack.shape == z["out__stack"].shape == (24, 3, meta["H"], meta["W"])
    assert np.array_equal(stack, z["out__stack"], equal_nan=True)
    # the inputs are those of the seeded case the GPU tests use
    b2, r2 = VR.seeded_case(meta["H"], meta["W"], meta["seed"], meta["variant"])
    assert all(np.array_equal(b2[k], batch[k]) for k in batch) and all(np.array_equal(r2[k], results[k], equal_nan=True) for k in results)


def test_tiles_by_hand():
    T = np.zeros((256, 3), np.uint8)
    T[:, 0] = np.arange(256)
    T[:, 1] = 255 - np.arange(256)
    T[:, 2] = 51
    H, W = 1, 4
    rgb = np.arange(12, dtype=F32).reshape(4, 3)
    batch = {"rgbs": rgb}
    res = {"depth_coarse": F32([2.0, np.nan, 4.0, 3.0]), "surface_normal_coarse": F32([[-1, 0, 1]] * 4),
           "x_surface_coarse": F32([[1, 2, 3], [3, 3, 3], [2, 2, 2], [1, 1, 1]]), "mirror_mask_coarse": F32([0, 1, 0.25, -2])}
    stack, names = VR.val_panel((W, H), batch, res, T)
    assert names == ["gt_img", "depth_coarse", "mirror_mask_pred_coarse", "normal_pred_coarse", "x_surface_coarse"]
    assert np.array_equal(stack[0, :, 0, :], rgb.T)                                    # (3, H, W): channel c of pixel p
    # depth: nan_to_num -> [2, 0, 4, 3]; mi 0, ma 4; k = trunc(255 x) = [127, 0, 255, 191]
    k = np.array([127, 0, 255, 191])
    assert np.array_equal(stack[1, 0, 0], k.astype(F32) / F32(255)) and np.array_equal(stack[1, 1, 0], (255 - k).astype(F32) / F32(255))
    assert np.array_equal(stack[1, 2, 0], np.full(4, F32(51) / F32(255)))
    assert np.array_equal(stack[2], np.broadcast_to(res["mirror_mask_coarse"], (3, 1, 4)))      # no clip: the raw mask
    assert np.array_equal(stack[3, :, 0, 0], F32([0, 0.5, 1]))
    assert np.array_equal(stack[4, :, 0, 0], F32([0, 0.5, 1])) and np.array_equal(stack[4, :, 0, 3], F32([0, 0, 0]))
    res["x_surface_coarse"] = np.full((4, 3), F32(7))                                  # min == max: ones
    assert np.array_equal(VR.val_panel((W, H), batch, res, T)[0][4], np.ones((3, 1, 4), F32))
    res["x_surface_coarse"] = F32([[1, 2, np.nan]] + [[0, 0, 0]] * 3)                  # a NaN anywhere: the whole tile
    assert np.isnan(VR.val_panel((W, H), batch, res, T)[0][4]).all()
    res["depth_coarse"] = np.full(4, F32(3.25))                                        # constant: (x - mi) / 1e-8 = 0
    assert np.array_equal(VR.val_panel((W, H), batch, res, T)[0][1][0, 0], np.zeros(4, F32))


@pytest.mark.parametrize("variant", VR.VARIANTS)
def test_presence_rules(variant):
    batch, res = VR.seeded_case(5, 13, 3, variant)
    _, names = VR.val_panel((13, 5), batch, res, np.zeros((256, 3), np.uint8))
    want = list(REFERENCE_NAMES)
    if variant == "coarse_only":
        want = [n for n in want if "fine" not in n]
    if variant == "no_reflect":
        want = [n for n in want if "reflect" not in n and "direct" not in n and not n.startswith("secondary")]
    assert names == want


def test_val_panel_tiles_follow_the_reference_order():
    """frames.val_panel_tiles (the list the launches are given) names the tiles as the restatement does, for every variant."""
    from mirror_nerf_amd import _lib, frames
    kinds = {"gt_img": _lib.MNRF_PANEL_COPY, "depth_fine": _lib.MNRF_PANEL_DEPTH, "gt_mirror_mask": _lib.MNRF_PANEL_MASK,
             "normal_grad_coarse": _lib.MNRF_PANEL_NORMAL, "secondary_rays_o": _lib.MNRF_PANEL_COPY,
             "secondary_rays_o_vis": _lib.MNRF_PANEL_GLOBAL, "x_surface_coarse": _lib.MNRF_PANEL_GLOBAL}
    for variant in VR.VARIANTS:
        batch, res = VR.seeded_case(3, 4, 5, variant)
        tiles = frames.val_panel_tiles(batch, res)
        assert [t[0] for t in tiles] == VR.val_panel((4, 3), batch, res, np.zeros((256, 3), np.uint8))[1]
        for name, kind, _ in tiles:
            assert kinds.get(name, kind) == kind, name
    del batch["mirror_mask"]
    assert "gt_mirror_mask" not in [t[0] for t in frames.val_panel_tiles(batch, res)]


def test_abi_validates_before_any_launch(L):
    """Null arrays, a null map, negative sizes, too many tiles, an unknown kind and a missing table or stats block are refused
    with the entry point's name in mnrf_last_error; no tile and H W == 0 are no-ops.  Nothing reaches a launch: no GPU needed."""
    from mirror_nerf_amd import _lib
    assert L.mnrf_val_panel_stats_floats() >= 5
    fake = ctypes.c_void_p(4096)        # never dereferenced: validation only
    ptrs = lambda *v: (ctypes.c_void_p * len(v))(*v)  # noqa: E731
    ints = lambda *v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    COPY, DEPTH, GLOBAL = _lib.MNRF_PANEL_COPY, _lib.MNRF_PANEL_DEPTH, _lib.MNRF_PANEL_GLOBAL
    for name, call in (("mnrf_val_panel_extrema", lambda m, k, t, H, W, st, tab=fake, out=fake: L.mnrf_val_panel_extrema(m, k, t, H, W, st, None)),
                       ("mnrf_val_panel_write", lambda m, k, t, H, W, st, tab=fake, out=fake: L.mnrf_val_panel_write(m, k, t, H, W, st, tab, out, None))):
        refused = lambda code: code < 0 and name.encode() in L.mnrf_last_error()  # noqa: E731
        assert refused(call(None, ints(COPY), 1, 4, 4, fake)) and b"null" in L.mnrf_last_error()
        assert refused(call(ptrs(4096), None, 1, 4, 4, fake))
        assert refused(call(ptrs(None), ints(COPY), 1, 4, 4, fake)) and b"null map" in L.mnrf_last_error()
        assert refused(call(ptrs(4096), ints(COPY), -1, 4, 4, fake))
        assert refused(call(ptrs(*[4096] * 33), ints(*[COPY] * 33), 33, 4, 4, fake))
        assert refused(call(ptrs(4096), ints(COPY), 1, -4, 4, fake)) and b"negative" in L.mnrf_last_error()
        assert refused(call(ptrs(4096), ints(COPY), 1, 4, -4, fake))
        assert refused(call(ptrs(4096), ints(5), 1, 4, 4, fake)) and b"kind" in L.mnrf_last_error()
        assert refused(call(ptrs(4096), ints(-1), 1, 4, 4, fake))
        assert refused(call(ptrs(4096, 4096), ints(COPY, GLOBAL), 2, 4, 4, None)) and b"stats" in L.mnrf_last_error()
        assert call(None, None, 0, 4, 4, None) == 0                                    # no tile
        assert call(ptrs(4096, 4096), ints(COPY, DEPTH), 2, 0, 7, fake) == 0           # H W == 0
        assert call(ptrs(4096, 4096), ints(COPY, DEPTH), 2, 7, 0, fake) == 0
    assert L.mnrf_val_panel_write(ptrs(4096), ints(DEPTH), 1, 4, 4, fake, None, fake, None) < 0
    assert b"mnrf_val_panel_write" in L.mnrf_last_error() and b"table" in L.mnrf_last_error()
    assert L.mnrf_val_panel_write(ptrs(4096), ints(COPY), 1, 4, 4, None, None, None, None) < 0
    assert b"output" in L.mnrf_last_error()


def test_cpu_maps_are_rejected():
    import mirror_nerf_amd as M
    batch, res = VR.seeded_case(2, 2, 0)
    with pytest.raises(RuntimeError, match="GPU only"):
        M.val_panel((2, 2), {k: torch.from_numpy(v) for k, v in batch.items()}, {k: torch.from_numpy(v) for k, v in res.items()})


# ----------------------------------------------------------------------------- checkpoint.py: the resumable training state
def _system(seed):
    import mirror_nerf_amd as M
    torch.manual_seed(seed)
    system = torch.nn.Module()
    for name in ("nerf_coarse", "nerf_fine"):
        setattr(system, name, M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=True))
    return system


def _stepped(system, steps=2):
    opt = torch.optim.Adam(list(system.parameters()), lr=5e-4)
    for i in range(steps):
        opt.zero_grad()
        sum((p * p).sum() * (0.5 + i) for p in system.parameters()).backward()
        opt.step()
        opt.param_groups[0]["lr"] *= 0.9
    return opt


def test_training_state_round_trip(tmp_path):
    import mirror_nerf_amd as M
    from mirror_nerf_amd import checkpoint as C
    a = _system(1)
    opt_a = _stepped(a)
    a.nerf_fine.__dict__["_mnrf_seed_reduction"] = 4
    torch.manual_seed(77)
    torch.rand(5)
    path = tmp_path / "last.ckpt"
    stream = dict(seed=3, step=17, epoch=2, stage=False, first=12, epoch_first=1)
    C.save_training_state(path, a, opt_a, epoch=2, global_step=17, stream=stream)
    expect = torch.rand(4)                                  # what the generator gives next

    b = _system(2)
    opt_b = torch.optim.Adam(list(b.parameters()), lr=1.0)
    torch.manual_seed(5)
    got = C.load_training_state(path, b, opt_b)             # trusted=False: tensors and plain containers only
    assert got == {"epoch": 2, "global_step": 17, "lr": opt_a.param_groups[0]["lr"], "stream": stream}
    assert torch.equal(torch.rand(4), expect)               # the CPU generator is where it was
    for (k, v), (k2, v2) in zip(a.state_dict().items(), b.state_dict().items()):
        assert k == k2 and torch.equal(v, v2), k
    sa, sb = opt_a.state_dict(), opt_b.state_dict()
    assert sa["param_groups"] == sb["param_groups"] and sb["param_groups"][0]["lr"] == pytest.approx(5e-4 * 0.81, rel=1e-12)
    assert sorted(sa["state"]) == sorted(sb["state"]) and len(sa["state"]) == 64
    for i in sa["state"]:
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(torch.as_tensor(sa["state"][i][k]), torch.as_tensor(sb["state"][i][k])), (i, k)
    assert b.nerf_fine.__dict__["_mnrf_seed_reduction"] == 4 and "_mnrf_seed_reduction" not in b.nerf_coarse.__dict__
    # one more identical step on either side: the resumed run continues as the original
    for s, o in ((a, opt_a), (b, opt_b)):
        o.zero_grad()
        sum((p * p).sum() for p in s.parameters()).backward()
        o.step()
    assert all(torch.equal(p, q) for p, q in zip(a.parameters(), b.parameters()))

    # the same file is an ordinary checkpoint: load_ckpt and extract_model_state_dict read it untrusted, like save_ckpt's
    C.save_training_state(path, a, opt_a, epoch=2, global_step=18, stream=stream)
    m = M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=True)
    C.load_ckpt(m, path, "nerf_fine", trusted=False)
    assert all(torch.equal(v, a.nerf_fine.state_dict()[k]) for k, v in m.state_dict().items())
    sd = C.extract_model_state_dict(str(path), "nerf_coarse", trusted=False)
    assert sorted(sd) == sorted(a.nerf_coarse.state_dict()) and torch.equal(sd["sigma.weight"], a.nerf_coarse.sigma.weight)
    raw = torch.load(path, map_location="cpu", weights_only=True)
    C.save_ckpt(tmp_path / "plain.ckpt", a, 2, 18)
    plain = torch.load(tmp_path / "plain.ckpt", weights_only=True)
    assert set(plain) <= set(raw) and raw["epoch"] == 2 and raw["global_step"] == 18
    assert all(torch.equal(raw["state_dict"][k], v) for k, v in plain["state_dict"].items())


def test_a_plain_checkpoint_cannot_be_resumed(tmp_path):
    from mirror_nerf_amd import checkpoint as C
    a = _system(1)
    C.save_ckpt(tmp_path / "w.ckpt", a, 1, 2)
    with pytest.raises(RuntimeError, match="cannot be resumed"):
        C.load_training_state(tmp_path / "w.ckpt", a, None)


def _same(a, b, path=""):
    assert type(a) is type(b) or {type(a), type(b)} <= {int, float}, (path, a, b)
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), (path, sorted(set(a) ^ set(b)))
        for k in a:
            _same(a[k], b[k], f"{path}.{k}")
    elif isinstance(a, list):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{i}]")
    else:
        assert a == b, (path, a, b)


@pytest.mark.skipif(not os.path.isdir("/root/reference/models"), reason="the reference tree is not on this machine (GPU box)")
def test_generator_reproduces_the_committed_fixtures(tmp_path):
    """tests/golden/make_golden_validation.py against the committed files, arrays bit for bit and the JSON meta: the panel
    and the geometry-stage validation step."""
    code = (f"import sys; sys.path.insert(0, {GOLDEN!r}); import make_golden_validation as G; G.panel_case(); "
            "G.step_case('val_step_stage', True, 0)")
    env = dict(os.environ, MNRF_GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, "-c", code], cwd=GOLDEN, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    for name in ("val_panel_6x8", "val_step_stage"):
        new, old = np.load(tmp_path / "validation" / f"{name}.npz"), np.load(os.path.join(VAL, f"{name}.npz"))
        assert sorted(new.files) == sorted(old.files), (name, sorted(set(new.files) ^ set(old.files)))
        for k in old.files:
            if k == "meta":
                _same(json.loads(str(new[k])), json.loads(str(old[k])), name + ".meta")
            else:
                assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape, (name, k)
                assert np.array_equal(new[k], old[k], equal_nan=True), (name, k)
