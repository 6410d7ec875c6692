"""The validation loop on the GPU (mirror_nerf_amd/validation.py, checkpoint.save_training_state, scripts/train_blender.py):

* validation_step against the `log` dicts captured from the reference's NeRFSystem.validation_step (fixture (b) of
  tests/golden/make_golden_validation.py), on both arithmetics;
* a validation between two training steps leaves the training bit for bit as it is without one, on the static route and on the
  captured graph;
* K + K steps through a checkpoint and --resume equal 2K steps straight;
* the driver end to end: val.jsonl, the panel PNG, checkpoints that scripts/eval_scene.py renders."""
import importlib.util
import json
import os
import shutil
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VAL = os.path.join(ROOT, "tests", "golden", "validation")


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ----------------------------------------------------------------------------- validation_step against the reference
@pytest.mark.parametrize("precision", ["split", "fp32"])
@pytest.mark.parametrize("name", ["val_step_stage", "val_step_traced"])
def test_validation_step_against_the_reference(name, precision):
    """Every entry of the reference's `log` dict.  Tolerances, from the tests that hold the same quantities:
    * val_loss and the loss terms: 2e-6 * max(1, |want|) -- tests/test_loss.py:62-63 (test_hip_total_loss_matches_reference);
    * val_psnr, val_psnr_coarse: the PSNR is computed from rgb_fine / rgb_coarse, which the eval-semantics recursion tests hold
      to 1e-4 absolute (tests/test_hip_parity.py:67 `FX.tolerance(k, meta, base)` with base 1e-4, used by
      test_recursion_eval_golden :543 and, for is_eval through NeRFSystem, test_recursion_train_golden :527), and metrics.psnr
      itself to 1e-4 dB (tests/test_loss.py:143).  A colour error of at most e changes the mean squared error m by at most
      2 e sqrt(m) + e^2, hence the PSNR by at most 10 / ln 10 * (2 e sqrt(m) + e^2) / (m - 2 e sqrt(m)); with e = 1e-4 and the
      fixture's own m that is the bound, plus the 1e-4 dB of the reduction.
    Both arithmetics, as those tests run on both (tests/test_hip_parity.py:27)."""
    import mirror_nerf_amd as M
    from mirror_nerf_amd import mirror_nerf as MN
    from tests.golden import fixtures as FX
    fx = FX.Fixture(os.path.join("validation", name))
    meta = fx.meta
    sds = fx.state_dicts()
    hp = dict(meta["hp"])
    hp.update(N_emb_xyz=10, N_emb_dir=4, model_type="nerf")
    hp = SimpleNamespace(**hp)
    old = MN.PRECISION
    MN.set_precision(precision)
    try:
        system = M.NeRFSystem(hp)
        system.nerf_coarse.load_state_dict({k: torch.from_numpy(v) for k, v in sds[0].items()})
        system.nerf_fine.load_state_dict({k: torch.from_numpy(v) for k, v in sds[1].items()})
        system.to(DEV)
        batch = {"rays": torch.from_numpy(fx.inputs["rays"]).to(DEV), "rgbs": torch.from_numpy(fx.inputs["rgbs"]).to(DEV),
                 "mirror_mask": torch.from_numpy(fx.inputs["gt_mask"]).to(DEV)}
        keep = {k: v.clone() for k, v in batch.items()}
        log = M.validation_step(system, batch, M.get_loss(hp), meta["epoch"], hp)
        assert all(isinstance(v, torch.Tensor) and v.is_cuda and v.numel() == 1 for v in log.values())      # nothing read yet
        got = {k: float(v) for k, v in log.items()}
    finally:
        MN.set_precision(old)
    assert all(torch.equal(batch[k], keep[k]) for k in keep)             # the geometry stage blackens a copy
    assert system.train_geometry_stage == meta["hp"]["train_geometry_stage"]
    want = {k: float(v) for k, v in fx.outputs.items()}
    assert list(got) == meta["keys"], (list(got), meta["keys"])
    figures, bad = [], []
    for k in meta["keys"]:
        if k.startswith("val_psnr"):
            m, e = 10.0 ** (-want[k] / 10.0), 1e-4
            tol = 1e-4 + 10.0 / np.log(10.0) * (2 * e * np.sqrt(m) + e * e) / (m - 2 * e * np.sqrt(m))
        else:
            tol = 2e-6 * max(1.0, abs(want[k]))
        figures.append(f"{k}: got {got[k]:.7f} want {want[k]:.7f} |diff| {abs(got[k] - want[k]):.2e} tol {tol:.2e}")
        if not abs(got[k] - want[k]) <= tol:
            bad.append(k)
    print(f"{name} [{precision}]\n  " + "\n  ".join(figures))
    assert not bad, (bad, figures)


# ----------------------------------------------------------------------------- a validation leaves training untouched
def _system(seed=0):
    import mirror_nerf_amd as M
    from mirror_nerf_amd import training as T
    torch.manual_seed(seed)
    system = M.NeRFSystem(T.default_hparams()).to(DEV)          # perturb = noise_std = 1: the steps draw
    with torch.no_grad():       # opaque density, a mirror head that straddles 0.5
        for m in system.models.values():
            m.sigma.weight.mul_(20.0)
            m.sigma.bias.fill_(1.0)
            m.is_mirror_net[2].weight.mul_(40.0)
    return system


def _val_bank(H=6, W=8, F=2):
    from mirror_nerf_amd import synthetic as SY
    from mirror_nerf_amd.data import RayBank
    rng = np.random.default_rng(4)
    poses = np.stack([SY.look_at_pose(eye=(1.5 - k, 2.0, 2.0)) for k in range(F)])
    images = rng.integers(0, 256, (F, H, W, 4), dtype=np.uint8)
    masks = np.zeros((F, H, W), np.int8)
    masks[:, 1:5, 2:6] = 1
    return RayBank(poses, images, masks, 0.5 * W / np.tan(0.5 * 0.6911112), 0.05, 8.0, DEV)


def _batches(n, steps):
    from oracle import mirror_nerf_oracle as O
    g = torch.Generator(device=DEV)
    g.manual_seed(3)
    rays = torch.from_numpy(O.synthetic_rays(64, 64)[:: 4096 // n][:n].copy()).to(DEV)
    return [(rays, torch.rand(n, 3, device=DEV, generator=g), (torch.rand(n, device=DEV, generator=g) < 0.25).float())
            for _ in range(steps)]


def _train(route, validate_after, n=128, steps=3):
    import mirror_nerf_amd as M
    from mirror_nerf_amd import training as T
    from mirror_nerf_amd.weights import params_of
    system = _system()
    torch.manual_seed(11)
    bank = _val_bank()
    crit = M.get_loss(SimpleNamespace(model_type="nerf"))
    if route == "graph":
        opt = T.FlatAdam(list(system.models.values()), lr=5e-4)
        step = T.GraphedTrainStep(system, opt, n, gt_valid=True)
    else:
        opt = torch.optim.Adam(list(system.parameters()), lr=5e-4, fused=True)
        step = lambda r, t, g: T.train_step(system, opt, r, t, g, gt_valid=True)  # noqa: E731
    losses, graphs, seen = [], [], None
    for i, (rays, target, gt) in enumerate(_batches(n, steps)):
        losses.append(step(rays, target, gt).detach().clone())
        graphs.append(getattr(step, "graph", None))
        if i == validate_after:
            flags = [m.training for m in system.modules()]
            grads = [q.grad is None for q in system.parameters()]
            words = [m.__dict__["_mnrf_packed"].packed[-1:].clone() for m in system.models.values()]
            scale = [m.__dict__.get("_mnrf_seed_reduction") for m in system.models.values()]
            before = [q.detach().clone() for q in system.parameters()]
            means, logs, panel = M.validate(system, bank, crit, 5, system.hparams)
            assert flags == [m.training for m in system.modules()]
            assert grads == [q.grad is None for q in system.parameters()]
            assert all(torch.equal(a, b) for a, b in zip(before, system.parameters()))
            assert all(torch.equal(w, m.__dict__["_mnrf_packed"].packed[-1:]) for w, m in zip(words, system.models.values()))
            assert scale == [m.__dict__.get("_mnrf_seed_reduction") for m in system.models.values()]
            assert all("_mnrf_precision" not in m.__dict__ for m in system.models.values())
            seen = (means, logs, panel)
    torch.cuda.synchronize()
    if route == "graph":
        assert not step.ended and all(g is graphs[0] for g in graphs)          # one capture, kept across the validation
    return [float(v) for v in losses], [q.detach().clone() for m in system.models.values() for q in params_of(m)], seen


@pytest.mark.parametrize("route", ["static", "graph"])
def test_a_validation_leaves_training_untouched(route):
    """Three steps with perturb = noise_std = 1 on 128 rays (the smallest batch the existing graph tests use), with and without
    a validate() of two 6 x 8 frames between steps 1 and 2: the loss of every step and the final parameters are bit-identical;
    the modules' training flags, .grad presence, guard words, gradient-scale state and precision are as before (checked inside)."""
    loss_a, w_a, _ = _train(route, None)
    loss_b, w_b, seen = _train(route, 0)
    means, logs, (stack, names) = seen
    assert {"val/loss", "val/psnr", "val/psnr_coarse", "val/color_loss", "val/mirror_mask_loss", "val/normal_loss",
            "val/normal_reg_loss"} == set(means) and all(isinstance(v, float) for v in means.values())
    assert len(logs) == 2 and abs(means["val/psnr"] - (logs[0]["val_psnr"] + logs[1]["val_psnr"]) / 2) <= 1e-5
    assert tuple(stack.shape) == (len(names), 3, 6, 8) and names[0] == "gt_img" and "depth_reflect_fine" in names
    assert loss_a == loss_b, (loss_a, loss_b)
    assert all(torch.equal(a, b) for a, b in zip(w_a, w_b))


def test_a_validation_frame_outside_the_split_range_is_rendered_again_on_fp32():
    """Rays that start 100 units out trip the range guard of the split arithmetic (|x| >= 64): the frame comes back finite, as
    the fp32 kernels give it, the models are on the split arithmetic afterwards and nothing is pinned."""
    import mirror_nerf_amd as M
    from mirror_nerf_amd import mirror_nerf as MN
    if MN.PRECISION != "split" or not MN.GUARD:
        pytest.skip("the range guard belongs to the split arithmetic")
    system = _system()
    bank = _val_bank()
    batch = bank.frame(0)
    batch["rays"][:, :3] += 100.0
    crit = M.get_loss(SimpleNamespace(model_type="nerf"))
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)      # the validation's own handling: no pinning warning
        log = M.validation_step(system, batch, crit, 5, system.hparams)
    MN.set_precision("fp32")
    try:
        want = M.validation_step(system, batch, crit, 5, system.hparams)
    finally:
        MN.set_precision("split")
    assert np.isfinite(float(log["val_psnr"])) and float(log["val_psnr"]) == float(want["val_psnr"])
    for m in system.models.values():
        assert MN.precision_of(m) == "split" and not m.__dict__.get("_mnrf_range_trips")
        assert int(m.__dict__["_mnrf_packed"].packed[-1:].view(torch.int32).item()) == 0


# ----------------------------------------------------------------------------- the driver
def _scene(root, w=8, h=8, n=3):
    """tests/test_raybank_cpu.make_dataset with look-at poses, and a validation split of its first two frames."""
    from mirror_nerf_amd import synthetic as SY
    from tests.test_raybank_cpu import make_dataset
    os.makedirs(root)
    make_dataset(root, w=w, h=h, n=n, mixed=False)
    for split in ("train", "test"):
        with open(os.path.join(root, f"transforms_{split}.json")) as f:
            meta = json.load(f)
        for k, fr in enumerate(meta["frames"]):
            pose = np.eye(4)
            pose[:3, :4] = SY.look_at_pose(eye=(1.5 - k, 2.0, 2.0))
            fr["transform_matrix"] = pose.tolist()
        with open(os.path.join(root, f"transforms_{split}.json"), "w") as f:
            json.dump(meta, f)
    meta["frames"] = meta["frames"][:2]
    with open(os.path.join(root, "transforms_val.json"), "w") as f:
        json.dump(meta, f)
    return root


def _drive(TB, root, out, *extra, steps=6, route="static"):
    TB.main(["--root_dir", root, "--img_wh", "8", "8", "--near", "0.05", "--far", "8", "--route", route, "--steps", str(steps),
             "--batch", "64", "--seed", "5", "--out", out] + [str(e) for e in extra])
    z = np.load(out)
    return {k: z[k] for k in z.files if k != "meta"}, json.loads(str(z["meta"]))


@pytest.mark.parametrize("route", ["static", "graph"])
def test_resume_equals_a_straight_run(tmp_path, route):
    """2K = 6 steps of scripts/train_blender.py on the static route and on the captured graph (three 8 x 8 frames, batch 64: an epoch is K = 3 steps; the
    shuffled stream, the perturb and noise draws and the learning-rate schedule all run), against the same run continued with
    --resume from the checkpoint written at the end of epoch 0 (step K).  profiles/resume_determinism.json: two straight runs of
    the parent commit's driver with one seed gave bit-identical weights and final loss on either route, so the resumed run must
    too.  (On the graph route the epoch's end captures again; the rehearsal steps of a capture draw, at the same point of either run.)"""
    TB = _script("train_blender")
    root = _scene(str(tmp_path / "scene"))
    straight, meta_a = _drive(TB, root, str(tmp_path / "a.npz"), route=route)
    saving, meta_b = _drive(TB, root, str(tmp_path / "b.npz"), "--ckpt_dir", tmp_path / "ck", route=route)
    assert sorted(os.listdir(tmp_path / "ck")) == ["best.json", "epoch=0.ckpt", "last.ckpt"]
    ck = torch.load(tmp_path / "ck" / "epoch=0.ckpt", weights_only=True)
    assert ck["global_step"] == 3 and ck["epoch"] == 0 and ck["mnrf_training"]["stream"]["step"] == 3
    resumed, meta_c = _drive(TB, root, str(tmp_path / "c.npz"), "--resume", tmp_path / "ck" / "epoch=0.ckpt", route=route)
    worst = {k: float(np.abs(resumed[k].astype(np.float64) - straight[k]).max()) for k in straight}
    print("final loss straight / saving / resumed:", meta_a["final_loss"], meta_b["final_loss"], meta_c["final_loss"],
          " largest weight difference resumed vs straight:", max(worst.values()))
    assert all(np.array_equal(saving[k], straight[k]) for k in straight)
    assert all(np.array_equal(resumed[k], straight[k]) for k in straight), {k: v for k, v in worst.items() if v}
    assert meta_a["final_loss"] == meta_b["final_loss"] == meta_c["final_loss"]
    with pytest.raises(SystemExit, match="--steps"):
        _drive(TB, root, str(tmp_path / "d.npz"), "--resume", tmp_path / "ck" / "epoch=0.ckpt", steps=8, route=route)


def test_train_blender_validates_logs_and_checkpoints(tmp_path):
    """Four steps on the graph route with --val_every 0.34 (an epoch is 3 steps: a validation per step), --ckpt_dir and
    --log_dir: val.jsonl carries the reference's names, the panel PNG has len(names) tiles (23 for a rendered frame), last.ckpt renders through
    scripts/eval_scene.py."""
    from PIL import Image
    TB = _script("train_blender")
    root = _scene(str(tmp_path / "scene"))
    ck, log = tmp_path / "ck", tmp_path / "log"
    _drive(TB, root, str(tmp_path / "w.npz"), "--val_every", 0.34, "--val_frames", 1, 0, "--ckpt_dir", ck, "--log_dir", log,
           steps=4, route="graph")
    lines = [json.loads(ln) for ln in open(log / "val.jsonl")]
    assert [ln["step"] for ln in lines] == [1, 2, 3, 4] and [ln["epoch"] for ln in lines] == [0, 0, 0, 1]
    want = {"val/loss", "val/psnr", "val/psnr_coarse", "val/color_loss", "val/mirror_mask_loss", "val/normal_loss", "val/normal_reg_loss"}
    assert all(want <= set(ln) and all(np.isfinite(ln[k]) for k in want) for ln in lines)
    for step in (1, 4):
        tiles = json.load(open(log / f"val_panel_{step}.json"))
        png = Image.open(log / f"val_panel_{step}.png")
        # (the recursion keeps the reflected depth of the model it traces with only: no depth_reflect_coarse, train.py:312-324)
        assert len(tiles["names"]) == 23 and tiles["names"][0] == "gt_img" and tiles["cols"] * tiles["rows"] >= 23
        assert "depth_reflect_fine" in tiles["names"] and "depth_reflect_coarse" not in tiles["names"]
        assert png.size == (tiles["cols"] * 9 - 1, tiles["rows"] * 9 - 1)
    # the first tile is the ground truth of validation frame 1 (--val_frames 1 0), blended onto black by its alpha
    grid = np.asarray(Image.open(log / "val_panel_1.png"))
    assert grid[:8, :8].any() and not grid[8, :].any()
    assert sorted(os.listdir(ck)) == ["best.json", "epoch=0.ckpt", "last.ckpt"]
    best = json.load(open(ck / "best.json"))
    assert best["best_epoch"] == 0 and best["best_score"] == lines[2]["val/psnr"] and best["monitor"] == "val/psnr"
    ES = _script("eval_scene")
    out = tmp_path / "results"
    assert ES.main(["--root_dir", root, "--split", "test", "--img_wh", "8", "8", "--near", "0.05", "--far", "8", "--ckpt_path",
                    str(ck / "last.ckpt"), "--N_samples", "64", "--N_importance", "64", "--trace_secondary_rays", "--out_dir",
                    str(out)]) == 0
    assert all((out / f"rgb_fine_{i:03d}.png").is_file() for i in range(3))
    shutil.rmtree(out)
