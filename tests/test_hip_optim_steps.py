"""training.FlatSGD and training.FlatRAdam in the training step and in scripts/train_blender.py, at the shapes of the existing
captured-step tests (tests/test_static_step.py: 256 rays) and on the tiny Blender directory of the validation tests
(tests/test_hip_validation.py: three 8 x 8 frames, batch 64, an epoch is three steps).

* GraphedTrainStep with FlatRAdam through 8 replays of ONE graph, from step 1 across the rectification threshold (step 6 with
  beta2 = 0.999, decided on the device from the device count), and with FlatSGD through 4: after every replay the loss and the
  weights equal, bit for bit, those of a twin stepped by train_step's static route with the same optimizer class -- the same
  launches issued by the host, the host-scalar entry point in place of the prep launch and the device-state update.
* A state loaded into a new optimizer continues the device count.
* The driver: --lr_scheduler steplr --decay_step 1 2 --num_epochs 3 runs three epochs at the fixture's rates; K + K epochs through
  --resume equal 2K straight, bit for bit, on the static route; another schedule, none, or another optimizer is refused."""
import json
import os

import numpy as np
import pytest
import torch

from tests.test_static_step import _batch, _system

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _weights(system):
    from mirror_nerf_amd.weights import params_of
    return [q.detach().clone() for m in system.models.values() for q in params_of(m)]


def _twins(name, **kw):
    from mirror_nerf_amd import training as T
    a, b = _system(perturb=0.0, noise_std=0.0), _system(perturb=0.0, noise_std=0.0)          # (same seed: the same weights)
    cls = getattr(T, name)
    return a, b, cls(list(a.models.values()), **kw), cls(list(b.models.values()), **kw)


@pytest.mark.parametrize("name,steps,kw", [("FlatRAdam", 8, dict(lr=5e-4)), ("FlatSGD", 4, dict(lr=5e-3, momentum=0.9))])
def test_graphed_step_equals_the_static_route_bit_for_bit(name, steps, kw):
    from mirror_nerf_amd import training as T
    from tests import optim_ref as R
    a, b, opt_a, opt_b = _twins(name, **kw)
    n = 256
    step = T.GraphedTrainStep(a, opt_a, n, gt_valid=True)
    graphs, flags, w0 = [], [], _weights(a)
    for i in range(steps):
        rays, target, gt = _batch(n=n, frac=(0.3, 0.0, 1.0, 0.25)[i % 4], seed=20 + i)
        la = step(rays, target, gt)
        graphs.append(step.graph)
        lb = T.train_step(b, opt_b, rays, target, gt, gt_valid=True)
        torch.cuda.synchronize()
        assert not step.ended and float(la) == float(lb.detach()), (i, float(la), float(lb.detach()))
        for j, (qa, qb) in enumerate(zip(_weights(a), _weights(b))):
            assert torch.equal(qa, qb), (i, j, float((qa - qb).abs().max()))
        if name == "FlatRAdam":
            flags.append(float(opt_a._state_dev[8].item()))
    assert all(g is graphs[0] for g in graphs)                                  # one capture
    assert opt_a._calls == opt_b._calls == steps and int(opt_a._step_dev.item()) == steps
    assert [int(t.item()) for t in opt_a._skipped + opt_b._skipped] == [0] * 4
    assert any(not torch.equal(x, y) for x, y in zip(w0, _weights(a)))         # ... and the weights did move
    if name == "FlatRAdam":
        k = R.first_rectified_step(0.999)
        assert 1 < k <= steps and flags == [0.0] * (k - 1) + [1.0] * (steps - k + 1), flags


def test_graphed_step_refuses_what_is_no_flat_optimizer():
    from mirror_nerf_amd import training as T
    a = _system(perturb=0.0, noise_std=0.0)
    with pytest.raises(ValueError, match="FlatAdam, training.FlatSGD or training.FlatRAdam"):
        T.GraphedTrainStep(a, torch.optim.RAdam(list(a.parameters()), lr=5e-4), 128)
    with pytest.raises(ValueError, match="kernel form"):
        T.GraphedTrainStep(a, T.FlatRAdam(list(a.models.values()), kernel=False), 128)


@pytest.mark.parametrize("name", ["FlatRAdam", "FlatSGD"])
def test_a_loaded_state_continues_the_device_count(name, tmp_path):
    """Three replays, the state through checkpoint.save_training_state / load_training_state into a twin with a NEW optimizer, a
    captured step built on it: its device count starts at 3, and its fourth step is the original's fourth, bit for bit."""
    from mirror_nerf_amd import checkpoint as C, training as T
    a, b, opt_a, opt_b = _twins(name, lr=5e-4, weight_decay=1e-3)
    n = 128
    step_a = T.GraphedTrainStep(a, opt_a, n, gt_valid=True)
    batches = [_batch(n=n, seed=40 + i) for i in range(4)]
    for rays, target, gt in batches[:3]:
        step_a(rays, target, gt)
    torch.cuda.synchronize()
    path = tmp_path / "state.ckpt"
    C.save_training_state(path, a, opt_a, epoch=0, global_step=3)
    got = C.load_training_state(path, b, opt_b)
    assert got["global_step"] == 3 and opt_b._calls == 3 and opt_b._steps == [3, 3]
    wrong = (T.FlatSGD if name == "FlatRAdam" else T.FlatRAdam)(list(_system(perturb=0.0, noise_std=0.0).models.values()))
    with pytest.raises(ValueError, match="was written by " + name):
        C.load_training_state(path, b, wrong)
    step_b = T.GraphedTrainStep(b, opt_b, n, gt_valid=True)
    assert int(opt_b._step_dev.item()) == 3
    la, lb = step_a(*batches[3]), step_b(*batches[3])
    torch.cuda.synchronize()
    assert float(la) == float(lb) and int(opt_b._step_dev.item()) == int(opt_a._step_dev.item()) == 4
    assert all(torch.equal(x, y) for x, y in zip(_weights(a), _weights(b)))
    for la_, lb_ in zip(opt_a._state_lists(), opt_b._state_lists()):
        assert all(torch.equal(x, y) for x, y in zip(la_, lb_))


# ----------------------------------------------------------------------------- the driver
@pytest.fixture(scope="module")
def rates():
    with open(os.path.join(ROOT, "tests", "golden", "schedules", "lr_sequences.json")) as f:
        return json.load(f)["cases"]["steplr_driver"]["lr"]


def test_driver_runs_the_schedule_over_three_epochs(tmp_path, rates, capsys):
    """--optimizer radam on the graph route (training.FlatRAdam) with --lr_scheduler steplr --decay_step 1 2 --num_epochs 3 and
    far more --steps than that: nine steps, the fixture's rate in every epoch, the last of them in the checkpoint."""
    from tests.test_hip_validation import _drive, _scene, _script
    TB = _script("train_blender")
    root = _scene(str(tmp_path / "scene"))
    _w, meta = _drive(TB, root, str(tmp_path / "w.npz"), "--optimizer", "radam", "--lr_scheduler", "steplr", "--decay_step", 1, 2,
                      "--num_epochs", 3, "--ckpt_dir", tmp_path / "ck", steps=1000, route="graph")
    assert meta["steps_run"] == 9 and meta["epochs"] == 3 and meta["optimizer"] == "radam"
    # (the closed form against torch's recursive sequence: within 2^-40 relative, the tolerance of tests/test_schedules_cpu.py)
    assert all(abs(meta["lr_by_epoch"][str(e)] - rates[e]) <= 2.0 ** -40 * rates[e] for e in range(3)), meta["lr_by_epoch"]
    out = capsys.readouterr().out
    assert all(f"epoch {e}  lr {rates[e]:.6e}" in out for e in range(3))
    ck = torch.load(tmp_path / "ck" / "last.ckpt", weights_only=True)
    extra = ck["mnrf_training"]
    assert abs(extra["lr"] - rates[2]) <= 2.0 ** -40 * rates[2] and extra["optimizer"] == "FlatRAdam" and ck["global_step"] == 9
    assert extra["schedule"]["epoch"] == 2 and extra["schedule"]["options"]["decay_step"] == [1, 2]
    assert ck["optimizer_states"][0]["calls"] == 9 and np.isfinite(meta["final_loss"])
    with pytest.raises(SystemExit, match="ranger"):
        _drive(TB, root, str(tmp_path / "x.npz"), "--optimizer", "ranger")
    with pytest.raises(SystemExit, match="cosine"):
        _drive(TB, root, str(tmp_path / "x.npz"), "--lr_scheduler", "cosine", "--warmup_epochs", 2)


def test_resume_with_a_schedule_equals_a_straight_run(tmp_path, rates):
    """2K = 2 epochs of SGD under steplr on the static route (torch's fused SGD there), against the same run continued with
    --resume from the checkpoint of the end of epoch 0: the same weights and final loss bit for bit; both ran epoch 1 at the
    fixture's second rate.  A resume with another decay_step, without the schedule, or with another optimizer is refused."""
    from tests.test_hip_validation import _drive, _scene, _script
    TB = _script("train_blender")
    root = _scene(str(tmp_path / "scene"))
    flags = ("--optimizer", "sgd", "--lr", 5e-4, "--lr_scheduler", "steplr", "--decay_step", 1, 2, "--num_epochs", 2)
    straight, meta_a = _drive(TB, root, str(tmp_path / "a.npz"), *flags, "--ckpt_dir", tmp_path / "ck", steps=1000)
    assert sorted(os.listdir(tmp_path / "ck")) == ["best.json", "epoch=0.ckpt", "last.ckpt"] and meta_a["steps_run"] == 6
    ck0 = tmp_path / "ck" / "epoch=0.ckpt"
    resumed, meta_b = _drive(TB, root, str(tmp_path / "b.npz"), *flags, "--resume", ck0, steps=1000)
    assert all(np.array_equal(resumed[k], straight[k]) for k in straight)
    assert meta_a["final_loss"] == meta_b["final_loss"] and meta_b["steps_run"] == 6
    assert sorted(meta_a["lr_by_epoch"]) == ["0", "1"] and meta_b["lr_by_epoch"] == meta_a["lr_by_epoch"]
    assert all(abs(meta_a["lr_by_epoch"][str(e)] - rates[e]) <= 2.0 ** -40 * rates[e] for e in range(2))
    with pytest.raises(SystemExit, match="decay_step"):
        _drive(TB, root, str(tmp_path / "c.npz"), "--optimizer", "sgd", "--lr_scheduler", "steplr", "--decay_step", 1, 3, "--num_epochs", 2,
               "--resume", ck0, steps=1000)
    with pytest.raises(SystemExit, match="with --lr_scheduler"):
        _drive(TB, root, str(tmp_path / "c.npz"), "--optimizer", "sgd", "--resume", ck0, steps=1000)
    with pytest.raises(SystemExit, match="written by SGD"):
        _drive(TB, root, str(tmp_path / "c.npz"), *flags[2:], "--resume", ck0, steps=1000)
