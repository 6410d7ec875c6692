"""Anchors of tests/rough_ref.py (no GPU): the roughness rule for partly mirrored chunks, restated over the oracle, IS the oracle
where every ray of a chunk is a mirror ray, runs where the oracle -- like the reference -- cannot add (M,3) to (N,3), and
leaves the rays that are no mirror rays with their one reflection sample.  And the parser of scripts/eval_scene.py takes the
reference's roughness flags."""
import os
import sys

import numpy as np
import pytest

from oracle import mirror_nerf_oracle as O
from tests import rough_ref as RR
from tests.golden import fixtures as FX
from tests.golden import weights as GW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMB = {"xyz": 10, "dir": 4}


def _draws(fx):
    n = len([k for k in fx.inputs if k.startswith("normal_noise_")])
    return [fx.inputs[f"normal_noise_{i}"] for i in range(n)]


@pytest.mark.parametrize("name", ["g8_rough_allmirror", "g8b_rough_l2_partial"])
def test_the_rule_is_the_oracle_where_the_oracle_can_add(name):
    fx = FX.Fixture(name)
    m = fx.meta
    sds = fx.state_dicts()
    models = {"coarse": sds[0], "fine": sds[1]}
    call = (models, EMB, fx.inputs["rays"], m["N_samples"], m["N_importance"], False, m["chunk"], m["args"])
    want = O.render_eval(*call, normal_noise=iter(_draws(fx)))
    got = RR.render_eval_rough(*call, normal_noise=iter(_draws(fx)))
    assert set(got) == set(want)
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
        assert got[k].dtype == want[k].dtype


def test_the_rule_runs_on_a_partly_mirrored_chunk_where_the_oracle_raises():
    fx = FX.Fixture("g7_eval_l1")
    m = fx.meta
    sds = fx.state_dicts()
    models = {"coarse": sds[0], "fine": sds[1]}
    rays = fx.inputs["rays"]
    args = dict(m["args"], app_control_mirror_roughness=True, trace_ray_times=2)
    rs = np.random.RandomState(0)
    draws = [rs.normal(size=(rays.shape[0], 3)).astype(np.float32) for _ in range(3)]
    call = (models, EMB, rays, m["N_samples"], m["N_importance"], False, m["chunk"], args)
    with pytest.raises(ValueError, match="broadcast"):
        O.render_eval(*call, normal_noise=iter(draws))
    got = RR.render_eval_rough(*call, normal_noise=iter(draws))
    mask = got["mirror_mask_fine"] != 0
    assert rays.shape[0] == 96 and int(mask.sum()) == 39
    assert got["rgb_fine"].shape == got["rgb_fine_reflect"].shape == (96, 3) and np.isfinite(got["rgb_fine"]).all()
    # a ray that is no mirror ray: its colour is the frame's without roughness, its reflection the single sample of draw 0
    off = O.render_eval(*call[:-1], dict(args, app_control_mirror_roughness=False))
    one = RR.render_eval_rough(*call[:-1], dict(args, trace_ray_times=0), normal_noise=iter(draws[:1]))
    assert np.array_equal(got["rgb_fine"][~mask], off["rgb_fine"][~mask])
    assert np.array_equal(got["rgb_fine_reflect"][~mask], one["rgb_fine_reflect"][~mask])
    assert not np.array_equal(got["rgb_fine_reflect"][mask], one["rgb_fine_reflect"][mask])


def test_one_mirror_ray_does_not_reach_the_other_rows():
    """STRADDLE, seed 0, synthetic_rays(64, 64)[::3][:200]: one ray of 200 is a mirror ray.  The reference's addition broadcasts
    its jitter colours over all 200 rows of the reflection image; under the rule the other 199 keep the trace_ray_times = 0 rows."""
    sds = [GW.apply_tweaks(sd, GW.STRADDLE) for sd in GW.make_state_dict(0, 2)]
    models = {"coarse": sds[0], "fine": sds[1]}
    rays = O.synthetic_rays(64, 64)[::3][:200].copy()
    args = dict(predict_normal=True, only_one_field=False, only_one_field_fine_epoch=2, max_recursive_level=1,
                app_control_mirror_roughness=True, trace_ray_times=2, normal_noise_std=0.01)
    rs = np.random.RandomState(1)
    draws = [rs.normal(size=(200, 3)).astype(np.float32) for _ in range(3)]
    got = RR.render_eval_rough(models, EMB, rays, 64, 128, False, 200, args, normal_noise=iter(draws))
    one = RR.render_eval_rough(models, EMB, rays, 64, 128, False, 200, dict(args, trace_ray_times=0), normal_noise=iter(draws[:1]))
    mask = got["mirror_mask_fine"] != 0
    assert int(mask.sum()) == 1
    assert np.array_equal(got["rgb_fine_reflect"][~mask], one["rgb_fine_reflect"][~mask])
    broadcast = O.render_eval(models, EMB, rays, 64, 128, False, 200, args, normal_noise=iter(draws))      # no error: M == 1
    assert not np.array_equal(broadcast["rgb_fine_reflect"][~mask], one["rgb_fine_reflect"][~mask])


def test_kernel_restatements_on_small_cases():
    """jitter_mean_ref: the additions in order, the finish, untouched rows; reflect_jitter_fan_ref: block j is the oracle's
    reflection with draw j to within the one rounding that x * (1 / s) and x / s differ by."""
    acc = np.full((5, 3), 7.0, np.float32)
    pieces = np.arange(2 * 2 * 3, dtype=np.float32).reshape(2, 2, 3)
    out = RR.jitter_mean_ref(acc, pieces, [3, 1], RR.MEAN_DIVIDE, 3.0)
    assert np.array_equal(out[[0, 2, 4]], acc[[0, 2, 4]])
    assert np.array_equal(out[3], ((acc[3] + pieces[0, 0]) + pieces[1, 0]) / np.float32(3))
    two = RR.jitter_mean_ref(RR.jitter_mean_ref(acc, pieces[:1], [3, 1]), pieces[1:], [3, 1], RR.MEAN_DIVIDE, 3.0)
    assert np.array_equal(two, out)
    assert RR.finish_value(2, RR.MEAN_MULTIPLY) == np.float32(1) / np.float32(3) and RR.finish_value(2, RR.MEAN_DIVIDE) == 3
    rs = np.random.RandomState(2)
    rays = rs.normal(size=(9, 8)).astype(np.float32)
    xs, nrm = rs.normal(size=(9, 3)).astype(np.float32), rs.normal(size=(9, 3)).astype(np.float32)
    noise = rs.normal(size=(2, 9, 3)).astype(np.float32)
    idx = np.array([0, 4, 8])
    sec = RR.reflect_jitter_fan_ref(rays, xs, nrm, noise, 0.05, idx, 0.1).reshape(2, 3, 8)
    for j in range(2):
        want = O.reflect(rays[idx, 3:6], nrm[idx] + (noise[j][idx] * np.float32(0.05)).astype(np.float32))[0]
        assert np.max(np.abs(sec[j, :, 3:6] - want)) <= 1e-6
        assert np.array_equal(sec[j, :, :3], xs[idx]) and np.array_equal(sec[j, :, 7], rays[idx, 7])
        assert (sec[j, :, 6] == np.float32(0.1)).all()


def _opts(extra):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import eval_scene as ES
    finally:
        sys.path.pop(0)
    return ES, ES.get_opts(["--root_dir", "d", "--ckpt_path", "c", "--out_dir", "o"] + extra)


def test_eval_scene_takes_the_roughness_flags(capsys):
    ES, plain = _opts([])
    assert (plain.app_control_mirror_roughness, plain.trace_ray_times, plain.normal_noise_std, plain.normal_noise_std_changes) == \
        (False, 4, 0.01, False)
    ES, a = _opts(["--app_control_mirror_roughness", "--trace_ray_times", "64", "--normal_noise_std", "0.0025"])
    assert a.app_control_mirror_roughness and a.trace_ray_times == 64 and a.normal_noise_std == 0.0025
    assert [ES.frame_noise_std(a, i, 10) for i in range(10)] == [0.0025] * 10
    ES, c = _opts(["--app_control_mirror_roughness", "--normal_noise_std", "0.01", "--normal_noise_std_changes"])
    want = []
    for i in range(10):                      # eval.py:1130-1136, restated
        progress = i / 10
        cycle = progress * 2 if progress < 0.5 else 1 - (progress - 0.5) * 2
        want.append(0.01 * cycle)
    assert [ES.frame_noise_std(c, i, 10) for i in range(10)] == want
    assert want[0] == 0 and want[5] == 0.01 and want[9] == pytest.approx(0.002)
    for other, text in ((["--app_place_new_mirror"], "app_control_mirror_roughness cannot be combined with app_place_new_mirror"),
                        (["--app_reflect_newly_placed_objects", "--obj_ckpt_path", "x"],
                         "app_reflect_newly_placed_objects cannot be combined with app_control_mirror_roughness"),
                        (["--mirrors_json", "m.json"], "app_control_mirror_roughness cannot be combined with new_mirrors=")):
        with pytest.raises(SystemExit):
            _opts(["--app_control_mirror_roughness"] + other)
        assert text in capsys.readouterr().err
