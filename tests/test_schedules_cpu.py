"""mirror_nerf_amd/schedules.py against tests/golden/schedules/lr_sequences.json: 40 epochs of torch's schedulers behind the
reference's warm-up class, recorded by tests/golden/make_golden_schedules.py.

Tolerance 2^-40 relative.  The fixture's sequences are torch's RECURSIVE double sequences (a factor per milestone, a ratio of
cosines per epoch), lr_at is a closed form: either carries a few float64 roundings per epoch at most, about 40 * 4 * 2^-53 =
2^-46 over 40 epochs (more near the cosine's minimum, where 1 + cos cancels: 2^-52 / 0.0055 = 2^-44.5 at the epoch after it);
a float32 ulp, the precision the kernels take the rate in, is 2^-24."""
import json
import os
from types import SimpleNamespace

import pytest

from mirror_nerf_amd import schedules as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2.0 ** -40


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "schedules", "lr_sequences.json")) as f:
        return json.load(f)


def _hp(meta, options, **over):
    return SimpleNamespace(**dict(dict(options, lr=meta["lr"], optimizer=meta["optimizer"]), **over))


def test_lr_at_follows_the_recorded_sequences(fixture):
    meta = fixture["meta"]
    assert sorted(fixture["cases"]) == ["cosine", "poly", "poly_warmup_m1", "poly_warmup_m2", "steplr_default", "steplr_driver",
                                        "steplr_run_sh", "steplr_warmup_m1", "steplr_warmup_m2"]
    worst = {}
    for name, case in fixture["cases"].items():
        sched = S.lr_schedule(_hp(meta, case["options"]))
        want = case["lr"]
        assert len(want) == meta["epochs"] == 40
        got = [sched.lr_at(e) for e in range(len(want))]
        worst[name] = max(abs(g - w) / w for g, w in zip(got, want))
    print("largest relative difference from the recorded sequences (torch " + meta["torch"] + "):", worst)
    assert all(w <= TOL for w in worst.values()), worst
    # run.sh's recipe, as the issue quotes it
    run_sh = [S.lr_schedule(_hp(meta, fixture["cases"]["steplr_run_sh"]["options"])).lr_at(e) for e in range(9)]
    assert run_sh == [5e-4, 5e-4, 2.5e-4, 2.5e-4, 1.25e-4, 1.25e-4, 1.25e-4, 1.25e-4, 6.25e-5]


def test_warm_up_is_for_sgd_and_adam_only(fixture):
    """utils/__init__.py:93: in front of radam (and ranger) the warm-up options are ignored -- the plain schedule's sequence."""
    meta = fixture["meta"]
    plain, warm = fixture["cases"]["steplr_run_sh"], fixture["cases"]["steplr_warmup_m2"]
    for optimizer, want in (("radam", plain["lr"]), ("ranger", plain["lr"]), ("sgd", warm["lr"]), ("adam", warm["lr"])):
        sched = S.lr_schedule(_hp(meta, warm["options"], optimizer=optimizer))
        assert all(abs(sched.lr_at(e) - w) <= TOL * w for e, w in enumerate(want)), optimizer


def test_refusals(fixture):
    meta = fixture["meta"]
    cosine = fixture["refused"]["cosine_warmup_w3_12"]
    with pytest.raises(ValueError, match="warm-up in front of cosine"):
        S.lr_schedule(_hp(meta, cosine["options"]))
    # what the reference's class does there is no cosine from lr * multiplier: above the base rate at epoch 4
    assert cosine["lr"][4] > meta["lr"] * 1.01
    S.lr_schedule(_hp(meta, cosine["options"], optimizer="radam"))              # (no warm-up in front of radam: nothing to refuse)
    with pytest.raises(ValueError, match="not recognized"):
        S.lr_schedule(SimpleNamespace(lr_scheduler="exponential"))
    with pytest.raises(ValueError, match="warmup_multiplier"):
        S.lr_schedule(SimpleNamespace(warmup_epochs=2, warmup_multiplier=0.5))
    poly = S.lr_schedule(SimpleNamespace(lr_scheduler="poly", num_epochs=4))
    assert poly.lr_at(4) == 0.0
    with pytest.raises(ValueError, match="past it"):
        poly.lr_at(5)
    with pytest.raises(ValueError, match="epoch >= 0"):
        poly.lr_at(-1)


def test_defaults_are_the_reference_options():
    """opt.py:82, 113-153: steplr at epoch 20 by 0.1 from 5e-4, no warm-up."""
    sched = S.lr_schedule(SimpleNamespace())
    assert [sched.lr_at(e) for e in (0, 19, 20, 39)] == [5e-4, 5e-4, 5e-4 * 0.1, 5e-4 * 0.1]
    assert sched.options["num_epochs"] == 16 and sched.options["warmup_epochs"] == 0


def test_state_round_trips_and_refuses_another_schedule():
    hp = SimpleNamespace(lr=1e-3, lr_scheduler="steplr", decay_step=(1, 2), decay_gamma=0.5, num_epochs=3)
    a = S.lr_schedule(hp)
    groups = SimpleNamespace(param_groups=[{"lr": 0.0}, {"lr": 0.0}])
    assert a.apply(groups, 2) == 2.5e-4 and [g["lr"] for g in groups.param_groups] == [2.5e-4, 2.5e-4]
    sd = json.loads(json.dumps(a.state_dict()))                    # plain data: survives a checkpoint's containers
    assert sd["epoch"] == 2 and sd["options"]["decay_step"] == [1, 2]
    b = S.lr_schedule(hp)
    assert b.epoch is None
    b.load_state_dict(sd)
    assert b.epoch == 2 and b.state_dict() == a.state_dict() and b.lr_at(2) == a.lr_at(2)
    other = S.lr_schedule(SimpleNamespace(lr=1e-3, lr_scheduler="steplr", decay_step=(1, 3), decay_gamma=0.5, num_epochs=3))
    with pytest.raises(ValueError, match="decay_step"):
        other.load_state_dict(sd)
