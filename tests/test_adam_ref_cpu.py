"""tests/adam_ref.py without a GPU: the float64 restatement against torch.optim.Adam on float64 CPU tensors, the veto bookkeeping,
and the float32 emulation of mnrf_optim.hip's operation order against the bounds tests/test_hip_adam_fp64.py holds the kernel to
-- inside them with 1 - beta rounded once, far outside with 1.f - (float)beta, so the bounds are attainable and they discriminate.
"""
import numpy as np
import pytest
import torch

from tests import adam_ref as R


@pytest.mark.parametrize("weight_decay", R.WEIGHT_DECAYS)
def test_step64_is_torch_adam_in_float64(weight_decay):
    """Five steps of step64 carrying its own state against torch.optim.Adam(foreach=False) on float64 tensors, parameter and both
    moments to 1e-13 relative (of each tensor's largest entry at least: the parameter update is a difference)."""
    n = 1027
    hyper = R.hyper_of(weight_decay)
    p, _g, _m, _v = R.inputs(n)
    a = torch.nn.Parameter(torch.from_numpy(p.astype(np.float64)))
    opt = torch.optim.Adam([a], lr=R.f32(hyper["lr"]), betas=(hyper["beta1"], hyper["beta2"]), eps=R.f32(hyper["eps"]),
                           weight_decay=R.f32(hyper["weight_decay"]), foreach=False)
    p64, m64, v64 = p.astype(np.float64), np.zeros(n), np.zeros(n)
    for t in range(1, 6):
        g = R.fresh_gradient(n, t).astype(np.float64)
        a.grad = torch.from_numpy(g.copy())
        opt.step()
        p64, m64, v64 = R.step64(p64, g, m64, v64, hyper, t)
        st = opt.state[a]
        for name, got, want in (("param", p64, a.detach().numpy()), ("exp_avg", m64, st["exp_avg"].numpy()),
                                ("exp_avg_sq", v64, st["exp_avg_sq"].numpy())):
            err = np.abs(got - want)
            assert np.all(err <= 1e-13 * np.maximum(np.abs(want), 1e-3 * np.abs(want).max())), (t, name, float(err.max()))


def test_grad_scale_divides_the_gradient_first():
    p, g, m, v = R.inputs(1027)
    hyper = R.hyper_of(1e-3)
    for a, b in zip(R.step64(p, g, m, v, hyper, 3, grad_scale=3.0), R.step64(p, g.astype(np.float64) / 3.0, m, v, hyper, 3)):
        assert np.array_equal(a, b)


def test_a_vetoed_call_does_not_count():
    """The caller's bookkeeping as the kernels keep it: calls advance always, skipped on a veto, the update is made for calls -
    skipped (at least 1), and a vetoed call changes nothing."""
    hyper = R.hyper_of(1e-3)
    p, g, m, v = (a.astype(np.float64) for a in R.inputs(1027))
    calls = skipped = 0
    state = (p, m, v)
    plain = (p, m, v)
    for k, veto in enumerate((False, True, False)):
        calls += 1
        if veto:
            skipped += 1                                    # (and nothing is computed)
            continue
        state = R.step64(state[0], g, state[1], state[2], hyper, R.effective_step(calls, skipped))
    for t in (1, 2):                                        # two real steps, no veto in between
        plain = R.step64(plain[0], g, plain[1], plain[2], hyper, t)
    assert calls == 3 and skipped == 1 and R.effective_step(calls, skipped) == 2
    assert all(np.array_equal(a, b) for a, b in zip(state, plain))
    assert R.effective_step(3, 5) == 1 and R.effective_step(3, 3) == 1 and R.effective_step(2 ** 31 + 5, 0) == 2 ** 31 + 5
    assert R.state64(hyper, 2, None, veto=True)[0] == 1.0 and R.state64(hyper, 2)[0] == 0.0


def _worst(exact):
    worst = {k: 0.0 for k in R.FACTORS}
    for n in R.SIZES:
        p, g, m, v = R.inputs(n)
        for wd, gs, calls, skipped in R.cases():
            hyper, t = R.hyper_of(wd), R.effective_step(calls, skipped)
            want = dict(zip(("param", "exp_avg", "exp_avg_sq"), R.step64(p, g, m, v, hyper, t, gs)))
            got = dict(zip(("param", "exp_avg", "exp_avg_sq"), R.emulate32(p, g, m, v, hyper, t, gs, exact_one_minus_beta=exact)))
            sc = R.scales(p, g, m, v, hyper, t, gs)
            bd = R.bounds(p, g, m, v, hyper, t, gs)
            for k in worst:
                e = R.in_units(got[k], want[k], sc[k])
                worst[k] = max(worst[k], e)
                if exact:
                    assert np.all(np.abs(got[k].astype(np.float64) - want[k]) <= bd[k]), (n, wd, gs, calls, skipped, k, e)
    return worst


def test_emulation_with_one_minus_beta_rounded_once_is_inside_the_bounds():
    worst = _worst(True)
    print("float32 emulation, 1 - beta rounded once, worst error in units of u * scale:", worst)
    for k, w in worst.items():
        assert w <= R.FACTORS[k], (k, w)
    # the margin hides nothing: the bounds are at most four times what the arithmetic reaches
    assert worst["exp_avg_sq"] >= R.FACTORS["exp_avg_sq"] / 4 and worst["exp_avg"] >= R.FACTORS["exp_avg"] / 4


def test_emulation_with_float_one_minus_float_beta_leaves_the_bounds():
    worst = _worst(False)
    print("float32 emulation, 1.f - (float)beta, worst error in units of u * scale:", worst)
    assert worst["exp_avg_sq"] > 10 * R.FACTORS["exp_avg_sq"], worst
    assert worst["param"] > R.FACTORS["param"], worst


def test_second_moment_weights_sum_to_one_over_many_steps():
    """Why the kernel updates exp_avg_sq as v + (1 - beta2)(G^2 - v) and uses no beta2 in float: with (float)beta2 and (float)(1 -
    beta2) rounded apart the two weights sum to 1 + 1.3e-8, which a single step cannot show (it is inside the bound) and 1 / (1 -
    beta2) steps turn into a bias of 1.3e-5 of v, the very size of the error of 1.f - (float)beta2 in one step.  N(0,1) gradients,
    the float32 chains against the float64 chain: the mean deviation over 2000 elements is a bias, the rounding noise averages out
    (it is under u = 6e-8 per step and element)."""
    f, n = np.float32, 2000
    hyper, r, z = R.hyper_of(), np.random.default_rng(0), np.zeros(2000, np.float32)
    forms = {"kernel": (True, True), "apart": (True, False), "before": (False, False)}
    v32, v64, bias = {k: z.copy() for k in forms}, np.zeros(n), {}
    for k in range(1, 2001):
        g = r.standard_normal(n).astype(f)
        for name, (exact, lerp) in forms.items():
            v32[name] = R.emulate32(z, g, z, v32[name], hyper, 1, None, exact, lerp)[2]
        v64 = R.step64(z, g, z, v64, hyper, 1)[2]
        if k in (20, 2000):
            bias[k] = {name: float(np.mean(v / v64 - 1.0)) for name, v in v32.items()}
    print("mean of v32 / v64 - 1 after 20 and 2000 steps:", bias)
    assert abs(bias[20]["kernel"]) <= 2e-7 and abs(bias[2000]["kernel"]) <= 2e-7
    assert bias[20]["before"] < -1e-5                      # 1.f - (float)0.999 is 1.3e-5 short: every early step is
    assert bias[2000]["apart"] > 5e-6                      # rounded apart: on the way to +1.3e-5
