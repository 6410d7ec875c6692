"""tests/optim_ref.py without a GPU: sgd64 and radam64 against torch.optim.SGD and torch.optim.RAdam on float64 CPU tensors (the
definitions hold to a few float64 ulps), RAdam's threshold steps from the formula, and the float32 emulations of sgd_body's and
radam_body's operation order against the bounds tests/test_hip_optim_fp64.py holds the kernels to.  The measured maxima are
printed."""
import numpy as np
import pytest
import torch

from tests import optim_ref as R

U64 = 2.0 ** -53


def _close64(got, want, bound, what):
    """Two float64 implementations of one update each stay inside the one-step bound counted for half-ulp 2^-53 (they take no
    more roundings than the float32 kernel), so after one step they differ by twice that at most.  Over several steps either
    carries its state: `bound` is then the sum of the steps' bounds, an earlier step's error being passed on by the later ones
    with a factor of at most one into the state and by the update's sensitivity into the parameter (the callers add that up)."""
    err = np.abs(got - want)
    assert np.all(err <= 2.0 * bound), (what, float((err / bound).max()))


@pytest.mark.parametrize("momentum", [0.9, 0.0])
@pytest.mark.parametrize("weight_decay", R.WEIGHT_DECAYS)
def test_sgd64_is_torch_sgd_in_float64(weight_decay, momentum):
    """Six steps of sgd64 from a ZERO buffer against torch.optim.SGD(foreach=False) on float64 tensors: torch's first step clones
    the gradient into the buffer, momentum * 0 + G is the same number."""
    n = 1027
    hyper = R.sgd_hyper(weight_decay, momentum=momentum)
    p = R.inputs(n)[0]
    a = torch.nn.Parameter(torch.from_numpy(p.astype(np.float64)))
    opt = torch.optim.SGD([a], lr=R.f32(hyper["lr"]), momentum=R.f32(momentum), weight_decay=R.f32(weight_decay), foreach=False)
    p64, b64 = p.astype(np.float64), np.zeros(n)
    acc = {"param": np.zeros(n), "momentum_buffer": np.zeros(n)}
    for t in range(1, 7):
        g = R.fresh_gradient(n, t).astype(np.float64)
        a.grad = torch.from_numpy(g.copy())
        opt.step()
        bd = R.sgd_bounds(p64, g, b64, hyper, U=U64)
        # the buffer's carried error comes in times momentum (+ weight_decay times the parameter's), the parameter's own times one
        acc["param"] += bd["param"] + R.f32(hyper["lr"]) * acc["momentum_buffer"]
        acc["momentum_buffer"] += bd["momentum_buffer"] + R.f32(weight_decay) * acc["param"]
        p64, b64 = R.sgd64(p64, g, b64, hyper)
        _close64(p64, a.detach().numpy(), acc["param"], ("param", t))
        if momentum:
            _close64(b64, opt.state[a]["momentum_buffer"].numpy(), acc["momentum_buffer"], ("momentum_buffer", t))


@pytest.mark.parametrize("weight_decay", R.WEIGHT_DECAYS)
def test_radam64_is_torch_radam_in_float64(weight_decay):
    """Nine steps of radam64 -- five unrectified, four rectified with beta2 = 0.999 -- against torch.optim.RAdam(foreach=False)."""
    n = 1027
    hyper = R.radam_hyper(weight_decay)
    p = R.inputs(n)[0]
    a = torch.nn.Parameter(torch.from_numpy(p.astype(np.float64)))
    opt = torch.optim.RAdam([a], lr=R.f32(hyper["lr"]), betas=(hyper["beta1"], hyper["beta2"]), eps=R.f32(hyper["eps"]),
                            weight_decay=R.f32(weight_decay), foreach=False)
    p64, m64, v64 = p.astype(np.float64), np.zeros(n), np.zeros(n)
    acc = {k: np.zeros(n) for k in ("param", "exp_avg", "exp_avg_sq")}
    assert R.first_rectified_step(hyper["beta2"]) in range(3, 9)
    for t in range(1, 10):
        g = R.fresh_gradient(n, t).astype(np.float64)
        a.grad = torch.from_numpy(g.copy())
        opt.step()
        bd = R.radam_bounds(p64, g, m64, v64, hyper, t, U=U64)
        K, upd, v2 = R.radam_sensitivity(p64, g, m64, v64, hyper, t)
        # carried errors: exp_avg's reaches the parameter times K, exp_avg_sq's relative one halved under the root
        with np.errstate(divide="ignore", invalid="ignore"):
            via_v = np.where(v2 > 0.0, 0.5 * acc["exp_avg_sq"] / v2 * upd, 0.0) if R.rectified(hyper["beta2"], t) else 0.0
        acc["param"] += bd["param"] + K * acc["exp_avg"] + via_v
        G = np.abs(g) + R.f32(weight_decay) * np.abs(p64)
        acc["exp_avg"] += bd["exp_avg"] + R.f32(weight_decay) * acc["param"]
        acc["exp_avg_sq"] += bd["exp_avg_sq"] + 2.0 * G * R.f32(weight_decay) * acc["param"]
        p64, m64, v64 = R.radam64(p64, g, m64, v64, hyper, t)
        st = opt.state[a]
        for name, got, want in (("param", p64, a.detach().numpy()), ("exp_avg", m64, st["exp_avg"].numpy()),
                                ("exp_avg_sq", v64, st["exp_avg_sq"].numpy())):
            _close64(got, want, acc[name], (name, t))


def test_threshold_steps_come_from_the_formula():
    """rho_t grows with t; with beta2 = 0.999 rho_5 = 4.99 and rho_6 = 5.99 (rho_t is close to t for small t), so step 6 is the
    first rectified one; with beta2 = 0.9 (rho_inf = 19) it is step 6 too, with beta2 = 0.5 (rho_inf = 3) no step ever is."""
    k = R.first_rectified_step(0.999)
    assert k == 6 and R.rho(0.999, 5)[1] <= 5.0 < R.rho(0.999, 6)[1]
    assert R.radam_steps() == (1, 5, 6, 10, 1000, 100000, 2 ** 31 + 5)
    assert all(R.rho(0.999, t + 1)[1] > R.rho(0.999, t)[1] for t in range(1, 200))
    assert R.rect_term(0.999, 5) is None and 0.0 < R.rect_term(0.999, 6) < R.rect_term(0.999, 7) < 1.0
    assert abs(R.rect_term(0.999, 2 ** 31 + 5) - 1.0) < 1e-12             # beta2^t = 0: rho_t = rho_inf, r_t = 1
    assert not any(R.rectified(0.5, t) for t in (1, 10, 1000, 10 ** 6))
    st = R.radam_state64(R.radam_hyper(), 5)
    assert st[2] == 0.0 and st[8] == 0.0 and R.radam_state64(R.radam_hyper(), 6)[8] == 1.0


def test_grad_scale_divides_the_gradient_first():
    p, g, m, v = R.inputs(1027)
    g64 = g.astype(np.float64)
    for a, b in zip(R.sgd64(p, g, m, R.sgd_hyper(1e-3), grad_scale=3.0), R.sgd64(p, g64 / 3.0, m, R.sgd_hyper(1e-3))):
        assert np.array_equal(a, b)
    for t in (3, 9):
        for a, b in zip(R.radam64(p, g, m, v, R.radam_hyper(1e-3), t, grad_scale=3.0), R.radam64(p, g64 / 3.0, m, v, R.radam_hyper(1e-3), t)):
            assert np.array_equal(a, b)


def test_sgd_emulation_is_inside_the_bounds():
    worst = {k: 0.0 for k in R.SGD_FACTORS}
    units = {k: 0.0 for k in R.SGD_FACTORS}
    for n in R.SIZES:
        p, g, m, _v = R.inputs(n)
        for buf in (m, np.zeros_like(m)):
            for wd, gs, _calls, _skipped in R.sgd_cases():
                hyper = R.sgd_hyper(wd)
                want = dict(zip(("param", "momentum_buffer"), R.sgd64(p, g, buf, hyper, gs)))
                got = dict(zip(("param", "momentum_buffer"), R.sgd_emulate32(p, g, buf, hyper, gs)))
                bd, sc = R.sgd_bounds(p, g, buf, hyper, gs), R.sgd_scales(p, g, buf, hyper, gs)
                for k in worst:
                    worst[k] = max(worst[k], R.in_bound_units(got[k], want[k], bd[k]))
                    units[k] = max(units[k], R.in_units(got[k], want[k], sc[k], steps=4))
    print("SGD float32 emulation: largest error as a fraction of its bound", worst, "; in units of u * scale", units)
    assert all(w <= 1.0 for w in worst.values()), worst
    assert worst["momentum_buffer"] >= 0.1          # the margin hides nothing: the arithmetic reaches a tenth of the bound at least


def test_radam_emulation_is_inside_the_bounds():
    names = ("param", "exp_avg", "exp_avg_sq")
    worst = {(k, r): 0.0 for k in names for r in (False, True)}
    units = dict(worst)
    for n in R.SIZES:
        p, g, m, v = R.inputs(n)
        for wd, gs, calls, skipped in R.radam_cases():
            hyper, t = R.radam_hyper(wd), R.effective_step(calls, skipped)
            rect = R.rectified(hyper["beta2"], t)
            want = dict(zip(names, R.radam64(p, g, m, v, hyper, t, gs)))
            got = dict(zip(names, R.radam_emulate32(p, g, m, v, hyper, t, gs)))
            bd, sc = R.radam_bounds(p, g, m, v, hyper, t, gs), R.radam_scales(p, g, m, v, hyper, t, gs)
            for k in names:
                worst[k, rect] = max(worst[k, rect], R.in_bound_units(got[k], want[k], bd[k]))
                units[k, rect] = max(units[k, rect], R.in_units(got[k], want[k], sc[k], steps=4))
    print("RAdam float32 emulation (quantity, rectified): largest error as a fraction of its bound", worst)
    print("... and in units of u * scale", units)
    assert all(w <= 1.0 for w in worst.values()), worst
    assert worst["exp_avg_sq", True] >= 0.25 and worst["exp_avg", True] >= 0.25      # as adam_ref's: at most four times the reach


def test_a_wrong_branch_leaves_the_bounds():
    """The bounds discriminate: the rectified update taken at the last unrectified step, and the other way round at the first
    rectified one, are far outside the parameter's bound."""
    p, g, m, v = R.inputs(1027)
    hyper = R.radam_hyper()
    k = R.first_rectified_step(hyper["beta2"])
    for t, other in ((k - 1, k), (k, k - 1)):
        want = R.radam64(p, g, m, v, hyper, t)[0]
        wrong = R.radam_emulate32(p, g, m, v, hyper, other)[0]
        assert R.in_bound_units(wrong, want, R.radam_bounds(p, g, m, v, hyper, t)["param"]) > 100.0
