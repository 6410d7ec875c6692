"""torch.optim.SGD's and torch.optim.RAdam's updates in float64 (numpy), the definitions the SGD and RAdam kernels of
csrc/mnrf_optim.hip are held to by tests/test_hip_optim_fp64.py, with the kernels' own operation order in float32 beside them and
the error bounds between the two.  Checked without a GPU by tests/test_optim_ref_cpu.py: sgd64 / radam64 against torch's optimizers
on float64 CPU tensors, the emulations against the bounds.  The inputs, sizes, gradient scales, weight decays and skipped-count
cases are tests/adam_ref.py's.

SGD (torch/optim/sgd.py _single_tensor_sgd: dampening 0, no Nesterov, L2 weight decay, `grad / grad_scale` first):

    G    = g / grad_scale + weight_decay * p
    buf' = momentum * buf + G                     (a zero buffer makes the first step torch's buf = G)
    p'   = p - lr * buf'

RAdam (torch/optim/radam.py _single_tensor_radam, decoupled_weight_decay=False), for the effective step t = calls - skipped, at
least 1:

    G  = g / grad_scale + weight_decay * p
    m' = m + (1 - beta1) (G - m)
    v' = beta2 v + (1 - beta2) G^2
    rho_inf = 2 / (1 - beta2) - 1,  rho_t = rho_inf - 2 t beta2^t / (1 - beta2^t)
    rho_t > 5:  p' = p - lr / (1 - beta1^t) * sqrt(1 - beta2^t) * r_t * m' / (sqrt(v') + eps)
                r_t = sqrt((rho_t - 4)(rho_t - 2) rho_inf / ((rho_inf - 4)(rho_inf - 2) rho_t))
    else:       p' = p - lr / (1 - beta1^t) * m'

lr, momentum, eps and weight_decay are rounded to float32 first (the C ABI takes them as floats); the betas are exact doubles.

Float32 roundings on each path of the kernels (sgd_body, radam_body; the library is built with -ffp-contract=off, so every
operation rounds once; u = 2^-24 is half an ulp relative).  A state quantity is measured in the sum of the magnitudes of its terms
(cancellation between them does not shrink the unit).  The parameter has two sources of error: the roundings of its own path,
counted in |p'| + |update|, and the error its state input arrives with, which the update multiplies by K = d update / d state --
so its bound is  F u (|p'| + |update|) + K * (the state's bound), and no cancellation inside the state is hidden in F.

  G           1 / grad_scale, g * that, weight_decay * p, the sum                                                   4
  SGD buf     G (4, on G's share), fmaf(momentum, buf, G): at most 5 on |momentum buf| + |G|                        5 -> 8
  SGD param   fmaf(-lr, buf', p): 1 (2 allowed: sgd_emulate32 forms the fused operation in float64 and rounds that to float32,
              two roundings where the kernel has one); K = lr on buf's bound                                        1 -> 2
  exp_avg     G (4), G - m, (float)(1 - beta1), the product, the sum                                                8
  exp_avg_sq  G (2 x 4), its square, G^2 - v, (float)(1 - beta2), the product, the sum: 13 on the (1 - beta2) G^2 term  13 -> 16
  RAdam param, rectified   a = (lr / (float)bc1) * (float)(sqrt(bc2) r_t): the rounded bc1, the quotient, the rounded product of
              the roots, the product: 4; the denominator: half of exp_avg_sq's 13 under the root (7), the root, the sum with eps:
              9; m' / that: 1; a * that: 1; the difference: 1; K = a / (sqrt(v') + eps) on exp_avg's bound          16
  RAdam param, not rectified   lr / (float)bc1 (2), the product with m', the difference; K = lr / bc1 on exp_avg's bound    4
Every bound also allows 4 * 2^-149: up to four products on a path (g / grad_scale, weight_decay p, the state's product, the
update's) may underflow and lose half a denormal each, and the result may.

rho_t and r_t are formed in double on either side; near the threshold rho_t - 4 is a difference of numbers near rho_inf = 1999,
exact to about 1999 * 2^-52 = 4e-13 of a quantity that is at least 1 where it is used -- far below u.
"""
import math

import numpy as np

from tests import adam_ref as A

U, TINY, f32 = A.U, A.TINY, A.f32
UNDERFLOW = 4 * TINY
SIZES, WEIGHT_DECAYS, GRAD_SCALES, SKIPPED_CASES = A.SIZES, A.WEIGHT_DECAYS, A.GRAD_SCALES, A.SKIPPED_CASES
inputs, fresh_gradient, effective_step, in_units = A.inputs, A.fresh_gradient, A.effective_step, A.in_units

SGD_FACTORS = {"momentum_buffer": 8.0, "param": 2.0}
RADAM_FACTORS = {"exp_avg": 8.0, "exp_avg_sq": 16.0, "param": 16.0, "param_unrectified": 4.0}
SGD_HYPER = dict(lr=5e-4, momentum=0.9, weight_decay=0.0)
RADAM_HYPER = dict(A.HYPER)


def sgd_hyper(weight_decay=0.0, **over):
    return dict(SGD_HYPER, weight_decay=weight_decay, **over)


def radam_hyper(weight_decay=0.0, **over):
    return dict(RADAM_HYPER, weight_decay=weight_decay, **over)


# ------------------------------------------------------------------------------------------------------------------ RAdam's scalars
def rho(beta2, t):
    """(rho_inf, rho_t) in double."""
    t = float(max(1, int(t)))
    b2t = beta2 ** t
    rho_inf = 2.0 / (1.0 - beta2) - 1.0
    return rho_inf, rho_inf - 2.0 * t * b2t / (1.0 - b2t)


def rectified(beta2, t):
    return rho(beta2, t)[1] > 5.0


def first_rectified_step(beta2):
    """The smallest t with rho_t > 5 (rho_t grows with t), found by walking the formula."""
    t = 1
    while not rectified(beta2, t):
        t += 1
        assert t < 10 ** 6
    return t


def radam_steps(beta2=RADAM_HYPER["beta2"]):
    """The steps of the one-step test: 1, the last unrectified and the first rectified step, then adam_ref's large ones."""
    k = first_rectified_step(beta2)
    assert k > 2 and not rectified(beta2, k - 1) and rectified(beta2, k)
    return tuple(sorted({1, k - 1, k, 10, 1000, 100000, 2 ** 31 + 5}))


def rect_term(beta2, t):
    """sqrt(1 - beta2^t) r_t in double, or None where the step is not rectified."""
    rho_inf, rho_t = rho(beta2, t)
    if not rho_t > 5.0:
        return None
    t = float(max(1, int(t)))
    r = math.sqrt((rho_t - 4.0) * (rho_t - 2.0) * rho_inf / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho_t))
    return math.sqrt(1.0 - beta2 ** t) * r


def sgd_cases():
    """(weight_decay, grad_scale, calls, skipped): SGD's update does not depend on the step, so one plain count beside the
    skipped-count cases."""
    return [(wd, gs, c, s) for wd in WEIGHT_DECAYS for gs in GRAD_SCALES for c, s in ((1, 0), (2 ** 31 + 5, 0)) + SKIPPED_CASES]


def radam_cases():
    out = [(wd, gs, t, 0) for wd in WEIGHT_DECAYS for gs in GRAD_SCALES for t in radam_steps()]
    out += [(wd, gs, c, s) for wd in WEIGHT_DECAYS for gs in (None, 3.0) for c, s in SKIPPED_CASES]
    return out


def _grad64(p, g, wd, grad_scale):
    gr = g / float(grad_scale) if grad_scale is not None else g
    return gr + wd * p if wd != 0.0 else gr


def _abs_grad(p, g, wd, grad_scale):
    return np.abs(g) / (float(grad_scale) if grad_scale is not None else 1.0) + wd * np.abs(p)


# ------------------------------------------------------------------------------------------------------------------------------ SGD
def _sgd_parts(p, g, buf, hyper, grad_scale):
    p, g, buf = (np.asarray(a, dtype=np.float64) for a in (p, g, buf))
    lr, mu, wd = f32(hyper["lr"]), f32(hyper["momentum"]), f32(hyper["weight_decay"])
    b2 = mu * buf + _grad64(p, g, wd, grad_scale)
    update = lr * b2
    return p - update, b2, update, np.abs(mu * buf) + _abs_grad(p, g, wd, grad_scale), lr


def sgd64(p, g, buf, hyper, grad_scale=None):
    """One update -> (p', buf') in float64."""
    return _sgd_parts(p, g, buf, hyper, grad_scale)[:2]


def sgd_state64(hyper, grad_scale=None, veto=False):
    """The five scalars mnrf_sgd_prep publishes: [veto, lr, momentum, 1 / grad_scale, weight_decay]."""
    return np.array([1.0 if veto else 0.0, f32(hyper["lr"]), f32(hyper["momentum"]),
                     1.0 / float(grad_scale) if grad_scale is not None else 1.0, f32(hyper["weight_decay"])], dtype=np.float64)


def sgd_emulate32(p, g, buf, hyper, grad_scale=None):
    """sgd_body's operation order in float32 -> (p', buf') as float32: G with one rounding per operation, the two fused
    multiply-adds as float64 expressions rounded to float32 (the product of two floats is exact in float64; the sum then rounds
    to 53 bits before it rounds to 24, which differs from the fused result only where the first rounding lands on a tie)."""
    f = np.float32
    p, g, buf = (np.asarray(a, dtype=f) for a in (p, g, buf))
    lr, mu, wd = f(hyper["lr"]), f(hyper["momentum"]), f(hyper["weight_decay"])
    inv_scale = f(1.0) / f(grad_scale) if grad_scale is not None else f(1.0)
    with np.errstate(under="ignore"):
        gr = g * inv_scale if inv_scale != f(1.0) else g
        if wd != f(0.0):
            gr = gr + wd * p
        b2 = (np.float64(mu) * buf.astype(np.float64) + gr.astype(np.float64)).astype(f)
        p2 = (p.astype(np.float64) - np.float64(lr) * b2.astype(np.float64)).astype(f)
    assert p2.dtype == f and b2.dtype == f
    return p2, b2


def sgd_scales(p, g, buf, hyper, grad_scale=None):
    p2, _b2, update, sb, _lr = _sgd_parts(p, g, buf, hyper, grad_scale)
    return {"momentum_buffer": sb, "param": np.abs(p2) + np.abs(update)}


def sgd_bounds(p, g, buf, hyper, grad_scale=None, U=U):
    """Per-element bounds of one float32 step against sgd64 (the derivation is the module's doc string).  `U`: the half-ulp of
    another format (2^-53: the same count for a float64 implementation against exact arithmetic)."""
    p2, _b2, update, sb, lr = _sgd_parts(p, g, buf, hyper, grad_scale)
    b = SGD_FACTORS["momentum_buffer"] * U * sb + UNDERFLOW
    return {"momentum_buffer": b, "param": SGD_FACTORS["param"] * U * (np.abs(p2) + np.abs(update)) + lr * b + UNDERFLOW}


# ---------------------------------------------------------------------------------------------------------------------------- RAdam
def _radam_parts(p, g, m, v, hyper, t, grad_scale):
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    lr, eps, wd = f32(hyper["lr"]), f32(hyper["eps"]), f32(hyper["weight_decay"])
    b1, b2 = float(hyper["beta1"]), float(hyper["beta2"])
    tf = float(max(1, int(t)))
    gr = _grad64(p, g, wd, grad_scale)
    m2 = m + (1.0 - b1) * (gr - m)
    v2 = b2 * v + (1.0 - b2) * gr * gr
    step_size = lr / (1.0 - b1 ** tf)
    c = rect_term(b2, t)
    K = step_size * c / (np.sqrt(v2) + eps) if c is not None else np.full_like(p, step_size)      # d update / d m'
    update = K * m2
    return p - update, m2, v2, update, K


def radam64(p, g, m, v, hyper, t, grad_scale=None):
    """One update -> (p', m', v') in float64.  `t` is the effective step."""
    return _radam_parts(p, g, m, v, hyper, t, grad_scale)[:3]


def radam_state64(hyper, t, grad_scale=None, veto=False):
    """The nine scalars mnrf_radam_prep publishes for the effective step t, exact in double: [veto, lr / bias correction 1,
    sqrt(bias correction 2) r_t or 0, 1 - beta1, 1 - beta2, 1 / grad_scale, eps, weight_decay, rectified]."""
    lr, eps, wd = f32(hyper["lr"]), f32(hyper["eps"]), f32(hyper["weight_decay"])
    b1, b2 = float(hyper["beta1"]), float(hyper["beta2"])
    c = rect_term(b2, t)
    tf = float(max(1, int(t)))
    return np.array([1.0 if veto else 0.0, lr / (1.0 - b1 ** tf), 0.0 if c is None else c, 1.0 - b1, 1.0 - b2,
                     1.0 / float(grad_scale) if grad_scale is not None else 1.0, eps, wd, 0.0 if c is None else 1.0], dtype=np.float64)


def radam_emulate32(p, g, m, v, hyper, t, grad_scale=None):
    """radam_body's operation order in float32, one rounding per operation -> (p', m', v') as float32."""
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    b1, b2 = float(hyper["beta1"]), float(hyper["beta2"])
    tf = float(max(1, int(t)))
    lr, eps, wd = f(hyper["lr"]), f(hyper["eps"]), f(hyper["weight_decay"])
    step_size = lr / f(1.0 - b1 ** tf)
    c = rect_term(b2, t)
    omb1, omb2 = f(1.0 - b1), f(1.0 - b2)
    inv_scale = f(1.0) / f(grad_scale) if grad_scale is not None else f(1.0)
    with np.errstate(under="ignore"):
        gr = g * inv_scale if inv_scale != f(1.0) else g
        if wd != f(0.0):
            gr = gr + wd * p
        m2 = m + omb1 * (gr - m)
        v2 = v + omb2 * (gr * gr - v)
        if c is not None:
            a = step_size * f(c)
            p2 = p - a * (m2 / (np.sqrt(v2) + eps))
        else:
            p2 = p - step_size * m2
    assert p2.dtype == f and m2.dtype == f and v2.dtype == f
    return p2, m2, v2


def _radam_state_scales(p, g, m, v, hyper, grad_scale):
    p64, g64, m64, v64 = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1, b2 = float(hyper["beta1"]), float(hyper["beta2"])
    G = _abs_grad(p64, g64, f32(hyper["weight_decay"]), grad_scale)
    return np.abs(m64) + (1.0 - b1) * (G + np.abs(m64)), b2 * v64 + (1.0 - b2) * G * G


def radam_scales(p, g, m, v, hyper, t, grad_scale=None):
    sm, sv = _radam_state_scales(p, g, m, v, hyper, grad_scale)
    p2, _m2, _v2, update, _K = _radam_parts(p, g, m, v, hyper, t, grad_scale)
    return {"exp_avg": sm, "exp_avg_sq": sv, "param": np.abs(p2) + np.abs(update)}


def radam_bounds(p, g, m, v, hyper, t, grad_scale=None, U=U):
    """Per-element bounds of one float32 step against radam64 (the derivation is the module's doc string); `U` as sgd_bounds'."""
    sm, sv = _radam_state_scales(p, g, m, v, hyper, grad_scale)
    p2, _m2, _v2, update, K = _radam_parts(p, g, m, v, hyper, t, grad_scale)
    bm = RADAM_FACTORS["exp_avg"] * U * sm + UNDERFLOW
    F = RADAM_FACTORS["param" if rectified(float(hyper["beta2"]), t) else "param_unrectified"]
    return {"exp_avg": bm, "exp_avg_sq": RADAM_FACTORS["exp_avg_sq"] * U * sv + UNDERFLOW,
            "param": F * U * (np.abs(p2) + np.abs(update)) + K * bm + UNDERFLOW}


def radam_sensitivity(p, g, m, v, hyper, t, grad_scale=None):
    """(K, |update|, v'): K = d update / d m' per element -- what an error that exp_avg carries in is multiplied by -- and what
    a relative error of v' scales (it passes into the update halved at most, under the root)."""
    _p2, _m2, v2, update, K = _radam_parts(p, g, m, v, hyper, t, grad_scale)
    return K, np.abs(update), v2


def in_bound_units(got, want, bound):
    """The largest error of `got` against `want` as a fraction of its bound."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    return float((err / bound).max()) if err.size else 0.0
