"""torch.optim.Adam's update in float64 (numpy), the definition csrc/mnrf_optim.hip is held to by tests/test_hip_adam_fp64.py, with
the kernel's own operation order in float32 beside it and the error bounds between the two.  Checked without a GPU by
tests/test_adam_ref_cpu.py: step64 against torch.optim.Adam on float64 CPU tensors, emulate32 against the bounds.

The update (torch/optim/adam.py _single_tensor_adam: non-amsgrad, L2 weight decay, `grad / grad_scale` first as GradScaler's
fused path does), for the effective step t = calls - skipped, at least 1:

    G  = g / grad_scale + weight_decay * p
    m' = m + (1 - beta1) (G - m)
    v' = beta2 v + (1 - beta2) G^2
    p' = p - lr / (1 - beta1^t) * m' / (sqrt(v') / sqrt(1 - beta2^t) + eps)

lr, eps and weight_decay are rounded to float32 first (the C ABI takes them as floats); the betas are exact doubles.

Float32 roundings on each path of the kernel (mnrf_optim.hip adam_body; the library is built with -ffp-contract=off, so every
operation rounds once; u = 2^-24 is half an ulp relative):
  G           1 / grad_scale, g * that, weight_decay * p, the sum                                                   4
  exp_avg     G (4), G - m, (float)(1 - beta1), the product, the sum                                                8
  exp_avg_sq  G (2 x 4), its square, G^2 - v, (float)(1 - beta2), the product, the sum: 13 on the (1 - beta2) G^2 term, 4 on v's   13
  param       |update|: half of exp_avg_sq's under the root (7), the root, the rounded root of bias correction 2, the quotient,
              the sum with eps, m' / that, lr's quotient by the rounded bias correction 1 (2), the product: 15, and exp_avg's
              own error where m' is not small beside |m| + (1 - beta1)(G + |m|); |p'|: the difference, 1           16
The factors of bounds() are those counts rounded up: 8, 16, 16.  emulate32 with 1 - beta rounded once measures at most 3.4, 5.9
and 8.4 on the cases below (tests/test_adam_ref_cpu.py prints them); with 1.f - (float)beta, the kernel before it was held to
this file, 220 in exp_avg_sq and 109 in param.
"""
import math

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -149                   # the smallest float32 denormal: what a result that underflows may lose
FACTORS = {"exp_avg": 8.0, "exp_avg_sq": 16.0, "param": 16.0}

BLOCK = 256 * 4                      # elements per thread block of adam_body
SIZES = (1, 2, 3, 4, 5, 7, 1020, 1023, 1024, 1025, 1027, 3 * 1024 + 2)
WEIGHT_DECAYS = (0.0, 1e-3)
GRAD_SCALES = (None, 65536.0, 3.0)
STEPS = (1, 2, 10, 1000, 100000, 2 ** 31 + 5)
# (calls, skipped) beside the plain steps: a count that did advance past skipped calls, and the clamp (skipped >= calls -> t = 1)
SKIPPED_CASES = ((10, 3), (3, 3), (3, 5))
HYPER = dict(lr=5e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0)


def hyper_of(weight_decay=0.0, **over):
    return dict(HYPER, weight_decay=weight_decay, **over)


def f32(x):
    """x rounded to float32, as a Python float."""
    return float(np.float32(x))


def effective_step(calls, skipped=0):
    return max(1, int(calls) - int(skipped))


def inputs(n, seed=0):
    """p, g, m, v as float32 arrays: p ~ 0.1 N(0,1) with exact zeros, m ~ 1e-3 N(0,1), v in [0, 1e-6], g = N(0,1) 10^U(-28, 2)
    with every seventh entry 0 (from index 3, so that n = 1 is an ordinary element and n = 4 has the corner), v = 0 at every
    other of those (the m / eps corner), and at index 115 p = g = v = 0 together."""
    r = np.random.default_rng(1000 * seed + n)
    p = (0.1 * r.standard_normal(n)).astype(np.float32)
    m = (1e-3 * r.standard_normal(n)).astype(np.float32)
    v = (1e-6 * r.random(n)).astype(np.float32)
    g = (r.standard_normal(n) * 10.0 ** r.uniform(-28.0, 2.0, n)).astype(np.float32)
    g[3::7] = 0.0
    v[3::14] = 0.0
    p[5::11] = 0.0
    assert float(np.abs(g).max(initial=0.0)) < 1e15          # g^2 stays finite in float32
    return p, g, m, v


def fresh_gradient(n, k, seed=0):
    """The gradient of step k of the many-step test: the same distribution as inputs()'s, other zeros at every step."""
    r = np.random.default_rng(7919 * (seed + 1) + 31 * k + n)
    g = (r.standard_normal(n) * 10.0 ** r.uniform(-28.0, 2.0, n)).astype(np.float32)
    g[k % 7::7] = 0.0
    return g


def cases():
    """(weight_decay, grad_scale, calls, skipped) of the one-step test, at every size of SIZES."""
    out = [(wd, gs, t, 0) for wd in WEIGHT_DECAYS for gs in GRAD_SCALES for t in STEPS]
    out += [(wd, gs, c, s) for wd in WEIGHT_DECAYS for gs in (None, 3.0) for c, s in SKIPPED_CASES]
    return out


def _parts64(p, g, m, v, hyper, t, grad_scale):
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    lr, eps, wd = f32(hyper["lr"]), f32(hyper["eps"]), f32(hyper["weight_decay"])
    b1, b2 = float(hyper["beta1"]), float(hyper["beta2"])
    t = float(max(1, int(t)))
    gr = g / float(grad_scale) if grad_scale is not None else g
    if wd != 0.0:
        gr = gr + wd * p
    m2 = m + (1.0 - b1) * (gr - m)
    v2 = b2 * v + (1.0 - b2) * gr * gr
    step_size = lr / (1.0 - b1 ** t)
    denom = np.sqrt(v2) / math.sqrt(1.0 - b2 ** t) + eps
    update = step_size * (m2 / denom)
    return p - update, m2, v2, update


def step64(p, g, m, v, hyper, t, grad_scale=None):
    """One update -> (p', m', v') in float64.  `t` is the effective step (effective_step)."""
    return _parts64(p, g, m, v, hyper, t, grad_scale)[:3]


def state64(hyper, t, grad_scale=None, veto=False):
    """The eight scalars mnrf_adam_prep publishes for the effective step t, exact in double: [veto, lr / bias correction 1,
    sqrt(bias correction 2), 1 - beta1, 1 - beta2, 1 / grad_scale, eps, weight_decay]."""
    lr, eps, wd = f32(hyper["lr"]), f32(hyper["eps"]), f32(hyper["weight_decay"])
    b1, b2 = float(hyper["beta1"]), float(hyper["beta2"])
    t = float(max(1, int(t)))
    return np.array([1.0 if veto else 0.0, lr / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t), 1.0 - b1, 1.0 - b2,
                     1.0 / float(grad_scale) if grad_scale is not None else 1.0, eps, wd], dtype=np.float64)


def emulate32(p, g, m, v, hyper, t, grad_scale=None, exact_one_minus_beta=True, lerp_second_moment=None):
    """adam_body's operation order in float32, one rounding per operation -> (p', m', v') as float32.  exact_one_minus_beta=True is
    the kernel: (float)(1 - beta) made in double, both moments as x + (1 - beta)(new - x).  False is the kernel before it was held
    to step64: 1.f - (float)beta, and v' = (float)beta2 * v + (1.f - (float)beta2) * G * G.  lerp_second_moment=False with
    exact_one_minus_beta=True is the form NOT taken: (float)beta2 * v + (float)(1 - beta2) * G * G, two weights rounded apart."""
    f = np.float32
    p, g, m, v = (np.asarray(a, dtype=f) for a in (p, g, m, v))
    b1, b2 = float(hyper["beta1"]), float(hyper["beta2"])
    t = float(max(1, int(t)))
    lr, eps, wd = f(hyper["lr"]), f(hyper["eps"]), f(hyper["weight_decay"])
    step_size = lr / f(1.0 - b1 ** t)
    bc2_sqrt = f(math.sqrt(1.0 - b2 ** t))
    fb2 = f(b2)
    omb1, omb2 = (f(1.0 - b1), f(1.0 - b2)) if exact_one_minus_beta else (f(1.0) - f(b1), f(1.0) - fb2)
    inv_scale = f(1.0) / f(grad_scale) if grad_scale is not None else f(1.0)
    lerp_v = exact_one_minus_beta if lerp_second_moment is None else lerp_second_moment
    with np.errstate(under="ignore"):
        gr = g * inv_scale if inv_scale != f(1.0) else g
        if wd != f(0.0):
            gr = gr + wd * p
        m2 = m + omb1 * (gr - m)
        v2 = v + omb2 * (gr * gr - v) if lerp_v else fb2 * v + omb2 * gr * gr
        denom = np.sqrt(v2) / bc2_sqrt + eps
        p2 = p - step_size * (m2 / denom)
    assert p2.dtype == f and m2.dtype == f and v2.dtype == f
    return p2, m2, v2


def scales(p, g, m, v, hyper, t, grad_scale=None):
    """The magnitudes the errors are measured in, per element: {"exp_avg": |m| + (1 - beta1)(G + |m|), "exp_avg_sq": beta2 v +
    (1 - beta2) G^2, "param": |p'| + |update|} with G = |g| / grad_scale + weight_decay |p|."""
    p64, g64, m64, v64 = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1, b2 = float(hyper["beta1"]), float(hyper["beta2"])
    G = np.abs(g64) / (float(grad_scale) if grad_scale is not None else 1.0) + f32(hyper["weight_decay"]) * np.abs(p64)
    p2, _m2, _v2, update = _parts64(p, g, m, v, hyper, t, grad_scale)
    return {"exp_avg": np.abs(m64) + (1.0 - b1) * (G + np.abs(m64)),
            "exp_avg_sq": b2 * v64 + (1.0 - b2) * G * G,
            "param": np.abs(p2) + np.abs(update)}


def bounds(p, g, m, v, hyper, t, grad_scale=None):
    """Per-element error bounds of one float32 step against step64: FACTORS[k] * u * scales()[k] + 2^-149."""
    return {k: FACTORS[k] * U * s + TINY for k, s in scales(p, g, m, v, hyper, t, grad_scale).items()}


def in_units(got, want, scale, steps=1):
    """The largest error of `got` against `want` in units of u * scale, past the 2^-149 every bound allows (inf where the scale is
    zero and the error is not within 2^-149).  `steps`: how many updates `got` has carried float32 state through -- each may have
    lost 2^-149 to underflow."""
    err = np.maximum(np.abs(np.asarray(got, dtype=np.float64) - want) - steps * TINY, 0.0)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / (U * scale))
    return float(q.max())
