"""The per-ray kernels of csrc/mnrf_render.hip / mnrf_composite.inc against float64 restatements (tests/torch_ref.py, proven
against the numpy oracle on the CPU by tests/test_torch_ref_cpu.py), at their block and range edges.

Every comparison is PER RAY: the largest error of a ray's row over the largest float64 entry of that row (`_row_rel`); a row
whose reference is exactly zero must be met by exact zeros, and a non-finite output where float64 is finite never passes.

Bars.  None is invented: for every comparison the same test also runs the float32 torch restatement (TR.* in float32, same
inputs, same GPU) against float64; the kernel's bar is the largest such figure of the regime times 4, rounded up to one digit
(the kernel's scans associate differently from torch's cumprod / sums).  `BARS` holds, per group and regime, the restatement's
measured error, the bar derived from it and what the kernel reached on the MI355X.  Where the float32 restatement of a ray is
itself non-finite the ray's bar is 1e-6 of its largest float64 entry instead (`_judge`).

One deviation from "a zero row is met by exact zeros": a row whose float64 entries are all below the smallest normal float32
(1.2e-38: 1e-10^k behind k >= 4 opaque samples) cannot be held by a float32 output; it must be met by entries below that same
number, zero or denormal (`_row_rel`), an absolute bound of 1.2e-38.  Inputs: tests/rays_cases.py (seeded, synthetic)."""
import math

import pytest
import torch

from tests import rays_cases as RC
from tests import torch_ref as TR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MNRF_ERR_UNSUPPORTED = -3
SENT = -777.25          # what output rows nobody may write are filled with
NAN = float("nan")

OUT_NAMES = ("weights", "opacity", "rgb", "depth", "mask", "sn", "sng", "nd", "xs")
GRAD_NAMES = ("sigma", "rgb", "m", "pn", "nrm", "rays")
OUT_NEEDS = dict(rgb=("rgb",), mask=("m",), sn=("pn",), sng=("nrm",), nd=("pn", "nrm"), xs=("rays",))    # include/mnrf.h

# (group, regime) -> (the float32 restatement's largest per-ray error against float64, measured on the MI355X over every case of
# this file that uses the key (`thin` and `opaque_straddle`: the absent-input and detach tests too); the kernel's bar = 4 x that,
# rounded up to one digit; the largest per-ray error the kernel reached over the same cases, every ray counted)
BARS = {
    ("composite_fwd", "thin"): (3.191e-06, 2e-05, 3.191e-06),
    ("composite_fwd", "opaque_inside"): (1.759e-06, 8e-06, 1.759e-06),
    ("composite_fwd", "opaque_straddle"): (3.721e-06, 2e-05, 3.721e-06),
    ("composite_fwd", "opaque_first"): (5.247e-07, 3e-06, 1.950e-07),
    ("composite_fwd", "opaque_last"): (4.547e-06, 2e-05, 4.083e-06),
    ("composite_fwd", "opaque_two"): (2.377e-06, 1e-05, 2.928e-06),
    ("composite_fwd", "empty"): (0.000e+00, 0, 0.000e+00),
    ("composite_fwd", "empty_zero"): (0.000e+00, 0, 0.000e+00),
    ("composite_fwd", "last_only"): (7.071e-07, 3e-06, 7.576e-07),
    ("composite_fwd", "duplicate"): (2.171e-06, 9e-06, 2.545e-06),
    ("composite_fwd", "noise"): (2.190e-06, 9e-06, 1.982e-06),
    ("composite_bwd", "thin"): (1.654e-05, 7e-05, 9.429e-06),
    ("composite_bwd", "opaque_inside"): (1.412e-06, 6e-06, 2.328e-06),
    ("composite_bwd", "opaque_straddle"): (2.941e-06, 2e-05, 4.220e-06),
    ("composite_bwd", "opaque_first"): (1.448e-05, 6e-05, 1.252e-05),
    ("composite_bwd", "opaque_last"): (3.038e-06, 2e-05, 1.016e-06),
    ("composite_bwd", "opaque_two"): (7.809e-07, 4e-06, 8.646e-07),
    ("composite_bwd", "empty"): (0.000e+00, 0, 0.000e+00),
    ("composite_bwd", "empty_zero"): (0.000e+00, 0, 0.000e+00),
    ("composite_bwd", "last_only"): (9.371e-06, 4e-05, 9.439e-06),
    ("composite_bwd", "duplicate"): (1.360e-06, 6e-06, 1.744e-06),
    ("composite_bwd", "noise"): (9.765e-06, 4e-05, 4.704e-06),
    ("resample", "uniform"): (5.085e-07, 3e-06, 2.583e-07),
    ("resample", "zero"): (9.244e-07, 4e-06, 4.486e-07),
    ("resample", "hot_1"): (1.450e-07, 6e-07, 1.256e-07),
    ("resample", "hot_S-2"): (1.133e-07, 5e-07, 1.133e-07),
    ("resample", "hot_0"): (1.318e-06, 6e-06, 4.848e-07),
    ("resample", "hot_S-1"): (1.270e-06, 6e-06, 3.734e-07),
    ("resample", "pow8"): (3.128e-05, 0.0002, 2.635e-05),
    ("reflect", "fwd"): (6.651e-07, 3e-06, 7.697e-07),
    ("reflect", "bwd"): (9.913e-06, 4e-05, 1.940e-05),
    ("embed_bwd", "F0"): (0.000e+00, 0, 0.000e+00),
    ("embed_bwd", "F1"): (7.348e-06, 3e-05, 2.451e-06),
    ("embed_bwd", "F4"): (5.358e-05, 0.0003, 1.910e-05),
    ("embed_bwd", "F10"): (2.126e-05, 9e-05, 1.525e-05),
    ("ray_grads", "all"): (3.034e-07, 2e-06, 2.983e-07),
}


def _bar(group, regime):
    return BARS[(group, regime)][1]


def _lib():
    from mirror_nerf_amd import _lib as L
    return L


FLT_MIN = 1.1754943508222875e-38      # the smallest normal float32


def _row_rel(got, ref):
    """(N,) float64: per ray, max |got - ref| / max |ref|; 0 for an exact-zero row met by zeros; inf for a wrong zero row or a
    non-finite output.  A row whose float64 entries are all below the smallest normal float32 (1e-10^k behind k opaque samples,
    or exp(-delta sigma) of a dense last sample) cannot be held by a float32 output at all: it is met by entries that are
    themselves below that number (zero or denormal), which counts as 0, and by nothing else."""
    n = ref.shape[0]
    g, r = got.double().reshape(n, -1), ref.double().reshape(n, -1)
    err = (g - r).abs().amax(1)
    scale = r.abs().amax(1)
    inf, zero = torch.full_like(err, math.inf), torch.zeros_like(err)
    rel = torch.where(scale >= FLT_MIN, err / scale.clamp_min(FLT_MIN),
                      torch.where(scale > 0, torch.where(g.abs().amax(1) < FLT_MIN, zero, inf), torch.where(err == 0, zero, inf)))
    return torch.where(torch.isfinite(g).all(1), rel, inf)


REST_POOLED = 1e-4      # the regime's figure is taken over the rays whose float32 restatement is within this of float64


def _judge(figs, group, regime, name, got, ref64, ref32):
    """Per-ray verdict of one tensor.  Every ray is held to the regime's bar (BARS), except that a ray whose float32
    restatement is not finite is held to 1e-6 of its largest float64 entry.  The regime's figure itself is the restatement's
    largest error over the rays where it is within 1e-4 of float64: on a few rays of 2 or 3 samples torch's float32
    `1 - alphas + 1e-10` rounds a transmittance of 3e-9 to 1e-10 and is up to 9 % off; counting them would widen the bar of
    every other ray, and the kernels (the backward takes the exponential itself) are held to the regime's bar there as well.
    How many rays may be left out is bounded by `_report`.  Appends (name, the regime figure of this tensor, the kernel's
    largest error over ALL rays, rays outside the pool) to figs; returns the failures."""
    ek = _row_rel(got, ref64)
    er = _row_rel(ref32, ref64)
    pooled = er <= REST_POOLED
    bar = torch.where(torch.isfinite(er), torch.full_like(ek, _bar(group, regime)), torch.full_like(ek, 1e-6))
    figs.append((name, float(er[pooled].max()) if bool(pooled.any()) else 0.0, float(ek.max()), int((~pooled).sum())))
    bad = (ek > bar).nonzero().flatten().tolist()
    return [(name, i, float(ek[i]), float(bar[i])) for i in bad]


def _report(group, regime, case, figs, unpooled_allowed=None):
    """Prints the figures of a case and bounds the rays that `_judge` left out of the regime's figure: none, except the tensors
    that `unpooled_allowed` names with their number.  Without a bound the pool could shrink until the figure said nothing."""
    for name, er, ek, n_inf in figs:
        print(f"FIG {group} {regime} {case} {name} rest={er:.3e} kern={ek:.3e} unpooled_rays={n_inf}")
    over = [(name, n_inf) for name, _, _, n_inf in figs if n_inf > (unpooled_allowed or {}).get(name, 0)]
    assert not over, (group, regime, case, "rays left out of the restatement's figure", over)


# The only rays whose float32 restatement is more than REST_POOLED off: d_sigma on rays of 2 or 3 samples, where a sample with a
# transmittance below 1e-7 behind it (lost by float32's `1 - alpha + 1e-10`) can hold the row's largest gradient; from 63 samples
# on, some thin sample always holds a larger one.  Of the 100 rays that a regime has per S (n_rays 1 + 3 + 4 + 5 + 37, white_back
# 0 and 1) at most 5; measured on the MI355X: 4 (thin, S = 3) and 2 (noise, S = 3), none anywhere else.
UNPOOLED_SHORT_RAYS = 5


# ------------------------------------------------------------------------------------------------ compositing
def _to(c, dtype=None):
    return {k: (None if v is None else (v.to(DEV) if dtype is None else v.to(DEV, dtype))) for k, v in c.items()}


def _outs_allowed(c):
    return tuple(k for k in OUT_NAMES if all(c[i] is not None for i in OUT_NEEDS.get(k, ())))


def _out_shape(k, N, S):
    return {"weights": (N, S), "rgb": (N, 3), "sn": (N, 3), "sng": (N, 3), "xs": (N, 3)}.get(k, (N,))


def hip_composite(c, white, want, n_live=None, fill=NAN, S=None):
    L = _lib()
    p = L.ptr
    N, S = c["z"].shape if S is None else (c["z"].shape[0], S)
    out = {k: (torch.full(_out_shape(k, N, S), fill, device=DEV) if k in want else None) for k in OUT_NAMES}
    args = [p(c["rays"]), N, S, p(c["sigma"]), p(c["z"]), p(c["noise"]), p(c["rgb"]), p(c["m"]), p(c["pn"]), p(c["nrm"]), int(white)]
    args += [p(out[k]) for k in OUT_NAMES]
    if n_live is None:
        code = L.lib().mnrf_composite(*args, L.stream())
    else:
        code = L.lib().mnrf_composite_n(*args, p(n_live), L.stream())
    return code, out


def _grad_shape(k, N, S):
    return {"sigma": (N, S), "rgb": (N, S, 3), "m": (N, S), "pn": (N, S, 3), "nrm": (N, S, 3), "rays": (N, 8)}[k]


def hip_composite_backward(c, white, weights, depth, cot, want, detach=0, keep=None, n_live=None, fill=NAN, S=None):
    L = _lib()
    p = L.ptr
    N, S = c["z"].shape if S is None else (c["z"].shape[0], S)
    d = {k: (torch.full(_grad_shape(k, N, S), fill, device=DEV) if k in want else None) for k in GRAD_NAMES}
    args = [p(c["rays"]), N, S, p(c["sigma"]), p(c["z"]), p(c["noise"]), p(c["rgb"]), p(c["m"]), p(c["pn"]), p(c["nrm"]), int(white),
            p(weights), p(depth)]
    args += [p(cot.get(k)) for k in OUT_NAMES] + [p(d[k]) for k in GRAD_NAMES] + [int(detach), p(keep)]
    if n_live is None:
        code = L.lib().mnrf_composite_backward(*args, L.stream())
    else:
        code = L.lib().mnrf_composite_backward_n(*args, p(n_live), L.stream())
    return code, d


def ref_composite(c, white, dtype, cot, want_out, want_grad, detach=0, keep=None):
    """TR.composite in `dtype` with autograd: (outputs, gradients) restricted to the wanted names.  Absent inputs are zeros whose
    outputs nobody reads."""
    N, S = c["z"].shape
    leaf = {}
    for k in GRAD_NAMES:
        shape = _grad_shape(k, N, S)
        v = c[k].to(dtype).reshape(shape) if c[k] is not None else torch.zeros(shape, device=DEV, dtype=dtype)
        leaf[k] = v.clone().requires_grad_(True)
    noise = None if c["noise"] is None else c["noise"].to(dtype)
    L = _lib()
    out = TR.composite(leaf["rays"], leaf["sigma"], c["z"].to(dtype), noise, leaf["rgb"], leaf["m"], leaf["pn"],
                       leaf["nrm"] if c["nrm"] is not None else None, bool(white), detach_mask=bool(detach & L.MNRF_DETACH_W_MASK),
                       keep_mirror=None if keep is None else keep != 0, detach_normal=bool(detach & L.MNRF_DETACH_W_NORMAL))
    out = {k: out[k] for k in want_out}
    grads = {}
    if want_grad:
        loss = sum((out[k] * cot[k].to(dtype)).sum() for k in want_out if cot.get(k) is not None)
        g = torch.autograd.grad(loss, [leaf[k] for k in want_grad], allow_unused=True)
        grads = {k: (torch.zeros_like(leaf[k]) if t is None else t) for k, t in zip(want_grad, g)}
    return {k: v.detach() for k, v in out.items()}, grads


def _cotangents(N, S, names, g):
    return {k: torch.randn(*_out_shape(k, N, S), generator=g).to(DEV) for k in names}


def _composite_check(c_cpu, regime, white, figs, absent=(), detach=0, keep=None, null_cot=()):
    """One forward and one backward launch against float64; returns the failures."""
    c = _to(c_cpu)
    for k in absent:
        c[k] = None
    N, S = c["z"].shape
    outs = _outs_allowed(c)
    grads = tuple(k for k in GRAD_NAMES if c[k] is not None)
    cot = _cotangents(N, S, [k for k in outs if k not in null_cot], RC.gen("cot", S, N, regime))
    code, got = hip_composite(c, white, outs)
    assert code == 0
    torch.cuda.synchronize()
    ref64, g64 = ref_composite(c, white, torch.float64, cot, outs, grads, detach, keep)
    ref32, g32 = ref_composite(c, white, torch.float32, cot, outs, grads, detach, keep)
    bad = []
    for k in outs:
        bad += _judge(figs, "composite_fwd", regime, k, got[k], ref64[k], ref32[k])
    if S <= 256:
        need_depth = "rays" in grads
        code, d = hip_composite_backward(c, white, got["weights"], got["depth"] if need_depth else None, cot, grads, detach,
                                         None if keep is None else keep.float())
        assert code == 0
        torch.cuda.synchronize()
        if "rays" in grads and cot.get("xs") is not None:      # the entry point takes the forward's depth as an input: so does the reference
            for gg, dep in ((g64, got["depth"].double()), (g32, got["depth"])):
                gg["rays"] = gg["rays"].clone()
                gg["rays"][:, 3:6] = cot["xs"].to(gg["rays"].dtype) * dep[:, None]
        for k in grads:
            bad += _judge(figs, "composite_bwd", regime, "d_" + k, d[k], g64[k], g32[k])
            if regime in ("empty", "empty_zero") and k == "sigma":
                assert not bool(d[k].any()), "d_sigma of an empty ray must be exactly 0"
    if regime in ("empty", "empty_zero"):
        assert not bool(got["weights"].any()), "weights of an empty ray must be exactly 0"
    return bad


def _regimes_for(S):
    return [r for r in RC.COMPOSITE_REGIMES if not (r == "opaque_straddle" and S <= 64)]


@pytest.mark.parametrize("S", RC.COMPOSITE_S + (257, 320))
def test_composite_forward_and_backward_against_float64(S):
    """mnrf_composite and mnrf_composite_backward (forward only at S = 257, 320) in every density regime, n_rays 1, 3, 4, 5 and
    37 (four rays per workgroup), white_back 0 and 1, cotangents on every output.  The opaque runs have sigma * delta >= 40, so
    alpha is exactly 1 in float32 and in float64 and t = 1e-10 in both: the comparison is of the scans, not of exp's last bit.
    Figures (restatement, bar, kernel): BARS, groups composite_fwd and composite_bwd.

    This test found the one kernel error of the file.  The backward formed 1 - alpha again from the rounded alpha = 1 - exp(..),
    in d alpha / d sigma = delta (1 - alpha) and in its own t = 1 - alpha + 1e-10: 0 once alpha is within an ulp of 1, a few ulp
    of 1 off before that.  Where such a sample carries the ray's largest gradient, on rays of 2 or 3 samples, d_sigma missed by
    up to 100 % of the row:
      - thin, S = 2, n_rays = 5, white_back = 1, ray 3 (sigma = 4.28, delta = 4.53, exp = 3.8e-9): d_sigma[0] is 5.3e-8 in
        float64 and the kernel returned 0;
      - duplicate, S = 3, n_rays = 5, ray 1 (alpha = 0.99999994): 22 % off;
      - thin, S = 3, n_rays = 4, ray 3: T[1] was 1e-10 for 2.9e-9, and d_sigma[1] was off by 9 % of the row;
      - the same at S = 2 and 3 in noise, opaque_inside and opaque_last;
      - opaque_first at every S up to 256: the opaque sample's own delta * exp(-40) is the largest entry of a row that lies
        at 1e-20, and the kernel returned 0 for it.
    The backward now takes the exponential itself in both places, and these rays meet the bar of their regime.  The forward
    keeps the reference's float32 expression: there the lost 3e-9 is 3e-9 of the ray's largest weight, and every ray meets
    composite_fwd.  float32 torch has the same loss: on the few rays named `unpooled_rays` in the printed figures it is up to
    9 % off, which is why those rays stay out of the regime's figure (`_judge`) and why their number is bounded below."""
    bad = []
    for regime in _regimes_for(S):
        figs = []
        for N, white in ((N, white) for N in (1, 3, 4, 5, 37) for white in (0, 1)):
            bad += [(regime, N, white) + b for b in _composite_check(RC.composite_inputs(S, N, regime), regime, white, figs)]
        agg = {}
        for name, er, ek, n_inf in figs:
            a = agg.setdefault(name, [0.0, 0.0, 0])
            a[0], a[1], a[2] = max(a[0], er), max(a[1], ek), a[2] + n_inf
        _report("composite", regime, f"S={S}", [(k,) + tuple(v) for k, v in agg.items()],
                {"d_sigma": UNPOOLED_SHORT_RAYS} if S in (2, 3) else None)
    assert not bad, bad[:20]


def test_composite_backward_refuses_more_than_four_blocks():
    """S = 257 is one sample past CB_MAXB * 64: MNRF_ERR_UNSUPPORTED, and nothing is written."""
    c = _to(RC.composite_inputs(257, 5, "thin"))
    cot = _cotangents(5, 257, OUT_NAMES, RC.gen("cot257"))
    w, dep = torch.rand(5, 257, device=DEV), torch.rand(5, device=DEV)
    code, d = hip_composite_backward(c, 0, w, dep, cot, GRAD_NAMES, fill=SENT)
    torch.cuda.synchronize()
    assert code == MNRF_ERR_UNSUPPORTED
    assert all(bool((t == SENT).all()) for t in d.values())


@pytest.mark.parametrize("absent", ["rgb", "m", "pn", "nrm", "rays", "noise", "cotangents"])
def test_composite_optional_inputs_absent_in_turn(absent):
    """Each optional input null in turn, with only the outputs the header allows; `cotangents`: every other upstream gradient
    null (null means zero)."""
    bad, figs = [], []
    for S, regime in ((65, "thin"), (192, "opaque_straddle")):
        c = RC.composite_inputs(S, 5, regime)
        if absent == "cotangents":
            bad += _composite_check(c, regime, 1, figs, null_cot=OUT_NAMES[::2])
            bad += _composite_check(c, regime, 0, figs, null_cot=OUT_NAMES[1::2])
        else:
            bad += _composite_check(c, regime, 1, figs, absent=(absent,))
    _report("composite", "absent", absent, figs)
    assert not bad, bad[:20]


@pytest.mark.parametrize("S", [65, 192])
@pytest.mark.parametrize("mode", ["none", "mask", "normal", "both", "keep"])
def test_composite_backward_detach_and_keep_mirror(S, mode):
    """models/rendering.py:223-247: the mirror mask / the normal outputs composited with weights.detach(), per ray with
    keep_mirror."""
    L = _lib()
    detach = {"none": 0, "mask": L.MNRF_DETACH_W_MASK, "normal": L.MNRF_DETACH_W_NORMAL, "both": L.MNRF_DETACH_W_MASK | L.MNRF_DETACH_W_NORMAL,
              "keep": 0}[mode]
    bad, figs = [], []
    for regime in ("thin", "opaque_straddle"):
        N = 37
        keep = (torch.arange(N, device=DEV) % 3 != 0) if mode == "keep" else None
        bad += _composite_check(RC.composite_inputs(S, N, regime), regime, 0, figs, detach=detach, keep=keep)
    _report("composite", "detach", f"S={S},{mode}", figs)
    assert not bad, bad[:20]


# ------------------------------------------------------------------------------------------------ resampling
def hip_sample_fine(z, w, u, n_imp, n_live=None, fill=NAN, S=None):
    L = _lib()
    p = L.ptr
    N = z.shape[0]
    S = z.shape[1] if S is None else S
    out = torch.full((N, S + n_imp), fill, device=DEV)
    args = [p(z), p(w), N, S, p(u), 1 if u.dim() == 2 else 0, n_imp, p(out)]
    code = L.lib().mnrf_sample_fine(*args, L.stream()) if n_live is None else L.lib().mnrf_sample_fine_n(*args, p(n_live), L.stream())
    torch.cuda.synchronize()
    return code, out


def _fine_part(row, coarse):
    """The sorted row minus the coarse depths as a multiset (both ascending lists); None if they are not a sub-multiset."""
    fine, j = [], 0
    for v in row:
        if j < len(coarse) and v == coarse[j]:
            j += 1
        else:
            fine.append(v)
    return fine if j == len(coarse) else None


@pytest.mark.parametrize("per_ray", [False, True])
@pytest.mark.parametrize("S,n_imp", RC.RESAMPLE_SHAPES)
def test_sample_fine_against_float64(S, n_imp, per_ray):
    """mnrf_sample_fine at every total that selects another register sort (64, 128, 256, 512 values) or sits beside one, n_rays
    1 and 5, shared and per-ray u, in every weight regime.  For EVERY sample: the row is sorted, finite, S + n_importance long,
    holds the coarse depths as a sub-multiset, and every fine sample lies in [mid[0], mid[-1]].  Values against TR.sample_pdf in
    float64 (float32 inputs as given), fine samples matched in the order of u (the inverse cdf is monotone), leaving out only
    what RC.resample_undecided names: at most 2 % of a case and never a whole ray."""
    bad, figs = [], []
    for N in (1, 5):
        for regime in RC.RESAMPLE_REGIMES:
            z, w, u = RC.resample_inputs(S, n_imp, N, regime, per_ray)
            code, got = hip_sample_fine(z.to(DEV), w.to(DEV), u.to(DEV), n_imp)
            assert code == 0
            got = got.cpu()
            assert got.shape == (N, S + n_imp) and bool(torch.isfinite(got).all())
            assert bool((got[:, 1:] >= got[:, :-1]).all()), "not sorted"
            mid = TR.mids(z)
            ref64, cdf, u64, raw, span = TR.sample_pdf_info(TR.mids(z.double()), w.double()[:, 1:-1], n_imp, u.double())
            ref32 = TR.sample_pdf(TR.mids(z.to(DEV)), w.to(DEV)[:, 1:-1], n_imp, u.to(DEV)).cpu()      # the restatement: on the GPU too
            skip = RC.resample_undecided(cdf, u64, raw, per_ray)
            assert float(skip.float().mean()) <= 0.02 and not bool(skip.all(1).any())
            order = torch.sort(u64, dim=1, stable=True)[1]
            fine = []
            for i in range(N):
                f = _fine_part(got[i].tolist(), z[i].tolist())
                assert f is not None and len(f) == n_imp, "the coarse depths are not a sub-multiset of the row"
                fine.append(f)
            fine = torch.tensor(fine, dtype=torch.float32)
            assert bool((fine >= mid[:, :1]).all() and (fine <= mid[:, -1:]).all()), "a fine sample outside [mid[0], mid[-1]]"
            r64, r32, sk = torch.gather(ref64, 1, order), torch.gather(ref32, 1, order), torch.gather(skip, 1, order)
            keep = (~sk).double()
            scale = ref64.abs().amax(1)
            ek = ((fine.double() - r64).abs() * keep).amax(1) / scale
            er = ((r32.double() - r64).abs() * keep).amax(1) / scale
            figs.append((f"N={N},{regime}", float(er.max()), float(ek.max()), 0))
            bar = _bar("resample", regime)
            bad += [(N, regime, i, float(ek[i])) for i in (ek > bar).nonzero().flatten().tolist()]
    for name, er, ek, _ in figs:
        print(f"FIG resample {name.split(',')[1]} S={S},n={n_imp},per_ray={per_ray},{name.split(',')[0]} z_fine rest={er:.3e} kern={ek:.3e}")
    assert not bad, bad[:20]


@pytest.mark.parametrize("S,n_imp", [(256, 257), (257, 1), (257, 255)])
def test_sample_fine_refuses_what_does_not_fit(S, n_imp):
    z, w = torch.rand(5, S, device=DEV), torch.rand(5, S, device=DEV)
    code, out = hip_sample_fine(z, w, torch.rand(n_imp, device=DEV), n_imp, fill=SENT)
    assert code == MNRF_ERR_UNSUPPORTED and bool((out == SENT).all())


@pytest.mark.parametrize("per_ray", [False, True])
@pytest.mark.parametrize("S,n_imp", RC.RESAMPLE_SHAPES)
def test_composite_sample_is_composite_then_sample_fine_bit_for_bit(S, n_imp, per_ray):
    L = _lib()
    p = L.ptr
    for N in (1, 5):
        for regime, white in (("thin", 1), ("opaque_inside", 0)):
            c = _to(RC.composite_inputs(S, N, regime))
            _, _, u = RC.resample_inputs(S, n_imp, N, "uniform", per_ray)
            u = u.to(DEV)
            live = torch.tensor([N], dtype=torch.int32, device=DEV)
            code, a = hip_composite(c, white, OUT_NAMES, n_live=live)
            assert code == 0
            code, za = hip_sample_fine(c["z"], a["weights"], u, n_imp, n_live=live)
            assert code == 0
            b = {k: torch.full(_out_shape(k, N, S), NAN, device=DEV) for k in OUT_NAMES}
            zb = torch.full((N, S + n_imp), NAN, device=DEV)
            code = L.lib().mnrf_composite_sample_n(
                p(c["rays"]), N, S, p(c["sigma"]), p(c["z"]), p(c["noise"]), p(c["rgb"]), p(c["m"]), p(c["pn"]), p(c["nrm"]), white,
                *[p(b[k]) for k in OUT_NAMES], p(u), int(per_ray), n_imp, p(zb), p(live), L.stream())
            torch.cuda.synchronize()
            assert code == 0
            for k in OUT_NAMES:
                assert torch.equal(a[k], b[k]), (N, regime, k)
            assert torch.equal(za, zb), (N, regime)


# ------------------------------------------------------------------------------------------------ glue kernels
GLUE_N = (0, 1, 1023, 1024, 1025, 2500)


def _glue_inputs(N, frac, soft, noise):
    g = RC.gen("glue", N, frac, soft, noise)
    rays, xs, normal = torch.randn(N, 8, generator=g), torch.randn(N, 3, generator=g), torch.randn(N, 3, generator=g)
    mask = (torch.rand(N, generator=g) < frac).float()
    if N > 1:
        normal[N // 2] = 0.0           # a zero normal
        normal[N // 3] = 1e-20         # and one inside the eps clamp of l2_normalize
    if soft and N:
        mask[N - 1] = 0.5              # a soft entry: selected, blended half and half
    nn = torch.randn(N, 3, generator=g) if noise else None
    return [None if t is None else t.to(DEV) for t in (rays, xs, normal, mask, nn)]


def hip_reflect_compact(rays, xs, normal, mask, nn, std, N, n_live=None, slot=False, near2=0.1):
    L = _lib()
    p = L.ptr
    sec = torch.full((max(N, 1), 8), SENT, device=DEV)
    index = torch.full((max(N, 1),), -7, dtype=torch.int32, device=DEV)
    sl = torch.full((max(N, 1),), -7, dtype=torch.int32, device=DEV) if slot else None
    count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    rdir = torch.full((max(N, 1), 3), SENT, device=DEV)
    args = [p(rays), p(xs), p(normal), p(nn), std, p(mask), N, 1, near2, p(sec), p(index), p(count), p(rdir)]
    if n_live is None and not slot:
        code = L.lib().mnrf_reflect_compact(*args, L.stream())
    else:
        code = L.lib().mnrf_reflect_compact_n(*args, p(n_live), p(sl), L.stream())
    torch.cuda.synchronize()
    assert code == 0
    return sec, index, sl, int(count.item()), rdir


@pytest.mark.parametrize("noise", [False, True])
@pytest.mark.parametrize("frac", [0.0, 1.0, 0.3])
@pytest.mark.parametrize("N", GLUE_N)
def test_reflect_compact_and_backward_against_float64(N, frac, noise):
    """mnrf_reflect_compact(_n with slot), mnrf_reflect_backward and mnrf_reflect_backward_gather_n: index is nonzero(mask),
    slot its inverse (-1 elsewhere), *count their number; secondary rays and gradients against TR.reflect in float64."""
    L = _lib()
    p = L.ptr
    rays, xs, normal, mask, nn = _glue_inputs(N, frac, True, noise)
    std = 0.25
    sec, index, slot, count, rdir = hip_reflect_compact(rays, xs, normal, mask, nn, std, N, slot=True)
    sel = mask.nonzero().flatten()
    assert count == sel.numel()
    assert torch.equal(index[:count].long(), sel) and bool((index[count:] == -7).all())
    want_slot = torch.full((N,), -1, dtype=torch.int32, device=DEV)
    want_slot[sel] = torch.arange(count, dtype=torch.int32, device=DEV)
    assert torch.equal(slot[:N], want_slot)
    assert bool((sec[count:] == SENT).all())
    sec2, index2, _, count2, rdir2 = hip_reflect_compact(rays, xs, normal, mask, nn, std, N)          # the namesake: same bits
    assert count2 == count and torch.equal(sec2, sec) and torch.equal(index2, index) and torch.equal(rdir2, rdir)
    if N == 0:
        return
    bad, figs = [], []
    res = {}
    g_sec = torch.randn(count, 8, generator=RC.gen("g_sec", N, frac)).to(DEV)
    for dtype in (torch.float64, torch.float32):
        leaf = [t.to(dtype).clone().requires_grad_(True) for t in (rays, xs, normal)]
        nrm = leaf[2] if nn is None else leaf[2] + nn.to(dtype) * std
        out = TR.reflect(leaf[0], leaf[1], nrm, mask, compact=False)
        g = torch.autograd.grad((out[sel] * g_sec.to(dtype)).sum(), leaf, allow_unused=True) if count else [torch.zeros_like(t) for t in leaf]
        res[dtype] = (out.detach(), [torch.zeros_like(t) if x is None else x for x, t in zip(g, leaf)])
    o64, g64 = res[torch.float64]
    o32, g32 = res[torch.float32]
    want = o64.clone()
    want[:, 6] = 0.1
    if count:
        bad += _judge(figs, "reflect", "fwd", "sec", sec[:count], want[sel], torch.cat([o32[sel][:, :6], sec[:count, 6:7], o32[sel][:, 7:]], 1))
        assert torch.equal(sec[:count, :3], xs[sel]) and torch.equal(sec[:count, 7], rays[sel, 7]) and bool((sec[:count, 6] == 0.1).all())
    bad += _judge(figs, "reflect", "fwd", "reflect_dir", rdir[:N], o64[:, 3:6], o32[:, 3:6])
    outs = []
    for gather in (False, True):
        gx, gn, gr = (torch.full(s, SENT, device=DEV) for s in ((N, 3), (N, 3), (N, 8)))
        if gather:
            gs = g_sec if count else torch.zeros(1, 8, device=DEV)
            code = L.lib().mnrf_reflect_backward_gather_n(p(rays), p(normal if nn is None else normal + nn * std), p(slot), p(gs), N,
                                                          p(gx), p(gn), p(gr), None, L.stream())
        else:
            code = L.lib().mnrf_reflect_backward(p(rays), p(normal if nn is None else normal + nn * std), p(index), count, p(g_sec if count else None),
                                                 N, p(gx), p(gn), p(gr), L.stream())
        torch.cuda.synchronize()
        assert code == 0
        outs.append((gx, gn, gr))
        tag = "gather" if gather else "scatter"
        bad += _judge(figs, "reflect", "bwd", f"g_xs_{tag}", gx, g64[1], g32[1])
        bad += _judge(figs, "reflect", "bwd", f"g_normal_{tag}", gn, g64[2], g32[2])
        bad += _judge(figs, "reflect", "bwd", f"g_rays_{tag}", gr, g64[0], g32[0])
    for a, b in zip(*outs):
        assert torch.equal(a, b)                  # the gather form: the same values
    _report("reflect", "all", f"N={N},frac={frac},noise={noise}", figs)
    assert not bad, bad[:20]


@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("frac", [0.0, 1.0, 0.3])
@pytest.mark.parametrize("N", GLUE_N)
def test_blend_forward_and_backward(N, frac, c):
    """mnrf_blend_scatter, mnrf_blend_backward, mnrf_blend2_n, mnrf_blend2_backward_n: forward values are TR.blend in float32
    bit for bit (and so meet float64 to one rounding of each of the three operations: 3 * 2^-24 of the row's largest entry
    times the 2 terms); tensor a or b may be null; g_sec rows past the count keep their sentinel."""
    L = _lib()
    p = L.ptr
    rays, xs, normal, mask, _ = _glue_inputs(N, frac, True, False)
    _, index, slot, count, _ = hip_reflect_compact(rays, xs, normal, mask, None, 0.0, N, slot=True)
    g = RC.gen("blend", N, frac, c)
    base_a, base_b = torch.rand(N, c, generator=g).to(DEV), torch.rand(N, c, generator=g).to(DEV)
    sec_a, sec_b = torch.rand(max(count, 1), c, generator=g).to(DEV), torch.rand(max(count, 1), c, generator=g).to(DEV)
    g_a, g_b = torch.randn(N, c, generator=g).to(DEV), torch.randn(N, c, generator=g).to(DEV)
    if N == 0:
        out = torch.full((1, c), SENT, device=DEV)
        assert L.lib().mnrf_blend_scatter(p(out), p(out), p(index), 0, p(out), 0, c, p(out), None, L.stream()) == 0
        assert L.lib().mnrf_blend2_n(p(out), p(out), None, None, p(slot), p(out), 0, c, p(out), None, None, L.stream()) == 0
        torch.cuda.synchronize()
        assert bool((out == SENT).all())
        return
    want_a, want_b = TR.blend(base_a, sec_a[:count], mask, True), TR.blend(base_b, sec_b[:count], mask, True)
    w64 = TR.blend(base_a.double(), sec_a[:count].double(), mask.double(), True)
    assert float(_row_rel(want_a, w64).max()) <= 6 * 2.0 ** -24
    assert float(_row_rel(want_b, TR.blend(base_b.double(), sec_b[:count].double(), mask.double(), True)).max()) <= 6 * 2.0 ** -24
    out, refl = torch.full((N, c), SENT, device=DEV), torch.full((N, c), SENT, device=DEV)
    assert L.lib().mnrf_blend_scatter(p(base_a), p(sec_a), p(index), count, p(mask), N, c, p(out), p(refl), L.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, want_a)
    want_refl = torch.zeros(N, c, device=DEV)
    want_refl[mask != 0] = sec_a[:count]
    assert torch.equal(refl, want_refl)
    for use_a, use_b in ((True, True), (True, False), (False, True)):
        oa, ob = torch.full((N, c), SENT, device=DEV), torch.full((N, c), SENT, device=DEV)
        assert L.lib().mnrf_blend2_n(p(base_a if use_a else None), p(sec_a if use_a else None), p(base_b if use_b else None),
                                     p(sec_b if use_b else None), p(slot), p(mask), N, c, p(oa if use_a else None), p(ob if use_b else None),
                                     None, L.stream()) == 0
        torch.cuda.synchronize()
        assert torch.equal(oa, want_a if use_a else torch.full_like(oa, SENT))
        assert torch.equal(ob, want_b if use_b else torch.full_like(ob, SENT))
    # backward: g_base = (1 - m) g_out, g_sec = m g_out gathered; exact products, so float32 torch is the bit-exact yardstick
    m = mask[:, None]
    sel = mask.nonzero().flatten()
    cap = count + 3
    gb, gs = torch.full((N, c), SENT, device=DEV), torch.full((cap, c), SENT, device=DEV)
    assert L.lib().mnrf_blend_backward(p(g_a), p(mask), p(index), count, N, c, p(gb), p(gs), L.stream()) == 0
    torch.cuda.synchronize()
    assert torch.equal(gb, (1 - m) * g_a) and torch.equal(gs[:count], (m * g_a)[sel]) and bool((gs[count:] == SENT).all())
    for use_a, use_b in ((True, True), (True, False), (False, True)):
        t = [torch.full(s, SENT, device=DEV) for s in ((N, c), (cap, c), (N, c), (cap, c))]
        assert L.lib().mnrf_blend2_backward_n(p(g_a if use_a else None), p(g_b if use_b else None), p(slot), p(mask), N, c,
                                              p(t[0]), p(t[1]), p(t[2]), p(t[3]), None, L.stream()) == 0
        torch.cuda.synchronize()
        for gg, used, tb, ts in ((g_a, use_a, t[0], t[1]), (g_b, use_b, t[2], t[3])):
            if used:
                assert torch.equal(tb, (1 - m) * gg) and torch.equal(ts[:count], (m * gg)[sel]) and bool((ts[count:] == SENT).all())
            else:
                assert bool((tb == SENT).all()) and bool((ts == SENT).all())


@pytest.mark.parametrize("n_freqs", [0, 1, 4, 10])
@pytest.mark.parametrize("c", [1, 3])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_embed_backward_against_float64(n, c, n_freqs):
    """mnrf_embed_backward against float64 autograd of TR.embed, |x| up to 8 (2^9 * 8 radians at n_freqs = 10)."""
    L = _lib()
    p = L.ptr
    g = RC.gen("embed", n, c, n_freqs)
    x = (torch.rand(n, c, generator=g) * 16 - 8).to(DEV)
    go = torch.randn(n, c * (2 * n_freqs + 1), generator=g).to(DEV)
    gx = torch.full((n, c), NAN, device=DEV)
    assert L.lib().mnrf_embed_backward(p(x), p(go), n, c, n_freqs, p(gx), L.stream()) == 0
    torch.cuda.synchronize()
    res = {}
    for dtype in (torch.float64, torch.float32):
        xl = x.to(dtype).requires_grad_(True)
        (res[dtype],) = torch.autograd.grad((TR.embed(xl, n_freqs) * go.to(dtype)).sum(), xl)
    figs = []
    bad = _judge(figs, "embed_bwd", f"F{n_freqs}", "g_x", gx, res[torch.float64], res[torch.float32])
    _report("embed_bwd", f"F{n_freqs}", f"n={n},c={c}", figs)
    assert not bad, bad[:20]


@pytest.mark.parametrize("n_rays", [1, 5])
@pytest.mark.parametrize("spr", [1, 63, 64, 65, 192, 256])
def test_ray_grads_against_float64(spr, n_rays):
    """mnrf_ray_grads against the sums of the header in float64 (TR.ray_grads); each output null in turn."""
    L = _lib()
    p = L.ptr
    g = RC.gen("ray_grads", spr, n_rays)
    d_xyz, z = torch.randn(n_rays * spr, 3, generator=g).to(DEV), (torch.rand(n_rays, spr, generator=g) * 6).to(DEV)
    d_dir = torch.randn(n_rays * spr, 32, generator=g).to(DEV)
    r64 = TR.ray_grads(d_xyz.double(), z.double(), d_dir.double(), spr)
    r32 = TR.ray_grads(d_xyz, z, d_dir, spr)
    bad, figs = [], []
    for want_r, want_e in ((True, True), (True, False), (False, True)):
        gr, ge = torch.full((n_rays, 8), SENT, device=DEV), torch.full((n_rays, 27), SENT, device=DEV)
        assert L.lib().mnrf_ray_grads(p(d_xyz if want_r else None), p(z if want_r else None), p(d_dir if want_e else None), n_rays, spr,
                                      p(gr if want_r else None), p(ge if want_e else None), L.stream()) == 0
        torch.cuda.synchronize()
        if want_r:
            bad += _judge(figs, "ray_grads", "all", "g_rays", gr, r64[0], r32[0])
            assert bool((gr[:, 6:] == 0).all())
        else:
            assert bool((gr == SENT).all())
        if want_e:
            bad += _judge(figs, "ray_grads", "all", "g_de", ge, r64[1], r32[1])
        else:
            assert bool((ge == SENT).all())
    _report("ray_grads", "all", f"spr={spr},n={n_rays}", figs)
    assert not bad, bad[:20]


# ------------------------------------------------------------------------------------------------ live row counts
CAP = 70
LIVE = (0, 1, 3, 4, 5, 69, 70)


def _cnt(k):
    return torch.tensor([k], dtype=torch.int32, device=DEV)


def _dead(t, k):
    """A copy of an input whose rows past the live count are NaN: a read of a dead row that reaches a live output shows."""
    t = t.clone()
    t[k:] = NAN
    return t


def _sent(*shape, dtype=torch.float32):
    return torch.full(shape, SENT if dtype == torch.float32 else -7, dtype=dtype, device=DEV)


def _rand(g, *shape):
    return torch.rand(*shape, generator=g).to(DEV)


def _live_inputs():
    g = RC.gen("live")
    S, n_imp, spr = 65, 33, 65
    c = _to(RC.composite_inputs(S, CAP, "thin"))
    d = dict(c=c, S=S, n_imp=n_imp, spr=spr, x=_rand(g, CAP, 3) * 16 - 8, g27=_rand(g, CAP, 27) - 0.5,
             rays=torch.cat([_rand(g, CAP, 6) - 0.5, _rand(g, CAP, 1) + 0.1, _rand(g, CAP, 1) + 4], 1),
             steps=torch.linspace(0, 1, 7).to(DEV), prand=_rand(g, CAP, 7), g8=[_rand(g, CAP, 8) - 0.5 for _ in range(4)],
             u=_rand(g, CAP, n_imp), w=_rand(g, CAP, S), mask=(_rand(g, CAP) < 0.4).float(), xs=_rand(g, CAP, 3), normal=_rand(g, CAP, 3) - 0.5,
             nn=_rand(g, CAP, 3) - 0.5, base=_rand(g, CAP, 3), base_b=_rand(g, CAP, 3), sec=_rand(g, CAP, 3), sec_b=_rand(g, CAP, 3),
             g_out=_rand(g, CAP, 3) - 0.5, g_out_b=_rand(g, CAP, 3) - 0.5, g_sec8=_rand(g, CAP, 8) - 0.5,
             d_xyz=_rand(g, CAP, spr, 3) - 0.5, zz=_rand(g, CAP, spr) * 6, d_dir=_rand(g, CAP, spr, 32) - 0.5,
             cot={k: _rand(g, *_out_shape(k, CAP, S)) - 0.5 for k in OUT_NAMES})
    d["mask"][CAP - 1] = 0.5
    return d


def _sel(d, k):
    """index / slot / count of the compaction of the first k rays (computed with torch: the compaction itself is an entry below)."""
    sel = d["mask"][:k].nonzero().flatten().int()
    slot = torch.full((CAP,), -1, dtype=torch.int32, device=DEV)
    slot[sel.long()] = torch.arange(sel.numel(), dtype=torch.int32, device=DEV)
    index = torch.zeros(CAP, dtype=torch.int32, device=DEV)       # dead entries name a valid row: a leak shows as a wrong value there
    index[:sel.numel()] = sel
    return index, slot, int(sel.numel())


def _entry(name, d, k, k2, live):
    """Runs entry point `name` once: live = True on the capacity-sized buffers with dead input rows and the device counts (k rays,
    k2 secondary rows), live = False the namesake on the inputs truncated to the live rows.  Returns [(output, live rows)]."""
    L = _lib()
    F, p, st = L.lib(), L.ptr, L.stream()
    n = CAP if live else k
    n2 = CAP if live else k2
    cnt, cnt2 = (_cnt(k), _cnt(k2)) if live else (None, None)
    I = (lambda t, kk=k: _dead(t, kk)) if live else (lambda t, kk=k: t[:kk].contiguous())       # noqa: E731,E741
    O = lambda *s, dtype=torch.float32: _sent(n, *s, dtype=dtype)                                # noqa: E731,E741
    O2 = lambda *s: _sent(n2, *s)                                                               # noqa: E731
    S, n_imp, spr, c = d["S"], d["n_imp"], d["spr"], d["c"]
    index, slot, _ = _sel(d, k)
    if not live:
        index, slot = index[:max(k2, 1)].contiguous(), slot[:max(k, 1)].contiguous()
    ci = {kk: (None if v is None else I(v)) for kk, v in c.items()}
    cargs = [p(ci["rays"]), n, S, p(ci["sigma"]), p(ci["z"]), p(ci["noise"]), p(ci["rgb"]), p(ci["m"]), p(ci["pn"]), p(ci["nrm"]), 1]
    tail = (p(cnt), st) if live else (st,)
    sfx = "_n" if live else ""
    if name == "embed":
        x, o = I(d["x"]), O(27)
        code = getattr(F, "mnrf_embed" + sfx)(p(x), n, 3, 4, p(o), *tail)
        outs = [(o, k)]
    elif name == "embed_backward":
        x, g, o = I(d["x"]), I(d["g27"]), O(3)
        code = getattr(F, "mnrf_embed_backward" + sfx)(p(x), p(g), n, 3, 4, p(o), *tail)
        outs = [(o, k)]
    elif name == "sample_coarse":
        r, pr, o = I(d["rays"]), I(d["prand"]), O(7)
        code = getattr(F, "mnrf_sample_coarse" + sfx)(p(r), n, p(d["steps"]), 7, 1, 1.0, p(pr), p(o), *tail)
        outs = [(o, k)]
    elif name == "ray_prologue":        # no namesake: n_live = null is the plain form
        r, pr, o, e = I(d["rays"]), I(d["prand"]), O(7), O(27)
        code = F.mnrf_ray_prologue_n(p(r), n, 4, p(d["steps"]), 7, 0, 1.0, p(pr), p(e), p(o), p(cnt), st)
        outs = [(o, k), (e, k)]
    elif name == "ray_fan_backward":
        gs, r, ga, gb, o = [I(t) for t in d["g8"]], I(d["rays"]), I(d["g27"]), I(d["g27"] * 0.5), O(8)
        code = F.mnrf_ray_fan_backward_n(p(gs[0]), p(gs[1]), None, p(gs[3]), p(r), p(ga), p(gb), n, 4, p(o), p(cnt), st)
        outs = [(o, k)]
    elif name in ("composite", "composite_sample"):
        o = {kk: _sent(*_out_shape(kk, n, S)) for kk in OUT_NAMES}
        if name == "composite":
            code = getattr(F, "mnrf_composite" + sfx)(*cargs, *[p(o[kk]) for kk in OUT_NAMES], *tail)
            outs = [(o[kk], k) for kk in OUT_NAMES]
        else:
            u, zf = I(d["u"]), O(S + n_imp)
            code = F.mnrf_composite_sample_n(*cargs, *[p(o[kk]) for kk in OUT_NAMES], p(u), 1, n_imp, p(zf), p(cnt), st)
            outs = [(o[kk], k) for kk in OUT_NAMES] + [(zf, k)]
    elif name == "composite_backward":
        w, dep = I(d["w"]), I(d["w"][:, 0].contiguous())
        cot = [I(d["cot"][kk]) for kk in OUT_NAMES]
        o = [_sent(*_grad_shape(kk, n, S)) for kk in GRAD_NAMES]
        code = getattr(F, "mnrf_composite_backward" + sfx)(*cargs, p(w), p(dep), *[p(t) for t in cot], *[p(t) for t in o], 0, None, *tail)
        outs = [(t, k) for t in o]
    elif name == "sample_fine":
        z, w, u, zf = I(c["z"]), I(d["w"]), I(d["u"]), O(S + n_imp)
        code = getattr(F, "mnrf_sample_fine" + sfx)(p(z), p(w), n, S, p(u), 1, n_imp, p(zf), *tail)
        outs = [(zf, k)]
    elif name == "threshold_mask":      # in place: the dead rows hold NaN and must still hold it
        m = I(d["w"][:, 0].contiguous() * (0.45 if k % 2 else 1.0))
        any_ = torch.zeros(1, dtype=torch.int32, device=DEV)
        code = getattr(F, "mnrf_threshold_mask" + sfx)(p(m), n, p(any_), *tail)
        torch.cuda.synchronize()
        assert code == 0
        if live:
            assert bool(torch.isnan(m[k:]).all())
            m = torch.cat([m[:k], _sent(CAP - k)])
        return [(m, k), (any_.float(), 1)]
    elif name == "reflect_compact":
        a = [I(d[t]) for t in ("rays", "xs", "normal", "nn")]
        m = I(d["mask"])
        sec, idx, cn, rd = O(8), O(dtype=torch.int32), _sent(1, dtype=torch.int32), O(3)
        args = [p(a[0]), p(a[1]), p(a[2]), p(a[3]), 0.25, p(m), n, 1, 0.1, p(sec), p(idx), p(cn), p(rd)]
        if live:
            sl = O(dtype=torch.int32)
            code = F.mnrf_reflect_compact_n(*args, p(cnt), p(sl), st)
            torch.cuda.synchronize()
            assert torch.equal(sl[:k], _sel(d, k)[1][:k]) and bool((sl[k:] == -7).all())
        else:
            code = F.mnrf_reflect_compact(*args, st)
        outs = [(sec, k2), (idx, k2), (cn, 1), (rd, k)]
    elif name in ("reflect_backward", "reflect_backward_gather"):
        r, nv, gs = I(d["rays"]), I(d["normal"]), I(d["g_sec8"], k2)
        if name == "reflect_backward":      # one count: the secondary rows; all n_rays rows of the outputs are written
            r, nv = d["rays"], d["normal"]
            full_index = _sel(d, k)[0]
            o = [_sent(CAP, 3), _sent(CAP, 3), _sent(CAP, 8)]
            code = getattr(F, "mnrf_reflect_backward" + sfx)(p(r), p(nv), p(full_index), n2, p(gs), CAP, *[p(t) for t in o], *((p(cnt2), st) if live else (st,)))
            outs = [(t, CAP) for t in o]
        else:
            gs = gs if gs.shape[0] else torch.zeros(1, 8, device=DEV)
            o = [O(3), O(3), O(8)]
            code = F.mnrf_reflect_backward_gather_n(p(r), p(nv), p(slot), p(gs), n, *[p(t) for t in o], p(cnt), st)
            outs = [(t, k) for t in o]
    elif name == "blend_scatter":
        b, s, m, o, ro = I(d["base"]), I(d["sec"], k2), I(d["mask"]), O(3), O(3)
        s = s if s.shape[0] else torch.zeros(1, 3, device=DEV)
        code = getattr(F, "mnrf_blend_scatter" + sfx)(p(b), p(s), p(index), n2, p(m), n, 3, p(o), p(ro), *((p(cnt2), p(cnt), st) if live else (st,)))
        outs = [(o, k), (ro, k)]
    elif name == "blend_backward":
        g, m, gb, gs = I(d["g_out"]), I(d["mask"]), O(3), O2(3)
        code = getattr(F, "mnrf_blend_backward" + sfx)(p(g), p(m), p(index), n2, n, 3, p(gb), p(gs), *((p(cnt2), p(cnt), st) if live else (st,)))
        outs = [(gb, k), (gs, k2)]
    elif name == "blend2":
        ba, sa, bb, sb, m, oa, ob = I(d["base"]), I(d["sec"], k2), I(d["base_b"]), I(d["sec_b"], k2), I(d["mask"]), O(3), O(3)
        sa, sb = (t if t.shape[0] else torch.zeros(1, 3, device=DEV) for t in (sa, sb))
        code = F.mnrf_blend2_n(p(ba), p(sa), p(bb), p(sb), p(slot), p(m), n, 3, p(oa), p(ob), p(cnt), st)
        outs = [(oa, k), (ob, k)]
    elif name == "blend2_backward":
        ga, gb, m = I(d["g_out"]), I(d["g_out_b"]), I(d["mask"])
        o = [O(3), _sent(max(n2, 1), 3), O(3), _sent(max(n2, 1), 3)]
        code = F.mnrf_blend2_backward_n(p(ga), p(gb), p(slot), p(m), n, 3, *[p(t) for t in o], p(cnt), st)
        outs = [(o[0], k), (o[1], k2), (o[2], k), (o[3], k2)]
    elif name == "ray_grads":
        dx, z, dd, gr, ge = I(d["d_xyz"]), I(d["zz"]), I(d["d_dir"]), O(8), O(27)
        code = getattr(F, "mnrf_ray_grads" + sfx)(p(dx), p(z), p(dd), n, spr, p(gr), p(ge), *tail)
        outs = [(gr, k), (ge, k)]
    else:
        raise KeyError(name)
    torch.cuda.synchronize()
    assert code == 0, (name, k, k2, live)
    return outs


LIVE_ENTRIES = ("embed", "embed_backward", "sample_coarse", "ray_prologue", "ray_fan_backward", "composite", "composite_sample",
                "composite_backward", "sample_fine", "threshold_mask", "reflect_compact", "reflect_backward", "reflect_backward_gather",
                "blend_scatter", "blend_backward", "blend2", "blend2_backward", "ray_grads")
TWO_COUNTS = ("blend_scatter", "blend_backward", "reflect_backward")


@pytest.fixture(scope="module")
def live_inputs():
    return _live_inputs()


@pytest.mark.parametrize("name", LIVE_ENTRIES)
def test_live_row_counts(name, live_inputs):
    """Every `_n` entry point of mnrf_render.hip at capacity 70 with 0, 1, 3, 4, 5, 69 and 70 live rows: the INPUT rows past the
    count are NaN, the output rows past it a sentinel.  The live output rows equal, bit for bit, the namesake run on the inputs
    truncated to the live rows (NaN included: a dead row that leaks into a live output differs); every other output element
    keeps its sentinel.  The entry points with a second count (the secondary rows) vary it the same way below the first."""
    d = live_inputs
    for k in LIVE:
        n_sel = _sel(d, k)[2]
        seconds = sorted({k2 for k2 in LIVE if k2 <= n_sel} | {n_sel}) if name in TWO_COUNTS else [n_sel]
        for k2 in seconds:
            full = _entry(name, d, k, k2, True)
            if k == 0 and name not in ("reflect_compact", "reflect_backward"):      # nothing to truncate to: nothing may be written
                for t, rows in full:
                    assert bool((t[rows:] == (SENT if t.dtype == torch.float32 else -7)).all()), (name, k)
                    assert rows == 0 or not bool(t.any()), (name, k)                # (`any` of the threshold: still 0)
                continue
            part = _entry(name, d, k, k2, False)
            for (t, rows), (s, _) in zip(full, part):
                i32 = lambda x: x.contiguous().view(torch.int32) if x.dtype == torch.float32 else x       # noqa: E731
                assert torch.equal(i32(t[:rows]), i32(s[:rows])), (name, k, k2)
                assert bool((t[rows:] == (SENT if t.dtype == torch.float32 else -7)).all()), (name, k, k2)
