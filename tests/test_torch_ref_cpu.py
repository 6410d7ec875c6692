"""CPU tests of the float64 reference the field-backward tests differentiate (tests/torch_ref.py `field(..., masks=)`)."""
import numpy as np
import pytest
import torch

from oracle import mirror_nerf_oracle as O
from tests import rays_cases as RC
from tests import torch_ref as TR


def _weights(seed):
    from tests.golden import weights as GW
    sd = GW.apply_tweaks(GW.make_state_dict(seed, 1)[0], GW.OPAQUE)
    return {k: torch.from_numpy(v).double() for k, v in sd.items()}


def _inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(B, 3, generator=g, dtype=torch.float64) * 4 - 2
    de = TR.embed(TR.l2n(torch.randn(B, 3, generator=g, dtype=torch.float64)), 4)
    return xyz, de


def test_masked_field_equals_the_relu_field_bit_for_bit():
    """With the masks of its own forward, y * mask is relu(y) / leaky_relu(y) exactly: outputs (the density-gradient normal
    included) and first-order gradients are the same bits as the plain version."""
    w = _weights(5)
    xyz, de = _inputs(64, 0)
    acts = {}
    with torch.no_grad():
        TR.field(w, xyz, de, acts=acts)
    masks = TR.masks_of({n: acts[n] for n in TR.MASK_NAMES})
    assert all(int((m != 1).sum()) > 0 for m in masks.values())          # every activation has inactive units here
    res = []
    for mk in (None, masks):
        wl = {k: v.clone().requires_grad_(True) for k, v in w.items()}
        x = xyz.clone().requires_grad_(True)
        d = de.clone().requires_grad_(True)
        outs = TR.field(wl, x, d, with_normal=True, masks=mk)
        sum((o * (i + 1)).sum() for i, o in enumerate(outs[:4])).backward()
        res.append([o.detach() for o in outs] + [x.grad, d.grad] + [wl[k].grad for k in sorted(wl)])
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_masked_field_double_backward_matches_gradcheck():
    """The second-order path (the density-gradient normal, differentiated again) of the masked reference against finite
    differences: with the masks held constant the function is smooth, so gradcheck holds at every point."""
    w = _weights(11)
    xyz, de = _inputs(3, 1)
    acts = {}
    with torch.no_grad():
        TR.field(w, xyz, de, acts=acts)
    masks = TR.masks_of({n: acts[n] for n in TR.MASK_NAMES})
    small = ("sigma.bias", "xyz_encoding_8.0.bias", "xyz_encoding_1.0.bias")

    def fn(x, d, *vals):
        wl = dict(w)
        for k, v in zip(small, vals):
            wl[k] = v
        sigma, rgb, pn, m, nrm = TR.field(wl, x, d, with_normal=True, masks=masks)
        return sigma, rgb, pn, m, nrm

    args = [xyz.clone().requires_grad_(True), de.clone().requires_grad_(True)] + \
           [w[k].clone().requires_grad_(True) for k in small]
    assert torch.autograd.gradcheck(fn, args, eps=1e-6, atol=1e-7, rtol=1e-5)


# ---- the per-ray references of tests/test_hip_rays_fp64.py: each restatement, run in float32, against the numpy oracle on the very
# inputs the GPU tests use (tests/rays_cases.py), so that the float64 runs of the same code are a proven yardstick
def _resample_cases():
    return [(S, n, N, regime, per_ray) for S, n in RC.RESAMPLE_SHAPES for N in (1, 5) for regime in RC.RESAMPLE_REGIMES
            for per_ray in (False, True)]


def test_sample_pdf_restatement_matches_the_oracle_and_the_skip_cap_holds():
    """TR.sample_pdf / TR.merge_sorted in float32 against O.sample_pdf and numpy's sort, at every shape, weight regime and kind
    of u of the GPU test.  Samples the float64 run cannot decide (RC.resample_undecided) are left out of the comparison of
    values: at most 2 % of a case, never a whole ray.  Elsewhere float32 torch and the float32 oracle differ by the rounding of
    the row sum (torch's and numpy's orders of summation), which moves every cdf entry by a few ulp of 1: the bound per sample
    is 1e-6 (16 ulp of 1: c0, c1 and u - c0, each a few roundings of numbers below 1) times 1 + (b1 - b0) / (c1 - c0), the
    slope of the inverse cdf in the selected bin, plus the rounding of the sample itself."""
    worst = 0.0
    for S, n_imp, N, regime, per_ray in _resample_cases():
        z, w, u = RC.resample_inputs(S, n_imp, N, regime, per_ray)
        got = TR.sample_pdf(TR.mids(z), w[:, 1:-1], n_imp, u)
        ref = O.sample_pdf(0.5 * (z.numpy()[:, :-1] + z.numpy()[:, 1:]), w.numpy()[:, 1:-1], n_imp, det=not per_ray, u=u.numpy())
        _, cdf, u64, raw, span = TR.sample_pdf_info(TR.mids(z.double()), w.double()[:, 1:-1], n_imp, u.double())
        skip = RC.resample_undecided(cdf, u64, raw, per_ray)
        case = (S, n_imp, N, regime, per_ray)
        assert float(skip.float().mean()) <= 0.02, (case, int(skip.sum()))
        assert not bool(skip.all(1).any()), case
        bound = 1e-6 * (1 + RC.resample_slope(raw, span)) + 1e-6
        err = ((got - torch.from_numpy(ref)).abs() / bound)[~skip]
        if err.numel():
            worst = max(worst, float(err.max()))
            assert float(err.max()) <= 1, (case, float(err.max()))
        merged = TR.merge_sorted(z, got)
        assert np.array_equal(merged.numpy(), np.sort(np.concatenate([z.numpy(), got.numpy()], -1), -1))
    print("sample_pdf float32 restatement vs oracle, worst decidable sample / its bound:", worst)


@pytest.mark.parametrize("regime", RC.COMPOSITE_REGIMES)
def test_composite_restatement_matches_the_oracle(regime, monkeypatch):
    """TR.composite in float32 against the compositing of O.render_rays (O._inference with the field's outputs injected), per
    ray: 1e-5 of the row's largest entry (float32 cumprod / sums in two orders), exact zeros where the oracle has a zero row.

    The oracle offers compositing only inside render_rays, behind the evaluation of a model, so this test reaches into two of
    its private functions: `_inference` (oracle/mirror_nerf_oracle.py, the deltas / alphas / weights / maps that follow its call
    of `_eval_field`, i.e. models/rendering.py:182-264) is called directly, and `_eval_field`, the only place where it touches
    the model, is replaced by the case's own sigma, rgb, is_mirror, normal and pred_normal.  If either is renamed or its
    keywords change, this test is what to adapt; nothing else in tests/ depends on them."""
    for S in RC.COMPOSITE_S:
        if (regime == "opaque_straddle" and S <= 64) or S == 1:     # (the oracle, like the reference, has no delta at S = 1)
            continue
        for N, white in ((3, False), (5, True)):
            c = RC.composite_inputs(S, N, regime)
            # the field's outputs injected where render_rays evaluates the model (O._eval_field), then its compositing (O._inference)
            field = dict(sigma=c["sigma"].numpy().reshape(-1), rgb=c["rgb"].numpy().reshape(-1, 3), is_mirror=c["m"].numpy().reshape(-1),
                         normal=c["nrm"].numpy().reshape(-1, 3), pred_normal=c["pn"].numpy().reshape(-1, 3))
            monkeypatch.setattr(O, "_eval_field", lambda *a, **k: field)
            res = {}
            O._inference(res, w=None, typ="fine", xyz=None, z_vals=c["z"].numpy(), dir_emb=None, test_time=False, has_fine=True,
                         noise=None if c["noise"] is None else c["noise"].numpy(), noise_std=1.0, white_back=white,
                         compute_normal=True, n_freqs_xyz=10, chunk=1 << 20)
            got = TR.composite(c["rays"], c["sigma"], c["z"], c["noise"], c["rgb"], c["m"], c["pn"], c["nrm"], white)
            names = dict(weights="weights_fine", opacity="opacity_fine", rgb="rgb_fine", depth="depth_fine", mask="mirror_mask_fine",
                         sn="surface_normal_fine", sng="surface_normal_grad_fine", nd="normal_dif_fine")
            for k, name in names.items():
                a, b = got[k].reshape(N, -1).double(), torch.from_numpy(res[name]).reshape(N, -1).double()
                scale = b.abs().amax(1)
                err = (a - b).abs().amax(1)
                assert bool((err[scale == 0] == 0).all()), (S, N, k)
                assert bool((err[scale > 0] <= 1e-5 * scale[scale > 0]).all()), (S, N, k, float((err / scale).max()))
            if regime in ("empty", "empty_zero"):
                assert not bool(got["weights"].any())


def test_composite_float64_is_float64_throughout():
    """No float32 constant sneaks into the float64 run: every output is float64, and with alpha exactly 1 in both formats the
    opaque sample leaves exactly 1e-10 of the light (the reference's `+ 1e-10`)."""
    c = {k: (v.double() if v is not None else None) for k, v in RC.composite_inputs(65, 4, "opaque_inside").items()}
    out = TR.composite(c["rays"], c["sigma"], c["z"], c["noise"], c["rgb"], c["m"], c["pn"], c["nrm"], True)
    assert all(v.dtype == torch.float64 for v in out.values())
    a, n = RC.opaque_runs(65, "opaque_inside", 0)[0]
    w = out["weights"][0]
    T_before = 1 - w[:a].sum()          # sum of weights = 1 - T up to the 1e-10 terms
    assert abs(float(w[a] / T_before) - 1) < 1e-6 and float(w[a + n:].abs().max()) <= 1.01e-10 ** n * 1.0


def test_reflect_blend_embed_restatements_match_the_oracle():
    g = RC.gen("glue")
    N = 257
    rays = torch.randn(N, 8, generator=g)
    normal = torch.randn(N, 3, generator=g)
    normal[3] = 0.0
    normal[5] = 1e-20
    xs = torch.randn(N, 3, generator=g)
    mask = (torch.rand(N, generator=g) < 0.3).float()
    sec = TR.reflect(rays, xs, normal, mask, compact=False)
    r, _, _ = O.reflect(rays[:, 3:6].numpy(), normal.numpy())
    assert np.allclose(sec[:, 3:6].numpy(), r, rtol=0, atol=1e-6)
    assert torch.equal(sec[:, :3], xs) and torch.equal(sec[:, 7], rays[:, 7])
    assert torch.equal(TR.reflect(rays, xs, normal, mask, compact=True), sec[mask != 0])
    assert TR.reflect(rays.double(), xs.double(), normal.double(), mask.double(), False).dtype == torch.float64
    x = torch.rand(N, 3, generator=g) * 16 - 8
    for n_freqs in (0, 1, 4, 10):
        assert np.allclose(TR.embed(x, n_freqs).numpy(), O.embedding(x.numpy(), n_freqs), rtol=0, atol=2e-6)
    assert TR.embed(x.double(), 4).dtype == torch.float64
    base, part = torch.rand(N, 3, generator=g), torch.rand(int(mask.sum()), 3, generator=g)
    out = TR.blend(base, part, mask, compact=True)
    full = base.clone()
    full[mask != 0] = part
    assert torch.equal(out, mask[:, None] * full + (1 - mask[:, None]) * base)
    assert TR.blend(base.double(), part.double(), mask.double(), True).dtype == torch.float64


def test_ray_grads_restatement_is_the_stated_sums():
    g = RC.gen("ray_grads")
    for spr in (1, 63, 65):
        n = 5
        d_xyz, z, d_dir = torch.randn(n * spr, 3, generator=g), torch.rand(n, spr, generator=g), torch.randn(n * spr, 32, generator=g)
        g_rays, g_de = TR.ray_grads(d_xyz.double(), z.double(), d_dir.double(), spr)
        assert g_rays.shape == (n, 8) and g_de.shape == (n, 27) and g_rays.dtype == torch.float64
        for i in range(n):
            rows = slice(i * spr, (i + 1) * spr)
            want = np.concatenate([d_xyz[rows].double().numpy().sum(0), (z[i].double().numpy()[:, None] * d_xyz[rows].double().numpy()).sum(0),
                                   [0, 0]])
            assert np.allclose(g_rays[i].numpy(), want, rtol=1e-13, atol=1e-13)
            assert np.allclose(g_de[i].numpy(), d_dir[rows, :27].double().numpy().sum(0), rtol=1e-13, atol=1e-13)
