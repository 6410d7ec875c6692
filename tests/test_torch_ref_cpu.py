"""CPU tests of the float64 reference the field-backward tests differentiate (tests/torch_ref.py `field(..., masks=)`)."""
import numpy as np
import pytest
import torch

from oracle import mirror_nerf_oracle as O
from tests import field_fp64 as FC
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


# ---- the extension of TR.field for tests/test_hip_forward_fp64.py: position bands as a parameter, absent heads
def _field_before(w, xyz, dir_emb, with_normal=False):
    """TR.field as it stood before the extension (10 bands, both heads), restated: what the extended function must still be."""
    if with_normal and not xyz.requires_grad:
        xyz = xyz.requires_grad_(True)
    enc = TR.embed(xyz, 10)
    h = enc
    for i in range(8):
        if i == 4:
            h = torch.cat([enc, h], -1)
        h = torch.relu(h @ w[f"xyz_encoding_{i+1}.0.weight"].T + w[f"xyz_encoding_{i+1}.0.bias"])
    sigma = (h @ w["sigma.weight"].T + w["sigma.bias"])[:, 0]
    fin = h @ w["xyz_encoding_final.weight"].T + w["xyz_encoding_final.bias"]
    hd = torch.relu(torch.cat([fin, dir_emb], -1) @ w["dir_encoding.0.weight"].T + w["dir_encoding.0.bias"])
    rgb = torch.sigmoid(hd @ w["rgb.0.weight"].T + w["rgb.0.bias"])
    hn = h @ w["normal_net.0.weight"].T + w["normal_net.0.bias"]
    pn = TR.l2n(hn @ w["normal_net.1.weight"].T + w["normal_net.1.bias"])
    hm = torch.nn.functional.leaky_relu(h @ w["is_mirror_net.0.weight"].T + w["is_mirror_net.0.bias"], 0.01)
    m = torch.sigmoid(hm @ w["is_mirror_net.2.weight"].T + w["is_mirror_net.2.bias"])[:, 0]
    if with_normal:
        (grad,) = torch.autograd.grad(sigma, xyz, torch.ones_like(sigma), create_graph=True, retain_graph=True)
        return sigma, rgb, pn, m, TR.l2n(-grad)
    return sigma, rgb, pn, m


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_extended_field_with_ten_bands_and_both_heads_is_the_field_of_before(dtype):
    w = {k: v.to(dtype) for k, v in _weights(5).items()}
    xyz, de = [t.to(dtype) for t in _inputs(257, 2)]
    for a, b in zip(TR.field(w, xyz.clone(), de, with_normal=True), _field_before(w, xyz.clone(), de, with_normal=True)):
        assert a.dtype == dtype and torch.equal(a, b)
    with torch.no_grad():
        for a, b in zip(TR.field(w, xyz, de, n_bands=10), _field_before(w, xyz, de)):
            assert torch.equal(a, b)


def test_extended_field_absent_heads_are_none_and_leave_the_rest_alone():
    w = _weights(5)
    xyz, de = _inputs(64, 3)
    with torch.no_grad():
        full = TR.field(w, xyz, de)
        for drop in (("normal_net.",), ("is_mirror_net.",), ("normal_net.", "is_mirror_net.")):
            acts = {}
            got = TR.field({k: v for k, v in w.items() if not k.startswith(drop)}, xyz, de, acts=acts)
            assert (got[2] is None) == ("normal_net." in drop) and (got[3] is None) == ("is_mirror_net." in drop)
            assert ("hn" in acts) == ("normal_net." not in drop) and ("hm" in acts) == ("is_mirror_net." not in drop)
            for a, b in zip(got, full):
                assert a is None or torch.equal(a, b)


def test_extended_field_meets_fixture_g2():
    """fp32 TR.field on the inputs of fixture G2 (the reference's MirrorNeRF.forward), at the oracle's bar of that fixture."""
    from tests.golden import fixtures as FX
    fx = FX.Fixture("g2_field")
    w = {k: torch.from_numpy(v) for k, v in fx.state_dicts()[0].items()}
    x30 = torch.from_numpy(fx.inputs["x30"])
    sigma, rgb, pn, m, nrm = TR.field(w, x30[:, :3].clone(), x30[:, 3:], with_normal=True)
    got = {"full__sigma": sigma[:, None], "full__rgb": rgb, "full__pred_normal": pn, "full__is_mirror": m[:, None], "full__normal": nrm,
           "sigma_only__sigma": sigma[:, None], "sigma_only__pred_normal": pn}
    for k, v in got.items():
        err = float((v.detach().double() - torch.from_numpy(fx.outputs[k]).double()).abs().max())
        print(f"MEAS g2_field {k}: {err:.2e}")
        assert err <= 2e-6, (k, err)


_MAP_KEYS = dict(weights="weights", opacity="opacity", rgb="rgb", depth="depth", mask="mirror_mask", sn="surface_normal",
                 sng="surface_normal_grad", nd="normal_dif", xs="x_surface")


def _render_restated(sds, n_xyz, n_dir, rays, z, white, want_grad_normal):
    """render_rays' two passes at given depths with TR.field and TR.composite, fp32: {fixture key: tensor}."""
    out = {}
    for typ, sd in zip(("coarse", "fine"), sds):
        w = {k: torch.from_numpy(v) for k, v in sd.items()}
        zz = z[typ]
        N, S = zz.shape
        x = FC.ray_positions(rays, zz)
        de = TR.embed(rays[:, 3:6], n_dir).repeat_interleave(S, 0)
        res = TR.field(w, x, de, with_normal=want_grad_normal, n_bands=n_xyz)
        sigma, rgb, pn, m = [None if t is None else t.detach() for t in res[:4]]
        nrm = res[4].detach().view(N, S, 3) if want_grad_normal else None
        comp = TR.composite(rays, sigma.view(N, S), zz, None, rgb.view(N, S, 3), None if m is None else m.view(N, S),
                            None if pn is None else pn.view(N, S, 3), nrm, white)
        for k, v in comp.items():
            out[f"{_MAP_KEYS[k]}_{typ}"] = v
    return out


def _meets(name, got, fx, skip=()):
    from tests.golden import fixtures as FX
    n = 0
    for k, want in fx.outputs.items():
        g = got.get(k[:-7] if k.endswith("_direct") else k)
        if g is None or k in skip or k in FX.PER_SAMPLE_FINE[:1]:
            continue
        err = float((g.double() - torch.from_numpy(want).double()).abs().max())
        print(f"MEAS {name} {k}: {err:.2e} (bar {FX.tolerance(k, fx.meta):.1e})")
        assert err <= FX.tolerance(k, fx.meta), (name, k, err)
        n += 1
    return n


@pytest.mark.parametrize("name", ["g13_mask_head_only_train", "g13_no_normal_head_eval", "g13_normal_head_only_train", "g13_plain_nerf_test",
                                  "g13_plain_nerf_train"])
def test_extended_field_meets_the_fixtures_without_optional_heads(name):
    """G13 (the reference's render_rays / eval on models without normal_net, is_mirror_net or both): TR.field on those state
    dicts, composited with TR.composite at the fixture's own depths, against every map of the fixture that a plain render
    forms, at the fixture's bars (tests/golden/fixtures.py tolerance)."""
    from tests.golden import fixtures as FX
    from tests.golden import weights as GW
    fx = FX.Fixture(name)
    m = fx.meta
    sds = GW.make_state_dict(m["seed"], 2, predict_normal=m["predict_normal"], predict_mirror_mask=m["predict_mirror_mask"])
    for sd in sds:
        GW.apply_tweaks(sd, m["tweaks"])
    assert ("normal_net.0.weight" in sds[1]) == m["predict_normal"] and ("is_mirror_net.0.weight" in sds[1]) == m["predict_mirror_mask"]
    rays = torch.from_numpy(fx.inputs["rays"])
    z = {t: torch.from_numpy(fx.outputs[f"z_vals_{t}"]) for t in ("coarse", "fine")}
    got = _render_restated(sds, 10, 4, rays, z, m.get("white_back", False), any(k.startswith("surface_normal_grad") for k in fx.outputs))
    # the eval fixture holds the frame behind the recursion: its colour is blended with the reflected level's, its mirror mask
    # is the thresholded one (eval.py: 1 where the composited value is not below 0.5; no ray of the fixture within 1e-3 of it)
    skip = ("rgb_fine",) if name.endswith("_eval") else ()
    if name.endswith("_eval"):
        assert float((got["mirror_mask_fine"] - 0.5).abs().min()) > 1e-3
        got["mirror_mask_fine"] = (got["mirror_mask_fine"] >= 0.5).float()
    assert _meets(name, got, fx, skip) >= (6 if name.endswith(("_test", "_eval")) else 10)


def test_extended_field_meets_the_fixture_with_fewer_bands():
    """G16 (--N_emb_xyz 6 --N_emb_dir 2 through the reference's NeRFSystem.forward): TR.field(n_bands=6) on the 39 / 15-channel
    state dicts; the primary level's maps (rgb: the `_direct` keys, in front of the blend with the reflected level)."""
    from tests.golden import fixtures as FX
    fx = FX.Fixture("g16_nemb_6_2_train_grads")
    sds = fx.state_dicts()
    assert sds[1]["xyz_encoding_5.0.weight"].shape == (256, 256 + 39)
    rays = torch.from_numpy(fx.inputs["rays"])
    z = {t: torch.from_numpy(fx.outputs[f"z_vals_{t}"]) for t in ("coarse", "fine")}
    got = _render_restated(sds, 6, 2, rays, z, False, True)
    assert _meets("g16", got, fx, skip=("rgb_coarse", "rgb_fine", "loss")) >= 18
    with torch.no_grad():      # no bands at all: the raw coordinates are the encoding
        w = FC.weights("bands_0_0", torch.float64)
        x, d = FC.cloud("init", "box", 16)
        s = TR.field(w, x.double(), d.double(), n_bands=0)[0]
        assert s.shape == (16,) and w["xyz_encoding_1.0.weight"].shape == (256, 3)


def test_ray_mode_model_shows_a_wrong_ray_index():
    """The condition of the ray-mode cases of tests/test_hip_forward_fp64.py, on the reference alone: with every ray given its
    neighbour's direction the float64 rgb of the model those cases use moves by >= 1e-3 (median over samples) at every
    samples-per-ray count with 7 rays -- a view-encoding row taken from the wrong ray cannot hide below the bars."""
    for spr in FC.RAY_SPR:
        shift = FC.neighbour_shift(FC.RAY_MODEL, 7, spr)
        print(f"MEAS neighbour direction, spr {spr}: median rgb shift {shift:.2e}")
        assert shift >= 1e-3, (spr, shift)


def test_adversarial_sincos_positions_are_exact_and_in_range():
    x = FC.adversarial_sincos_positions()
    assert x.shape == (3072, 3) and x.dtype == torch.float32 and float(x.abs().max()) < 64.0
