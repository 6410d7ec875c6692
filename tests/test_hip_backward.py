"""GPU tests of the hand-written backward kernels against torch.autograd over the plain-torch
restatements in tests/torch_ref.py (fp32 on the same GPU; tolerance: relative 2e-3 of the largest
gradient entry, the bar SURVEY 8c sets for fixture G9)."""
import numpy as np
import pytest
import torch

from tests import torch_ref as TR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(autouse=True, params=["split", "fp32"])
def precision(request):
    """The training forward runs on either arithmetic of the field kernel (split-f16 default, bit-exact fp32); the
    backward kernels and tolerances are the same."""
    from mirror_nerf_amd import mirror_nerf as MN
    old = MN.PRECISION
    MN.set_precision(request.param)
    yield request.param
    MN.set_precision(old)


def _rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


@pytest.mark.parametrize("S,white", [(64, False), (192, True), (70, False)])
def test_composite_backward_matches_autograd(S, white):
    from mirror_nerf_amd.autograd import CompositeFn
    torch.manual_seed(S)
    N = 37
    rays = torch.randn(N, 8, device=DEV)
    z = torch.sort(torch.rand(N, S, device=DEV) * 6 + 0.1, 1)[0]
    noise = torch.randn(N, S, device=DEV) * 0.3
    base = dict(sigma=torch.randn(N, S, device=DEV) * 3, rgb=torch.rand(N, S, 3, device=DEV),
                m=torch.rand(N, S, device=DEV), pn=TR.l2n(torch.randn(N, S, 3, device=DEV)),
                nrm=TR.l2n(torch.randn(N, S, 3, device=DEV)))
    cot = {k: torch.randn(*s, device=DEV) for k, s in dict(weights=(N, S), opacity=(N,), rgb=(N, 3), depth=(N,),
                                                              mask=(N,), sn=(N, 3), sng=(N, 3), nd=(N,), xs=(N, 3)).items()}

    def leafs():
        r = rays.clone().requires_grad_(True)
        d = {k: v.clone().requires_grad_(True) for k, v in base.items()}
        return r, d

    r1, d1 = leafs()
    ref = TR.composite(r1, d1["sigma"], z, noise, d1["rgb"], d1["m"], d1["pn"], d1["nrm"], white)
    sum(((ref[k] * cot[k]).sum() for k in cot)).backward()
    r2, d2 = leafs()
    w, op, rgb_map, depth, mask, sn, sng, nd, xs = CompositeFn.apply(
        r2, d2["sigma"], z, noise, d2["rgb"].view(-1, 3), d2["m"].view(-1), d2["pn"].view(-1, 3), d2["nrm"].view(-1, 3), white)
    got = dict(weights=w, opacity=op, rgb=rgb_map, depth=depth, mask=mask, sn=sn, sng=sng, nd=nd, xs=xs)
    for k in cot:
        assert _rel(got[k], ref[k]) <= 1e-5, k
    sum(((got[k] * cot[k]).sum() for k in cot)).backward()
    assert _rel(r2.grad, r1.grad) <= 1e-5
    for k in base:
        assert _rel(d2[k].grad, d1[k].grad) <= 2e-4, (k, _rel(d2[k].grad, d1[k].grad))


@pytest.mark.parametrize("mode", ["mask", "outside", "normal", "mask+normal"])
def test_composite_backward_detach_options(mode):
    """rendering.py:223-247: the mirror mask / the normal outputs composited with weights.detach()."""
    from mirror_nerf_amd import _lib
    from mirror_nerf_amd.autograd import CompositeFn
    torch.manual_seed(11)
    N, S = 29, 96
    rays = torch.randn(N, 8, device=DEV)
    z = torch.sort(torch.rand(N, S, device=DEV) * 6 + 0.1, 1)[0]
    base = dict(sigma=torch.randn(N, S, device=DEV) * 3, rgb=torch.rand(N, S, 3, device=DEV),
                m=torch.rand(N, S, device=DEV), pn=TR.l2n(torch.randn(N, S, 3, device=DEV)),
                nrm=TR.l2n(torch.randn(N, S, 3, device=DEV)))
    cot = {k: torch.randn(*s, device=DEV) for k, s in dict(rgb=(N, 3), mask=(N,), sn=(N, 3), sng=(N, 3), nd=(N,)).items()}
    keep = (torch.rand(N, device=DEV) < 0.5) if mode == "outside" else None
    flags = (_lib.MNRF_DETACH_W_MASK if "mask" in mode else 0) | (_lib.MNRF_DETACH_W_NORMAL if "normal" in mode else 0)
    d1 = {k: v.clone().requires_grad_(True) for k, v in base.items()}
    ref = TR.composite(rays, d1["sigma"], z, None, d1["rgb"], d1["m"], d1["pn"], d1["nrm"], False,
                       detach_mask="mask" in mode, keep_mirror=keep, detach_normal="normal" in mode)
    sum(((ref[k] * cot[k]).sum() for k in cot)).backward()
    d2 = {k: v.clone().requires_grad_(True) for k, v in base.items()}
    w, op, rgb_map, depth, mask, sn, sng, nd, xs = CompositeFn.apply(
        rays, d2["sigma"], z, None, d2["rgb"].view(-1, 3), d2["m"].view(-1), d2["pn"].view(-1, 3), d2["nrm"].view(-1, 3), False,
        flags, None if keep is None else keep.float())
    got = dict(rgb=rgb_map, mask=mask, sn=sn, sng=sng, nd=nd)
    sum(((got[k] * cot[k]).sum() for k in cot)).backward()
    for k in base:
        assert _rel(d2[k].grad, d1[k].grad) <= 2e-4, (k, _rel(d2[k].grad, d1[k].grad))
    # and the option is not a no-op: the flag-less gradient of sigma differs
    d3 = {k: v.clone().requires_grad_(True) for k, v in base.items()}
    ref0 = TR.composite(rays, d3["sigma"], z, None, d3["rgb"], d3["m"], d3["pn"], d3["nrm"], False)
    sum(((ref0[k] * cot[k]).sum() for k in cot)).backward()
    assert _rel(d3["sigma"].grad, d1["sigma"].grad) > 1e-2


def _field_setup(seed=5):
    import mirror_nerf_amd as M
    from tests.golden import weights as GW
    sd = GW.apply_tweaks(GW.make_state_dict(seed, 1)[0], GW.OPAQUE)
    m = M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=True)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to(DEV), sd


@pytest.mark.parametrize("B", [200, 1000])
def test_field_backward_matches_autograd_xyz_mode(B):
    """All 32 parameter gradients, dL/dxyz and dL/d(view encoding) of the fused field kernel."""
    from mirror_nerf_amd.autograd import FieldFn
    m, sd = _field_setup()
    torch.manual_seed(B)
    xyz = (torch.rand(B, 3, device=DEV) * 6 - 3)
    d = TR.l2n(torch.randn(B, 3, device=DEV))
    de = TR.embed(d, 4)
    cot = [torch.randn(B, device=DEV), torch.randn(B, 3, device=DEV), torch.randn(B, 3, device=DEV), torch.randn(B, device=DEV)]
    # reference
    w = {k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in sd.items()}
    x1 = xyz.clone().requires_grad_(True)
    de1 = de.clone().requires_grad_(True)
    outs = TR.field(w, x1, de1)
    sum((o * c).sum() for o, c in zip(outs, cot)).backward()
    # HIP
    x2 = xyz.clone().requires_grad_(True)
    de2 = de.clone().requires_grad_(True)
    params = list(m.parameters())
    got = FieldFn.apply(m, 1, x2, None, None, de2, False, *params)
    for o, r in zip(got[:4], outs):
        assert _rel(o, r) <= 2e-5
    sum((o * c).sum() for o, c in zip(got[:4], cot)).backward()
    names = [n for n, _ in m.named_parameters()]
    worst = 0.0
    for n, p in zip(names, params):
        e = _rel(p.grad, w[n].grad)
        worst = max(worst, e)
        assert e <= 2e-3, (n, e)
    assert _rel(x2.grad, x1.grad) <= 2e-3
    assert _rel(de2.grad, de1.grad) <= 2e-3
    print("worst relative parameter-gradient error", worst)


@pytest.mark.parametrize("mode", ["normal", "mirror", "outside", "normal+mirror"])
def test_field_backward_cut_heads(mode):
    """mirror_nerf.py:154-183: normal_net / is_mirror_net evaluated on geo_feat.detach() (all samples, or the samples of rays
    outside the GT mirror mask): their own weights still get gradients, the trunk does not see them."""
    from mirror_nerf_amd import _lib
    from mirror_nerf_amd.autograd import FieldFn
    m, sd = _field_setup()
    torch.manual_seed(21)
    N, S = 20, 16
    rays = torch.randn(N, 8, device=DEV)
    rays[:, 3:6] = TR.l2n(rays[:, 3:6])
    z = torch.sort(torch.rand(N, S, device=DEV) * 4 + 0.2, 1)[0]
    de = TR.embed(rays[:, 3:6], 4)
    B = N * S
    # small cotangents on sigma / rgb, large on the mirror probability (its sigmoid and 1/sqrt(128)-sized output weights
    # make its share of dL/dh8 ~1 % otherwise): the cut heads dominate the trunk gradient
    cot = [torch.randn(B, device=DEV) * 0.01, torch.randn(B, 3, device=DEV) * 0.01, torch.randn(B, 3, device=DEV),
           torch.randn(B, device=DEV) * 30]
    keep = (torch.rand(N, device=DEV) < 0.5) if mode == "outside" else None
    cut = (_lib.MNRF_CUT_NORMAL_HEAD if "normal" in mode else 0) | (_lib.MNRF_CUT_MIRROR_HEAD if "mirror" in mode else 0)
    w = {k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in sd.items()}
    xyz = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3)
    outs = TR.field(w, xyz, de.repeat_interleave(S, 0), cut_normal="normal" in mode, cut_mirror="mirror" in mode,
                    keep_mirror=None if keep is None else keep.repeat_interleave(S, 0))
    sum((o * c).sum() for o, c in zip(outs, cot)).backward()
    params = list(m.parameters())
    got = FieldFn.apply(m, S, None, rays, z, de, (False, cut, None if keep is None else keep.float()), *params)
    sum((o * c).sum() for o, c in zip(got[:4], cot)).backward()
    names = [n for n, _ in m.named_parameters()]
    for n, p in zip(names, params):
        assert _rel(p.grad, w[n].grad) <= 2e-3, (n, _rel(p.grad, w[n].grad))
    # not a no-op: without the cut the trunk gradient is different
    w0 = {k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in sd.items()}
    outs0 = TR.field(w0, xyz, de.repeat_interleave(S, 0))
    sum((o * c).sum() for o, c in zip(outs0, cot)).backward()
    assert _rel(w0["xyz_encoding_8.0.weight"].grad, w["xyz_encoding_8.0.weight"].grad) > 0.1


def test_field_backward_ray_mode_accumulates_over_samples():
    from mirror_nerf_amd.autograd import FieldFn
    m, sd = _field_setup(7)
    torch.manual_seed(0)
    N, S = 24, 16      # 384 samples: 3 tiles of 128
    rays = torch.randn(N, 8, device=DEV)
    rays[:, 3:6] = TR.l2n(rays[:, 3:6])
    z = torch.sort(torch.rand(N, S, device=DEV) * 4 + 0.2, 1)[0]
    de = TR.embed(rays[:, 3:6], 4)
    cot = [torch.randn(N * S, device=DEV), torch.randn(N * S, 3, device=DEV), torch.randn(N * S, 3, device=DEV),
           torch.randn(N * S, device=DEV)]
    w = {k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in sd.items()}
    r1 = rays.clone().requires_grad_(True)
    de1 = de.clone().requires_grad_(True)
    xyz = (r1[:, None, 0:3] + r1[:, None, 3:6] * z[..., None]).reshape(-1, 3)
    outs = TR.field(w, xyz, de1.repeat_interleave(S, 0))
    sum((o * c).sum() for o, c in zip(outs, cot)).backward()
    r2 = rays.clone().requires_grad_(True)
    de2 = de.clone().requires_grad_(True)
    params = list(m.parameters())
    got = FieldFn.apply(m, S, None, r2, z, de2, True, *params)
    assert got[4].shape == (N * S, 3)
    sum((o * c).sum() for o, c in zip(got[:4], cot)).backward()
    assert _rel(r2.grad[:, :6], r1.grad[:, :6]) <= 2e-3
    assert _rel(de2.grad, de1.grad) <= 2e-3
    for (n, p) in zip([n for n, _ in m.named_parameters()], params):
        assert _rel(p.grad, w[n].grad) <= 2e-3, n


@pytest.mark.parametrize("name", ["g9_train_grads", "g9_train_grads_full", "g9b_detach_mask", "g9b_detach_outside_mirror",
                                  "g9b_detach_normal", "g9b_detach_ref_color", "g16_nemb_6_2_train_grads", "g11_trained_grads_full"])
def test_train_step_gradients_golden(name):
    _golden_gradients(name)


def _golden_gradients(name):
    """G9: gradients of a first-order loss through the whole train-semantics render (coarse + fine
    pass, GT mirror mask, compacted reflected rays, blend) against the reference's autograd,
    captured by tests/golden/make_golden.py.  Tolerance: 1e-3 of each tensor's largest gradient.
    G9b (tests/golden/make_golden_flags.py): the same step with ONE gradient-steering option on each
    (--detach_density_for_mask_loss, --detach_density_outside_mirror_for_mask_loss, --detach_density_for_normal_loss,
    --detach_ref_color_for_blend; models/rendering.py:223-247, models/mirror_nerf.py:154-183, train.py:284-289); the
    generator asserted that each option moves the reference's gradients by >= 100 % on some tensor.
    g11_trained_grads_full (tests/golden/make_golden_trained_capture.py): the full loss -- normal terms, hence the second-order
    pass -- on the briefly TRAINED pair, where the signals of that pass have realistic magnitudes (|b| up to 50); the planes
    and the rows route of its weight gradients give the same error figures to three digits there (<= 9e-3 against a floor of
    1.5e-2)."""
    from types import SimpleNamespace
    import mirror_nerf_amd as M
    from tests.golden import fixtures as FX
    from tests.golden import make_golden_loss as GL
    from tests.golden.make_golden_loss import grad_summary
    fx = FX.Fixture(name)
    first_order_loss = getattr(GL, fx.meta.get("loss", "first_order_loss"))
    sds = fx.state_dicts()
    hp = dict(fx.meta["hp"])
    # (G16, tests/golden/make_golden_nemb.py: --N_emb_xyz 6 --N_emb_dir 2 on the kernels built for 10 / 4 bands)
    hp.update(N_emb_xyz=fx.meta.get("N_emb_xyz", 10), N_emb_dir=fx.meta.get("N_emb_dir", 4), predict_normal=True,
              predict_mirror_mask=True, model_type="nerf")
    system = M.NeRFSystem(SimpleNamespace(**hp))
    system.nerf_coarse.load_state_dict({k: torch.from_numpy(v) for k, v in sds[0].items()})
    system.nerf_fine.load_state_dict({k: torch.from_numpy(v) for k, v in sds[1].items()})
    system.to(DEV)
    t = lambda k: torch.from_numpy(fx.inputs[k]).to(DEV)  # noqa: E731
    extra = {"mirror_mask": t("gt_mask"), "is_eval": False, "train_geometry_stage": False}
    extra.update(fx.meta.get("extra", {}))
    res = system(t("rays"), extra)
    loss = first_order_loss(res, t("target"), t("gt_mask"))
    assert abs(loss.item() - float(fx.outputs["loss"])) <= (2e-3 if fx.meta.get("loss") == "full_loss" else 1e-5)
    if name.startswith("g16"):      # this fixture also holds the forward dict of the step
        from tests.golden.fixtures import PER_SAMPLE_FINE, tolerance
        n_cmp = 0
        for k, want in fx.outputs.items():
            if k == "loss" or k.startswith("grad__") or k in PER_SAMPLE_FINE or k not in res:
                continue
            d = float(np.max(np.abs(res[k].detach().cpu().numpy().astype(np.float64) - want))) if want.size else 0.0
            assert d <= tolerance(k, fx.meta), (k, d)
            n_cmp += 1
        assert n_cmp >= 15
    loss.backward()
    worst = 0.0
    report = []
    for mname, mod in (("coarse", system.nerf_coarse), ("fine", system.nerf_fine)):
        for pn_, p_ in mod.named_parameters():
            want = fx.outputs[f"grad__{mname}__{pn_}"]
            got = grad_summary(p_.grad.cpu() if p_.grad is not None else None, p_.detach().cpu())
            scale = max(want[2], 1e-12)
            err = np.max(np.abs(got[3:] - want[3:])) / scale
            worst = max(worst, err)
            nerr = abs(got[1] - want[1]) / max(want[1], 1e-12)
            report.append((err, nerr, mname, pn_))
    report.sort(reverse=True)
    print("G9 relative gradient errors (entry-wise / norm), worst first:")
    for err, nerr, mname, pn_ in report[:8]:
        print(f"  {err:.2e} {nerr:.2e} {mname} {pn_}")
    floor = fx.meta.get("grad_floor", 0.0)
    # G9b with the density detached from the dominant loss term: what is left of d/d sigma.{weight,bias} is a cancellation
    # residue (~6 % of the flag-less gradient) of per-sample terms, on which the reference itself moves by `floor` = 0.9 %
    # between fp32 and fp64; the split arithmetic's 3e-6 on sigma shows as 4 x that (fp32 arithmetic: 5e-4): 8 x floor there
    tol = max(1e-3, (8 if name.startswith("g9b_detach_mask") or name.startswith("g9b_detach_outside") else 4) * floor)
    bad = [r for r in report if r[0] > tol or r[1] > tol]
    assert not bad, bad[:4]
    # whole tensors, entry by entry (g9_train_grads_full: first trunk layer, skip layer, density head, colour branch's first layer
    # of both models = 268 k entries instead of 8 x 48), against the reference's fp32 gradients AND its float64 run of the same
    # step: within 1e-3 of the tensor's largest entry of the fp32 capture (or 4 x the capture's own distance from float64), and
    # no further from the float64 truth than twice the reference's fp32 run is (+ 1e-3)
    full = [k for k in fx.outputs if k.startswith("gradfull__")]
    if name == "g9_train_grads_full":
        assert len(full) == 8, full
    for k in full:
        _, mname, pn_ = k.split("__")
        want32 = fx.outputs[k].astype(np.float64)
        want64 = fx.outputs[k.replace("gradfull__", "gradfull64__")].astype(np.float64)
        mod = system.nerf_coarse if mname == "coarse" else system.nerf_fine
        got = dict(mod.named_parameters())[pn_].grad.detach().cpu().numpy().astype(np.float64)
        assert got.shape == want32.shape, (k, got.shape, want32.shape)
        scale = float(np.abs(want64).max())
        own = float(np.abs(want32 - want64).max()) / scale
        e32 = float(np.abs(got - want32).max()) / scale
        e64 = float(np.abs(got - want64).max()) / scale
        print(f"  full tensor {mname} {pn_}: vs fp32 capture {e32:.2e}, vs float64 {e64:.2e} (reference fp32 vs float64 {own:.2e})")
        assert e32 <= max(1e-3, 4 * own), (k, e32, own)
        assert e64 <= 2 * own + 1e-3, (k, e64, own)
    return {f"{mname}.{pn_}": p_.grad.detach().clone() for mname, mod in (("coarse", system.nerf_coarse), ("fine", system.nerf_fine))
            for pn_, p_ in mod.named_parameters() if p_.grad is not None}


@pytest.mark.parametrize("name", ["g9_train_grads", "g9_train_grads_full", "g16_nemb_6_2_train_grads", "g11_trained_grads_full"])
def test_half_dy_planes_hold_the_gradient_bar(name, monkeypatch):
    """MNRF_DW_PLANES_HALF=1 (round 6, opt-in; include/mnrf.h MNRF_PLANES_Y_HALF): the activation gradients reach the weight-gradient
    GEMM as ONE f16 per element -- the producer's lo tiles are dropped by a zero-record buffer descriptor, the GEMM fetches and
    multiplies the hi tiles only.  The reference's captured gradients are met at the fixtures' own tolerances, and every tensor is
    within 1e-3 of its largest entry of the exact (hi/lo) route -- what scripts/exp_half_planes.py predicted from the reference in
    float64 (profiles/r06_half_planes_emulation.json: 1.2e-4 .. 7.4e-4)."""
    from mirror_nerf_amd import autograd as AG
    exact = _golden_gradients(name)
    monkeypatch.setattr(AG, "DW_PLANES_HALF", True)
    half = _golden_gradients(name)
    worst = 0.0
    for k, g in exact.items():
        scale = float(g.abs().max())
        if scale == 0.0:
            continue
        err = float((half[k] - g).abs().max()) / scale
        worst = max(worst, err)
        assert err <= 1e-3, (k, err)
    from mirror_nerf_amd import mirror_nerf as MN
    if MN.PRECISION.startswith("split"):      # (the fp32 arithmetic has no operand planes: the flag means nothing there)
        assert worst > 1e-7, "the half route produced the exact route's bits: the flag did not reach the kernels"
    print(f"  {name}: dY as one f16 vs hi/lo planes, worst tensor {worst:.2e} of its largest entry")


def test_field_second_order_backward_matches_double_backward():
    """The gradient that reaches the weights (and xyz) through normal = l2n(-d sigma/d xyz):
    hand-written tangent pass vs torch's double backward (create_graph=True)."""
    from mirror_nerf_amd.autograd import FieldFn
    m, sd = _field_setup(11)
    torch.manual_seed(3)
    B = 300
    xyz = (torch.rand(B, 3, device=DEV) * 4 - 2)
    de = TR.embed(TR.l2n(torch.randn(B, 3, device=DEV)), 4)
    cot_n = torch.randn(B, 3, device=DEV)
    cot_s = torch.randn(B, device=DEV)
    w = {k: torch.from_numpy(v).to(DEV).requires_grad_(True) for k, v in sd.items()}
    x1 = xyz.clone().requires_grad_(True)
    outs = TR.field(w, x1, de, with_normal=True)
    ((outs[4] * cot_n).sum() + (outs[0] * cot_s).sum()).backward()
    x2 = xyz.clone().requires_grad_(True)
    params = list(m.parameters())
    got = FieldFn.apply(m, 1, x2, None, None, de, True, *params)
    # forward normals agree where the gradient is well conditioned
    assert float((got[4] - outs[4]).abs().median()) <= 1e-5
    ((got[4] * cot_n).sum() + (got[0] * cot_s).sum()).backward()
    names = [n for n, _ in m.named_parameters()]
    report = sorted(((_rel(p.grad, w[n].grad if w[n].grad is not None else torch.zeros_like(p)), n)
                     for n, p in zip(names, params)), reverse=True)
    print("second-order: worst relative gradient errors", report[:4])
    assert report[0][0] <= 5e-3, report[:4]
    assert _rel(x2.grad, x1.grad) <= 5e-3


@pytest.mark.parametrize("compact", [True, False])
def test_reflect_blend_embed_backward(compact):
    """Per-ray glue of the training path: HIP forward + HIP backward vs torch.autograd."""
    from mirror_nerf_amd.autograd import BlendFn, EmbedFn, ReflectFn
    torch.manual_seed(4)
    N = 1500
    rays = torch.randn(N, 8, device=DEV)
    xs = torch.randn(N, 3, device=DEV)
    nrm = torch.randn(N, 3, device=DEV)
    nrm[3] = 0                                     # eps-clamped normal
    mask = (torch.rand(N, device=DEV) < 0.3).float()
    M = int(mask.sum().item()) if compact else N
    cot = torch.randn(M, 8, device=DEV)
    leaf = lambda t: t.clone().requires_grad_(True)  # noqa: E731
    r1, x1, n1 = leaf(rays), leaf(xs), leaf(nrm)
    (TR.reflect(r1, x1, n1, mask, compact) * cot).sum().backward()
    r2, x2, n2 = leaf(rays), leaf(xs), leaf(nrm)
    sec, index, rdir, _count = ReflectFn.apply(r2, x2, n2, mask, compact)
    assert sec.shape == (M, 8)
    (sec * cot).sum().backward()
    assert _rel(x2.grad, x1.grad) <= 1e-6 and _rel(n2.grad, n1.grad) <= 1e-5 and _rel(r2.grad, r1.grad) <= 1e-5
    # blend
    base = torch.rand(N, 3, device=DEV)
    srgb = torch.rand(M, 3, device=DEV)
    cot2 = torch.randn(N, 3, device=DEV)
    b1, s1 = leaf(base), leaf(srgb)
    (TR.blend(b1, s1, mask, compact) * cot2).sum().backward()
    b2, s2 = leaf(base), leaf(srgb)
    out = BlendFn.apply(b2, s2, index, mask, compact)
    assert _rel(out, TR.blend(base, srgb, mask, compact)) <= 1e-6
    (out * cot2).sum().backward()
    assert _rel(b2.grad, b1.grad) <= 1e-6 and _rel(s2.grad, s1.grad) <= 1e-6
    # embedding
    d = TR.l2n(torch.randn(N, 3, device=DEV))
    cot3 = torch.randn(N, 27, device=DEV)
    d1, d2 = leaf(d), leaf(d)
    (TR.embed(d1, 4) * cot3).sum().backward()
    (EmbedFn.apply(d2, 4) * cot3).sum().backward()
    assert _rel(d2.grad, d1.grad) <= 1e-5


def test_split_training_path_agrees_with_fp32_path(precision):
    """The whole training path of the field -- forward with saved activations, activation gradients, the second-order
    pass through the density-gradient normal, weight gradients -- on the split arithmetic (f16 hi/lo pairs forward and backward, one power-of-two scale per sample in the
    backward, exact bf16 triples in the dW GEMMs) against the bit-exact fp32 kernels on the same inputs, with upstream
    gradients spread over 12 orders of magnitude (compositing weights do that).  Bound: 2e-5 of each tensor's largest
    entry (measured: printed)."""
    if precision != "split":
        pytest.skip("one comparison covers both")
    from mirror_nerf_amd.autograd import FieldFn
    from mirror_nerf_amd import mirror_nerf as MN
    m, sd = _field_setup(11)
    torch.manual_seed(1)
    N, S = 64, 24
    rays = torch.randn(N, 8, device=DEV)
    rays[:, 3:6] = TR.l2n(rays[:, 3:6])
    z = torch.sort(torch.rand(N, S, device=DEV) * 4 + 0.2, 1)[0]
    de = TR.embed(rays[:, 3:6], 4)
    scale = 10.0 ** (-12 * torch.rand(N * S, device=DEV))          # per-sample magnitudes 1 .. 1e-12
    cot = [torch.randn(N * S, device=DEV) * scale, torch.randn(N * S, 3, device=DEV) * scale[:, None],
           torch.randn(N * S, 3, device=DEV) * scale[:, None], torch.randn(N * S, device=DEV) * scale,
           torch.randn(N * S, 3, device=DEV) * scale[:, None] * 1e-2]     # the density-gradient normal: second-order pass
    res = {}
    for mode in ("fp32", "split"):
        MN.set_precision(mode)
        r = rays.clone().requires_grad_(True)
        d = de.clone().requires_grad_(True)
        params = list(m.parameters())
        for p in params:
            p.grad = None
        got = FieldFn.apply(m, S, None, r, z, d, True, *params)
        sum((o * c).sum() for o, c in zip(got[:5], cot)).backward()
        res[mode] = [r.grad.clone(), d.grad.clone()] + [p.grad.clone() for p in params]
    worst = max(_rel(a, b) for a, b in zip(res["split"], res["fp32"]))
    print("split vs fp32 training path: worst relative gradient difference", worst)
    assert worst <= 2e-5, worst


@pytest.mark.parametrize("fused", [True, False])
def test_optimizer_steps_are_seen_by_the_next_launch(fused):
    """The kernels read a packed image of the weights, cached per module.  torch's FUSED optimizers update parameters
    without bumping Tensor._version (the cache key of round 1): the image went stale and training stood still.  Now any
    optimizer step invalidates the images (weights._GENERATION): the loss of a repeated batch must fall, and the image
    must follow the parameters, with either Adam implementation."""
    from types import SimpleNamespace
    import mirror_nerf_amd as M
    from mirror_nerf_amd import synthetic as SY, training
    torch.manual_seed(0)
    system = M.NeRFSystem(training.default_hparams(N_importance=64, perturb=0.0, noise_std=0.0)).to(DEV)
    opt = torch.optim.Adam(list(system.parameters()), lr=5e-4, fused=fused)
    rays = SY.device_rays(32, 32, DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    tgt, gt = torch.rand(1024, 3, device=DEV, generator=g), (torch.rand(1024, device=DEV, generator=g) < 0.25).float()
    loss_fn = training.total_loss_fn(SimpleNamespace(), epoch=5)
    losses, images = [], []
    for _ in range(12):
        losses.append(float(training.train_step(system, opt, rays, tgt, gt, loss_fn, epoch=5)))
        images.append(system.nerf_fine.__dict__["_mnrf_packed"].packed[:4096].clone())
    assert min(losses[6:]) < losses[0] - 5e-3, losses
    assert all(not torch.equal(images[i], images[i + 1]) for i in range(1, 11)), "the packed image does not follow the optimizer"


@pytest.mark.parametrize("B,n_eval", [(200, 1), (4096 + 77, 2)])
def test_planes_route_agrees_with_rows_route(B, n_eval, precision):
    """Through the C ABI on the same samples and seeds (eight orders of magnitude apart): mnrf_field_forward_train with
    MNRF_TRAIN_PLANES gives bit-identical outputs and ReLU masks, mnrf_field_backward_planes bit-identical dL/dxyz and
    dL/d(view encoding), and mnrf_dw_planes -- one launch over n_eval evaluations -- the 32 parameter gradients of
    mnrf_field_backward to 1e-5 of each tensor's largest entry (measured 5e-6: hi/lo f16 operands with one power-of-two
    scale per evaluation against fp32 rows split into bf16 x 3)."""
    import ctypes
    import mirror_nerf_amd as M
    from mirror_nerf_amd import _lib
    from mirror_nerf_amd.weights import PARAM_NAMES, PARAM_SHAPES, packed_of
    if precision != "split":
        pytest.skip("the plane route belongs to the split arithmetic")
    L, p = _lib.lib(), _lib.ptr
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=DEV)  # noqa: E731
    torch.manual_seed(B)
    model = M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=True).to(DEV)
    with torch.no_grad():
        model.sigma.weight.mul_(20.0)
    packed = packed_of(model)
    xyz = (torch.rand(B, 3, device=DEV) * 6 - 3).contiguous()
    de = M.Embedding(4)(torch.nn.functional.normalize(torch.randn(B, 3, device=DEV), dim=1))
    outs, saves = {}, {}
    for mode in ("rows", "planes"):
        o = (f(B), f(B, 3), f(B, 3), f(B), f(B, 3))
        sx = f(L.mnrf_train_save_floats(B)) if mode == "rows" else \
            torch.zeros(L.mnrf_train_planes_bytes(B), dtype=torch.uint8, device=DEV)
        sm = torch.zeros(L.mnrf_train_mask_words(B), dtype=torch.int64, device=DEV)
        si, sj = f(B), f(B)
        flags = _lib.MNRF_SPLIT_F16 | (_lib.MNRF_TRAIN_PLANES if mode == "planes" else 0)
        _lib.check(L.mnrf_field_forward_train(p(packed), B, p(xyz), 3, None, None, 1, p(de), 27, *[p(t) for t in o], p(sx), p(sm),
                                              p(si), p(sj), flags, _lib.stream()), "forward " + mode)
        outs[mode], saves[mode] = o, (sx, sm, si, sj)
    for a, b in zip(outs["rows"], outs["planes"]):
        assert torch.equal(a, b)
    assert torch.equal(saves["rows"][1], saves["planes"][1])
    scale = 10.0 ** (torch.rand(B, device=DEV) * 8 - 8)
    g_sigma = torch.randn(B, device=DEV) * scale
    g_rgb, g_pn, g_m = (torch.randn(B, 3, device=DEV) * scale[:, None], torch.randn(B, 3, device=DEV) * scale[:, None],
                        torch.randn(B, device=DEV) * scale)
    _, rgb, pn, mir, _ = outs["rows"]
    ws = f(L.mnrf_train_workspace_floats(B))
    d_r = [f(*PARAM_SHAPES[n]) for n in PARAM_NAMES]
    dx_r, dd_r = f(B, 3), f(B, 32)
    _lib.check(L.mnrf_field_backward(p(packed), B, p(xyz), 3, None, None, 1, p(g_sigma), p(g_rgb), p(g_pn), p(g_m), p(rgb), p(pn),
                                     p(mir), p(saves["rows"][0]), p(saves["rows"][1]), p(saves["rows"][2]), p(ws),
                                     (ctypes.c_void_p * 32)(*[t.data_ptr() for t in d_r]), p(dx_r), p(dd_r), None,
                                     _lib.MNRF_SPLIT_F16, _lib.stream()), "backward rows")
    dy = torch.zeros(L.mnrf_train_dy_planes_bytes(B), dtype=torch.uint8, device=DEV)
    seedmax = torch.zeros(1, dtype=torch.int32, device=DEV)
    dx_p, dd_p = f(B, 3), f(B, 32)
    _lib.check(L.mnrf_field_backward_planes(p(packed), B, p(xyz), 3, None, None, 1, p(g_sigma), p(g_rgb), p(g_pn), p(g_m), p(rgb),
                                            p(pn), p(mir), p(saves["planes"][1]), p(saves["planes"][2]), p(dy), p(seedmax),
                                            p(dx_p), p(dd_p), None, 0, _lib.stream()), "backward planes")
    assert torch.equal(dx_r, dx_p) and torch.equal(dd_r, dd_p)
    d_p = [f(*PARAM_SHAPES[n]) for n in PARAM_NAMES]
    bs = (ctypes.c_int64 * n_eval)(*[B] * n_eval)
    wsp = f(L.mnrf_dw_planes_workspace_floats(n_eval, bs))
    _lib.check(L.mnrf_dw_planes(n_eval, (ctypes.c_void_p * n_eval)(*[saves["planes"][0].data_ptr()] * n_eval),
                                (ctypes.c_void_p * n_eval)(*[dy.data_ptr()] * n_eval), bs,
                                (ctypes.c_void_p * n_eval)(*[seedmax.data_ptr()] * n_eval), p(wsp),
                                (ctypes.c_void_p * 32)(*[t.data_ptr() for t in d_p]), 0, _lib.stream()), "dw planes")
    torch.cuda.synchronize()
    for n, a, b in zip(PARAM_NAMES, d_p, d_r):
        assert _rel(a, n_eval * b) <= 1e-5, n


@pytest.mark.parametrize("r", [4, 8])
def test_lowered_gradient_scale_gives_the_same_weight_gradients(r):
    """mnrf_field_backward_planes with the per-sample seed scale lowered by 2^r (flags r << 16: what training does when scaled
    gradients outgrow the f16 range, mirror_nerf._lower_gradient_scale) + mnrf_dw_planes2 told the same r (kinds r << 8): the
    same dL/dxyz / dL/d(view encoding) and the same 32 weight gradients as r = 0 up to what the lower scale costs at torch's
    default initialisation, where gradients SHRINK on the way down the trunk and lose their low f16 halves earlier (measured:
    1.3e-4 of the first layer's largest entry at r = 4) -- the scale is only lowered after gradients have outGROWN the range."""
    import ctypes
    import mirror_nerf_amd as M
    from mirror_nerf_amd import _lib
    from mirror_nerf_amd.weights import PARAM_NAMES, PARAM_SHAPES, packed_of
    L, p = _lib.lib(), _lib.ptr
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=DEV)  # noqa: E731
    torch.manual_seed(11)
    B = 3000
    model = M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=True).to(DEV)
    with torch.no_grad():
        model.sigma.weight.mul_(20.0)
    packed = packed_of(model)
    xyz = (torch.rand(B, 3, device=DEV) * 6 - 3).contiguous()
    de = M.Embedding(4)(torch.nn.functional.normalize(torch.randn(B, 3, device=DEV), dim=1))
    o = (f(B), f(B, 3), f(B, 3), f(B), f(B, 3))
    sx = torch.zeros(L.mnrf_train_planes_bytes(B), dtype=torch.uint8, device=DEV)
    sm = torch.zeros(L.mnrf_train_mask_words(B), dtype=torch.int64, device=DEV)
    si, sj = f(B), f(B)
    _lib.check(L.mnrf_field_forward_train(p(packed), B, p(xyz), 3, None, None, 1, p(de), 27, *[p(t) for t in o], p(sx), p(sm),
                                          p(si), p(sj), _lib.MNRF_SPLIT_F16 | _lib.MNRF_TRAIN_PLANES, _lib.stream()), "forward")
    g_sigma, g_rgb, g_pn, g_m = torch.randn(B, device=DEV), torch.randn(B, 3, device=DEV), torch.randn(B, 3, device=DEV), torch.randn(B, device=DEV)
    TOL = {4: (1e-4, 5e-4), 8: (2e-3, 1e-2)}      # (dL/dx, weight gradients) -- measured: see the print below
    res = {}
    for red in (0, r):
        dy = torch.zeros(L.mnrf_train_dy_planes_bytes(B), dtype=torch.uint8, device=DEV)
        seedmax = torch.zeros(1, dtype=torch.int32, device=DEV)
        dx, dd = f(B, 3), f(B, 32)
        _lib.check(L.mnrf_field_backward_planes(p(packed), B, p(xyz), 3, None, None, 1, p(g_sigma), p(g_rgb), p(g_pn), p(g_m), p(o[1]),
                                                p(o[2]), p(o[3]), p(sm), p(si), p(dy), p(seedmax), p(dx), p(dd), None, red << 16,
                                                _lib.stream()), "backward planes")
        d_p = [f(*PARAM_SHAPES[n]) for n in PARAM_NAMES]
        bs, kd = (ctypes.c_int64 * 1)(B), (ctypes.c_int * 1)(red << 8)
        ws = f(L.mnrf_dw_planes2_workspace_floats(1, bs, kd))
        _lib.check(L.mnrf_dw_planes2(1, (ctypes.c_void_p * 1)(sx.data_ptr()), (ctypes.c_void_p * 1)(dy.data_ptr()), bs,
                                     (ctypes.c_void_p * 1)(seedmax.data_ptr()), kd, p(ws),
                                     (ctypes.c_void_p * 32)(*[t.data_ptr() for t in d_p]), 0, _lib.stream()), "dw planes2")
        torch.cuda.synchronize()
        res[red] = (dx, dd, d_p)
    # (a power-of-two scale is exact in fp32; the f16 halves of small gradients fall into subnormals earlier at the lower scale)
    worst = max((_rel(a, b), n) for n, a, b in zip(PARAM_NAMES, res[r][2], res[0][2]))
    print(f"r = {r}: dL/dxyz {_rel(res[r][0], res[0][0]):.2e}, dL/d(view encoding) {_rel(res[r][1], res[0][1]):.2e}, worst weight gradient {worst}")
    assert _rel(res[r][0], res[0][0]) <= TOL[r][0] and _rel(res[r][1], res[0][1]) <= TOL[r][0]
    assert worst[0] <= TOL[r][1], worst


@pytest.mark.parametrize("B,ray_mode", [(200, False), (4096 + 77, False), (96 * 64, True)])
def test_second_order_planes_route_agrees_with_rows_route(B, ray_mode):
    """The second-order term through the C ABI on the same samples: mnrf_field_backward2_planes + mnrf_dw_planes2 (kind 1)
    against mnrf_field_backward2 (fp32 rows, bf16 x 3 GEMMs).  dL/dxyz bit-identical (the tangent pass is the same code); the
    nine weight gradients the term reaches to 6e-5 of each tensor's largest entry; every other gradient untouched.  g_normal
    spans eight orders of magnitude, so the per-sample scale 2^k_s and the launch scale 2^K2 both matter.  Then mixed: a
    first-order and a second-order evaluation in ONE mnrf_dw_planes2 launch = the sum of the two routes.
    (Why 6e-5 and not the 1e-5 of the first-order planes: at torch's default initialisation the signals b_1..b_3 are ~1e-4, and
    16 b then has a subnormal low f16 half.  Against float64 both routes sit at 2e-5..5e-5 there, scripts/check_so_routes.py;
    on trained weights the median |b| is 0.05..0.6, scripts/probe_b_magnitudes.py, and the halves are normal.)"""
    import ctypes
    import mirror_nerf_amd as M
    from mirror_nerf_amd import _lib
    from mirror_nerf_amd.weights import PARAM_NAMES, PARAM_SHAPES, packed_of
    L, p = _lib.lib(), _lib.ptr
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=DEV)  # noqa: E731
    torch.manual_seed(B + 5)
    model = M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=True).to(DEV)
    with torch.no_grad():
        model.sigma.weight.mul_(20.0)
    packed = packed_of(model)
    if ray_mode:
        spr, n_rays = 64, B // 64
        rays = torch.cat([torch.rand(n_rays, 3, device=DEV) - 0.5, torch.nn.functional.normalize(torch.randn(n_rays, 3, device=DEV), dim=1),
                          torch.full((n_rays, 1), 0.5, device=DEV), torch.full((n_rays, 1), 4.0, device=DEV)], 1).contiguous()
        z = (torch.rand(n_rays, spr, device=DEV).sort(1).values * 3.5 + 0.5).contiguous()
        xyz, xs = None, 3
        de = M.Embedding(4)(rays[:, 3:6]).contiguous()
    else:
        spr, rays, z, xs = 1, None, None, 3
        xyz = (torch.rand(B, 3, device=DEV) * 6 - 3).contiguous()
        de = M.Embedding(4)(torch.nn.functional.normalize(torch.randn(B, 3, device=DEV), dim=1))
    o = (f(B), f(B, 3), f(B, 3), f(B), f(B, 3))
    sx = torch.zeros(L.mnrf_train_planes_bytes(B), dtype=torch.uint8, device=DEV)
    sm = torch.zeros(L.mnrf_train_mask_words(B), dtype=torch.int64, device=DEV)
    si, sj = f(B), f(B)
    _lib.check(L.mnrf_field_forward_train(p(packed), B, p(xyz), xs, p(rays), p(z), spr, p(de), 27, *[p(t) for t in o], p(sx), p(sm),
                                          p(si), p(sj), _lib.MNRF_SPLIT_F16 | _lib.MNRF_TRAIN_PLANES, _lib.stream()), "forward")
    normal = o[4]
    scale = 10.0 ** (torch.rand(B, device=DEV) * 8 - 8)
    g_n = (torch.randn(B, 3, device=DEV) * scale[:, None]).contiguous()
    g_n[::17] = 0.0                                   # samples without a gradient (zero J^: k_s = 0, zero tangents)
    arr = lambda ts: (ctypes.c_void_p * 32)(*[t.data_ptr() for t in ts])  # noqa: E731
    # rows
    d_r = [torch.zeros(*PARAM_SHAPES[n], device=DEV) for n in PARAM_NAMES]
    dx_r = torch.zeros(B, 3, device=DEV)
    ws2 = f(L.mnrf_train_workspace2_floats(B))
    _lib.check(L.mnrf_field_backward2(p(packed), B, p(xyz), xs, p(rays), p(z), spr, p(g_n), p(normal), p(sj), p(sm), p(ws2),
                                      arr(d_r), p(dx_r), _lib.MNRF_SPLIT_F16, _lib.stream()), "backward2 rows")
    # planes
    x2 = torch.zeros(L.mnrf_train_planes2_bytes(B), dtype=torch.uint8, device=DEV)
    y2 = torch.zeros(L.mnrf_train_dy_planes2_bytes(B), dtype=torch.uint8, device=DEV)
    jmax = torch.zeros(1, dtype=torch.int32, device=DEV)
    dx_p = torch.zeros(B, 3, device=DEV)
    _lib.check(L.mnrf_field_backward2_planes(p(packed), B, p(xyz), xs, p(rays), p(z), spr, p(g_n), p(normal), p(sj), p(sm),
                                             p(x2), p(y2), p(jmax), p(dx_p), _lib.stream()), "backward2 planes")
    assert torch.equal(dx_r, dx_p)
    d_p = [torch.full(PARAM_SHAPES[n], 7.0, device=DEV) for n in PARAM_NAMES]      # overwritten (accumulate = 0)
    bs = (ctypes.c_int64 * 1)(B)
    kd = (ctypes.c_int * 1)(1)
    wsp = f(L.mnrf_dw_planes2_workspace_floats(1, bs, kd))
    _lib.check(L.mnrf_dw_planes2(1, (ctypes.c_void_p * 1)(x2.data_ptr()), (ctypes.c_void_p * 1)(y2.data_ptr()), bs,
                                 (ctypes.c_void_p * 1)(jmax.data_ptr()), kd, p(wsp), arr(d_p), 0, _lib.stream()), "dw planes2")
    torch.cuda.synchronize()
    reached = 0
    for n, a, b in zip(PARAM_NAMES, d_p, d_r):
        if float(b.abs().max()) == 0.0:
            assert float(a.abs().max()) == 0.0, n      # heads, biases: the term does not reach them
        else:
            reached += 1
            assert _rel(a, b) <= 6e-5, (n, _rel(a, b))
    assert reached == 9
    # mixed launch: first-order planes of the same samples + the second-order planes
    g_sigma = torch.randn(B, device=DEV)
    g_rgb, g_pn, g_m = torch.randn(B, 3, device=DEV), torch.randn(B, 3, device=DEV), torch.randn(B, device=DEV)
    dy = torch.zeros(L.mnrf_train_dy_planes_bytes(B), dtype=torch.uint8, device=DEV)
    seedmax = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(L.mnrf_field_backward_planes(p(packed), B, p(xyz), xs, p(rays), p(z), spr, p(g_sigma), p(g_rgb), p(g_pn), p(g_m),
                                            p(o[1]), p(o[2]), p(o[3]), p(sm), p(si), p(dy), p(seedmax), None, None, None, 0,
                                            _lib.stream()), "backward planes")
    d_1 = [f(*PARAM_SHAPES[n]) for n in PARAM_NAMES]
    bs1 = (ctypes.c_int64 * 1)(B)
    ws1 = f(L.mnrf_dw_planes_workspace_floats(1, bs1))
    _lib.check(L.mnrf_dw_planes(1, (ctypes.c_void_p * 1)(sx.data_ptr()), (ctypes.c_void_p * 1)(dy.data_ptr()), bs1,
                                (ctypes.c_void_p * 1)(seedmax.data_ptr()), p(ws1), arr(d_1), 0, _lib.stream()), "dw planes")
    d_m = [f(*PARAM_SHAPES[n]) for n in PARAM_NAMES]
    bs2 = (ctypes.c_int64 * 2)(B, B)
    kd2 = (ctypes.c_int * 2)(0, 1)
    wsm = f(L.mnrf_dw_planes2_workspace_floats(2, bs2, kd2))
    _lib.check(L.mnrf_dw_planes2(2, (ctypes.c_void_p * 2)(sx.data_ptr(), x2.data_ptr()), (ctypes.c_void_p * 2)(dy.data_ptr(), y2.data_ptr()),
                                 bs2, (ctypes.c_void_p * 2)(seedmax.data_ptr(), jmax.data_ptr()), kd2, p(wsm), arr(d_m), 0,
                                 _lib.stream()), "dw planes2 mixed")
    torch.cuda.synchronize()
    for n, a, b, c in zip(PARAM_NAMES, d_m, d_1, d_p):
        assert _rel(a, b + c) <= 1e-5, (n, _rel(a, b + c))      # (another plan deals the stages differently: another summation order)


def _two_evals(model, x1, x2, d):
    """Two evaluations of one module in one graph (the primary / reflected pattern of a training step)."""
    from mirror_nerf_amd.autograd import FieldFn
    from mirror_nerf_amd.weights import params_of
    o1 = FieldFn.apply(model, 1, x1, None, None, d[: x1.shape[0]], False, *params_of(model))
    o2 = FieldFn.apply(model, 1, x2, None, None, d[: x2.shape[0]], False, *params_of(model))
    return o1, o2


def test_folded_gradient_accumulation_with_other_consumers_of_the_parameters():
    """the evaluations of a module fold their weight gradients into one private set of tensors that is
    handed to autograd only when complete.  With ANOTHER consumer of the parameters in the graph (a weight regulariser)
    the sums must equal what autograd's own accumulation gives (fold off); an evaluation whose outputs never reach the
    loss must not lose gradients (end-of-pass callback); a backward pass that raises must not poison the next one."""
    import mirror_nerf_amd as M
    from mirror_nerf_amd import autograd as AG
    from mirror_nerf_amd.weights import params_of
    torch.manual_seed(11)
    model = M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=True).to(DEV)
    x1 = (torch.rand(300, 3, device=DEV) * 4 - 2).contiguous()
    x2 = (torch.rand(200, 3, device=DEV) * 4 - 2).contiguous()
    d = M.Embedding(4)(torch.nn.functional.normalize(torch.randn(300, 3, device=DEV), dim=1))

    def loss_fn(use_second=True, reg=True):
        o1, o2 = _two_evals(model, x1, x2, d)
        loss = o1[0].sum() + (o1[1] ** 2).sum()
        if use_second:
            loss = loss + 0.5 * o2[0].sum() + o2[3].sum()
        if reg:
            loss = loss + 1e-2 * sum((q ** 2).sum() for q in params_of(model))
        return loss

    def grads(fold, **kw):
        old = AG.FOLD_GRADS
        AG.FOLD_GRADS = fold
        try:
            for q in model.parameters():
                q.grad = None
            loss_fn(**kw).backward()
            return [q.grad.clone() for q in params_of(model)]
        finally:
            AG.FOLD_GRADS = old

    for kw in (dict(use_second=True, reg=True), dict(use_second=False, reg=True), dict(use_second=True, reg=False)):
        want, got = grads(False, **kw), grads(True, **kw)
        for a, b in zip(got, want):
            assert _rel(a, b) <= 2e-6, kw
        assert model.__dict__.get("_mnrf_pending") is None and model.__dict__.get("_mnrf_uses", 0) == 0

    # a backward pass that dies between two evaluations leaves state behind; the next forward clears it
    o1, o2 = _two_evals(model, x1, x2, d)
    model.__dict__["_mnrf_pending"] = ([torch.zeros_like(q) for q in params_of(model)], [])     # as after an exception
    want, got = grads(False), grads(True)
    for a, b in zip(got, want):
        assert _rel(a, b) <= 2e-6
    # gradient accumulation over two backward passes without zero_grad (p.grad += ...)
    for q in model.parameters():
        q.grad = None
    loss_fn().backward()
    loss_fn().backward()
    for q, b in zip(params_of(model), want):
        assert _rel(q.grad, 2 * b) <= 2e-6


def test_adam_kernel_against_torch_fused_adam():
    """mnrf_adam_step on one flat tensor against torch.optim.Adam(fused=True): gradients over 30 orders of magnitude (and exact
    zeros), five steps, weight decay on; then a step with found_inf set changes nothing and does not count."""
    from mirror_nerf_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    torch.manual_seed(0)
    n = 595_333                                  # not a multiple of four: the ragged tail
    p0 = torch.randn(n, device=DEV) * 0.1
    a = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([a], lr=5e-4, weight_decay=1e-3, fused=True)
    b = torch.empty(n + 4, device=DEV)[:n]       # (16-byte aligned base, as the flat parameter tensors are)
    b.copy_(p0)
    m, v = torch.zeros_like(b), torch.zeros_like(b)
    skipped = torch.zeros(1, dtype=torch.int32, device=DEV)
    for step in range(1, 6):
        g = torch.randn(n, device=DEV) * 10.0 ** (torch.rand(n, device=DEV) * 30 - 28)
        g[::7] = 0.0
        a.grad = g.clone()
        opt.step()
        _lib.check(L.mnrf_adam_step(p(b), p(g), p(m), p(v), n, 5e-4, 0.9, 0.999, 1e-8, 1e-3, step, p(skipped), None, None,
                                    _lib.stream()), "mnrf_adam_step")
        assert float((a.detach() - b).abs().max()) <= 2e-7, step        # (one ulp of 0.4 per step at most)
    before = (b.clone(), m.clone(), v.clone())
    found = torch.ones((), device=DEV)
    _lib.check(L.mnrf_adam_step(p(b), p(g), p(m), p(v), n, 5e-4, 0.9, 0.999, 1e-8, 1e-3, 6, p(skipped), None, p(found), _lib.stream()), "skip")
    assert torch.equal(b, before[0]) and torch.equal(m, before[1]) and torch.equal(v, before[2]) and int(skipped.item()) == 1
    # the next real call is the SIXTH step of torch's optimizer although it is the seventh call here
    a.grad = g.clone()
    opt.step()
    _lib.check(L.mnrf_adam_step(p(b), p(g), p(m), p(v), n, 5e-4, 0.9, 0.999, 1e-8, 1e-3, 7, p(skipped), None,
                                p(torch.zeros((), device=DEV)), _lib.stream()), "after skip")
    assert float((a.detach() - b).abs().max()) <= 2e-7


def test_flat_adam_state_dict_round_trip():
    """FlatAdam (mnrf_adam_step) interrupted after two steps -- state_dict() into a NEW FlatAdam over the same modules -- takes
    the same third step as an uninterrupted run: moments, step count and skip count travel (checkpoint / resume)."""
    from mirror_nerf_amd import training
    import mirror_nerf_amd as M
    from mirror_nerf_amd import synthetic as SY
    rays_all = SY.device_rays(32, 32, DEV)

    def run(interrupt):
        torch.manual_seed(0)
        system = M.NeRFSystem(training.default_hparams(perturb=0.0, noise_std=0.0)).to(DEV)
        with torch.no_grad():
            for m in system.models.values():
                m.sigma.weight.mul_(20.0)
                m.sigma.bias.fill_(1.0)
        opt = training.FlatAdam(list(system.models.values()), lr=5e-4, kernel=True)
        g = torch.Generator(device=DEV)
        g.manual_seed(7)
        for it in range(3):
            if interrupt and it == 2:
                sd = opt.state_dict()
                opt = training.FlatAdam(list(system.models.values()), lr=1e-3, kernel=True)      # (another lr: the saved groups win)
                opt.load_state_dict(sd)
            idx = torch.randint(0, rays_all.shape[0], (256,), device=DEV, generator=g)
            target = torch.rand(256, 3, device=DEV, generator=g)
            gt = (torch.rand(256, device=DEV, generator=g) < 0.25).float()
            training.train_step(system, opt, rays_all[idx].contiguous(), target, gt)
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in system.named_parameters()}
    a, b = run(False), run(True)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("kernel", [False, True])
def test_flat_adam_takes_the_same_steps_as_torch_adam(kernel):
    """training.FlatAdam (one flat parameter tensor per model, its .grad = the backward pass's flat gradient buffer) against
    torch.optim.Adam(fused=True) over the 64 tensors: three training steps from the same initial weights on the same batches.
    kernel=False (torch's fused kernel over the flat tensors): the same parameters (same arithmetic; the weight-gradient sums are
    order-dependent in the last bits).  kernel=True (mnrf_adam_step, the default): the update agrees to one ulp per step (test
    above) -- and these three steps amplify one ulp enormously: with torch's OWN Adam on both sides, initial weights that differ
    by one ulp end 8e-4 apart in the worst entry and 1.7e-4 on average in the worst tensor (scripts/check_adam_sensitivity.py:
    an ulp moves a sample across a bin of the fine pass or a ray across the mirror threshold, and Adam's normalised step passes
    the change of a near-zero gradient on at full size, lr = 5e-4).  The kernel stays inside that: measured 5.6e-4 / 7e-5.
    """
    from mirror_nerf_amd import training
    import mirror_nerf_amd as M
    from mirror_nerf_amd import synthetic as SY
    rays_all = SY.device_rays(32, 32, DEV)

    def run(flat):
        torch.manual_seed(0)
        system = M.NeRFSystem(training.default_hparams(perturb=0.0, noise_std=0.0)).to(DEV)
        with torch.no_grad():
            for m in system.models.values():
                m.sigma.weight.mul_(20.0)
                m.sigma.bias.fill_(1.0)
        opt = training.FlatAdam(list(system.models.values()), lr=5e-4, kernel=kernel) if flat else \
            torch.optim.Adam(list(system.parameters()), lr=5e-4, fused=True)
        g = torch.Generator(device=DEV)
        g.manual_seed(7)
        losses = []
        for _ in range(3):
            idx = torch.randint(0, rays_all.shape[0], (256,), device=DEV, generator=g)
            target = torch.rand(256, 3, device=DEV, generator=g)
            gt = (torch.rand(256, device=DEV, generator=g) < 0.25).float()
            losses.append(float(training.train_step(system, opt, rays_all[idx].contiguous(), target, gt)))
        torch.cuda.synchronize()
        return losses, {k: v.detach().clone() for k, v in system.named_parameters()}, system
    la, pa, sa = run(True)
    lb, pb, _ = run(False)
    assert all(abs(a - b) <= 1e-5 * abs(b) for a, b in zip(la, lb)), (la, lb)
    assert la[2] != la[0]                                           # the weights moved (the packed images were refreshed)
    for k in pb:
        if kernel:
            assert float((pa[k] - pb[k]).abs().max()) <= 3 * 5e-4 and float((pa[k] - pb[k]).abs().mean()) <= 2e-4, k
        else:
            assert float((pa[k] - pb[k]).abs().max()) <= 2e-5 * float(pb[k].abs().max()) + 1e-7, k
    # the parameters still are what state_dict / checkpoints see, and are views of the flat tensors
    sd = sa.nerf_fine.state_dict()
    assert torch.equal(sd["sigma.weight"], sa.nerf_fine.sigma.weight.detach())


def test_gradient_spike_is_the_reference_s():
    """Fixture G18 (tests/golden/make_golden_spike.py): on the committed trained pair, the batch of the analytic
    scene with the largest TotalLoss gradient of a 400-batch scan (profiles/r06_spike_scan.json) against a median batch, through the
    REFERENCE's NeRFSystem.forward + TotalLoss + backward in float32 and float64 (train.py:102-348, 439-446, losses.py:54-78).
    The HIP step must show the reference's numbers: per-model gradient norms of both batches within the reference's own float32-vs-
    float64 distance (the median batch's fine-model gradient is noise-dominated in the reference itself: its float32 norm is 37 % off
    its float64 norm), the loss to 2e-4, and the spike -- fine-model gradient >= 2.5 x the median batch's -- where the reference has it."""
    import sys
    from types import SimpleNamespace
    import mirror_nerf_amd as M
    from mirror_nerf_amd import training as T
    from mirror_nerf_amd.weights import params_of
    from tests.golden import fixtures as FX
    sys.path.insert(0, FX.HERE)
    import make_golden_trained as SC
    fx = FX.Fixture("g18_grad_spike")
    m = fx.meta
    hp = T.default_hparams(**{k: v for k, v in m["hp"].items()})
    system = M.NeRFSystem(hp)
    z = np.load(f"{FX.HERE}/{m['weights_file']}")
    for name, mod in (("coarse", system.nerf_coarse), ("fine", system.nerf_fine)):
        mod.load_state_dict({k[len(name) + 2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(name + "__")})
    system.to(DEV)
    rays, rgbs, masks = SC.scene_views(*m["views"])
    loss_fn = T.total_loss_fn(SimpleNamespace(model_type="nerf"), epoch=m["epoch"])
    got = {}
    for which in ("spike", "median"):
        idx = np.random.RandomState(m[f"{which}_batch"]).randint(rays.shape[0], size=1024)
        r, c, k = (torch.from_numpy(a[idx].copy()).to(DEV) for a in (rays, rgbs, masks))
        system.zero_grad(set_to_none=True)
        res = system(r, T.extra_info(system.hparams, k, m["epoch"]))
        loss = loss_fn(res, c, k, r)
        loss.backward()
        want32, want64 = m[f"{which}_f32"], m[f"{which}_f64"]
        assert abs(float(loss) - want32["loss"]) <= 2e-4 * max(1.0, abs(want32["loss"])) + abs(want32["loss"] - want64["loss"]), (which, float(loss), want32["loss"])
        for mn, mod in (("coarse", system.nerf_coarse), ("fine", system.nerf_fine)):
            g = torch.cat([q.grad.reshape(-1) for q in params_of(mod)]).double()
            norm = float(g.norm())
            own = abs(want32[f"{mn}_norm"] - want64[f"{mn}_norm"]) / want64[f"{mn}_norm"]
            err = abs(norm - want32[f"{mn}_norm"]) / want64[f"{mn}_norm"]
            print(f"  {which:6s} {mn:6s} |g| HIP {norm:.4e}  reference f32 {want32[f'{mn}_norm']:.4e}  f64 {want64[f'{mn}_norm']:.4e}  (own distance {own:.1e})")
            assert err <= max(2e-2, 1.5 * own), (which, mn, norm, want32[f"{mn}_norm"], want64[f"{mn}_norm"])
            got[(which, mn)] = norm
    ratio = got[("spike", "fine")] / got[("median", "fine")]
    lo, hi = sorted((m["ratio_fine_f32"], m["ratio_fine_f64"]))
    print(f"  fine-model gradient, spike / median batch: HIP {ratio:.2f}, reference f32 {m['ratio_fine_f32']:.2f}, f64 {m['ratio_fine_f64']:.2f}")
    assert lo >= 2.5 and ratio >= 2.5 and 0.8 * lo <= ratio <= 1.2 * hi, (ratio, lo, hi)
