"""csrc/mnrf_loss.hip against tests/loss_ref.py (TotalLoss in float64 torch ops, gradients by autograd) past one block of every
kernel: 2500 rays with 5 and 7 samples -- ten ray blocks with a tail of 196, three passes of the count kernel's 1024-thread loop with
a last wave of 4 rays, ray = j / S across block boundaries with S dividing neither 64 nor 256, and (M ~ 1285 mirror rays) two
plane blocks with a tail -- through mirror_nerf_amd.get_loss on non-leaf float32 inputs, for every flag and optional input of the
file, the partly invalid GT mask, the mask loss over invalid targets, and the four empty selections.

Bars (tests/test_loss.py's): 2e-6 relative on the terms and the sum (floor 1.0), 1e-6 of each gradient tensor's largest entry, for
every input: rgb, mirror_mask, normal_dif, pred_normal, weights, x_surface of both typs and normal_fine; the predicted masks' rows
past the six planted edge values are held to the same bar of THEIR largest entry as well, since an edge row's gradient is up to 1e7
times an ordinary row's (loss_ref.grad_parts).  An entry the reference leaves exactly zero must be exactly zero.  The float32 floor measured on the CPU (tests/test_loss_ref_cpu.py: the same
restatement in float32 against float64) is at most 1.8e-7 of a gradient tensor's largest entry and 1.3e-7 on a value over these
very cases, under a quarter of either bar, so no tensor has a bar of its own.
"""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests import loss_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROUTES = ("host", "device")


def _run(c, route="host", plane=True, backward="plain"):
    """One TotalLoss call on the case's inputs -> (sum, terms, gradients, predictions after the call), as numpy / Python floats
    holding the kernel's float32 bits."""
    import mirror_nerf_amd as M
    from mirror_nerf_amd import losses
    leaves = {k: torch.from_numpy(v.copy()).to(DEV).requires_grad_(True) for k, v in c["inputs"].items()}
    res = {k: v * 1.0 for k, v in leaves.items()}        # non-leaf, as render_rays returns them
    tb = {k: torch.from_numpy(np.asarray(v).copy()).to(DEV) for k, v in c["batch"].items()}
    if plane:
        tb["_plane_u"] = torch.from_numpy(c["u"].copy()).to(DEV)
    if route == "device":
        tb["_plane_on_device"] = True
    crit = M.get_loss(types.SimpleNamespace(**c["hp"]))
    loss_sum, loss_dict = crit(res, tb, train_geometry_stage=c["stage"], epoch=c["epoch"])
    terms = {k: v.cpu().numpy()[()] for k, v in loss_dict.items()}
    total = loss_sum.detach().cpu().numpy()[()]
    if backward == "plain":
        loss_sum.backward()
    elif backward == "unit":
        loss_sum.backward(gradient=losses.unit_gradient(DEV))
    elif backward == "x1024":
        loss_sum.backward(gradient=torch.tensor(1024.0, device=DEV))
    grads = {k: v.grad.cpu().numpy() for k, v in leaves.items()} if backward else {}
    return total, terms, grads, {k: v.detach().cpu().numpy() for k, v in res.items()}, loss_sum


def _hold(name, got, ref):
    """Terms, sum and every gradient of one call against the reference of the case, figures printed before they are asserted."""
    total, terms, grads = got[:3]
    assert set(terms) == set(ref["terms"]), (set(terms), set(ref["terms"]))
    for k, w in ref["terms"].items():
        e = R.value_error(terms[k], w)
        print(f"{name} {k}: got {float(terms[k])!r} want {float(w)!r} ({e:.2e})")
        assert e <= R.VALUE_BAR, (name, k, float(terms[k]), float(w))
    e = R.value_error(total, ref["total"])
    print(f"{name} sum: got {float(total)!r} want {float(ref['total'])!r} ({e:.2e})")
    assert e <= R.VALUE_BAR, (name, float(total), float(ref["total"]))
    assert set(grads) == set(ref["grads"])
    for key, ref_g in ref["grads"].items():
        for k, g, w in R.grad_parts(key, grads[key], ref_g):
            err, scale = R.grad_error(g, w)
            print(f"{name} grad {k}: {err:.3e} (largest entry {scale:.3e}, {err / max(scale, 1e-300):.2e} of it)")
            assert err <= R.GRAD_BAR * scale, f"{name}: grad {k} max-abs {err:.3e} (largest entry {scale:.3e})"
        zero = ref_g == 0
        assert not grads[key][zero].any(), f"{name}: grad {key} is not exactly zero where the reference's is"


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32) if np.asarray(a).dtype == np.float32 else np.asarray(a),
                          np.asarray(b).view(np.uint32) if np.asarray(b).dtype == np.float32 else np.asarray(b))


def _both_routes(name):
    c = R.case(name)
    got = {route: _run(c, route) for route in ROUTES}
    for route in ROUTES:
        _hold(f"{name}/{route}", got[route], c["ref"])
    # the same picks on both routes: every term and the sum bit for bit (tests/test_static_step.py holds this at 256 rays)
    for k in got["host"][1]:
        assert _same_bits(got["host"][1][k], got["device"][1][k]), (k, got["host"][1][k], got["device"][1][k])
    assert _same_bits(got["host"][0], got["device"][0])
    for k, g in got["host"][2].items():
        if not k.startswith("x_surface"):       # atomics
            assert _same_bits(g, got["device"][2][k]), k
    return c, got


def test_default_flags_with_the_plane_term_on_both_routes():
    c, got = _both_routes("default")
    assert float(got["host"][1]["plane_consistent_loss"]) > 0.0
    gt = c["batch"]["mirror_mask"].reshape(-1)
    for t in R.TYPS:      # only mirror rows can be picked
        assert not got["device"][2][f"x_surface_{t}"][gt == 0].any() and got["device"][2][f"x_surface_{t}"][gt != 0].any()
        assert np.array_equal(got["host"][3][f"mirror_mask_{t}"], c["inputs"][f"mirror_mask_{t}"])


def test_tcnn_bce_without_the_log_clamp():
    _both_routes("tcnn_bce")


@pytest.mark.parametrize("epoch", [0, 1, 2])
def test_stage_with_a_partly_invalid_gt_mask(epoch):
    """About 10 % of the GT entries are -1: the colour term follows the thresholded prediction, which is left holding 0 / 0.5 / 1
    (the other typ's is untouched); at epoch 2 the mask loss runs over the invalid targets and the plane term is present and 0."""
    name = f"stage_invalid_ep{epoch}"
    c, got = _both_routes(name)
    ref = c["ref"]
    want_keys = {0: {"color_loss"}, 1: {"color_loss", "normal_loss", "normal_reg_loss"},
                 2: {"color_loss", "mirror_mask_loss", "plane_consistent_loss", "normal_loss", "normal_reg_loss"}}[epoch]
    for route in ROUTES:
        total, terms, grads, after, _ = got[route]
        assert set(terms) == want_keys
        if epoch == 2:
            assert float(terms["plane_consistent_loss"]) == 0.0
            assert not grads["x_surface_fine"].any() and not grads["x_surface_coarse"].any()
        assert set(np.unique(after["mirror_mask_fine"])) == {0.0, 0.5, 1.0}
        assert np.array_equal(after["mirror_mask_fine"], ref["inputs"]["mirror_mask_fine"].astype(np.float32))
        assert np.array_equal(after["mirror_mask_coarse"], c["inputs"]["mirror_mask_coarse"])
        sel = after["mirror_mask_fine"] == 0
        for t in R.TYPS:
            assert not grads[f"rgb_{t}"][~sel].any() and grads[f"rgb_{t}"][sel].any()


def test_stage_with_a_valid_gt_black_target_inside_only_and_a_valid_mask():
    c, got = _both_routes("stage_black_inside_valid")
    gt = c["batch"]["mirror_mask"].reshape(-1)
    vm = c["batch"]["valid_mask"]
    g = got["host"][2]
    assert 0.75 < vm.mean() < 0.85
    assert not g["rgb_fine"][gt != 0].any() and not g["normal_dif_fine"][gt == 0].any()
    assert not g["weights_fine"][~vm].any() and not g["pred_normal_coarse"][~vm].any() and not g["normal_fine"][~vm].any()


def test_coarse_only_inputs_with_a_valid_mask():
    c, got = _both_routes("coarse_only")
    assert not any(k.endswith("_fine") for k in c["inputs"]) and set(got["host"][2]) == set(c["inputs"])


@pytest.mark.parametrize("name", ["empty_gt_zeros", "empty_gt_ones", "empty_valid_mask", "empty_stage_pred_high"])
def test_empty_selection(name):
    """A mean over nothing: NaN in exactly the terms where the reference has it, and in the sum; every gradient finite and the
    reference's, exactly zero wherever the reference's is."""
    c, got = _both_routes(name)
    for route in ROUTES:
        total, terms, grads = got[route][:3]
        assert {k for k, v in terms.items() if np.isnan(v)} == R.EMPTY_NAN_TERMS[name]
        assert np.isnan(total)
        for k, g in grads.items():
            assert np.isfinite(g).all(), (name, route, k)


@pytest.mark.parametrize("n", R.SWEEP_SIZES)
def test_size_sweep(n):
    """1, 3 (fewer than four mirror rays: the plane term is exactly 0 and x_surface gets nothing from it), 63 (a partial wave),
    256 (exactly one ray block), 1024 and 1025 (one pass of the count loop, and one ray into its second)."""
    name = f"size_{n}"
    c, got = _both_routes(name)
    m = int((c["batch"]["mirror_mask"] != 0).sum())
    for route in ROUTES:
        total, terms, grads = got[route][:3]
        assert {k for k, v in terms.items() if np.isnan(v)} == R.EMPTY_NAN_TERMS.get(name, set())
        if m < 4:
            assert float(terms["plane_consistent_loss"]) == 0.0
            assert not grads["x_surface_fine"].any() and not grads["x_surface_coarse"].any()
        else:
            assert float(terms["plane_consistent_loss"]) > 0.0


def test_incoming_gradient_scales_the_stored_gradients():
    c = R.case("default")
    plain = _run(c, "device")
    unit = _run(c, "device", backward="unit")
    big = _run(c, "device", backward="x1024")
    for k, g in plain[2].items():
        if k.startswith("x_surface"):       # atomics: the stored bits differ from call to call; _hold below covers these two
            continue
        assert _same_bits(unit[2][k], g), k
        assert _same_bits(big[2][k], (g * np.float32(1024.0)).astype(np.float32)), k
    assert _same_bits(unit[0], plain[0]) and _same_bits(big[0], plain[0])
    _hold("default/unit", unit, c["ref"])
    _hold("default/x1024", (big[0], big[1], {k: g / np.float32(1024.0) for k, g in big[2].items()}), c["ref"])


def test_a_second_backward_over_the_same_node_raises():
    c = R.case("size_63")
    import mirror_nerf_amd as M
    leaves = {k: torch.from_numpy(v.copy()).to(DEV).requires_grad_(True) for k, v in c["inputs"].items()}
    tb = {k: torch.from_numpy(np.asarray(v).copy()).to(DEV) for k, v in c["batch"].items()}
    loss_sum, _ = M.get_loss(types.SimpleNamespace(**c["hp"]))({k: v * 1.0 for k, v in leaves.items()}, tb, False, 5)
    loss_sum.backward(retain_graph=True)
    with pytest.raises(RuntimeError):
        loss_sum.backward()


def test_two_calls_give_the_same_bits():
    c = R.case("default")
    for route in ROUTES:
        a, b = _run(c, route), _run(c, route)
        assert len(a[1]) == 5
        assert _same_bits(a[0], b[0])
        for k in a[1]:
            assert _same_bits(a[1][k], b[1][k]), (route, k)
        for k in a[2]:
            if not k.startswith("x_surface"):       # the plane term scatters with atomics
                assert _same_bits(a[2][k], b[2][k]), (route, k)


def test_count_words_are_numpys_counts():
    """mnrf_loss_count on the partly invalid batch with a valid_mask: #gt < 0, #gt != 0, #valid, #thresholded prediction below 0.5."""
    from mirror_nerf_amd import _lib, losses
    inputs, batch = R.make_inputs(2500, seed=31, invalid_frac=0.1, valid_frac=0.8)
    gt = batch["mirror_mask"].reshape(-1)
    n = gt.shape[0]
    L = _lib.lib()
    t_gt = torch.from_numpy(gt.copy()).to(DEV)
    t_vm = torch.from_numpy(batch["valid_mask"]).to(DEV).to(torch.uint8).contiguous()
    t_mc = torch.from_numpy(inputs["mirror_mask_coarse"].copy()).to(DEV)
    t_mf = torch.from_numpy(inputs["mirror_mask_fine"].copy()).to(DEV)
    for fine in (True, False):
        a = losses._Args()
        a.gt_mask, a.valid_mask, a.n_rays = t_gt.data_ptr(), t_vm.data_ptr(), n
        a.mirror_mask[0] = t_mc.data_ptr()
        if fine:
            a.mirror_mask[1] = t_mf.data_ptr()
        ws = torch.full((L.mnrf_loss_workspace_floats(n, 1, 1, 0),), -7.0, dtype=torch.float32, device=DEV)
        _lib.check(L.mnrf_loss_count(ctypes.byref(a), _lib.ptr(ws), _lib.stream()), "mnrf_loss_count")
        got = [int(v) for v in ws[:4].tolist()]
        key = inputs["mirror_mask_fine" if fine else "mirror_mask_coarse"]
        want = [int((gt < 0).sum()), int((gt != 0).sum()), int(batch["valid_mask"].sum()), int((key < 0.5).sum())]
        assert got == want, (fine, got, want)
        assert want[0] > 0 and want[2] < n
        assert bool((ws[4:] == -7.0).all())       # without a row list to fill, nothing past the four count words is written
