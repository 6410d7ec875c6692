"""tests/loss_ref.py (TotalLoss in float64 torch ops, gradients by autograd) held to what is known without a GPU:

  * the six G10 fixtures captured from the reference's losses.TotalLoss: same term keys, every term, the sum and every grad__*
    array, at the bars of tests/test_loss.py (2e-6 relative on scalars with floor 1.0; 1e-6 of each gradient tensor's largest entry).
    Measured: worst value error 4.3e-8, worst gradient error 1.6e-7 of the largest entry (the fixtures are float32 results).
  * on the multi-block inputs of tests/test_hip_loss_fp64.py (loss_ref.CASES): the float32 numpy oracle's terms against the float64
    reference.  Measured: worst term is the plane term at 1.7e-7 relative, the worst total 1.6e-7.
  * the float32 floor: the same restatement run in float32 against float64 differs by at most 1.8e-7 of any gradient tensor's
    largest entry over all cases (x_surface_fine at 256 rays; the predicted masks' rows past the planted edges, held on their own:
    8.7e-8) and by 1.3e-7 on a value.  The bars therefore leave 15x (values) and 5x (gradients) over what float32 arithmetic itself
    costs, and no tensor needs a bar of its own: test_float32_floor_stays_under_a_quarter_of_the_bars asserts that every floor stays
    below a quarter of its bar, so a case added later that does not must be given 4x its measured floor here, by name, with the
    reason.
  * the PSNR / MSE reduction: a float32 numpy emulation of the two kernels' order of summation (loss_ref.mse_emulate) against the
    float64 mean on the cases of tests/test_hip_psnr_fp64.py, inside the bar derived from that order (loss_ref.mse_bar).
"""
import json

import numpy as np
import pytest
import torch

from oracle import mirror_nerf_oracle as O
from tests import loss_ref as R
from tests.golden import fixtures as FX

G10 = FX.names("g10_loss_")


def _load(name):
    z = np.load(f"{FX.HERE}/{name}.npz")
    meta = json.loads(str(z["meta"]))
    pick = lambda prefix: {k[len(prefix):]: z[k] for k in z.files if k.startswith(prefix)}  # noqa: E731
    return meta, pick("in__"), pick("batch__"), pick("plane__"), pick("out__")


@pytest.mark.parametrize("name", G10)
def test_reference_matches_the_captured_total_loss(name):
    meta, inputs, batch, plane, outs = _load(name)
    hp = dict(O.LOSS_DEFAULTS, **meta["hp"])
    got = R.evaluate(inputs, batch, hp, meta["stage"], meta["epoch"], plane)
    want = {k[6:]: v for k, v in outs.items() if k.startswith("loss__")}
    assert set(got["terms"]) == set(want)
    for k in want:
        e = R.value_error(got["terms"][k], want[k])
        print(f"{name} {k}: {e:.2e}")
        assert e <= R.VALUE_BAR, (k, float(got["terms"][k]), float(want[k]))
    assert R.value_error(got["total"], outs["loss_sum"]) <= R.VALUE_BAR
    grads = {k[6:]: v for k, v in outs.items() if k.startswith("grad__")}
    assert set(grads) == set(inputs)
    for k, w in grads.items():
        err, scale = R.grad_error(got["grads"][k], w)
        print(f"{name} grad {k}: {err / max(scale, 1e-300):.2e} of the largest entry")
        assert err <= R.GRAD_BAR * scale, (k, err, scale)


def test_fixture_count():
    assert len(G10) == 6, G10


def test_base_inputs_reach_every_second_block():
    """The shape the GPU tests lean on: ten ray blocks with a tail of 196, three passes of the 1024-thread count loop whose last
    wave holds 4 rays, two plane blocks with a tail, and sample counts that divide neither 64 nor 256."""
    c = R.case("default")
    n = c["batch"]["rgbs"].shape[0]
    assert n == 2500 and (n + 255) // 256 == 10 and n - 9 * 256 == 196
    assert 2048 < n <= 3072 and (n - 2048) % 64 == 4
    m = int((c["batch"]["mirror_mask"] != 0).sum())
    assert 256 < m // 4 < 512 and (m // 4) % 256 != 0, m
    assert all(64 % s and 256 % s for s in (R.S_COARSE, R.S_FINE))
    assert c["batch"]["rays"].shape[1] == 11
    assert c["picks"]["fine"].shape == (m // 4, 4) and 0 in c["picks"]["fine"] and c["picks"]["fine"].max() <= m - 1
    for t in R.TYPS:
        assert np.array_equal(c["inputs"][f"mirror_mask_{t}"][:6], R.MASK_EDGES)


@pytest.mark.parametrize("name", list(R.CASES))
def test_oracle_terms_against_the_float64_reference(name):
    c = R.case(name)
    with np.errstate(all="ignore"):
        total, d = O.total_loss({k: v.copy() for k, v in c["inputs"].items()}, c["batch"], c["hp"], c["stage"], c["epoch"], c["picks"])
    ref = c["ref"]
    assert set(d) == set(ref["terms"])
    for k in d:
        e = R.value_error(d[k], ref["terms"][k])
        print(f"{name} {k}: {e:.2e}")
        assert e <= R.VALUE_BAR, (k, float(d[k]), float(ref["terms"][k]))
    assert R.value_error(total, ref["total"]) <= R.VALUE_BAR
    nan = {k for k, v in ref["terms"].items() if np.isnan(v)}
    assert nan == R.EMPTY_NAN_TERMS.get(name, set()), nan
    assert np.isnan(ref["total"]) == bool(nan)


@pytest.mark.parametrize("name", list(R.CASES))
def test_float32_floor_stays_under_a_quarter_of_the_bars(name):
    c = R.case(name)
    ref = c["ref"]
    f32 = R.evaluate(c["inputs"], c["batch"], c["hp"], c["stage"], c["epoch"], c["picks"], dtype=torch.float32)
    for k, v in ref["terms"].items():
        e = R.value_error(f32["terms"][k], v)
        print(f"{name} {k}: {e:.2e}")
        assert e <= R.VALUE_BAR / 4, (k, e)
    assert R.value_error(f32["total"], ref["total"]) <= R.VALUE_BAR / 4
    for key, ref_g in ref["grads"].items():
        for k, g, w in R.grad_parts(key, f32["grads"][key], ref_g):
            err, scale = R.grad_error(g, w)
            print(f"{name} grad {k}: {err / max(scale, 1e-300):.2e} of the largest entry")
            assert err <= R.GRAD_BAR / 4 * scale, (k, err, scale)


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_gradients_are_finite_and_agree_with_a_finite_difference(name):
    """The autograd gradients of the reference along one random direction of all inputs at once, against a central difference of
    the reference's own value (float64, step 1e-6; relu / abs / clamp kinks are a measure-zero set away from the seeded inputs,
    except the planted mask edges, which the direction leaves alone)."""
    c = R.case(name)
    ref = c["ref"]
    for k, g in ref["grads"].items():
        assert np.isfinite(g).all(), k
    if np.isnan(ref["total"]) or c["stage"] and (c["batch"]["mirror_mask"] < 0).any():
        return      # the value is NaN, or piecewise constant in the thresholded prediction: nothing to difference
    rs = np.random.RandomState(7)
    d = {k: rs.normal(size=v.shape) for k, v in c["inputs"].items()}
    for t in R.TYPS:
        if f"mirror_mask_{t}" in d:
            d[f"mirror_mask_{t}"][:6] = 0.0
    eps = 1e-6
    at = lambda s: float(R.evaluate({k: v.astype(np.float64) + s * d[k] for k, v in c["inputs"].items()}, c["batch"], c["hp"],  # noqa: E731
                                    c["stage"], c["epoch"], c["picks"])["total"])
    fd = (at(eps) - at(-eps)) / (2 * eps)
    an = sum(float((ref["grads"][k] * d[k]).sum()) for k in d)
    assert abs(fd - an) <= 1e-6 * max(abs(an), 1.0), (fd, an)


def test_empty_selections_are_nan_with_zero_gradient():
    for name, nan in R.EMPTY_NAN_TERMS.items():
        ref = R.case(name)["ref"]
        assert {k for k, v in ref["terms"].items() if np.isnan(v)} == nan, name
        assert all(np.isfinite(g).all() for g in ref["grads"].values()), name
    g = R.case("empty_valid_mask")["ref"]["grads"]
    for k in ("pred_normal_coarse", "pred_normal_fine", "weights_coarse", "weights_fine", "normal_fine"):
        assert not g[k].any(), k
    g = R.case("empty_stage_pred_high")["ref"]["grads"]
    assert not g["rgb_coarse"].any() and not g["rgb_fine"].any()


# ------------------------------------------------------------------------------------------------------------------ PSNR and MSE
def test_psnr_bar_counts_the_roundings_of_the_kernel():
    """The geometry the bar is built from, and the reach of the cases: below one wave, one block and one pass; two, four and 65
    passes; masks whose selection starts in a later pass."""
    assert R.mse_geometry(1) == (1, 1) and R.mse_geometry(256) == (1, 1) and R.mse_geometry(257) == (2, 1)
    assert R.mse_geometry(R.MSE_SWEEP) == (1024, 1) and R.mse_geometry(R.MSE_SWEEP + 1) == (1024, 2)
    assert R.mse_geometry(3 * R.MSE_SWEEP + 5) == (1024, 4) and R.mse_geometry(2 ** 24 + 257) == (1024, 65)
    assert R.mse_bar(1) == 13 * 2.0 ** -24 and R.mse_bar(R.MSE_SWEEP + 1) == (3 + 1 + 9 + 1023 + 1) * 2.0 ** -24
    assert float(np.float32(2 ** 24 + 257)) != 2 ** 24 + 257      # the count of the largest case is not a float32
    late = R.psnr_case("mask_late_passes")
    first = int(np.nonzero(late["sel"])[0][0])
    assert R.MSE_SWEEP <= first and int(np.nonzero(late["sel"])[0][-1]) < 3 * R.MSE_SWEEP and late["ref"][2] > 100000
    last = R.psnr_case("mask_last_only")
    assert last["ref"][2] == 1 and last["sel"][-1] and last["sel"].size > 3 * R.MSE_SWEEP
    for name, per in (("mask_pixel3", 3), ("mask_pixel4", 4), ("mask_pixel5", 5)):
        c = R.psnr_case(name)
        assert c["per"] == per and c["a"].size % per == 0 and c["mask"].size == c["a"].size // per and 0 < c["ref"][2] < c["a"].size
    assert R.MSE_TPB % 3 and R.MSE_TPB % 5      # a pixel of 3 or 5 channels straddles block edges
    one = R.psnr_case("one_element_2^-20")
    assert one["ref"][0] == 2.0 ** -40 / 1000 and float(np.float32(one["ref"][0])) > 0


@pytest.mark.parametrize("name", list(R.PSNR_CASES))
def test_float32_emulation_of_the_mse_kernels_stays_inside_the_derived_bar(name):
    """The kernels' order of summation in float32 numpy against the float64 mean: the derived bar is attainable by the
    arithmetic it was derived for, without reference to the kernel.  Largest fractions of the bar over the cases: MSE 0.151
    (size_255), PSNR 0.323 (size_1, numpy's log10), count 0.001 (2^24 + 257: the float32 count; exact in every other case)."""
    c = R.psnr_case(name)
    partials, out = R.mse_emulate(c["a"], c["b"], c["sel"])
    blocks, _ = R.mse_geometry(c["a"].size)
    assert partials.shape == (blocks, 2) and out.dtype == np.float32
    fm, fp, fc = R.psnr_errors(c, out)
    print(f"{name}: n = {c['a'].size}, mse {float(out[0]):.6e} (fp64 {c['ref'][0]:.6e}), errors as fractions of the bar: "
          f"mse {fm:.3f}, psnr {fp:.3f}, count {fc:.3f}")
    assert fm <= 1 and fp <= 1 and fc <= 1
    if c["a"].size < 2 ** 24:
        assert float(out[2]) == c["ref"][2]
    if name == "mask_all_true":      # an all-true mask selects what no mask selects: the same bits
        _, plain = R.mse_emulate(c["a"], c["b"], np.ones(c["a"].size, bool))
        assert plain.tobytes() == out.tobytes()
    if name == "identical":
        assert float(out[0]) == 0.0 and float(out[1]) == np.inf
    if name == "mask_none_selected":
        assert np.isnan(out[0]) and np.isnan(out[1]) and float(out[2]) == 0.0


@pytest.mark.parametrize("name", ["stage_invalid_ep0", "stage_invalid_ep2"])
def test_threshold_in_place_keeps_the_gradient_path(name):
    c = R.case(name)
    ref = c["ref"]
    m0 = c["inputs"]["mirror_mask_fine"]
    after = ref["inputs"]["mirror_mask_fine"]
    assert set(np.unique(after)) == {0.0, 0.5, 1.0}
    assert np.array_equal(after, np.where(m0 > 0.5, 1.0, np.where(m0 < 0.5, 0.0, m0)))
    assert np.array_equal(ref["inputs"]["mirror_mask_coarse"], c["inputs"]["mirror_mask_coarse"].astype(np.float64))
    sel = after == 0
    for t in R.TYPS:
        assert not ref["grads"][f"rgb_{t}"][~sel].any() and ref["grads"][f"rgb_{t}"][sel].any()
    gm = ref["grads"]["mirror_mask_fine"]
    gt = c["batch"]["mirror_mask"].reshape(-1)
    if name.endswith("ep2"):
        # thresholded values sit outside the clamp interval (no gradient); 0.5 stays inside; gt < 0 rows give nothing
        assert gm[2] != 0.0 or gt[2] < 0
        assert not gm[after != 0.5].any()
        assert not ref["grads"]["mirror_mask_coarse"][gt < 0].any() and ref["grads"]["mirror_mask_coarse"][gt >= 0].any()
        assert ref["terms"]["plane_consistent_loss"] == 0.0
    else:
        assert not gm.any() and "mirror_mask_loss" not in ref["terms"]
