"""TotalLoss (losses.py:7-255 of the reference, as restated in oracle/mirror_nerf_oracle.py) in float64 torch ops on the CPU, with
gradients by autograd: what tests/test_hip_loss_fp64.py holds csrc/mnrf_loss.hip to.  Plain indexing and `.mean()`; nothing fused.

Conventions that matter for the gradients:
  * a mean over an empty selection is NaN in value and gives zero gradient (torch's own `x[empty].mean()`);
  * the BCE clamp bounds are the float32 values as doubles, and clamp passes the gradient inside the CLOSED interval only;
  * the -100 clamp of the logs applies unless model_type == "nerf_tcnn";
  * in the train_geometry_stage branch with an invalid GT entry the thresholded prediction (fine if present, else coarse) is
    overwritten IN PLACE through .detach() with 0 / 0.5-stays / 1 while its autograd path stays on the original tensor: the mask
    loss afterwards reads the thresholded values, rows with value exactly 0 are the colour selection, the other typ is untouched;
  * a row with gt < 0 adds nothing to the mask loss, value or gradient; its mean still divides by all n rows;
  * plane picks are handed in as (times, 4) index arrays per typ, "fine" first (plane_picks() restates the kernel's picks from
    injected uniform numbers).

The second half of the module makes the seeded inputs shared by tests/test_loss_ref_cpu.py and tests/test_hip_loss_fp64.py.
"""
import numpy as np
import torch

from oracle.mirror_nerf_oracle import LOSS_DEFAULTS

TYPS = ("coarse", "fine")
BCE_LO = float(np.float32(1e-7))
BCE_HI = float(np.float32(1) - np.float32(1e-7))


def thresholded_key(inputs):
    return "mirror_mask_fine" if "mirror_mask_fine" in inputs else ("mirror_mask_coarse" if "mirror_mask_coarse" in inputs else None)


def _mse(a, b):
    return ((a - b) ** 2).mean()


def color_loss(inputs, batch, hp, train_geometry_stage=False):
    targets = batch["rgbs"].reshape(-1, 3)
    gt = batch.get("mirror_mask")
    sel = None
    if train_geometry_stage and gt is not None and bool((gt < 0).any()):
        key = thresholded_key(inputs)
        if key is None:
            return targets.new_zeros(())
        m = inputs[key].detach()        # shares storage: the dict entry holds the thresholded values from here on
        m[m > 0.5] = 1
        m[m < 0.5] = 0
        sel = ~(m != 0)
    elif train_geometry_stage and gt is not None and hp["woMaskRGBtoBlack"]:
        sel = ~(gt.reshape(-1) != 0)
    loss = targets.new_zeros(())
    for typ in TYPS:
        if f"rgb_{typ}" in inputs:
            rgb = inputs[f"rgb_{typ}"]
            loss = loss + (_mse(rgb, targets) if sel is None else _mse(rgb[sel], targets[sel]))
    return hp["color_loss_weight"] * loss


def _valid_gt_mirror(batch):
    gt = batch.get("mirror_mask")
    return (gt.reshape(-1) != 0) if (gt is not None and not bool((gt < 0).any())) else None


def normal_loss(inputs, batch, hp):
    mm = _valid_gt_mirror(batch)
    loss = batch["rgbs"].new_zeros(())
    for typ in TYPS:
        k = f"normal_dif_{typ}"
        if k not in inputs:
            continue
        if mm is not None:
            if not hp["normal_loss_only_inside_mirror"]:
                loss = loss + inputs[k][~mm].mean()
            loss = loss + inputs[k][mm].mean() * 100
        else:
            loss = loss + inputs[k].mean()
    return hp["normal_loss_weight"] * loss


def plane_consistent_loss(inputs, batch, hp, plane_idx):
    mm = _valid_gt_mirror(batch)
    loss = batch["rgbs"].new_zeros(())
    if mm is not None:
        for typ in ("fine", "coarse"):
            k = f"x_surface_{typ}"
            if k not in inputs:
                continue
            pts = inputs[k][mm]
            times = pts.shape[0] // 4
            if times > 0:
                ix = torch.as_tensor(np.asarray(plane_idx[typ]).reshape(times, 4))
                p0, p1, p2, p3 = (pts[ix[:, j]] for j in range(4))
                tri = (torch.linalg.cross(p1 - p0, p2 - p0) * (p3 - p0)).sum(-1)
                loss = loss + tri.abs().mean()
    return hp["plane_consistent_loss_weight"] * loss


def normal_reg_loss(inputs, batch, hp, ext_supervise_grad_normal=True):
    rays_d = batch["rays"][..., 3:6].reshape(-1, 3)
    mask = batch["valid_mask"].reshape(-1).bool() if "valid_mask" in batch else torch.ones(rays_d.shape[0], dtype=torch.bool)
    loss = rays_d.new_zeros(())

    def term(nkey, wkey):
        n = inputs[nkey][mask]
        return (torch.relu(n * rays_d[mask][:, None, :]).sum(-1) * inputs[wkey][mask]).mean()

    for typ in TYPS:
        if f"pred_normal_{typ}" in inputs:
            loss = loss + term(f"pred_normal_{typ}", f"weights_{typ}")
    if ext_supervise_grad_normal and "normal_fine" in inputs:
        loss = loss + term("normal_fine", "weights_fine")
    return hp["normal_reg_loss_weight"] * loss


def mirror_mask_loss(inputs, batch, hp):
    loss = batch["rgbs"].new_zeros(())
    if "mirror_mask" not in batch:
        return loss
    gt = batch["mirror_mask"].reshape(-1)
    valid = (gt >= 0).to(gt.dtype)
    for typ in TYPS:
        k = f"mirror_mask_{typ}"
        if k not in inputs:
            continue
        p = torch.clamp(inputs[k], BCE_LO, BCE_HI)
        lp, l1p = torch.log(p), torch.log(1 - p)
        if hp["model_type"] != "nerf_tcnn":
            lp, l1p = torch.clamp(lp, min=-100.0), torch.clamp(l1p, min=-100.0)
        loss = loss + (-(gt * lp + (1 - gt) * l1p) * valid).mean()
    return hp["mirror_mask_loss_weight"] * loss


def total_loss(inputs, batch, hp=None, train_geometry_stage=False, epoch=-1, plane_idx=None):
    """TotalLoss.forward -> (loss_sum, loss_dict) on torch tensors of one dtype.  `inputs` may be mutated (see color_loss)."""
    h = dict(LOSS_DEFAULTS)
    h.update(hp or {})
    d = {"color_loss": color_loss(inputs, batch, h, train_geometry_stage)}
    if not train_geometry_stage or epoch >= h["train_mirror_mask_start_epoch"]:
        d["mirror_mask_loss"] = mirror_mask_loss(inputs, batch, h)
    if epoch >= h["smooth_mirror_start_epoch"] and h["use_plane_consistent_loss"]:
        d["plane_consistent_loss"] = plane_consistent_loss(inputs, batch, h, plane_idx)
    if not train_geometry_stage or epoch >= h["train_normal_start_epoch"]:
        d["normal_loss"] = normal_loss(inputs, batch, h)
        d["normal_reg_loss"] = normal_reg_loss(inputs, batch, h)
    total = d["color_loss"].new_zeros(())
    for v in d.values():
        total = total + v
    return total, d


def evaluate(inputs, batch, hp=None, train_geometry_stage=False, epoch=-1, plane_idx=None, dtype=torch.float64):
    """numpy in, numpy out: {"total", "terms": {name: value}, "grads": {input: d(total)/d(input), zeros where autograd reaches none},
    "inputs": the predictions after the call (the thresholded key changes in one branch)}.  dtype=torch.float32 runs the same
    statement in single precision: its distance from float64 is the floor a float32 kernel can be held to."""
    leaves = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in inputs.items()}
    res = {k: v * 1.0 for k, v in leaves.items()}         # non-leaf, as render_rays returns them
    tb = {k: torch.as_tensor(np.asarray(v)) for k, v in batch.items()}
    tb = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in tb.items()}
    total, d = total_loss(res, tb, hp, train_geometry_stage, epoch, plane_idx)
    if total.requires_grad:
        total.backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in leaves.items()}
    return {"total": total.detach().numpy()[()], "terms": {k: v.detach().numpy()[()] for k, v in d.items()}, "grads": grads,
            "inputs": {k: v.detach().numpy() for k, v in res.items()}}


def plane_picks(u, gt, present=("fine", "coarse")):
    """The picks both routes of the kernel form from injected uniform numbers `u` (2, 4 * (n // 4)) float32, row 0 for the first
    typ present in "fine", "coarse" order: min(int64(float32(u) * float32(M)), M - 1) for the M // 4 live quadruples."""
    gt = np.asarray(gt).reshape(-1)
    if (gt < 0).any():
        return None
    m = int((gt != 0).sum())
    if m // 4 == 0:
        return None
    order = [t for t in ("fine", "coarse") if t in present]
    return {t: np.minimum((np.asarray(u, np.float32)[k, :4 * (m // 4)] * np.float32(m)).astype(np.int64), m - 1).reshape(m // 4, 4)
            for k, t in enumerate(order)}


# ------------------------------------------------------------------------------------------------------------------ shared inputs
MASK_EDGES = np.array([0.0, 1.0, 0.5, 1e-9, np.float32(1e-7), np.float32(1) - np.float32(1e-7)], np.float32)
S_COARSE, S_FINE = 5, 7       # divide neither 64 nor 256: ray = j / S crosses wave and block boundaries mid-ray


def make_inputs(n, seed=0, fine=True, gt="half", invalid_frac=0.0, valid_frac=None, pred="uniform"):
    """Seeded float32 inputs and batch of n rays (5 coarse, 7 fine samples).  The first entries of every predicted mask are
    MASK_EDGES; `rays` has 11 columns, so the wrapper's [:, :8] slice is non-contiguous.
    gt: "half" (about half ones; rows 0 and 1 are pinned to 1 and 0 so neither side is empty from n = 2 on), "zeros", "ones".
    invalid_frac: that share of GT entries set to -1.  valid_frac: share of true entries of a `valid_mask` (None: no mask).
    pred: "uniform", or "high" (every predicted mask entry above 0.5)."""
    rs = np.random.RandomState(seed)

    def unit(*shape):
        v = rs.normal(size=shape + (3,)).astype(np.float32)
        return v / np.linalg.norm(v, axis=-1, keepdims=True)

    inputs = {}
    for typ, s in (("coarse", S_COARSE), ("fine", S_FINE)):
        d = {}
        d[f"rgb_{typ}"] = rs.uniform(size=(n, 3)).astype(np.float32)
        m = rs.uniform(0.01, 0.99, size=n).astype(np.float32)
        m[:min(n, 6)] = MASK_EDGES[:min(n, 6)]
        if pred == "high":
            m = (0.5 + 0.5 * rs.uniform(0.02, 0.98, size=n)).astype(np.float32)
        d[f"mirror_mask_{typ}"] = m
        d[f"normal_dif_{typ}"] = rs.uniform(size=n).astype(np.float32)
        d[f"pred_normal_{typ}"] = unit(n, s)
        w = rs.uniform(size=(n, s)).astype(np.float32)
        d[f"weights_{typ}"] = w / w.sum(-1, keepdims=True)
        d[f"x_surface_{typ}"] = rs.normal(size=(n, 3)).astype(np.float32)
        if typ == "fine":
            d["normal_fine"] = unit(n, s)
        if fine or typ == "coarse":
            inputs.update(d)
    g = (rs.uniform(size=n) < 0.5).astype(np.float32)
    if n >= 2:
        g[0], g[1] = 1.0, 0.0
    if gt == "zeros":
        g[:] = 0.0
    elif gt == "ones":
        g[:] = 1.0
    inv = rs.uniform(size=n) < invalid_frac
    g[inv] = -1.0
    batch = {"rgbs": rs.uniform(size=(n, 3)).astype(np.float32), "mirror_mask": g.reshape(n, 1),
             "rays": np.concatenate([rs.normal(size=(n, 3)), unit(n), np.tile([0.05, 8.0], (n, 1)), rs.normal(size=(n, 3))], 1).astype(np.float32)}
    vm = rs.uniform(size=n)
    if valid_frac is not None:
        batch["valid_mask"] = vm < valid_frac
    return inputs, batch


def make_plane_u(n, seed=0):
    """Injected draws (2, 4 * (n // 4)) float32 in [0, 1) with both ends of the range among them: 0 and the largest float32 below 1."""
    rs = np.random.RandomState(1000 + seed)
    u = rs.uniform(size=(2, 4 * (n // 4))).astype(np.float32)
    u = np.minimum(u, np.nextafter(np.float32(1), np.float32(0)))
    if u.shape[1] >= 4:
        u[0, 0], u[0, 1] = 0.0, np.nextafter(np.float32(1), np.float32(0))
        u[1, 2], u[1, 3] = np.nextafter(np.float32(1), np.float32(0)), 0.0
    return u


PLANE = dict(use_plane_consistent_loss=True)
# name -> (make_inputs arguments, hparams over LOSS_DEFAULTS, train_geometry_stage, epoch)
CASES = {
    "default": (dict(n=2500), PLANE, False, 5),
    "tcnn_bce": (dict(n=2500, seed=1), dict(PLANE, model_type="nerf_tcnn"), False, 5),
    "stage_invalid_ep0": (dict(n=2500, seed=2, invalid_frac=0.1), PLANE, True, 0),
    "stage_invalid_ep1": (dict(n=2500, seed=3, invalid_frac=0.1), PLANE, True, 1),
    "stage_invalid_ep2": (dict(n=2500, seed=4, invalid_frac=0.1), PLANE, True, 2),
    "stage_black_inside_valid": (dict(n=2500, seed=5, valid_frac=0.8),
                                 dict(PLANE, woMaskRGBtoBlack=True, normal_loss_only_inside_mirror=True), True, 3),
    "coarse_only": (dict(n=2500, seed=6, fine=False, valid_frac=0.8), PLANE, False, 5),
    "empty_gt_zeros": (dict(n=2500, seed=7, gt="zeros"), PLANE, False, 5),
    "empty_gt_ones": (dict(n=2500, seed=8, gt="ones"), PLANE, False, 5),
    "empty_valid_mask": (dict(n=2500, seed=9, valid_frac=0.0), PLANE, False, 5),
    "empty_stage_pred_high": (dict(n=2500, seed=10, invalid_frac=0.1, pred="high"), PLANE, True, 2),
}
SWEEP_SIZES = (1, 3, 63, 256, 1024, 1025)
for _n in SWEEP_SIZES:
    CASES[f"size_{_n}"] = (dict(n=_n, seed=20 + _n), PLANE, False, 5)
EMPTY_NAN_TERMS = {"empty_gt_zeros": {"normal_loss"}, "empty_gt_ones": {"normal_loss"}, "empty_valid_mask": {"normal_reg_loss"},
                   "empty_stage_pred_high": {"color_loss"}, "size_1": {"normal_loss"}}      # one ray: one side of the GT mask is empty

_BUILT = {}


def case(name):
    """-> dict(inputs, batch, hp, stage, epoch, u, picks, ref): built once, shared by every test and left unchanged (callers copy)."""
    c = _BUILT.get(name)
    if c is None:
        kw, hp, stage, epoch = CASES[name]
        inputs, batch = make_inputs(**kw)
        hp = dict(LOSS_DEFAULTS, **hp)
        u = make_plane_u(kw["n"], kw.get("seed", 0))
        picks = plane_picks(u, batch["mirror_mask"], [t for t in ("fine", "coarse") if f"x_surface_{t}" in inputs])
        ref = evaluate(inputs, batch, hp, stage, epoch, picks)
        c = _BUILT[name] = dict(inputs=inputs, batch=batch, hp=hp, stage=stage, epoch=epoch, u=u, picks=picks, ref=ref)
    return c


VALUE_BAR, GRAD_BAR = 2e-6, 1e-6       # tests/test_loss.py: relative on scalars (floor 1.0); of each gradient tensor's largest entry


def value_error(got, want):
    """|got - want| / max(1, |want|); NaN must meet NaN (-> 0.0), anything else against NaN is inf."""
    got, want = float(got), float(want)
    if np.isnan(want) or np.isnan(got):
        return 0.0 if (np.isnan(want) and np.isnan(got)) else float("inf")
    return abs(got - want) / max(1.0, abs(want))


def grad_error(got, want):
    """(largest |got - want|, largest |want|) in float64; a non-finite entry of `got` is an infinite error."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.size == 0:
        return 0.0, 0.0
    if not np.isfinite(got).all():
        return float("inf"), float(np.abs(want).max())
    return float(np.abs(got - want).max()), float(np.abs(want).max())


def grad_parts(key, got, want):
    """The pieces of one gradient tensor that are each held to GRAD_BAR of their own largest entry: the tensor itself, and for a
    predicted mask also the rows past the planted MASK_EDGES -- an edge row's gradient is up to 1 / float32(1e-7) times an ordinary
    row's, and a bar taken from it alone would let every other row pass with any value."""
    yield key, got, want
    if key.startswith("mirror_mask_") and np.asarray(want).shape[0] > len(MASK_EDGES):
        yield key + "[6:]", np.asarray(got)[len(MASK_EDGES):], np.asarray(want)[len(MASK_EDGES):]


# ------------------------------------------------------------------------------------------------------------------ PSNR and MSE
# metrics.mse / metrics.psnr (mse_partial_kernel + mse_finish_kernel of csrc/mnrf_loss.hip), for tests/test_hip_psnr_fp64.py and, on
# the CPU, tests/test_loss_ref_cpu.py.  The reference is the float64 mean of (float64(a) - float64(b))^2 over the selected elements
# and -10 log10 of it.  The bar is derived from the kernel's float32 summation, not measured:
#
#   every term (a - b)^2 carries 3 roundings (the subtraction, doubled by the square, and the square's own);
#   a thread adds its q = ceil(n / (blocks * 256)) terms serially, the first onto an exact 0: q - 1 roundings;
#   block_sum: six shuffle levels and the four wave sums added onto an exact 0: 6 + 3 = 9;
#   mse_finish_kernel adds the `blocks` partials serially onto an exact 0: blocks - 1;  the division: 1.
#
# All terms are non-negative, so to first order the relative error of the sum is at most the largest number of roundings any one
# term passes through, times 2^-24: (3 + (q - 1) + 9 + (blocks - 1) + 1) * 2^-24 with blocks = min(1024, ceil(n / 256)).  The PSNR
# adds the derivative of -10 log10, 10 / ln 10, times that, and 2 ulp of the PSNR value for log10f.
MSE_TPB, MSE_MAX_BLOCKS = 256, 1024
MSE_SWEEP = MSE_TPB * MSE_MAX_BLOCKS          # 262 144 elements per pass of the grid-stride loop
U32 = 2.0 ** -24


def mse_geometry(n):
    """(blocks, q): the launch of mnrf_mse_psnr for n elements and the number of terms its busiest thread adds."""
    blocks = min(MSE_MAX_BLOCKS, max(1, -(-n // MSE_TPB)))
    return blocks, -(-n // (blocks * MSE_TPB))


def mse_bar(n):
    """The relative bar of the MSE (and of the count) for n elements."""
    blocks, q = mse_geometry(n)
    return (3 + max(q - 1, 0) + 9 + (blocks - 1) + 1) * U32


def psnr_bar(n, psnr):
    """The absolute bar of the PSNR in dB around the float64 value `psnr`."""
    return 10.0 / np.log(10.0) * mse_bar(n) + 2.0 * float(np.spacing(np.float32(abs(psnr))))


def mse_selection(n, mask, per_mask):
    """(n,) bool: element i is selected when there is no mask or mask[i // per_mask] is set."""
    if mask is None:
        return np.ones(n, dtype=bool)
    return np.asarray(mask).reshape(-1).astype(bool)[np.arange(n) // per_mask]


def mse_fp64(a, b, sel):
    """(mse, psnr, count) in float64 over the selected elements; an empty selection is (nan, nan, 0)."""
    d = np.asarray(a, np.float32).reshape(-1).astype(np.float64)[sel] - np.asarray(b, np.float32).reshape(-1).astype(np.float64)[sel]
    if d.size == 0:
        return float("nan"), float("nan"), 0
    m = float((d * d).mean())
    with np.errstate(divide="ignore"):
        return m, float(-10.0 * np.log10(m)), int(d.size)


def _block_sum_f32(v):
    """block_sum of csrc/mnrf_loss.hip on a (blocks, 256) float32 array: per wave of 64 the shuffle-down tree (lane 0 holds
    the sum), then the four wave sums added in order onto 0."""
    v = v.reshape(v.shape[0], MSE_TPB // 64, 64).copy()
    for o in (32, 16, 8, 4, 2, 1):
        v[..., :o] = v[..., :o] + v[..., o:2 * o]
    r = np.zeros(v.shape[0], dtype=np.float32)
    for w in range(MSE_TPB // 64):
        r = r + v[:, w, 0]
    return r


def mse_emulate(a, b, sel):
    """The kernels' own order in float32 numpy: (partials (blocks, 2) float32, out (3,) float32 = [mse, psnr, count]).  The MSE
    and the count are what the kernel computes bit for bit (IEEE float32 adds, multiplies and one division, nothing contracted);
    the PSNR goes through numpy's log10 and may differ from log10f in the last place."""
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    n = a.size
    blocks, q = mse_geometry(n)
    d = a - b
    pad = max(q, 1) * blocks * MSE_TPB
    term, one = np.zeros(pad, np.float32), np.zeros(pad, np.float32)
    term[:n] = np.where(sel, d * d, np.float32(0))
    one[:n] = sel
    term, one = term.reshape(-1, blocks, MSE_TPB), one.reshape(-1, blocks, MSE_TPB)
    s, c = np.zeros((blocks, MSE_TPB), np.float32), np.zeros((blocks, MSE_TPB), np.float32)
    for j in range(term.shape[0]):      # thread (block, t) visits i = block * 256 + t + j * blocks * 256; a skipped term adds an exact 0
        s, c = s + term[j], c + one[j]
    partials = np.stack([_block_sum_f32(s), _block_sum_f32(c)], 1)
    ts, tc = np.float32(0), np.float32(0)
    for k in range(blocks):
        ts, tc = ts + partials[k, 0], tc + partials[k, 1]
    with np.errstate(all="ignore"):
        m = np.float32(ts / tc)
        out = np.array([m, np.float32(-10) * np.log10(m), tc], dtype=np.float32)
    return partials, out


PSNR_SIZES = (1, 63, 64, 65, 255, 256, 257, MSE_SWEEP - 1, MSE_SWEEP, MSE_SWEEP + 1, 3 * MSE_SWEEP + 5, 2 ** 24 + 257)
PSNR_MASK_N = 3 * MSE_SWEEP + 6          # 786 438 = 3 * 262 146: three full passes and a tail, whole pixels of 3 channels
# name -> (n, per_mask or None, kind of mask, kind of images)
PSNR_CASES = {f"size_{n}": (n, None, None, "noise") for n in PSNR_SIZES}
PSNR_CASES.update({
    "mask_element": (PSNR_MASK_N, 1, "random", "noise"),
    "mask_pixel3": (PSNR_MASK_N, 3, "random", "noise"),
    "mask_pixel4": (PSNR_MASK_N + 2, 4, "random", "noise"),        # 786 440 = 4 * 196 610 = 5 * 157 288
    "mask_pixel5": (PSNR_MASK_N + 2, 5, "random", "noise"),
    "mask_all_true": (PSNR_MASK_N, 3, "all", "noise"),
    "mask_late_passes": (PSNR_MASK_N, 1, "late", "noise"),
    "mask_last_only": (PSNR_MASK_N, 1, "last", "noise"),
    "mask_none_selected": (PSNR_MASK_N, 3, "none", "noise"),
    "identical": (MSE_SWEEP + 1, None, None, "identical"),
    "one_element_2^-20": (1000, None, None, "one"),
    "scale_255": (MSE_SWEEP + 1, None, None, "255"),
})
_PSNR_BUILT = {}


def psnr_case(name):
    """-> dict(a, b (n,) float32, mask (n // per,) uint8 or None, per, sel (n,) bool, ref = mse_fp64(...)): seeded, built once,
    left unchanged."""
    c = _PSNR_BUILT.get(name)
    if c is None:
        n, per, mkind, ikind = PSNR_CASES[name]
        rs = np.random.RandomState(list(PSNR_CASES).index(name) + 100)
        b = rs.uniform(0, 1, n).astype(np.float32)
        if ikind == "identical":
            a = b.copy()
        elif ikind == "one":
            b[:] = np.round(b * 256) / 256
            b[n // 2] = 0.5
            a = b.copy()
            a[n // 2] = np.float32(0.5 + 2.0 ** -20)
        else:
            a = np.clip(b + rs.normal(0, 0.05, n), 0, 1).astype(np.float32)
            if ikind == "255":
                a, b = a * np.float32(255), b * np.float32(255)
        mask = None
        if mkind is not None:
            m = n // per
            mask = {"random": lambda: rs.uniform(size=m) < 0.5, "all": lambda: np.ones(m, bool), "none": lambda: np.zeros(m, bool),
                    "late": lambda: (rs.uniform(size=m) < 0.5) & (np.arange(m) >= MSE_SWEEP) & (np.arange(m) < 3 * MSE_SWEEP),
                    "last": lambda: np.arange(m) == m - 1}[mkind]().astype(np.uint8)
        sel = mse_selection(n, mask, per or 1)
        c = _PSNR_BUILT[name] = dict(a=a, b=b, mask=mask, per=per or 1, sel=sel, ref=mse_fp64(a, b, sel))
        if n > 2 ** 24:      # (the one large case is not kept: 200 MB)
            del _PSNR_BUILT[name]
    return c


def psnr_errors(c, out):
    """c: a psnr_case; out = [mse, psnr, count] as float32 -> (mse error / bar, psnr error / bar, count error / bar) against the
    float64 reference of the case, each a fraction of its derived bar; the caller asserts <= 1.  NaN must meet NaN, 0 must meet
    0, +inf +inf."""
    n = c["a"].size
    m, p, cnt = c["ref"]
    gm, gp, gc = (float(x) for x in out)
    if cnt == 0:
        return (0.0 if np.isnan(gm) else np.inf, 0.0 if np.isnan(gp) else np.inf, 0.0 if gc == 0.0 else np.inf)
    if m == 0.0:
        return (0.0 if gm == 0.0 else np.inf, 0.0 if gp == np.inf else np.inf, abs(gc - cnt) / cnt / mse_bar(n))
    return (abs(gm - m) / m / mse_bar(n), abs(gp - p) / psnr_bar(n, p), abs(gc - cnt) / cnt / mse_bar(n))
