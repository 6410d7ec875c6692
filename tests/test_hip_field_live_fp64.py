"""The four launches that carry a captured training step's arithmetic, under a live row count on the device (include/mnrf.h
"live row counts on the device"): mnrf_field_forward_train_n, mnrf_field_backward_planes_n (with its seed_max pre-pass),
mnrf_field_backward2_planes_n (with its jhat_max pre-pass) and mnrf_dw_planes2_n (with dwp_plan_kernel, which makes the GEMM's
work plan on the device).  Called through the C ABI on buffers the test owns, split arithmetic, planes route.

Every case runs the chain twice: (a) at the capacity with a device count `live`, everything past the live rows poisoned --
NaN in every input, cotangent and keep_mirror row, a sentinel in every float output, 0xFF bytes (an f16 NaN pattern) in the mask
words and the four plane buffers, a sentinel in the 32 gradient tensors; (b) as the namesake form (n_live = null) on contiguous
copies of the live rows.  Asserted, as the header promises them:
  * every per-sample output of (a) equals (b) bit for bit on the live rows and keeps its sentinel past them (d_xyz before and
    after the second-order pass adds to it); the seedmax / jmax words are equal;
  * the mask words and the plane buffers equal (b)'s over the first ceil(live spr / 128) tiles and are untouched past them;
  * the DwpDevPlan block at the head of the workspace is the plan of the header's closed forms (tests/dwp_plan_ref.py, held to
    the header by tests/test_dwp_plan_ref_cpu.py);
  * the range-guard word of the weight image does not move (a NaN that was read would set it);
  * the 32 weight gradients are finite and, with dL/dxyz and dL/d(view encoding) of the live rows, within the bars of
    tests/test_hip_backward_fp64.py of the masked float64 reference of the live rows alone;
  * sharpness, on the reference: the float64 gradients of live - 1 and of live + 1 rows of the clean twin (whose dead rows hold
    finite draws) differ from those of `live` rows by >= 10 x the bar in some tensor, so an off-by-one row in any launch fails.

Counts sit on both sides of the 32-sample block (PL_SB) and of the 128-sample workgroup tile (WG_SAMPLES); ray mode ends the
live samples on half tiles (64 and 192 samples per ray are the product's coarse and fine counts).

Every bar is a constant of tests/test_hip_backward_fp64.py.  Measured (MI355X), worst over each group against its bar:
  xyz first order      9.51e-6 at live = 127, xyz_encoding_1.0.weight (FIRST_BAR 2e-5)
  ray first order      1.05e-5 at 16 x 33, 4 live, xyz_encoding_1.0.weight (FIRST_BAR 2e-5)
  both orders          4.85e-5 at live = 128, xyz_encoding_1.0.weight (SECOND_BAR split 1e-4)
  trained, FieldFn     2.02e-5, is_mirror_net.2.bias; 1.98e-5 with the gradient scale lowered by 2^4 (SECOND_BAR split 1e-4,
                       is_mirror_net.* MIRROR_SPLIT_BAR 1e-4, both as they stand)
  eight evaluations    4.46e-5 after either call, xyz_encoding_1.0.weight (trunk weights and sigma.weight SECOND_BAR split 1e-4,
                       the rest FIRST_BAR 2e-5)
The seeded weights under a scale lowered by r = 4 (test_ray_live_count_with_a_lowered_gradient_scale) are held to the relations
with the namesake and the plan only: no existing bar covers seeded weights at a lowered scale, so none is asserted there.
Informational only, printed per case and not asserted (the header does not promise it): whether the 32 weight gradients of (a)
equal (b)'s bit for bit."""
import ctypes

import pytest
import torch

from tests import dwp_plan_ref as PR
from tests.field_fp64 import DEV, F64, _rel, _rows_forward, _saved
from tests.test_hip_backward_fp64 import (FIRST_BAR, MIRROR_SPLIT_BAR, SECOND_BAR, _compare, _cots, _inputs, _kernel_masks,
                                          _lowering_scale, _model, _reference)

pytestmark = pytest.mark.gpu

SENT = -7.0            # every float output of (a) starts as this
GSENT = 3.0            # ... and every gradient entry in front of an overwriting GEMM


@pytest.fixture(autouse=True)
def _split_arithmetic():
    from mirror_nerf_amd import mirror_nerf as MN
    old = MN.PRECISION
    MN.set_precision("split")
    yield
    MN.set_precision(old)


# ---------------------------------------------------------------------------------------------- inputs
class Twin:
    """Clean inputs of `rows` rows (rays of spr samples, or positions: spr0 = 0), their cotangents, and the float64 reference of
    a prefix of them under the masks of the kernel's own forward."""

    def __init__(self, kind, rows, spr0, seed, second=False, keep_frac=None, cut=0, null_heads=False):
        self.model, self.w64 = _model(kind)
        self.inp = _inputs(rows * (spr0 or 1), spr0, seed)
        self.rows, self.spr, self.B = rows, self.inp["spr"], self.inp["B"]
        self.cots = [c.contiguous() for c in _cots(self.B, "flat", seed)]
        if null_heads:      # the planes route passes a missing cotangent as a null pointer
            self.cots[2] = self.cots[3] = None
        g = torch.Generator(device=DEV).manual_seed(seed + 9)
        self.gn = torch.randn(self.B, 3, device=DEV, generator=g) if second else None
        self.keep = None if keep_frac is None else (torch.rand(rows, device=DEV, generator=g) < keep_frac).float()
        self.cut = cut
        self._masks = None

    def cut_to(self, t, per, rows=None, poison_from=None):
        """A contiguous copy of the first `rows` rows of t, which holds `per` entries per row (1: per ray / position, spr: per
        sample); the entries of rows >= poison_from hold NaN.  None stays None."""
        if t is None:
            return None
        t = t[:None if rows is None else rows * per].clone()
        if poison_from is not None:
            t[poison_from * per:] = float("nan")
        return t

    def args(self, rows=None, poison_from=None):
        """What a chain of launches reads, cut and poisoned by cut_to: (x = xyz / rays / z / de, cotangents, g_normal, keep_mirror)."""
        c = lambda t, per: self.cut_to(t, per, rows, poison_from)  # noqa: E731
        return ({k: c(self.inp[k], 1) for k in ("xyz", "rays", "z", "de")}, [c(t, self.spr) for t in self.cots], c(self.gn, self.spr),
                c(self.keep, 1))

    def prepare(self, rows):
        """The kernel's own forward (rows route, same arithmetic) of the first `rows` rows: positions and masks of the reference."""
        n = rows * self.spr
        x = self.args(rows)[0]
        fw = _rows_forward(self.model, dict(B=n, spr=self.spr, xyz=x["xyz"], rays=x["rays"], z=x["z"], de=x["de"]), True)
        saved = _saved(fw["sx"], n)
        self._de64 = x["de"].to(F64).repeat_interleave(self.spr, 0)
        self._masks = _kernel_masks(self.w64, saved, self._de64)
        self._pos = saved["enc"][:, :3]
        self._prepared = rows

    def ref(self, rows, first=True, second=None):
        """Float64 gradients of the first `rows` rows: ({param: grad}, dL/dxyz per sample, dL/d(view encoding) per sample)."""
        from mirror_nerf_amd import _lib
        second = (self.gn is not None) if second is None else second
        if rows == 0:
            return {k: torch.zeros_like(v) for k, v in self.w64.items()}, torch.zeros(0, 3, device=DEV, dtype=F64), torch.zeros(0, 27, device=DEV, dtype=F64)
        assert rows <= self._prepared
        n = rows * self.spr
        cots = [None if (c is None or not first) else c[:n] for c in self.cots] + ([self.gn[:n]] if second else [])
        keep = None if self.keep is None else (self.keep[:rows] != 0).repeat_interleave(self.spr, 0)
        return _reference(self.w64, self._pos[:n], self._de64[:n], {k: v[:n] for k, v in self._masks.items()}, cots, with_normal=second,
                          cut_normal=bool(self.cut & _lib.MNRF_CUT_NORMAL_HEAD), cut_mirror=bool(self.cut & _lib.MNRF_CUT_MIRROR_HEAD), keep=keep)


def _sharp(tw, live, ref, bar, **kw):
    """One row fewer or one row more would move some gradient tensor by >= 10 x the bar (asserted on the reference)."""
    for other in (live - 1, live + 1):
        if other < 0 or other > tw.rows:
            continue
        r = tw.ref(other, **kw)[0]
        moved = max(float((r[n] - ref[n]).abs().max()) / max(float(ref[n].abs().max()), 1e-300) for n in ref)
        assert moved >= 10 * bar, (live, other, moved)


# ---------------------------------------------------------------------------------------------- the launches
def _guard(model):
    from mirror_nerf_amd.weights import packed_of
    return int(packed_of(model)[-1:].view(torch.int32).item())


def _chain(tw, args, rows, nl, red=0):
    """forward_train_n -> backward_planes_n [-> backward2_planes_n] at B = rows * spr on fresh buffers: float outputs hold SENT,
    mask words and planes 0xFF bytes; red: the r of mnrf_field_backward_planes' flags (a gradient scale lowered by 2^r).  Returns
    the buffers and the tape entries of the weight-gradient GEMM."""
    from mirror_nerf_amd import _lib
    from mirror_nerf_amd.weights import packed_of
    L, p = _lib.lib(), _lib.ptr
    x, cots, gn, keep = args
    spr, B = tw.spr, rows * tw.spr
    packed = packed_of(tw.model)
    s = lambda *sh: torch.full(sh, SENT, dtype=torch.float32, device=DEV)  # noqa: E731
    by = lambda n: torch.full((int(n),), 0xFF, dtype=torch.uint8, device=DEV)  # noqa: E731
    word = lambda: torch.full((1,), -1, dtype=torch.int32, device=DEV)  # noqa: E731
    second = gn is not None
    o = dict(sigma=s(B), rgb=s(B, 3), pred_normal=s(B, 3), is_mirror=s(B), save_inv=s(B), d_xyz=s(B, 3), d_dir=s(B, 32))
    if second:
        o.update(normal=s(B, 3), save_invj=s(B))
    pl = dict(save_x=by(L.mnrf_train_planes_bytes(B)), dy=by(L.mnrf_train_dy_planes_bytes(B)),
              save_mask=torch.full((int(L.mnrf_train_mask_words(B)),), -1, dtype=torch.int64, device=DEV))
    words = dict(seedmax=word())
    _lib.check(L.mnrf_field_forward_train_n(
        p(packed), B, p(x["xyz"]), 3, p(x["rays"]), p(x["z"]), spr, p(x["de"]), 27, p(o["sigma"]), p(o["rgb"]), p(o["pred_normal"]),
        p(o["is_mirror"]), p(o.get("normal")), p(pl["save_x"]), p(pl["save_mask"]), p(o["save_inv"]), p(o.get("save_invj")),
        _lib.MNRF_SPLIT_F16 | _lib.MNRF_TRAIN_PLANES, p(nl), _lib.stream()), "forward_train_n")
    _lib.check(L.mnrf_field_backward_planes_n(
        p(packed), B, p(x["xyz"]), 3, p(x["rays"]), p(x["z"]), spr, p(cots[0]), p(cots[1]), p(cots[2]), p(cots[3]), p(o["rgb"]),
        p(o["pred_normal"]), p(o["is_mirror"]), p(pl["save_mask"]), p(o["save_inv"]), p(pl["dy"]), p(words["seedmax"]), p(o["d_xyz"]),
        p(o["d_dir"]), p(keep), tw.cut | (red << 16), p(nl), _lib.stream()), "backward_planes_n")
    tape = [(pl["save_x"], pl["dy"], B, words["seedmax"], red << 8, nl, spr)]
    if second:
        o["d_xyz_first"] = o["d_xyz"].clone()
        pl.update(x2=by(L.mnrf_train_planes2_bytes(B)), y2=by(L.mnrf_train_dy_planes2_bytes(B)))
        words["jmax"] = word()
        _lib.check(L.mnrf_field_backward2_planes_n(
            p(packed), B, p(x["xyz"]), 3, p(x["rays"]), p(x["z"]), spr, p(gn), p(o["normal"]), p(o["save_invj"]), p(pl["save_mask"]),
            p(pl["x2"]), p(pl["y2"]), p(words["jmax"]), p(o["d_xyz"]), p(nl), _lib.stream()), "backward2_planes_n")
        tape.append((pl["x2"], pl["y2"], B, words["jmax"], 1, nl, spr))
    return dict(out=o, planes=pl, words=words, tape=tape)


_WS = {}


def _workspace():
    from mirror_nerf_amd import _lib
    if "ws" not in _WS:      # the room of eight evaluations serves every smaller call
        _WS["ws"] = torch.empty(int(_lib.lib().mnrf_dw_planes2_n_workspace_floats(PR.MAX_EVAL)), dtype=torch.float32, device=DEV)
    return _WS["ws"]


def _grads(fill=None, seed=0):
    from mirror_nerf_amd.weights import PARAM_NAMES, PARAM_SHAPES
    if fill is not None:
        return [torch.full(PARAM_SHAPES[n], fill, dtype=torch.float32, device=DEV) for n in PARAM_NAMES]
    g = torch.Generator(device=DEV).manual_seed(seed)
    return [torch.randn(*PARAM_SHAPES[n], device=DEV, generator=g) for n in PARAM_NAMES]


def _dw(tape, grads, accumulate):
    """mnrf_dw_planes2_n over the tape; returns the DwpDevPlan block it left at the head of the workspace, parsed."""
    from mirror_nerf_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    n = len(tape)
    ws = _workspace()
    assert L.mnrf_dw_planes2_n_workspace_floats(n) <= ws.numel()
    ws[:PR.DEVPLAN_FLOATS].fill_(float("nan"))
    vp = lambda k: (ctypes.c_void_p * n)(*[None if t[k] is None else t[k].data_ptr() for t in tape])  # noqa: E731
    _lib.check(L.mnrf_dw_planes2_n(n, vp(0), vp(1), (ctypes.c_int64 * n)(*[t[2] for t in tape]), vp(5), (ctypes.c_int * n)(*[t[6] for t in tape]),
                                   vp(3), (ctypes.c_int * n)(*[t[4] for t in tape]), p(ws), (ctypes.c_void_p * 32)(*[t.data_ptr() for t in grads]),
                                   accumulate, _lib.stream()), "dw_planes2_n")
    torch.cuda.synchronize()
    return PR.parse(ws[:PR.DEVPLAN_FLOATS].view(torch.uint8).cpu().numpy().tobytes())


def _check_plan(got, tape, lives):
    """The block dwp_plan_kernel wrote against the header's closed forms (tests/dwp_plan_ref.py)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_sb = [PR.live_blocks(lv, t[6], t[2]) for t, lv in zip(tape, lives)]
    want = PR.plan(n_sb, [t[4] & 0xff for t in tape], cus)
    pad = [0] * (PR.MAX_EVAL - len(tape))
    assert got["n_eval"] == want["n_eval"]
    assert got["n_sb"] == want["n_sb"] + pad and got["kind"] == want["kind"] + pad, (got["n_sb"], want["n_sb"], got["kind"])
    assert (got["T"], got["G"]) == (want["T"], want["G"]), (got["T"], got["G"], want["T"], want["G"])
    assert got["g_lo"] == want["g_lo"] and got["g_hi"] == want["g_hi"]


def _untouched(a, eff, spr):
    for k, t in a["out"].items():
        assert bool((t[eff * spr:] == SENT).all()), f"{k}: a row past the live count was written"


# ---------------------------------------------------------------------------------------------- one case
def _case(rows, spr0, live, second=False, cut=0, keep_frac=None, null_heads=False, seed=0, tag="", red=0, mixed_keep=False):
    from mirror_nerf_amd import _lib
    from mirror_nerf_amd.weights import PARAM_NAMES
    L = _lib.lib()
    tw = Twin("init", rows, spr0, 1000 * rows + 10 * (spr0 or 1) + seed, second=second, keep_frac=keep_frac, cut=cut, null_heads=null_heads)
    spr = tw.spr
    eff = min(max(live, 0), rows)      # the clamps of the kernels: a count above the capacity is the capacity, a negative one zero
    assert eff > 0
    guard = _guard(tw.model)
    nl = torch.tensor([live], dtype=torch.int32, device=DEV)
    if mixed_keep:      # the mirror head is cut on some live rows and kept on others
        assert 0 < int(tw.keep[:eff].sum()) < eff
    a = _chain(tw, tw.args(poison_from=eff), rows, nl, red)
    ga = _grads(GSENT)
    plan = _dw(a["tape"], ga, 0)
    b = _chain(tw, tw.args(eff), eff, None, red)
    gb = _grads(GSENT)
    _dw(b["tape"], gb, 0)
    # ---- the live rows are the namesake's bit for bit, the dead rows were not written
    n = eff * spr
    for k, t in a["out"].items():
        assert torch.equal(t[:n], b["out"][k]), f"{k}: live rows differ from the namesake's"
    _untouched(a, eff, spr)
    for k, t in a["words"].items():
        assert torch.equal(t, b["words"][k]), (k, int(t), int(b["words"][k]))
    tiles = -(-n // 128)      # (b)'s buffers are the header's sizes for n samples: whole 128-sample tiles
    assert b["planes"]["save_x"].numel() == L.mnrf_train_planes_bytes(128 * tiles) and b["planes"]["save_mask"].numel() == L.mnrf_train_mask_words(128 * tiles)
    for k, t in a["planes"].items():
        nb = b["planes"][k].numel()
        assert torch.equal(t[:nb], b["planes"][k]), f"{k}: the live tiles differ from the namesake's"
        assert bool((t[nb:] == (-1 if k == "save_mask" else 0xFF)).all()), f"{k}: written past the live tiles"
    _check_plan(plan, a["tape"], [live] * len(a["tape"]))
    assert _guard(tw.model) == guard, "the range guard moved: a poisoned row was read"
    same = all(torch.equal(x, y) for x, y in zip(ga, gb))
    assert all(bool(torch.isfinite(t).all()) for t in ga), [nm for nm, t in zip(PARAM_NAMES, ga) if not bool(torch.isfinite(t).all())]
    name = f"live {tag}rows={rows} spr={spr} live={live}{' both orders' if second else ''}"
    print(f"MEAS {name}: weight gradients {'equal' if same else 'differ from'} the namesake's bit for bit (informational)")
    if red:      # no existing bar covers the seeded weights under a lowered scale: the relations above are what this case holds
        return None
    # ---- float64 of the live rows alone
    bar = SECOND_BAR["split"] if second else FIRST_BAR
    tw.prepare(min(eff + 1, rows))
    ref = tw.ref(eff)
    live_inp = dict(B=n, spr=1, rays=None)
    worst = _compare((dict(zip(PARAM_NAMES, ga)), a["out"]["d_xyz"][:n], a["out"]["d_dir"][:n]), ref, live_inp, name, bar)
    _compare((dict(zip(PARAM_NAMES, gb)), b["out"]["d_xyz"], b["out"]["d_dir"]), ref, live_inp, name + " (namesake)", bar)
    _sharp(tw, eff, ref[0], bar)
    return worst


# ================================================================ 1. positions: four full tiles and a one-sample fifth
XYZ_ROWS = 513
XYZ_LIVE = [1, 31, 32, 33, 127, 128, 129, 255, 256, 257, 384, 512, 513]


@pytest.mark.parametrize("live", XYZ_LIVE + [600])
def test_xyz_live_count_first_order(live):
    """Capacity 513 positions, counts on both sides of every 32-sample block and 128-sample tile edge that matters; 600 (above
    the capacity) behaves as 513.  Bar: FIRST_BAR."""
    _case(XYZ_ROWS, 0, live)


@pytest.mark.parametrize("live", [1, 33, 128, 129, 257])
def test_xyz_live_count_both_orders(live):
    """The second-order pass takes part: mnrf_field_backward2_planes_n adds to d_xyz and leaves one more tape entry (kind 1) for
    the same GEMM launch.  Bar: SECOND_BAR["split"]."""
    _case(XYZ_ROWS, 0, live, second=True)


def _nothing_live(rows, spr0, live, second):
    """No row exists: nothing is written, an overwriting GEMM leaves exact zeros, an accumulating one changes no bit."""
    tw = Twin("init", rows, spr0, 77, second=second)
    guard = _guard(tw.model)
    nl = torch.tensor([live], dtype=torch.int32, device=DEV)
    a = _chain(tw, tw.args(poison_from=0), rows, nl)
    _untouched(a, 0, tw.spr)
    for k, t in a["planes"].items():
        assert bool((t == (-1 if k == "save_mask" else 0xFF)).all()), f"{k}: written although nothing is live"
    g = _grads(GSENT)
    plan = _dw(a["tape"], g, 0)
    _check_plan(plan, a["tape"], [live] * len(a["tape"]))
    assert plan["T"] == 0 and all(lo > hi for lo, hi in zip(plan["g_lo"], plan["g_hi"]))
    assert all(bool((t == 0).all()) for t in g), "an overwriting GEMM over nothing must leave exact zeros"
    g = _grads(seed=5)
    start = [t.clone() for t in g]
    _dw(a["tape"], g, 1)
    assert all(torch.equal(x, y) for x, y in zip(g, start)), "an accumulating GEMM over nothing must not change a bit"
    assert _guard(tw.model) == guard


@pytest.mark.parametrize("live", [0, -3])
def test_xyz_nothing_live(live):
    """A count of zero, and a negative one (which behaves as zero), with both orders on the tape."""
    _nothing_live(XYZ_ROWS, 0, live, True)


# ================================================================ 2. rays: live samples that end on half tiles
RAY_CASES = [(33, 16, lv) for lv in (1, 3, 4, 15)] + [(64, 9, lv) for lv in (1, 2, 3, 8)] + [(192, 5, lv) for lv in (1, 2, 3)]


@pytest.mark.parametrize("spr,rows,live", RAY_CASES)
def test_ray_live_count_first_order(spr, rows, live):
    """Ray mode: positions from rays and depths, the view encoding and keep_mirror per ray.  33 samples per ray put every ray edge
    inside a block; 64 and 192 are the product's coarse and fine counts.  Bar: FIRST_BAR."""
    _case(rows, spr, live, keep_frac=0.5 if (spr, live) in ((64, 8), (192, 3)) else None)


def test_ray_live_count_cut_normal_head_and_keep_mirror():
    """MNRF_CUT_NORMAL_HEAD and a per-ray keep_mirror that is 0 on some live rays (its dead rows hold NaN)."""
    from mirror_nerf_amd import _lib
    _case(16, 33, 15, cut=_lib.MNRF_CUT_NORMAL_HEAD, keep_frac=0.5, seed=3, tag="cut ", mixed_keep=True)


def test_ray_live_count_missing_cotangents():
    """g_pred_normal and g_is_mirror null: the planes route passes a missing cotangent as a null pointer."""
    _case(9, 64, 3, null_heads=True, seed=4, tag="null heads ")


def test_ray_live_count_both_orders():
    _case(9, 64, 3, second=True, seed=5)


def test_ray_live_count_with_a_lowered_gradient_scale():
    """r = 4 in the flags of mnrf_field_backward_planes_n and in the evaluation's kind (what training sets after a saturated
    gradient): bit identity with the namesake, untouched dead rows and planes, equal seedmax, the plan block, finite gradients.
    No float64 comparison: the trained FieldFn case below holds a lowered scale to float64 under the bars that exist for it."""
    _case(9, 64, 3, seed=6, tag="r=4 ", red=4)


def test_ray_nothing_live():
    _nothing_live(9, 64, 0, False)


# ================================================================ 3. trained weights through FieldFn
def test_trained_weights_through_fieldfn_with_a_live_count():
    """FieldFn on the trained pair, 9 rays x 64 samples of which 3 are live, both orders, the gradient scale lowered as training
    lowers it (the `red << 16` flag meets a live count); NaN in every dead input and cotangent row.  The parameter gradients and the
    live rows of rays.grad / dir_emb.grad against float64 (mnrf_ray_grads_n leaves their dead rows as allocated).
    Bars: SECOND_BAR["split"], is_mirror_net.* MIRROR_SPLIT_BAR."""
    from mirror_nerf_amd.autograd import FieldFn
    rows, spr, live = 9, 64, 3
    tw = Twin("trained", rows, spr, 4242, second=True)
    model = tw.model
    x, cots, gn, _ = tw.args(poison_from=live)
    cots = cots + [gn]
    nl = torch.tensor([live], dtype=torch.int32, device=DEV)
    params = list(model.parameters())
    names = [n for n, _ in model.named_parameters()]

    def step():
        for q in params:
            q.grad = None
        r = x["rays"].clone().requires_grad_(True)
        d = x["de"].clone().requires_grad_(True)
        outs = FieldFn.apply(model, spr, None, r, x["z"], d, (True, 0, None, nl), *params)
        torch.autograd.backward(list(outs), cots)
        return [q.grad for q in params] + [r.grad[:live, :6], d.grad[:live]]

    res = _lowering_scale(model, step)
    assert all(bool(torch.isfinite(t).all()) for t in res)
    tw.prepare(live + 1)
    ref = tw.ref(live)
    inp = dict(B=live * spr, spr=spr, rays=tw.inp["rays"][:live], z=tw.inp["z"][:live])
    _compare((dict(zip(names, res[:-2])), res[-2], res[-1]), ref, inp, "live trained FieldFn 9 x 64, 3 live, both orders", SECOND_BAR["split"],
             MIRROR_SPLIT_BAR)
    _sharp(tw, live, ref[0], SECOND_BAR["split"])
    # 192 samples do not saturate the planes, so nothing was lowered above: the scale as training leaves it after a larger batch
    # did (r = GRAD_SCALE_STEP in the flags and the kinds), under the same bars (test_hip_backward_fp64 holds its lowered runs to them).
    from mirror_nerf_amd import mirror_nerf as MN
    model.__dict__["_mnrf_seed_reduction"] = MN.GRAD_SCALE_STEP
    try:
        res = step()
    finally:
        model.__dict__["_mnrf_seed_reduction"] = 0
    assert all(bool(torch.isfinite(t).all()) for t in res)
    _compare((dict(zip(names, res[:-2])), res[-2], res[-1]), ref, inp, f"live trained FieldFn 9 x 64, 3 live, both orders, scale lowered by 2^{MN.GRAD_SCALE_STEP}",
             SECOND_BAR["split"], MIRROR_SPLIT_BAR)


# ================================================================ 4. eight evaluations on one tape
def test_eight_evaluations_on_one_tape_and_the_plan_the_device_made():
    """One mnrf_dw_planes2_n call over DWP_MAX_EVAL = 8 tape entries of small, different capacities: kinds 0 and 1 mixed; live
    counts that are the capacity, partial, end inside a tile, zero (two entries, one of each kind), and one n_live = null (its
    capacity).  First overwriting sentinel-filled gradients, then once more with accumulate = 1: the float64 sum of the live rows'
    references, then twice that.  The DwpDevPlan block at the head of the workspace equals the header's closed forms field by
    field after either call."""
    from mirror_nerf_amd.weights import PARAM_NAMES
    #        rows spr0 live  second  entries taken (kind)
    evals = [(200, 0, 200, False, (0,)),       # everything live
             (300, 0, 77, True, (0, 1)),       # partial, ends inside the first tile; both orders
             (6, 33, 0, False, (0,)),          # nothing live (kind 0)
             (130, 0, None, True, (1, 0)),     # n_live = null: the capacity, which ends inside a tile
             (150, 0, 0, True, (1,)),          # nothing live (kind 1)
             (5, 64, 3, False, (0,))]          # 192 live samples: a tile and a half
    tape, lives, keepalive = [], [], []
    total = None
    for e, (rows, spr0, live, second, take) in enumerate(evals):
        tw = Twin("init", rows, spr0, 900 + e, second=second)
        eff = rows if live is None else live
        nl = None if live is None else torch.tensor([live], dtype=torch.int32, device=DEV)
        pf = None if live is None else eff
        a = _chain(tw, tw.args(poison_from=pf), rows, nl)
        _untouched(a, eff, tw.spr)
        keepalive.append(a)
        by_kind = {t[4]: t for t in a["tape"]}
        for k in take:
            tape.append(by_kind[k])
            lives.append(live)
        if eff:
            tw.prepare(eff)
            r = tw.ref(eff, first=0 in take, second=1 in take)[0]
            total = r if total is None else {n: total[n] + r[n] for n in r}
    assert len(tape) == PR.MAX_EVAL and {t[4] for t in tape} == {0, 1}
    g = _grads(GSENT)
    second_order = [n for n in PARAM_NAMES if n == "sigma.weight" or (n.startswith("xyz_encoding_") and n.endswith(".0.weight"))]
    for call, factor in ((0, 1.0), (1, 2.0)):
        plan = _dw(tape, g, call)
        _check_plan(plan, tape, lives)
        assert all(bool(torch.isfinite(t).all()) for t in g)
        errs = sorted(((_rel(t, factor * total[n]), n) for n, t in zip(PARAM_NAMES, g)), reverse=True)
        print(f"MEAS live eight evaluations, call {call + 1}: worst {errs[0][0]:.2e} ({errs[0][1]})")
        bad = [x for x in errs if not x[0] <= (SECOND_BAR["split"] if x[1] in second_order else FIRST_BAR)]
        assert not bad, bad[:4]
