"""The field backward -- activation gradients (mnrf_field_bwd.inc, mnrf_field_split_bwd.inc), the weight-gradient GEMMs of
the rows route (mnrf_dw.hip) and of the planes route (mnrf_dwp.hip), the second-order pass -- against a float64 reference
that differentiates the same piecewise function as the kernels: tests/torch_ref.py `field(..., masks=)` with the ReLU /
LeakyReLU masks of the kernel's own training forward held constant.  Every case runs under both arithmetics (split: planes
route; fp32: rows route).

Tile sizes: every training launch (mnrf_field_forward_train, mnrf_field_backward[_planes], mnrf_field_backward2[_planes]) runs
the h2x tuning, 128 samples per workgroup (mnrf_field_split.hip launch_split with grad = true, s2 for the fp32 arithmetic);
the 192-sample kernels and their tile queue belong to the forward-only launches, so no B here is chosen for them.

Sample counts cross the boundaries of the GEMMs' work split: 32-sample stages, 128-sample tiles (and dw_small_kernel's
128-sample splits), dw_splits' 512 samples per split and its cap of 64 splits (B > 32768), dw_small_splits' cap of 2048
(B > 262144).  The bars are stated with their measured figures.

Trained weights amplify activation gradients on their way down the trunk: on the planes route a scaled gradient can outgrow the
f16 range of the planes (non-finite weight gradients), which training answers by lowering that module's gradient scale by 2^4
(mirror_nerf._lower_gradient_scale).  `_lowering_scale` does the same here, at most twice, and reports it."""
import ctypes

import pytest
import torch

from tests import torch_ref as TR
from tests.field_fp64 import DEV, F64, _rel, _rows_forward, _saved, _sec      # shared with tests/test_hip_forward_fp64.py

pytestmark = pytest.mark.gpu

LADDER = [1, 31, 32, 33, 127, 128, 129, 191, 192, 193, 511, 512, 513, 4096 + 77, 32769]
BIG = 262145          # dw_small_splits hits its cap of 2048 splits


@pytest.fixture(autouse=True, params=["split", "fp32"])
def precision(request):
    from mirror_nerf_amd import mirror_nerf as MN
    old = MN.PRECISION
    MN.set_precision(request.param)
    yield request.param
    MN.set_precision(old)


DY_L, DY_FIN, DY_DIR, DY_NRM1, DY_MIR1, DY_RGB, DY_NRM2, DY_MIR2 = 0, 2048, 2304, 2432, 2560, 2688, 2704, 2720


# ---------------------------------------------------------------------------------------------- weights and inputs
_MODELS = {}


def _model(kind):
    """("init": the seeded weights of test_hip_backward._field_setup; "trained": the fine model of fixture G11)."""
    import mirror_nerf_amd as M
    if kind not in _MODELS:
        if kind == "init":
            from tests.golden import weights as GW
            sd = GW.apply_tweaks(GW.make_state_dict(5, 1)[0], GW.OPAQUE)
        else:
            from tests.golden import fixtures as FX
            sd = FX.Fixture("g11_trained_grads_full").state_dicts()[1]
        m = M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=True)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        _MODELS[kind] = (m.to(DEV), {k: torch.from_numpy(v).to(DEV, F64) for k, v in sd.items()})
    return _MODELS[kind]


def _inputs(B, spr, seed):
    """spr = 0: xyz mode (B rows); else ray mode, B // spr rays of spr samples."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    if not spr:
        xyz = (torch.rand(B, 3, device=DEV, generator=g) * 6 - 3).contiguous()
        de = TR.embed(TR.l2n(torch.randn(B, 3, device=DEV, generator=g)), 4).contiguous()
        return dict(B=B, spr=1, xyz=xyz, rays=None, z=None, de=de)
    N = B // spr
    rays = torch.randn(N, 8, device=DEV, generator=g)
    rays[:, 3:6] = TR.l2n(rays[:, 3:6])
    z = (torch.sort(torch.rand(N, spr, device=DEV, generator=g) * 4 + 0.2, 1)[0]).contiguous()
    return dict(B=N * spr, spr=spr, xyz=None, rays=rays.contiguous(), z=z, de=TR.embed(rays[:, 3:6], 4).contiguous())


def _cots(B, profile, seed, normal=None):
    """Cotangents of sigma, rgb, pred_normal, is_mirror[, normal]: N(0,1), or per-sample magnitudes over 12 orders."""
    g = torch.Generator(device=DEV).manual_seed(seed + 1000)
    sc = torch.ones(B, device=DEV) if profile == "flat" else 10.0 ** (-12 * torch.rand(B, device=DEV, generator=g))
    c = [torch.randn(B, device=DEV, generator=g) * sc, torch.randn(B, 3, device=DEV, generator=g) * sc[:, None],
         torch.randn(B, 3, device=DEV, generator=g) * sc[:, None], torch.randn(B, device=DEV, generator=g) * sc]
    if normal is not None:
        c.append(normal)
    return c


def _kernel_masks(w64, saved, de64, tag=""):
    """Masks of the kernel's forward (from its saved post-activation values).  Asserted on the way: the saved activations
    are within 2e-5 of each section's largest entry of the float64 forward (measured 1.2e-6: the forward arithmetic's error,
    not only fp32 rounding of the values; it also pins the column order of every section), and every mask
    the kernel disagrees on sits at a near tie of the float64 pre-activation (|y| <= 1e-5 of the layer's largest)."""
    acts = {}
    with torch.no_grad():
        TR.field(w64, saved["enc"][:, :3], de64, acts=acts)
    worst = 0.0
    for k in ["enc"] + [f"h{i + 1}" for i in range(8)] + ["fin", "hd", "hn", "hm"]:
        e = _rel(saved[k], acts[k])
        worst = max(worst, e)
        assert e <= 2e-5, (k, e)
    assert _rel(saved["dire"][:, :27], de64) <= 1e-6
    post = {f"L{i + 1}": saved[f"h{i + 1}"] for i in range(8)}
    post.update(dir=saved["hd"], mir=saved["hm"])
    km = TR.masks_of(post)
    own = TR.masks_of({n: acts[n] for n in TR.MASK_NAMES})
    ties = 0
    for n in TR.MASK_NAMES:
        flip = km[n] != own[n]
        if bool(flip.any()):
            y = acts[n]
            far = float(y[flip].abs().max()) / float(y.abs().max())
            assert far <= 1e-5, (n, far)
            ties += int(flip.sum())
    print(f"MEAS forward{tag}: saved activations vs float64 {worst:.2e}, mask ties {ties}")
    return km


# ---------------------------------------------------------------------------------------------- the float64 reference
def _reference(w64, xyz64, de64, masks, cots, with_normal=False, cut_normal=False, cut_mirror=False, keep=None):
    """Gradients of sum(out . cot) through the masked float64 field: {param: grad}, dL/dxyz, dL/d(view encoding)."""
    wl = {k: v.clone().requires_grad_(True) for k, v in w64.items()}
    x = xyz64.clone().requires_grad_(True)
    d = de64.clone().requires_grad_(True)
    outs = TR.field(wl, x, d, with_normal=with_normal, cut_normal=cut_normal, cut_mirror=cut_mirror, keep_mirror=keep, masks=masks)
    loss = sum((o * c.to(F64)).sum() for o, c in zip(outs, cots) if c is not None)
    loss.backward()
    z = lambda v, t: v.grad if v.grad is not None else torch.zeros_like(t)  # noqa: E731   (a path that does not reach a leaf)
    return {k: z(v, v) for k, v in wl.items()}, z(x, x), z(d, d)


def _lowering_scale(model, step):
    """step() -> list of gradient tensors; on the split arithmetic, non-finite gradients (scaled activation gradients past the
    f16 range) lower the module's gradient scale by GRAD_SCALE_STEP bits and the step runs again, as training does."""
    from mirror_nerf_amd import mirror_nerf as MN
    model.__dict__["_mnrf_seed_reduction"] = 0
    try:
        while True:
            res = step()
            r = model.__dict__.get("_mnrf_seed_reduction", 0)
            flat = [t for t in res if t is not None]
            if all(bool(torch.isfinite(t).all()) for t in flat) or MN.precision_of(model) != "split" or r + MN.GRAD_SCALE_STEP > MN.GRAD_SCALE_MAX:
                if r:
                    print(f"MEAS gradient scale lowered by 2^{r}")
                return res
            model.__dict__["_mnrf_seed_reduction"] = r + MN.GRAD_SCALE_STEP
    finally:
        model.__dict__["_mnrf_seed_reduction"] = 0


def _kernel(model, inp, cots, want_normal=False, cut=0, keep=None):
    """FieldFn forward + backward: the 32 parameter gradients by name, dL/dxyz or dL/drays, dL/d(view encoding)."""
    names = [n for n, _ in model.named_parameters()]
    res = _lowering_scale(model, lambda: _kernel_once(model, inp, cots, want_normal, cut, keep))
    return dict(zip(names, res[:-2])), res[-2], res[-1]


def _kernel_once(model, inp, cots, want_normal, cut, keep):
    from mirror_nerf_amd.autograd import FieldFn
    params = list(model.parameters())
    for q in params:
        q.grad = None
    x = inp["xyz"].clone().requires_grad_(True) if inp["xyz"] is not None else None
    r = inp["rays"].clone().requires_grad_(True) if inp["rays"] is not None else None
    d = inp["de"].clone().requires_grad_(True)
    wn = (want_normal, cut, keep) if (cut or keep is not None) else want_normal
    got = FieldFn.apply(model, inp["spr"], x, r, inp["z"], d, wn, *params)
    sum((o * c).sum() for o, c in zip(got, cots) if c is not None).backward()
    return [q.grad for q in params] + [x.grad if x is not None else r.grad[:, :6], d.grad]


def _compare(got, ref, inp, tag, bar, mirror_bar=None):
    """Every gradient tensor against the reference, relative to the tensor's largest entry; returns the worst."""
    g, gx, gd = got
    r, rx, rd = ref
    B, spr = inp["B"], inp["spr"]
    if inp["rays"] is not None:       # x = o + d z: dL/do = sum_s dL/dx, dL/dd = sum_s z dL/dx; the view encoding per ray
        dx = rx.view(-1, spr, 3)
        rx = torch.cat([dx.sum(1), (dx * inp["z"].to(F64)[..., None]).sum(1)], 1)
        rd = rd.view(-1, spr, 27).sum(1)
    errs = [(_rel(g[n], r[n]), n) for n in r]
    errs += [(_rel(gx, rx), "d_xyz"), (_rel(gd[:, :27], rd), "d_view")]
    errs.sort(reverse=True)
    print(f"MEAS {tag}: worst {errs[0][0]:.2e} ({errs[0][1]})")
    bad = [e for e in errs if not e[0] <= (mirror_bar if mirror_bar and e[1].startswith("is_mirror_net.") else bar)]
    assert not bad, (tag, bad[:4])
    return errs[0][0]


def _run(kind, B, spr, profile, precision, bar, seed=0, with_normal=False, cut=0, keep_frac=None, normal_only=False, mirror_bar=None):
    model, w64 = _model(kind)
    inp = _inputs(B, spr, seed + B + spr)
    B = inp["B"]
    fw = _rows_forward(model, inp, precision == "split")
    saved = _saved(fw["sx"], B)
    de64 = inp["de"].to(F64).repeat_interleave(inp["spr"], 0)
    masks = _kernel_masks(w64, saved, de64)
    keep = None
    if keep_frac is not None:
        g = torch.Generator(device=DEV).manual_seed(seed + 7)
        keep = torch.rand(B, device=DEV, generator=g) < keep_frac
    gn = None
    if with_normal:
        g = torch.Generator(device=DEV).manual_seed(seed + 9)
        sc = torch.ones(B, device=DEV) if profile == "flat" else 10.0 ** (-8 * torch.rand(B, device=DEV, generator=g))
        gn = torch.randn(B, 3, device=DEV, generator=g) * sc[:, None]
    cots = _cots(B, profile, seed, gn)
    if normal_only:
        cots[:4] = [None] * 4
    from mirror_nerf_amd import _lib
    ref = _reference(w64, saved["enc"][:, :3], de64, masks, cots, with_normal=with_normal,
                     cut_normal=bool(cut & _lib.MNRF_CUT_NORMAL_HEAD), cut_mirror=bool(cut & _lib.MNRF_CUT_MIRROR_HEAD), keep=keep)
    got = _kernel(model, inp, cots, want_normal=with_normal, cut=cut, keep=None if keep is None else keep.float())
    mb = mirror_bar if (precision == "split" and kind == "trained") else None
    return _compare(got, ref, inp, f"{precision} {kind} B={B} spr={spr} {profile}", bar, mb)


# ================================================================ 2. the rows-route GEMMs in isolation
DW_C = 4e-6              # measured worst 1.06e-6 (fp32 arithmetic, B = 511); the ceiling is 2^-16


def _gemm_layers(saved, dy, g_sigma):
    X = saved
    enc = X["enc"]
    L = []
    for i in range(8):
        xi = enc if i == 0 else (torch.cat([enc, X["h4"]], 1) if i == 4 else X[f"h{i}"])
        L.append((i, dy(DY_L + 256 * i, 256), xi))
    L += [(8, dy(DY_FIN, 256), X["h8"]), (9, dy(DY_DIR, 128), torch.cat([X["fin"], X["dire"][:, :27]], 1)),
          (10, g_sigma[:, None], X["h8"]), (11, dy(DY_RGB, 16)[:, :3], X["hd"]), (12, dy(DY_NRM1, 128), X["h8"]),
          (13, dy(DY_NRM2, 16)[:, :3], X["hn"]), (14, dy(DY_MIR1, 128), X["h8"]), (15, dy(DY_MIR2, 16)[:, :1], X["hm"])]
    return L


def _gemm_case(B, precision):
    from mirror_nerf_amd import _lib
    from mirror_nerf_amd.weights import PARAM_NAMES, PARAM_SHAPES
    L, p = _lib.lib(), _lib.ptr
    model, _ = _model("init")
    inp = _inputs(B, 0, 3 * B + 1)
    split = precision == "split"
    fw = _rows_forward(model, inp, split)
    gs, grgb, gpn, gm = [c.contiguous() for c in _cots(B, "spread", B)]
    o = fw["out"]
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=DEV)  # noqa: E731
    ws = f(L.mnrf_train_workspace_floats(B))
    worst = 0.0
    for acc in (0, 1):
        gen = torch.Generator(device=DEV).manual_seed(B + 77)
        d = [torch.randn(*PARAM_SHAPES[n], device=DEV, generator=gen) for n in PARAM_NAMES]
        start = [t.clone() for t in d]
        flags = (_lib.MNRF_SPLIT_F16 if split else 0) | (_lib.MNRF_DW_ACCUMULATE if acc else 0)
        _lib.check(L.mnrf_field_backward(p(fw["packed"]), B, p(inp["xyz"]), 3, None, None, 1, p(gs), p(grgb), p(gpn), p(gm), p(o[1]),
                                         p(o[2]), p(o[3]), p(fw["sx"]), p(fw["sm"]), p(fw["si"]), p(ws),
                                         (ctypes.c_void_p * 32)(*[t.data_ptr() for t in d]), None, None, None, flags,
                                         _lib.stream()), "backward rows")
        torch.cuda.synchronize()
        dy = lambda off, w: _sec(ws, off, w, B).to(F64)  # noqa: E731
        for li, Y, X in _gemm_layers(_saved(fw["sx"], B), dy, gs.to(F64)):
            for kind, want, bound in ((0, Y.T @ X, Y.abs().T @ X.abs()), (1, Y.sum(0), Y.abs().sum(0))):
                n = PARAM_NAMES[2 * li + kind]
                got = d[2 * li + kind].to(F64).view(want.shape)
                if acc:       # added to the values the tensors held (one more fp32 rounding of the sum)
                    base = start[2 * li + kind].to(F64).view(want.shape)
                    want = want + base
                    err = (got - want).abs() - 2.0 ** -24 * want.abs()
                else:
                    err = (got - want).abs()
                zero = bound == 0
                assert bool((err[zero] <= 0).all()), (n, "entries without any contribution must be exact")
                r = float((err.clamp_min(0) / bound.clamp_min(1e-300))[~zero].max()) if bool((~zero).any()) else 0.0
                worst = max(worst, r)
                assert r <= DW_C, (n, B, acc, r)
    print(f"MEAS gemm {precision} B={B}: worst |dW - dW64| / sum|dY||X| = {worst:.2e}")
    return worst


@pytest.mark.parametrize("B", LADDER)
def test_rows_gemm_matches_float64_of_its_own_operands(B, precision):
    """mnrf_field_backward's weight gradients (dw_gemm_bf16p_kernel for the 128-wide tiles, dw_gemm_bf16_kernel<64/32> for
    the encoding and view columns, dw_small_kernel for the 1- and 3-row heads, dw_finish_kernel) against dY^T X and
    sum dY in float64 of the kernel's own operands (dY rows of the workspace, X rows of save_x), entry by entry within
    c * sum_s |dY_sn| |X_sk|; then the same launch with MNRF_DW_ACCUMULATE into tensors that hold random values."""
    _gemm_case(B, precision)


def test_rows_gemm_at_the_small_split_cap(precision):
    """B = 262145: dw_small_splits is capped at 2048 (ragged 129-sample splits), dw_splits at 64."""
    _gemm_case(BIG, precision)


# ================================================================ 3. end to end, first order
FIRST_BAR = 2e-5          # the ceiling; measured worst 1.86e-5 (fp32, trained, 4 rays x 33 samples, is_mirror_net.2.bias)
# DESIGN.md 6.1 "Accuracy of the per-sample seed scale": the split arithmetic scales all seeds of a sample by ONE power of two (mnrf_field_split_bwd.inc: 2^k * max seed in [2^6, 2^7)), so a
# head whose seed sits ~2^-20 below the sample's largest reaches its f16 hi/lo planes as subnormals.  On the trained pair the mirror
# probability saturates (1.4e-7 on some samples) and is_mirror_net.* can take their whole gradient from such seeds: at B = 1 that is
# 1.2e-2 (flat) and 2.7e-2 (spread cotangents) of the tensor's largest entry.  On the planes route with the trained weights the
# is_mirror_net.* tensors are held to MIRROR_SPLIT_BAR (measured 4.6e-5 at B = 4173, spread), at B = 1 to MIRROR_SPLIT_BAR_B1.
MIRROR_SPLIT_BAR = 1e-4
MIRROR_SPLIT_BAR_B1 = 0.1


SHAPES = [(1, 0), (129, 0), (513, 0), (4096 + 77, 0), (32769, 0), (33 * 4, 33), (33 * 125, 33), (64 * 2, 64), (64 * 513, 64)]


@pytest.mark.parametrize("kind", ["init", "trained"])
@pytest.mark.parametrize("B,spr", SHAPES)
@pytest.mark.parametrize("profile", ["flat", "spread"])
def test_field_backward_matches_float64(kind, profile, B, spr, precision):
    """All 32 parameter gradients, dL/dxyz (dL/drays in ray mode) and dL/d(view encoding) of FieldFn against the masked
    float64 reference, relative to each tensor's largest entry: <= FIRST_BAR (measured: 1.86e-5 fp32, 1.52e-5 split), except
    the split arithmetic's is_mirror_net.* on the trained pair (MIRROR_SPLIT_BAR, MIRROR_SPLIT_BAR_B1 at B = 1)."""
    _run(kind, B, spr, profile, precision, FIRST_BAR, mirror_bar=MIRROR_SPLIT_BAR_B1 if B == 1 else MIRROR_SPLIT_BAR)


@pytest.mark.parametrize("cut", ["normal", "mirror", "keep", "normal+keep"])
def test_field_backward_cut_heads_match_float64(cut, precision):
    """MNRF_CUT_NORMAL_HEAD / MNRF_CUT_MIRROR_HEAD and a per-row keep_mirror (the heads see geo_feat.detach()) on the trained
    pair at B = 4173, against the float64 reference with the same cuts: <= FIRST_BAR (measured 5.8e-6 split, 1.4e-6 fp32)."""
    from mirror_nerf_amd import _lib
    flags = (_lib.MNRF_CUT_NORMAL_HEAD if "normal" in cut else 0) | (_lib.MNRF_CUT_MIRROR_HEAD if "mirror" in cut else 0)
    _run("trained", 4096 + 77, 0, "flat", precision, FIRST_BAR, cut=flags, keep_frac=0.5 if "keep" in cut else None,
         mirror_bar=MIRROR_SPLIT_BAR)


# ================================================================ 4. sentinel samples
def _dw_splits(B):
    return min(64, max(1, -(-B // 512)))


def _pipelined_per(B, tiles=8 * 4 + 3 * 2):
    """Samples per split of dw_gemm_bf16p_kernel: mnrf_dw.hip dw_splits_rounds, rounded up to a 32-sample stage."""
    best, best_cost = 1, -1
    for sp in range(1, _dw_splits(B) + 1):
        cost = (sp * tiles + 255) // 256 * ((-(-B // sp) + 31) // 32 + 6)
        if best_cost < 0 or cost < best_cost:
            best, best_cost = sp, cost
    return (-(-B // best) + 31) // 32 * 32


def _sentinels(B):
    """First / last sample, both sides of the pipelined GEMM's split boundary (also a 32-sample stage boundary), of the phased
    GEMMs' split boundary, of a 128-sample tile (and of dw_small_kernel's 129-sample splits at the cap), inside the last partial
    32-sample block; then 31 | 32 and 511 | 512 while fewer than nine."""
    per = -(-B // _dw_splits(B))
    pp = _pipelined_per(B)
    small = -(-B // min(2048, max(1, -(-B // 128))))
    last = (B // 32) * 32 + (B % 32) // 2 if B % 32 else B - 17
    cand = [0, B - 1, pp - 1, pp, per - 1, per, small - 1, small, last, 31, 32, 511, 512]
    out = []
    for c in cand:
        if 0 <= c < B and c not in out and len(out) < 9:
            out.append(c)
    return sorted(out)


def _sentinel_case(B, precision):
    model, w64 = _model("init")       # (the trained pair's saturated mirror head: see MIRROR_SPLIT_BAR)
    inp = _inputs(B, 0, 11 * B)
    fw = _rows_forward(model, inp, precision == "split")
    pos = _sentinels(B)
    idx = torch.tensor(pos, device=DEV)
    saved = _saved(fw["sx"], B, idx)
    de64 = inp["de"].to(F64)[idx]
    masks = _kernel_masks(w64, saved, de64, f" sentinels B={B}")
    g = torch.Generator(device=DEV).manual_seed(B)
    full = [torch.zeros(B, device=DEV), torch.zeros(B, 3, device=DEV), torch.zeros(B, 3, device=DEV), torch.zeros(B, device=DEV)]
    mag = torch.tensor([2.0 ** -j for j in range(len(pos))], device=DEV)[torch.randperm(len(pos), generator=torch.Generator().manual_seed(B))
                                                                          .to(DEV)]
    for c in full:
        v = torch.randn(len(pos), *c.shape[1:], device=DEV, generator=g)
        c[idx] = v * mag.view(-1, *[1] * (c.dim() - 1))
    few = [c[idx] for c in full]
    r, rx, rd = _reference(w64, saved["enc"][:, :3], de64, masks, few)
    gp, gx, gd = _kernel(model, inp, full)
    dead = torch.ones(B, dtype=torch.bool, device=DEV)
    dead[idx] = False
    assert all(bool(torch.isfinite(t).all()) for t in gp.values())
    assert float(gx[dead].abs().max() if bool(dead.any()) else 0.0) == 0.0, "a zero-cotangent sample moved dL/dxyz"
    assert float(gd[dead].abs().max() if bool(dead.any()) else 0.0) == 0.0
    worst = _compare((gp, gx[idx], gd[idx]), (r, rx, rd), dict(B=len(pos), spr=1, rays=None), f"sentinels {precision} B={B}", FIRST_BAR)
    # sharpness: the reference without any single sentinel moves some tensor by >= 10 x the bar
    for j in range(len(pos)):
        only = [torch.zeros_like(c) for c in few]
        for a, c in zip(only, few):
            a[j] = c[j]
        rj, _, _ = _reference(w64, saved["enc"][:, :3], de64, masks, only)
        moved = max(float(rj[n].abs().max()) / max(float(r[n].abs().max()), 1e-300) for n in r)
        assert moved >= 10 * FIRST_BAR, (pos[j], moved)
    return worst


@pytest.mark.parametrize("B", LADDER)
def test_sentinel_samples(B, precision):
    """Cotangents exactly zero except on up to nine sentinel samples (_sentinels), of distinct power-of-two magnitudes
    2^0 .. 2^-8.  Every gradient matches the float64 reference of the sentinels alone, the
    zero-cotangent samples contribute exactly nothing, and dropping any one sentinel would move some tensor by >= 10 x
    the bar (asserted on the reference).  Seeded weights (the trained pair's saturated mirror head is covered above): <= FIRST_BAR,
    measured 1.87e-5 split, 2.6e-6 fp32.  (Whether a zero-cotangent sample adds exactly nothing to the WEIGHT gradients is
    pinned by the GEMM test: entries without any contribution must be exact.)"""
    _sentinel_case(B, precision)


def test_sentinel_samples_at_the_small_split_cap(precision):
    _sentinel_case(BIG, precision)


# ================================================================ 5. second order
# measured: split 8.0e-5 (seeded weights, B = 511, flat; xyz_encoding_1.0.weight: the small density-gradient signals b_i of these
# weights give 16 b subnormal low f16 halves, test_hip_backward.test_second_order_planes_route_agrees_with_rows_route), fp32 6.7e-6;
# the ceiling is 1e-4
SECOND_BAR = {"split": 1e-4, "fp32": 2e-5}


@pytest.mark.parametrize("profile", ["flat", "spread"])
@pytest.mark.parametrize("B", [1, 31, 32, 33, 127, 128, 129, 191, 192, 193, 511, 512, 513, 4096 + 77])
def test_second_order_matches_float64_double_backward(B, profile, precision):
    """The gradient through normal = l2n(-d sigma/d xyz) alone (mnrf_field_backward2 on the rows route,
    mnrf_field_backward2_planes + mnrf_dw_planes2 kind 1 on the planes route) against float64 double backward through the
    masked reference; g_normal N(0,1) or spread over 8 orders.  Bars: SECOND_BAR."""
    _run("init", B, 0, profile, precision, SECOND_BAR[precision], seed=5, with_normal=True, normal_only=True)


@pytest.mark.parametrize("kind", ["init", "trained"])
@pytest.mark.parametrize("B,spr", [(4096 + 77, 0), (64 * 65, 64)])
def test_first_and_second_order_together_match_float64(kind, B, spr, precision):
    """Both orders in one backward (kind 0 and kind 1 entries on one tape), spread cotangents (measured: split 5.1e-5, fp32
    3.8e-6; on the trained pair the planes route's gradient scale is lowered once, see the module docstring)."""
    _run(kind, B, spr, "spread", precision, {"split": 1e-4, "fp32": 1.5e-5}[precision], seed=6, with_normal=True,
         mirror_bar=MIRROR_SPLIT_BAR)


# ================================================================ 6. many evaluations of one module
def test_many_evaluations_of_one_module(precision):
    """Ten evaluations of one module in one backward pass (more than the 8 per mnrf_dw_planes2 call: the tape is contracted in
    two groups, the second accumulating into the first), ragged sizes, first- and second-order entries mixed, one evaluation
    whose rows are all dead (n_live = 0; planes route only: a live row count needs it), and a weight regulariser adding to
    .grad: the float64 sum of the evaluations' references (measured: split 8.2e-6 after one lowering of the gradient scale,
    fp32 6.5e-6)."""
    from mirror_nerf_amd.autograd import FieldFn
    model, w64 = _model("trained")
    evals = [(1, False), (31, True), (33, False), (200, True), (4096 + 77, False), (1, True), (31, False), (33, True), (200, False),
             (4096 + 77, True)]
    params = list(model.parameters())
    names = [n for n, _ in model.named_parameters()]
    ref = {n: 2e-2 * w64[n] for n in names}
    runs = []
    for e, (B, wn) in enumerate(evals):
        inp = _inputs(B, 0, 100 + e)
        saved = _saved(_rows_forward(model, inp, precision == "split")["sx"], B)
        masks = _kernel_masks(w64, saved, inp["de"].to(F64), f" eval {e}")
        cots = _cots(B, "flat", 200 + e, torch.randn(B, 3, device=DEV) if wn else None)
        r, _, _ = _reference(w64, saved["enc"][:, :3], inp["de"].to(F64), masks, cots, with_normal=wn)
        for n in names:
            ref[n] = ref[n] + r[n]
        runs.append((inp, wn, cots))
    dead = _inputs(64, 0, 99)

    def step():
        for q in params:
            q.grad = None
        loss = 1e-2 * sum((q ** 2).sum() for q in params)
        for inp, wn, cots in runs:
            got = FieldFn.apply(model, 1, inp["xyz"], None, None, inp["de"], wn, *params)
            loss = loss + sum((o * c).sum() for o, c in zip(got, cots) if c is not None)
        if precision == "split":       # no live rows: the cotangents reach the launch, the samples must contribute nothing
            nl = torch.zeros(1, dtype=torch.int32, device=DEV)
            got = FieldFn.apply(model, 1, dead["xyz"], None, None, dead["de"], (False, 0, None, nl), *params)
            loss = loss + sum((torch.nan_to_num(o) * c).sum() for o, c in zip(got, _cots(64, "flat", 300)))
        loss.backward()
        return [q.grad for q in params]

    grads = _lowering_scale(model, step)
    errs = sorted(((_rel(g, ref[n]), n) for n, g in zip(names, grads)), reverse=True)
    print(f"MEAS many evaluations {precision}: worst {errs[0][0]:.2e} ({errs[0][1]})")
    assert errs[0][0] <= {"split": 3e-5, "fp32": 2.5e-5}[precision], errs[:4]
