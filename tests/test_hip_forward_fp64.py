"""The forward-only field kernels -- mnrf_field_forward in every tuning (fp32: s2, and s1 with the density-gradient normal;
split-f16: h3 = 48 samples per wave / 192 per workgroup on the folded stream and sigma-only, h2 when geo_feat is asked for, h2x
with the density-gradient normal) and the four ray-fused launches behind mnrf_field_composite_fused[_pn] -- against a float64
reference of the same function: tests/torch_ref.py `field` and `composite`, evaluated at the kernel's own fp32 inputs.

The rule of every comparison: with K the kernel's output, R64 the float64 reference and R32 the same torch_ref function in plain
fp32 torch (no reduced-precision matmul),
    err(K, R64) <= max(project bar, 4 x err(R32, R64))
where the project bars are the ones the suite already holds these outputs to (tests/test_hip_parity.py, tests/golden/fixtures.py
`tolerance`, whose factor 4 this is): sigma 2e-5 x max(1, max |sigma|), pred_normal 2e-5, rgb and is_mirror 1e-5, geo_feat
2e-5 x max(1, largest entry), the density-gradient normal 1e-4 away from ReLU ties; composited maps and weights 1e-4, depth and
x_surface 8e-4.  Each case prints a MEAS line with both errors of every output.

Sample counts cross a wave and a workgroup of every tuning (16-sample groups; 32 / 48 samples per wave; 64 / 128 / 192 per
workgroup) and, for the 192-sample kernels, the point where the launch stops being a static grid and becomes one resident
workgroup per CU that draws tiles from a queue (192 x CUs samples; CUs rays for the ray-fused launches).  Every output buffer
ends in a guard row that must keep its sentinel, and the range-guard word of the weight image must stay 0.

Measured (MI355X; worst err(K, R64) | worst err(R32, R64) over all cases of this file):
  (sigma and geo_feat are absolute figures; the largest |sigma| is 155, on the trained model, where the worst ones arise)
  tuning            output       err(K, R64)  err(R32, R64)
  s2                sigma          7.8e-05      9.7e-05
  s2                rgb            5.0e-06      4.0e-06
  s2                pred_normal    2.8e-06      3.1e-06
  s2                is_mirror      2.7e-06      3.1e-06
  s2 (geo_feat)     geo_feat       1.5e-05      2.3e-05
  s1                sigma          6.5e-05      5.6e-05
  s1                rgb            3.5e-06      3.1e-06
  s1                pred_normal    2.8e-06      3.1e-06
  s1                is_mirror      1.9e-06      1.7e-06
  s1                normal         1.0e-05      1.1e-05
  h3, h3 sigma-only sigma          1.9e-04      9.7e-05
  h3                rgb            9.0e-06      4.0e-06
  h3                pred_normal    6.1e-06      3.1e-06
  h3                is_mirror      5.0e-06      3.1e-06
  h2                sigma          9.7e-05      5.0e-05
  h2                rgb            4.2e-06      3.1e-06
  h2                pred_normal    6.1e-06      3.1e-06
  h2                is_mirror      5.0e-06      1.7e-06
  h2                geo_feat       2.9e-05      2.3e-05
  h2x               sigma          1.5e-04      5.6e-05
  h2x               rgb            5.2e-06      3.1e-06
  h2x               pred_normal    4.8e-06      3.1e-06
  h2x               is_mirror      5.0e-06      1.7e-06
  h2x               normal         6.1e-05      1.1e-05
  absent heads and fewer bands (seeded weights), worst of s2 / h3 / h2: sigma 1.3e-06 | 4.4e-07, rgb 7.2e-08 | 5.9e-08,
      pred_normal 1.3e-06 | 2.7e-07, is_mirror 6.3e-08 | 5.7e-08, geo_feat 1.1e-07 | 4.5e-08
  fused plain, pn   weights 2.4e-06 | 2.7e-06, opacity 9.9e-07 | 6.8e-07, rgb 8.9e-07 | 6.3e-07, mask 1.4e-06 | 4.0e-07,
                    sn 9.7e-07 | 6.5e-07, depth 5.4e-06 | 3.5e-06, xs 5.2e-06 | 3.3e-06, pred_normal (pn) 7.5e-07 | 3.0e-07
  fused rgb_depth,  weights 1.9e-07 | 5.4e-08, opacity 1.2e-07 | 1.8e-07, rgb 1.7e-07 | 2.2e-07, mask 1.4e-06 | 1.4e-07,
  blended           sn 2.7e-07 | 1.9e-07, depth 3.5e-07 | 6.2e-07, xs 4.6e-07 | 5.9e-07   (straddling model only)
  two kernels (s2)  weights 1.7e-06 | 2.7e-06, opacity 3.3e-07 | 6.8e-07, rgb 5.1e-07 | 6.3e-07, mask 4.0e-07 | 4.0e-07,
                    sn 3.4e-07 | 6.5e-07, depth 1.7e-06 | 3.5e-06, xs 1.6e-06 | 3.3e-06
  saved sin / cos against float64 over |x| < 64: split 1.05e-07, fp32 6.6e-08
  density-gradient normal, samples left out as ReLU ties at B = 4096: init 6.9 %, straddle 6.7 %, trained 12.0 %
No ray of the blended-level cases lies within 1e-4 of 0.5; no case misses its bar.
"""
import contextlib

import pytest
import torch

from tests import field_fp64 as FC
from tests import torch_ref as TR
from tests.field_fp64 import DEV, ENCPOS, F64, SEC_ENC, _rows_forward, _sec

pytestmark = pytest.mark.gpu

LADDER = [1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 127, 128, 129, 191, 192, 193, 383, 384, 385, 1000]
SENTINEL = 1234.5
TUNING = {("fp32", "full"): "s2", ("fp32", "sigma"): "s2 sigma-only", ("fp32", "geo"): "s2 geo_feat", ("fp32", "grad"): "s1",
          ("split", "full"): "h3", ("split", "sigma"): "h3 sigma-only", ("split", "geo"): "h2", ("split", "grad"): "h2x"}
VARIANTS = ("full", "sigma", "geo", "grad")
# project bars: (absolute bar, relative to max(1, largest |R64|)?)
BARS = {"sigma": (2e-5, True), "pred_normal": (2e-5, False), "rgb": (1e-5, False), "is_mirror": (1e-5, False), "geo_feat": (2e-5, True),
        "normal": (1e-4, False)}
MAP_BARS = {"weights": 1e-4, "opacity": 1e-4, "rgb": 1e-4, "mask": 1e-4, "sn": 1e-4, "depth": 8e-4, "xs": 8e-4}
WORST = {}


@pytest.fixture(autouse=True, params=["split", "fp32"])
def precision(request):
    from mirror_nerf_amd import mirror_nerf as MN
    old = MN.PRECISION
    MN.set_precision(request.param)
    yield request.param
    MN.set_precision(old)


@pytest.fixture(autouse=True, scope="module")
def _worst_table():
    yield
    for (tuning, name), (ek, er) in sorted(WORST.items()):
        print(f"MEAS worst | {tuning} | {name} | {ek:.2e} | {er:.2e}")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@contextlib.contextmanager
def _plain_fp32():
    """fp32 torch without any reduced-precision matmul."""
    old = torch.backends.cuda.matmul.allow_tf32, torch.get_float32_matmul_precision()
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")
    try:
        yield
    finally:
        torch.backends.cuda.matmul.allow_tf32 = old[0]
        torch.set_float32_matmul_precision(old[1])


# ---------------------------------------------------------------------------------------------- models and references
_MODELS = {}


def _model(kind):
    """(module on the device, float64 weights, fp32 weights, position bands, view bands)"""
    import mirror_nerf_amd as M
    if kind not in _MODELS:
        sd = FC.state_dict(kind)
        nb, nd = FC.bands(kind)
        m = M.MirrorNeRF(in_channels_xyz=3 + 6 * nb, in_channels_dir=3 + 6 * nd, predict_normal="normal_net.0.weight" in sd,
                         predict_mirror_mask="is_mirror_net.0.weight" in sd)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        _MODELS[kind] = (m.to(DEV), FC.weights(kind, F64, DEV), FC.weights(kind, torch.float32, DEV), nb, nd)
    return _MODELS[kind]


def _eval(w, x, de, nb, want_normal, chunk=16384):
    """TR.field in the dtype of its arguments: {sigma, rgb, pred_normal, is_mirror, geo_feat[, normal, near]} (absent heads:
    None).  near (B,) bool: some unit of L1..L8 has a pre-activation within 1e-5 of its layer's largest magnitude."""
    parts = []
    for i in range(0, x.shape[0], x.shape[0] if want_normal else chunk):
        j = x.shape[0] if want_normal else min(x.shape[0], i + chunk)
        acts = {}
        with torch.enable_grad() if want_normal else torch.no_grad():
            res = TR.field(w, x[i:j].clone(), de[i:j], with_normal=want_normal, acts=acts, n_bands=nb)
        d = dict(sigma=res[0], rgb=res[1], pred_normal=res[2], is_mirror=res[3], geo_feat=acts["h8"])
        if want_normal:
            d["normal"] = res[4]
            pre = torch.stack([acts[f"L{k + 1}"].detach().abs().amin(1) for k in range(8)], 1)
            top = torch.stack([acts[f"L{k + 1}"].detach().abs().max() for k in range(8)])
            d["near"] = (pre <= 1e-5 * top[None]).any(1)
        parts.append({k: (None if v is None else v.detach()) for k, v in d.items()})
    return {k: (None if parts[0][k] is None else torch.cat([p[k] for p in parts])) for k in parts[0]}


_REFS = {}


def _refs(key, kind, x32, de32, want_normal=False):
    """R64 and R32 of a set of samples (fp32 positions (N, 3) and view encodings (N, 3 + 6 nd) on the device), computed once per
    `key` and never written to afterwards."""
    key = (key, want_normal)
    if key not in _REFS:
        _m, w64, w32, nb, _nd = _model(kind)
        r64 = _eval(w64, x32.double(), de32.double(), nb, want_normal)
        with _plain_fp32():
            r32 = _eval(w32, x32, de32, nb, want_normal)
        _REFS[key] = (r64, r32)
    return _REFS[key]


# ---------------------------------------------------------------------------------------------- the launch under test
def _guard(model):
    from mirror_nerf_amd.weights import folded_of
    return int(folded_of(model)[-1:].view(torch.int32).item())


def _launch(model, variant, precision, B, xyz=None, xyz_stride=3, rays=None, z=None, spr=1, de=None, dir_stride=27):
    """mnrf_field_forward of a tuning on B samples.  Every output buffer holds one row more than B, filled with a sentinel that
    must survive; after a split launch the guard word of the image must be 0.  Returns {name: (B, ...) tensor}."""
    from mirror_nerf_amd import _lib
    from mirror_nerf_amd.weights import folded_of
    L, p = _lib.lib(), _lib.ptr
    widths = {"sigma": 1}
    if variant != "sigma":
        widths["rgb"] = 3
        if model.predict_normal:
            widths["pred_normal"] = 3
        if model.predict_mirror_mask:
            widths["is_mirror"] = 1
    if variant == "grad":
        widths["normal"] = 3
    if variant == "geo":
        widths["geo_feat"] = 256
    o = {k: torch.full((B + 1, w), SENTINEL, device=DEV) for k, w in widths.items()}
    flags = (_lib.MNRF_SPLIT_F16 if precision == "split" else 0) | (_lib.MNRF_SIGMA_ONLY if variant == "sigma" else 0) | \
        (_lib.MNRF_GRAD_NORMAL if variant == "grad" else 0)
    image = folded_of(model)
    _lib.check(L.mnrf_field_forward(p(image), flags, B, p(xyz), xyz_stride, p(rays), p(z), spr, None if variant == "sigma" else p(de),
                                    dir_stride, p(o["sigma"]), p(o.get("rgb")), p(o.get("pred_normal")), p(o.get("is_mirror")),
                                    p(o.get("normal")), p(o.get("geo_feat")), _lib.stream()), "mnrf_field_forward")
    torch.cuda.synchronize()
    for k, t in o.items():
        assert bool((t[B] == SENTINEL).all()), (k, "the guard row behind B was written")
    if precision == "split":
        assert _guard(model) == 0, "range guard"
    return {k: (t[:B, 0] if widths[k] == 1 else t[:B]) for k, t in o.items()}


def _measure(tuning, got, r64, r32, rows, keep=None):
    """[(name, err(K, R64), err(R32, R64), bar)] of the outputs of a launch over the reference rows `rows` (normal: over the kept
    rows); the bar is max(project bar, 4 x err(R32, R64))."""
    out = []
    for name, k in got.items():
        a, b = r64[name][rows], r32[name][rows].double()
        k = k.double()
        if name == "normal":
            sel = keep[rows]
            k, a, b = k[sel], a[sel], b[sel]
        if not a.numel():
            continue
        bar, relative = BARS[name]
        if relative:
            bar *= max(1.0, float(a.abs().max()))
        ek, er = float((k - a).abs().max()), float((b - a).abs().max())
        ek = float("inf") if ek != ek else ek
        out.append((name, ek, er, max(bar, 4 * er)))
        w = WORST.get((tuning, name), (0.0, 0.0))
        WORST[(tuning, name)] = (max(w[0], ek), max(w[1], er))
    return out


def _report(tag, res, bad):
    print(f"MEAS {tag}: " + ", ".join(f"{n} {ek:.2e} (fp32 torch {er:.2e}, bar {bar:.1e})" for n, ek, er, bar in res))
    bad += [(tag, n, ek, bar) for n, ek, _er, bar in res if not ek <= bar]


# ================================================================ 1. mnrf_field_forward, xyz mode, every tuning
CLOUDS = [("init", "box"), ("straddle", "box"), ("trained", "box"), ("init", "wide"), ("straddle", "wide")]
N_LADDER = 1000


def _cloud(kind, which, n):
    """Positions, view encodings (27 wide, the absent bands of the model as zeros; the leading 3 + 6 nd columns are what the
    reference takes) of the first n samples of the cloud, on the device."""
    import mirror_nerf_amd as M
    nd = _model(kind)[4]
    xyz, d = FC.cloud(kind if kind in ("init", "straddle", "trained") else "init", which, n)
    xyz, d = xyz.to(DEV), d.to(DEV)
    de = M.Embedding(nd)(d.contiguous())
    de27 = torch.cat([de, torch.zeros(n, 27 - de.shape[1], device=DEV)], 1).contiguous()
    return xyz.contiguous(), de27, de


def _xyz_case(kind, which, variant, precision, sizes, n_ref, want_normal_ref):
    model = _model(kind)[0]
    xyz, de27, de = _cloud(kind, which, n_ref)
    r64, r32 = _refs(("cloud", kind, which, n_ref), kind, xyz, de, want_normal_ref)
    tuning = TUNING[(precision, variant)]
    bad = []
    for B in sizes:
        got = _launch(model, variant, precision, B, xyz=xyz, de=de27)
        res = _measure(tuning, got, r64, r32, slice(0, B), r64.get("near") is not None and ~r64["near"])
        _report(f"{tuning} {kind} {which} B={B}", res, bad)
    assert not bad, bad


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("kind,which", CLOUDS)
def test_field_forward_matches_float64_across_wave_and_workgroup_edges(kind, which, variant, precision):
    """Every tuning at B = 1 .. 1000 across the edges of 16-sample groups, waves and workgroups, on the seeded, the straddling
    and the trained model in their boxes, and on the seeded models out to |x| <= 63.9 (the range the split kernels claim)."""
    _xyz_case(kind, which, variant, precision, LADDER, N_LADDER, variant == "grad")


@pytest.mark.parametrize("variant", ["full", "sigma"])
@pytest.mark.parametrize("kind", ["init", "straddle", "trained"])
def test_field_forward_matches_float64_across_the_queue_seam(kind, variant, precision):
    """192 x CUs samples is where a launch of the 192-sample kernels (h3) turns from a static grid into one resident workgroup
    per CU that draws further tiles from a queue: one tile less, exactly, one sample more, and a ragged launch of 2 CUs + 5
    tiles in which workgroups take a second and a third tile.  (The fp32 arithmetic runs the same sizes on s2.)"""
    c = _cus()
    sizes = [192 * c - 1, 192 * c, 192 * c + 1, 192 * (2 * c + 5) - 7]
    _xyz_case(kind, "box", variant, precision, sizes, 192 * (2 * c + 5), False)


# ================================================================ 2. ray mode
@pytest.mark.parametrize("n_rays", [1, 7])
@pytest.mark.parametrize("spr", FC.RAY_SPR)
def test_ray_mode_matches_float64(spr, n_rays, precision):
    """Positions formed in the kernel as o + d z, one view-encoding row per ray (row = sample / spr), tiles that span rays and a
    ragged last tile.  The reference forms the positions in fp32 torch with a separate multiply and add.  On this model a view
    row taken from the neighbouring ray moves rgb by >= 1e-3 (tests/test_torch_ref_cpu.py)."""
    import mirror_nerf_amd as M
    kind = FC.RAY_MODEL
    model = _model(kind)[0]
    rays, z = [t.to(DEV) for t in FC.ray_inputs(n_rays, spr)]
    de = M.Embedding(4)(rays[:, 3:6].contiguous()).contiguous()
    x = FC.ray_positions(rays, z).contiguous()
    B = n_rays * spr
    bad = []
    for variant in VARIANTS:
        r64, r32 = _refs(("rays", spr, n_rays), kind, x, de.repeat_interleave(spr, 0), variant == "grad")
        got = _launch(model, variant, precision, B, rays=rays, z=z, spr=spr, de=de)
        tuning = TUNING[(precision, variant)]
        res = _measure(tuning, got, r64, r32, slice(0, B), r64.get("near") is not None and ~r64["near"])
        _report(f"{tuning} rays {n_rays} x {spr}", res, bad)
    assert not bad, bad


# ================================================================ 3. strides and layouts
@pytest.mark.parametrize("dir_stride", [27, 28, 30])
@pytest.mark.parametrize("xyz_stride", [3, 4, 30])
def test_strided_inputs_equal_the_dense_call_and_match_float64(xyz_stride, dir_stride, precision):
    """Rows xyz_stride / dir_stride floats apart with NaN in the padding: the outputs of the dense call bit for bit."""
    B = 385
    kind = "init"
    model = _model(kind)[0]
    xyz, de27, de = _cloud(kind, "box", N_LADDER)
    r64, r32 = _refs(("cloud", kind, "box", N_LADDER), kind, xyz, de, True)
    xs = torch.full((B, xyz_stride), float("nan"), device=DEV)
    xs[:, :3] = xyz[:B]
    ds = torch.full((B, dir_stride), float("nan"), device=DEV)
    ds[:, :27] = de27[:B]
    bad = []
    for variant in VARIANTS:
        dense = _launch(model, variant, precision, B, xyz=xyz, de=de27)
        got = _launch(model, variant, precision, B, xyz=xs, xyz_stride=xyz_stride, de=ds, dir_stride=dir_stride)
        for k in dense:
            assert torch.equal(got[k], dense[k]), (variant, k)
        tuning = TUNING[(precision, variant)]
        _report(f"{tuning} strides {xyz_stride}/{dir_stride}", _measure(tuning, got, r64, r32, slice(0, B), ~r64["near"]), bad)
    assert not bad, bad


# ================================================================ 4. absent heads and reduced encodings
@pytest.mark.parametrize("variant", ["full", "geo"])
@pytest.mark.parametrize("kind", ["no_normal", "no_mirror", "no_heads", "bands_6_2", "bands_0_0"])
def test_absent_heads_and_fewer_bands_match_float64(kind, variant, precision):
    """Models without normal_net, is_mirror_net or both (their outputs are not requested), MirrorNeRF(39, 15) and
    MirrorNeRF(3, 3) (the weight columns of the absent bands are packed as zeros), on h3, h2 and s2 against the reference with
    that many bands and heads."""
    model = _model(kind)[0]
    sd = FC.state_dict(kind)
    assert model.predict_normal == ("normal_net.0.weight" in sd) and model.predict_mirror_mask == ("is_mirror_net.0.weight" in sd)
    xyz, de27, de = _cloud(kind, "box", 385)
    assert de.shape[1] == 3 + 6 * FC.bands(kind)[1]
    r64, r32 = _refs(("cloud", kind, "box", 385), kind, xyz, de)
    tuning = TUNING[(precision, variant)]
    bad = []
    for B in (1, 47, 49, 191, 193, 385):
        got = _launch(model, variant, precision, B, xyz=xyz, de=de27)
        assert ("pred_normal" in got) == model.predict_normal and ("is_mirror" in got) == model.predict_mirror_mask
        _report(f"{tuning} {kind} B={B}", _measure(tuning + " (" + kind + ")", got, r64, r32, slice(0, B)), bad)
    assert not bad, bad


# ================================================================ 5. density-gradient normal
LEFT_OUT = {}


@pytest.mark.parametrize("kind", ["init", "straddle", "trained"])
def test_density_gradient_normal_matches_float64_autograd(kind, precision):
    """normal = l2n(-d sigma / dx) of h2x / s1 against float64 autograd at B = 4096.  Left out: samples where a unit of L1..L8 has
    a float64 pre-activation within 1e-5 of its layer's largest magnitude (the kernel may take the other piece there): at most
    20 % -- a condition on the reference, which gives 7 % (init, straddle) and 15 % (trained)."""
    B = 4096
    model = _model(kind)[0]
    xyz, de27, de = _cloud(kind, "box", B)
    r64, r32 = _refs(("cloud", kind, "box", B), kind, xyz, de, True)
    out = float(r64["near"].float().mean())
    LEFT_OUT[kind] = out
    print(f"MEAS normal {kind}: {100 * out:.1f} % of the samples left out")
    assert out <= 0.20, out
    got = _launch(model, "grad", precision, B, xyz=xyz, de=de27)
    tuning = TUNING[(precision, "grad")]
    bad = []
    _report(f"{tuning} {kind} B={B}", _measure(tuning, got, r64, r32, slice(0, B), ~r64["near"]), bad)
    assert not bad, bad


# ================================================================ 6. ray-fused launches
def _fused_refs(kind, n_max):
    """R64 / R32 of the field on the samples of the first n_max rays of FC.fused_inputs, per sample, and those inputs."""
    import mirror_nerf_amd as M
    key = ("fused", kind, n_max)
    if key not in _REFS:
        rays, z = [t.to(DEV) for t in FC.fused_inputs(n_max)]
        de = M.Embedding(4)(rays[:, 3:6].contiguous()).contiguous()
        x = FC.ray_positions(rays, z).contiguous()
        _REFS[key] = (rays, z, de) + _refs(("fused samples", kind, n_max), kind, x, de.repeat_interleave(192, 0))
    return _REFS[key]


def _composited(r, rays, z, n, white):
    S = z.shape[1]
    v = lambda t, *s: t[:n * S].view(n, S, *s)  # noqa: E731
    return TR.composite(rays[:n].to(r["sigma"].dtype), v(r["sigma"]), z[:n].to(r["sigma"].dtype), None, v(r["rgb"], 3), v(r["is_mirror"]),
                        v(r["pred_normal"], 3), None, bool(white))


def _fused_launch(model, rays, z, de, flags, which):
    """A ray-fused launch with guard rows behind every map: {weights, opacity, rgb, depth, mask, sn, xs[, pred_normal]}."""
    from mirror_nerf_amd import _lib
    from mirror_nerf_amd.weights import folded_of
    L, p = _lib.lib(), _lib.ptr
    n, spr = z.shape
    w = {"weights": spr, "opacity": 1, "rgb": 3, "depth": 1, "xs": 3}
    if which != "rgb_depth":
        w.update(mask=1, sn=3)
    o = {k: torch.full((n + 1, c), SENTINEL, device=DEV) for k, c in w.items()}
    if which == "pn":
        o["pred_normal"] = torch.full((n + 1, spr, 3), SENTINEL, device=DEV)
    head = (p(folded_of(model)), n, p(rays), p(z), p(de), 27, flags, p(o["weights"]), p(o["opacity"]), p(o["rgb"]), p(o["depth"]),
            p(o.get("mask")), p(o.get("sn")), p(o["xs"]))
    if which == "pn":
        _lib.check(L.mnrf_field_composite_fused_pn(*head, p(o["pred_normal"]), _lib.stream()), "mnrf_field_composite_fused_pn")
    else:
        _lib.check(L.mnrf_field_composite_fused(*head, _lib.stream()), "mnrf_field_composite_fused")
    torch.cuda.synchronize()
    for k, t in o.items():
        assert bool((t[n] == SENTINEL).all()), (k, "the guard row behind the last ray was written")
    assert _guard(model) == 0, "range guard"
    return {k: (t[:n, 0] if t.dim() == 2 and t.shape[1] == 1 else t[:n]) for k, t in o.items()}


def _two_kernels(model, precision, rays, z, de, white):
    """mnrf_field_forward on the rays' samples, then mnrf_composite: the maps under the names of _fused_launch."""
    from mirror_nerf_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    n, spr = z.shape
    f = _launch(model, "full", precision, n * spr, rays=rays, z=z, spr=spr, de=de)
    o = {k: torch.empty(n, c, device=DEV) for k, c in dict(weights=spr, opacity=1, rgb=3, depth=1, mask=1, sn=3, xs=3).items()}
    _lib.check(L.mnrf_composite(p(rays), n, spr, p(f["sigma"].contiguous()), p(z), None, p(f["rgb"]), p(f["is_mirror"].contiguous()),
                                p(f["pred_normal"]), None, int(white), p(o["weights"]), p(o["opacity"]), p(o["rgb"]), p(o["depth"]),
                                p(o["mask"]), p(o["sn"]), None, None, p(o["xs"]), _lib.stream()), "mnrf_composite")
    torch.cuda.synchronize()
    out = {k: (t[:, 0] if t.shape[1] == 1 else t) for k, t in o.items()}
    out["pred_normal"] = f["pred_normal"].view(n, spr, 3)
    return out


def _ray_counts():
    c = _cus()
    return [1, 2, 3, c - 1, c, c + 1, 2 * c + 7]


@pytest.mark.parametrize("white", [0, 1])
@pytest.mark.parametrize("kind,which", [("straddle", "plain"), ("straddle", "rgb_depth"), ("straddle", "blended"), ("straddle", "pn"),
                                        ("trained", "plain"), ("trained", "pn")])
def test_ray_fused_launches_match_float64_compositing(kind, which, white, precision):
    """The maps of every ray-fused launch against TR.composite in float64 of the float64 field, at ray counts below, at and above
    the CU count (static grid | tile queue: workgroups that composite a second and a third ray from the LDS slots of the first)
    and both backgrounds.  The plain launch equals mnrf_field_forward + mnrf_composite bit for bit at every count.  Blended level:
    the rays whose float64 mirror value is not below 0.5 have rgb exactly 0; rays within 1e-4 of 0.5 are left out of the rgb
    comparison (at most 2 %).  Under the fp32 arithmetic the two-kernel path is what a level runs: it is held to the same
    reference; the fused launches are split-f16 kernels."""
    from mirror_nerf_amd import _lib
    if precision == "fp32" and which != "plain":
        pytest.skip("the ray-fused launches are split-f16 kernels; the fp32 two-kernel path runs as `plain`")
    model = _model(kind)[0]
    counts = _ray_counts()
    rays, z, de, r64, r32 = _fused_refs(kind, counts[-1])
    flags = white | {"plain": 0, "pn": 0, "rgb_depth": _lib.MNRF_FUSED_RGB_DEPTH, "blended": _lib.MNRF_FUSED_BLENDED_LEVEL}[which]
    tuning = "two kernels (s2)" if precision == "fp32" else "fused " + which
    bad = []
    for n in counts:
        ra, zn, den = rays[:n].contiguous(), z[:n].contiguous(), de[:n].contiguous()
        c64, c32 = _composited(r64, rays, z, n, white), _composited(r32, rays, z, n, white)
        two = _two_kernels(model, precision, ra, zn, den, white)
        got = two if precision == "fp32" else _fused_launch(model, ra, zn, den, flags, which)
        if which in ("plain", "pn") and precision == "split":
            for k in got:
                assert torch.equal(got[k], two[k]), (n, k, "the fused launch differs from field_forward + mnrf_composite")
        res = []
        for k, bar in MAP_BARS.items():
            if k not in got:
                continue
            a, b, g = c64[k], c32[k].double(), got[k].double()
            if which == "blended" and k == "rgb":
                m64 = c64["mask"]
                fence = (m64 - 0.5).abs() <= 1e-4
                assert float(fence.float().mean()) <= 0.02, (n, "rays on the fence")
                above = (m64 >= 0.5) & ~fence
                assert bool((got["rgb"][above] == 0).all()), (n, "a ray the blend discards has a colour")
                a, b, g = a[~above & ~fence], b[~above & ~fence], g[~above & ~fence]
                if n == counts[-1]:
                    assert 0 < int(above.sum()) < n, "both kinds of ray in one launch"
            if not a.numel():
                continue
            ek, er = float((g - a).abs().max()), float((b - a).abs().max())
            ek = float("inf") if ek != ek else ek
            res.append((k, ek, er, max(bar, 4 * er)))
            w = WORST.get((tuning, k), (0.0, 0.0))
            WORST[(tuning, k)] = (max(w[0], ek), max(w[1], er))
        if "pred_normal" in got:
            res += _measure(tuning, {"pred_normal": got["pred_normal"].reshape(-1, 3)}, r64, r32, slice(0, n * 192))
        _report(f"{tuning} {kind} rays={n} white={white}", res, bad)
    assert not bad, bad


# ================================================================ 7. the encoding the GPU computes
def test_saved_encoding_matches_float64_sin_cos_over_the_claimed_range(precision):
    """The rows-route training forward saves the position encoding it computed (SEC_ENC; split: fast_sincos of
    mnrf_field_split_common.inc, fp32: the device library's sincosf).  4096 positions uniform in |x| < 64 and the adversarial
    arguments of FC.adversarial_sincos_positions: every sin / cos within 1.5e-7 of float64 sin / cos(2^f x) under the split flag
    (the bar scripts/check_fast_sincos.py asserts for its emulation; it prints 1.12e-7) -- fp32 arithmetic: 2.4e-7 = 4 ulp of
    values in [0.5, 1), the bound OpenCL sets for sin and cos and the device library is built to --, raw coordinates bit for
    bit, the guard word 0; at x = +-64 the guard reports MNRF_GUARD_ENC_RANGE."""
    import mirror_nerf_amd as M
    from mirror_nerf_amd import _lib
    model = _model("init")[0]
    g = torch.Generator().manual_seed(64)
    x = torch.cat([(torch.rand(4096, 3, generator=g) * 2 - 1) * 64.0, FC.adversarial_sincos_positions()]).to(DEV).contiguous()
    assert float(x.abs().max()) < 64.0
    B = x.shape[0]
    de = M.Embedding(4)(TR.l2n(torch.ones(B, 3, device=DEV))).contiguous()
    fw = _rows_forward(model, dict(B=B, spr=1, xyz=x, rays=None, z=None, de=de), precision == "split")
    torch.cuda.synchronize()
    enc = _sec(fw["sx"], SEC_ENC, 64, B)[:, ENCPOS]
    assert torch.equal(enc[:, :3], x), "raw coordinates"
    want = TR.embed(x.double(), 10)
    err = float((enc.double() - want).abs().max())
    print(f"MEAS encoding {precision}: saved sin / cos against float64 {err:.3e} over {B} positions, |x| < 64")
    WORST[("encoding " + precision, "sin / cos")] = (err, 0.0)
    assert err <= (1.5e-7 if precision == "split" else 2.4e-7), err
    if precision == "split":
        word = fw["packed"][-1:].view(torch.int32)
        assert int(word.item()) == 0, "range guard"
        try:
            for v in (64.0, -64.0):
                far = torch.zeros(3, 3, device=DEV)
                far[1, 2] = v
                _rows_forward(model, dict(B=3, spr=1, xyz=far, rays=None, z=None, de=de[:3].contiguous()), True)
                torch.cuda.synchronize()
                assert int(word.item()) & _lib.MNRF_GUARD_ENC_RANGE, v
                word.zero_()
        finally:
            word.zero_()
            torch.cuda.synchronize()
