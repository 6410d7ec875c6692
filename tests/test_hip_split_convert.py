"""The fp32 -> (hi, lo) conversion of the forward-only split kernels in its short form (csrc/mnrf_field_split_common.inc split2:
lo from two mixed-precision FMAs under a round-toward-zero f16 mode, 8 vector instructions per value pair instead of 11).

1. The conversion alone (mnrf_split2_probe: the kernels' own device function under the kernels' mode setting) against a numpy
   restatement of the DEFINITION, bit for bit:
       hi = f16 toward zero of x, saturating at 65504;      lo = f16 toward zero of (x - hi).
2. The kernels at their smallest shapes: every output and the guard word equal, bit for bit, those of the SAME launch with the
   conversion in its long form (mnrf_split_convert_long)."""
import numpy as np
import pytest
import torch

from tests.golden import fixtures as FX

DEV = "cuda:0"
gpu = pytest.mark.gpu


# --------------------------------------------------------------------------- the definition, in numpy
def f16_toward_zero(x):
    """float32 array -> the bits (uint16) of its f16 value rounded toward zero: a finite value beyond the f16 range becomes
    +-65504, an infinity stays one, a NaN stays a NaN."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        h = x.astype(np.float16)                            # to nearest
        too_big = np.abs(h.astype(np.float64)) > np.abs(x.astype(np.float64))      # (an overflow to inf of a finite x included)
    bits = h.view(np.uint16).copy()
    bits[too_big] -= 1                                      # sign-magnitude: one step toward zero
    return bits


def split_model(x):
    """-> (hi bits, lo bits) of the definition."""
    x = np.asarray(x, dtype=np.float32)
    hi = f16_toward_zero(x)
    with np.errstate(invalid="ignore"):
        r = x - hi.view(np.float16).astype(np.float32)      # fp32 subtraction (exact for finite x)
    return hi, f16_toward_zero(r)


def relu_bits(x):
    """The kernels' ReLU: an integer max on the bit pattern (negative values, -0 and NaNs with the sign bit set -> +0)."""
    return np.maximum(np.asarray(x, dtype=np.float32).view(np.int32), 0).view(np.float32)


def conversion_inputs():
    f32 = np.float32
    v = [0.0, -0.0]
    sub32 = np.array([1, 2, 0x400000, 0x7FFFFF], dtype=np.uint32)               # fp32 subnormals
    v += list(sub32.view(f32)) + list((sub32 | 0x80000000).astype(np.uint32).view(f32))
    k = np.arange(1, 1024, dtype=np.float64)                                     # the f16 subnormal range, and between its values
    v += list((k * 2.0 ** -24).astype(f32)) + list(((k + 0.5) * 2.0 ** -24).astype(f32)) + list(((k + 0.25) * -2.0 ** -24).astype(f32))
    for end in (f32(2.0 ** -24), f32(2.0 ** -14)):
        v += [end, np.nextafter(end, f32(0)), np.nextafter(end, f32(1))]
    for e in range(-26, 18):
        p = f32(2.0 ** e)
        for s in (p, np.nextafter(p, f32(0)), np.nextafter(p, f32(np.inf))):
            v += [s, -s]
    v += [65503.996, 65504.0, 65520.0, 131008.0, 131072.0, 1e6, -65503.996, -65504.0, -65520.0, -131008.0, -131072.0, -1e6]
    v += [np.inf, -np.inf, np.nan]
    rng = np.random.default_rng(20240607)
    draws = rng.standard_normal(4096).astype(f32)
    v = np.concatenate([np.array(v, dtype=f32), draws, draws * f32(1e-3), draws * f32(1e3)])
    if v.size % 2:
        v = np.concatenate([v, np.zeros(1, dtype=f32)])
    return v


def test_numpy_model_of_the_split():
    """hi + lo reproduces x within 2^-20 |x| and lo has the sign of x.  (The relative bound is checked from |x| = 2^-4 up: below,
    lo falls into the f16 subnormals, whose ulp is 2^-24 whatever x is.)"""
    x = conversion_inputs()
    x = x[np.isfinite(x) & (np.abs(x) < 65504.0)]
    hi, lo = split_model(x)
    h, l = hi.view(np.float16).astype(np.float64), lo.view(np.float16).astype(np.float64)
    assert np.all((l == 0) | (np.sign(l) == np.sign(x))), "lo has the sign of x"
    assert np.all(np.abs(h) <= np.abs(x.astype(np.float64))), "hi is rounded toward zero"
    big = np.abs(x) >= 2.0 ** -4
    err = np.abs(x.astype(np.float64) - h - l)
    assert np.all(err[big] <= 2.0 ** -20 * np.abs(x[big].astype(np.float64)))
    assert np.all(err[~big] <= 2.0 ** -24)
    # the saturating end
    hi, lo = split_model(np.array([65520.0, 131008.0, 1e6, -1e6], dtype=np.float32))
    assert list(hi) == [0x7BFF, 0x7BFF, 0x7BFF, 0xFBFF] and list(lo) == [0x4C00, 0x7BFF, 0x7BFF, 0xFBFF]


def _same_halves(got, want, what):
    """uint16 arrays: equal as integers, except that a NaN is any NaN."""
    nan_w = (want & 0x7FFF) > 0x7C00
    nan_g = (got & 0x7FFF) > 0x7C00
    bad = np.where(nan_w, ~nan_g, got != want)
    assert not bad.any(), (what, int(bad.sum()), [(hex(int(g)), hex(int(w))) for g, w in zip(got[bad][:8], want[bad][:8])])


@gpu
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("form", ["short", "long"])
def test_conversion_matches_the_definition_bit_for_bit(relu, form):
    from mirror_nerf_amd import _lib
    L = _lib.lib()
    base = conversion_inputs()
    for x in (base, np.roll(base, 1)):      # every value once in the low and once in the high half of a pair
        xin = relu_bits(x) if relu else x
        want_hi, want_lo = split_model(xin)
        xd = torch.from_numpy(x).to(DEV)
        n = x.size // 2
        hi = torch.zeros(n, dtype=torch.int32, device=DEV)
        lo = torch.zeros(n, dtype=torch.int32, device=DEV)
        _lib.check(L.mnrf_split2_probe(_lib.ptr(xd), n, relu, int(form == "long"), _lib.ptr(hi), _lib.ptr(lo), _lib.stream()),
                   "mnrf_split2_probe")
        torch.cuda.synchronize()
        got_hi = hi.cpu().numpy().view(np.uint16)      # little endian: value 2i in the low half of word i
        got_lo = lo.cpu().numpy().view(np.uint16)
        _same_halves(got_hi, want_hi, ("hi", form, relu))
        _same_halves(got_lo, want_lo, ("lo", form, relu))


# --------------------------------------------------------------------------- the kernels, short form against long form
def _module(sd):
    import mirror_nerf_amd as M
    m = M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal="normal_net.0.weight" in sd,
                     predict_mirror_mask="is_mirror_net.0.weight" in sd)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()})
    return m.to(DEV)


def _tripping(sd):
    """One weight of the first layer, on the raw x coordinate (input column 0), set to 2000: a sample at x = 63.5 drives that
    channel to 127 000, beyond the f16 maximum, and raises the range guard; samples at |x| <= 1.2 stay far below it and a
    sample at x = 0 does not see the weight at all."""
    sd = {k: np.array(v, copy=True) for k, v in sd.items()}
    sd["xyz_encoding_1.0.weight"][5, 0] = 2000.0
    return sd


@pytest.fixture(scope="module")
def g4_model():
    return _module(_tripping(FX.Fixture("g4_fine_test").state_dicts()[-1]))


@pytest.fixture(autouse=True)
def split_precision():
    from mirror_nerf_amd import mirror_nerf as MN
    old = MN.PRECISION
    MN.set_precision("split")
    yield
    MN.set_precision(old)


def _guard_word(model):
    from mirror_nerf_amd import mirror_nerf as MN
    from mirror_nerf_amd.weights import packed_of
    packed_of(model)
    w = MN.guard_words([model])[0]
    model.__dict__["_mnrf_packed"].packed[-1:].zero_()
    return w


def _both_forms(model, launch):
    """launch() -> dict of tensors; run under the short and the long form, compare every tensor and the guard word."""
    from mirror_nerf_amd import _lib
    L = _lib.lib()
    out = {}
    was = L.mnrf_split_convert_long(-1)
    try:
        for form in (0, 1):
            L.mnrf_split_convert_long(form)
            res = launch()
            torch.cuda.synchronize()
            out[form] = ({k: v.clone() for k, v in res.items() if v is not None}, _guard_word(model))
    finally:
        L.mnrf_split_convert_long(was)
    (short, gs), (long_, gl) = out[0], out[1]
    assert gs == gl, ("guard word", hex(gs), hex(gl))
    assert short.keys() == long_.keys()
    for k in short:
        a, b = short[k].view(torch.int32), long_[k].view(torch.int32)
        same = (a == b) | (torch.isnan(short[k]) & torch.isnan(long_[k]))
        assert bool(same.all()), (k, int((~same).sum()))
    return short, gs


def _samples(B):
    g = torch.Generator(device="cpu").manual_seed(11)
    xyz = torch.rand(B, 3, generator=g) * 2.4 - 1.2
    xyz[7, 0] = 63.5                                        # the sample that trips the range guard
    d = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=1)
    import mirror_nerf_amd as M
    return xyz.to(DEV).contiguous(), M.Embedding(4)(d.to(DEV)).contiguous()


@gpu
@pytest.mark.parametrize("B", [191, 192, 193])
@pytest.mark.parametrize("sigma_only", [True, False])
def test_field_launch_48_samples_per_wave(g4_model, B, sigma_only):
    from mirror_nerf_amd import _lib
    from mirror_nerf_amd import mirror_nerf as MN
    xyz, de = _samples(B)
    _guard_word(g4_model)
    res, word = _both_forms(g4_model, lambda: MN.field_forward(g4_model, B, xyz=xyz, dir_emb=de, dir_stride=27, sigma_only=sigma_only))
    assert word & _lib.MNRF_GUARD_SATURATED
    assert bool(torch.isfinite(res["sigma"][8:]).all())


@gpu
@pytest.mark.parametrize("B", [127, 128, 129])
def test_field_launch_32_samples_per_wave(g4_model, B):
    """A geo_feat request takes the S = 2 forward kernel."""
    from mirror_nerf_amd import _lib
    from mirror_nerf_amd import mirror_nerf as MN
    xyz, de = _samples(B)
    _guard_word(g4_model)
    res, word = _both_forms(g4_model, lambda: MN.field_forward(g4_model, B, xyz=xyz, dir_emb=de, dir_stride=27, want_geo=True))
    assert word & _lib.MNRF_GUARD_SATURATED
    assert "geo_feat" in res


def _rays(n):
    """Ray 0 runs along +x and its last sample sits at x = 63.5 (the guard trips); ray 1 runs along +y in the plane x = 0."""
    import mirror_nerf_amd as M
    rays = torch.zeros(n, 8)
    rays[:, 6], rays[:, 7] = 0.05, 8.0
    rays[0, 0:6] = torch.tensor([0.0, 0.1, 0.2, 1.0, 0.0, 0.0])
    if n > 1:
        rays[1, 0:6] = torch.tensor([0.0, -1.0, 0.3, 0.0, 1.0, 0.0])
    z = torch.linspace(0.05, 2.0, 192).repeat(n, 1)
    z[0, -1] = 63.5
    de = M.Embedding(4)(rays[:, 3:6].to(DEV)).contiguous()
    return rays.to(DEV).contiguous(), z.to(DEV).contiguous(), de


@gpu
@pytest.mark.parametrize("n_rays", [1, 2])
@pytest.mark.parametrize("kind", ["fused", "rgb_depth", "blended_all_mirror", "blended_opaque"])
def test_ray_fused_launches(g4_model, n_rays, kind):
    from mirror_nerf_amd import _lib
    from mirror_nerf_amd import synthetic as SY
    from mirror_nerf_amd.weights import folded_of
    L, p = _lib.lib(), _lib.ptr
    assert L.mnrf_fused_samples_per_ray() == 192
    if kind.startswith("blended"):
        sd = SY.apply_tweaks(SY.make_state_dict(0, n_models=2)[1], SY.ALL_MIRROR if kind == "blended_all_mirror" else SY.OPAQUE)
        model = _module(_tripping(sd))
    else:
        model = g4_model
    rays, z, de = _rays(n_rays)
    f = lambda *s: torch.zeros(*s, dtype=torch.float32, device=DEV)  # noqa: E731

    def launch():
        o = dict(opacity=f(n_rays), rgb=f(n_rays, 3), depth=f(n_rays))
        if kind == "rgb_depth":
            _lib.check(L.mnrf_field_composite_fused(p(folded_of(model)), n_rays, p(rays), p(z), p(de), 27, _lib.MNRF_FUSED_RGB_DEPTH, None,
                                                    p(o["opacity"]), p(o["rgb"]), p(o["depth"]), None, None, None, _lib.stream()), kind)
            return o
        o.update(mask=f(n_rays), sn=f(n_rays, 3), xs=f(n_rays, 3), weights=f(n_rays, 192))
        if kind == "fused":
            _lib.check(L.mnrf_field_composite_fused(p(folded_of(model)), n_rays, p(rays), p(z), p(de), 27, 0, p(o["weights"]), p(o["opacity"]),
                                                    p(o["rgb"]), p(o["depth"]), p(o["mask"]), p(o["sn"]), p(o["xs"]), _lib.stream()), kind)
            return o
        o["pn"] = f(n_rays, 192, 3)
        _lib.check(L.mnrf_field_composite_fused_pn(p(folded_of(model)), n_rays, p(rays), p(z), p(de), 27, _lib.MNRF_FUSED_BLENDED_LEVEL,
                                                   p(o["weights"]), p(o["opacity"]), p(o["rgb"]), p(o["depth"]), p(o["mask"]), p(o["sn"]),
                                                   p(o["xs"]), p(o["pn"]), _lib.stream()), kind)
        return o

    folded_of(model)
    _guard_word(model)
    res, word = _both_forms(model, launch)
    assert word & _lib.MNRF_GUARD_SATURATED
    if kind.startswith("blended") and n_rays == 2:      # ray 1 never meets the tweaked weight: the branch it takes is the model's
        skipped = bool((res["rgb"][1] == 0).all())
        assert skipped == (kind == "blended_all_mirror"), (kind, res["mask"][1].item(), res["rgb"][1].tolist())
