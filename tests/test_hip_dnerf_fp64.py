"""The D-NeRF object field (csrc/mnrf_dnerf.hip) against the float64 restatement (tests/dnerf_ref.py, pinned to the reference by
tests/test_dnerf_ref_cpu.py) beyond the box and the times of fixture G27-model, whose weights it uses: seeded positions in
|x| <= 1.5 and in |x| <= 8 (an object's rays run from near 2 to far 6), times -0.5, 0, 0.37, 1.0 and 2.5, sizes at every seam of
the 16-sample groups, the 32-sample waves and the 128-sample workgroups, and one launch of more workgroups than the card has CUs.
The restatement runs on the GPU, in float64 and in float32.

Every comparison is PER SAMPLE (the largest absolute error of a row), and a non-finite output where float64 is finite never
passes.

Two stages at t != 0.  The field is canonical(x + dx) with dx = deformation(x, t), and an error of 1e-7 in dx becomes 2^9 times
that in the phase of the last encoding channel of x + dx and is then multiplied by the density gain: compared as a whole, the
canonical trunk hides under the deformation's amplification.  So
  stage 1: the kernel's dx against deformation() in float64 at the input point;
  stage 2: the kernel's sigma and rgb against canonical() in float64 at p = fl32(x + dx_kernel), dx_kernel being the dx the
           kernel wrote: the one fp32 add that include/mnrf.h documents.  The canonical trunk is held to its own floor.
The whole-field comparison stays beside them, on its own (far wider) bar.  At t = 0 with MNRF_DNERF_CANONICAL there is one
stage: dx is exactly zero and p = x.

Bars.  None is invented: the same test runs the restatement in float32 on the same inputs, on the same GPU, against float64;
the kernel's bar is 4 x the largest such figure of the regime (box, moving or canonical, output group), rounded up to one digit.
4 is the project's factor (FX.tolerance); it leaves room for the MFMA's accumulation order and the time columns folded into the
first bias.  `BARS` holds the restatement's figure, the bar and what the kernel reached on the MI355X."""
import math

import numpy as np
import pytest
import torch

from tests import dnerf_ref as DR
from tests.golden import fixtures as FX
from tests.golden import weights as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WG = 128                        # samples of one workgroup (csrc/mnrf_dnerf.hip WG_SAMPLES)
BIG = 300 * WG + 5              # more workgroups than CUs: the LDS ring and the bias region of a CU serve a second workgroup
SIZES = [1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 401, BIG]
BOXES = [1.5, 8.0]
# (name, time, the module keeps t = 0 canonical, regime)
TIMES = [("t-0.5", -0.5, True, "moving"), ("t0_canonical", 0.0, True, "canonical"), ("t0_moving", 0.0, False, "moving"),
         ("t0.37", 0.37, True, "moving"), ("t1", 1.0, True, "moving"), ("t2.5", 2.5, True, "moving")]
GUARD = 7.5
NAN = float("nan")

# (box, regime, group) -> (the float32 restatement's largest per-sample error against float64 over the times and sizes of
# test_two_stages and the cases of test_ray_mode, on the MI355X; the kernel's bar = 4 x that, rounded up to one digit; the largest
# per-sample error the kernel reached over the same cases).  Groups: dx (stage 1), rgb2 / alpha2 (stage 2, or the only stage of
# the canonical regime), rgb1 / alpha1 (the whole field).  alpha runs up to 36 in the small box and 48 in the large one.
BARS = {
    (1.5, "canonical", "alpha2"): (3.103e-05, 2e-04, 3.294e-05),
    (1.5, "canonical", "rgb2"): (5.488e-08, 3e-07, 7.895e-08),
    (1.5, "moving", "alpha1"): (8.196e-04, 4e-03, 8.859e-04),
    (1.5, "moving", "alpha2"): (3.393e-05, 2e-04, 3.333e-05),
    (1.5, "moving", "dx"): (1.938e-07, 8e-07, 2.024e-07),
    (1.5, "moving", "rgb1"): (1.986e-07, 8e-07, 2.242e-07),
    (1.5, "moving", "rgb2"): (6.559e-08, 3e-07, 9.378e-08),
    (8.0, "canonical", "alpha2"): (6.012e-05, 3e-04, 5.404e-05),
    (8.0, "canonical", "rgb2"): (6.103e-08, 3e-07, 7.679e-08),
    (8.0, "moving", "alpha1"): (2.347e-03, 1e-02, 2.050e-03),
    (8.0, "moving", "alpha2"): (6.685e-05, 3e-04, 5.768e-05),
    (8.0, "moving", "dx"): (3.104e-07, 2e-06, 3.222e-07),
    (8.0, "moving", "rgb1"): (5.831e-07, 3e-06, 5.410e-07),
    (8.0, "moving", "rgb2"): (6.787e-08, 3e-07, 9.214e-08),
}

FIGS = {}                       # what this session measured: key -> [restatement, kernel]


def round_up_one_digit(v):
    if v == 0.0:
        return 0.0
    e = math.floor(math.log10(v))
    return float(f"{math.ceil(v / 10.0 ** e - 1e-9)}e{e}")


def _bar(key):
    return BARS[key][1] if key in BARS else None


class _Model:
    """The weights of fixture G27-model on the device, and per box the seeded positions and directions."""

    def __init__(self):
        fx = FX.Fixture("g27_dnerf_model")
        self.sd = DR.make_state_dicts(fx.meta["seed"], 1)[0]
        W.apply_tweaks(self.sd, fx.meta["tweaks"])
        c = fx.meta["checksum"][0]
        assert abs(W.checksum(self.sd) - c) <= 1e-9 * max(1.0, abs(c))
        self.sd_dev = {k: torch.from_numpy(v).to(DEV) for k, v in self.sd.items()}
        self.modules = {True: DR.module_of(self.sd, DEV), False: DR.module_of(self.sd, DEV, zero_canonical=False)}
        self.inputs, self.cache = {}, {}
        from mirror_nerf_amd.rendering import _embed
        for box in BOXES:
            rs = np.random.RandomState(int(box * 10))
            xyz = rs.uniform(-box, box, (BIG, 3)).astype(np.float32)
            xyz[:6] = np.array([[box, -box, box], [-box, box, -box], [0, 0, 0], [box, 0, 0], [0, -box, 0], [0, 0, box]], np.float32)   # the box's corners and faces
            view = rs.normal(size=(BIG, 3))
            view = (view / np.linalg.norm(view, axis=1, keepdims=True)).astype(np.float32)
            xyz, view = torch.from_numpy(xyz).to(DEV), torch.from_numpy(view).to(DEV)
            self.inputs[box] = (xyz, view, _embed(view, 4).contiguous())

    def whole(self, box, t, zero_canonical):
        """The whole field and the deformation alone on all BIG points of the box, in float64 and in float32: computed once."""
        key = (box, t, zero_canonical)
        if key not in self.cache:
            xyz, view, _ = self.inputs[box]
            out = {}
            for tag, x, v in (("64", xyz.double(), view.double()), ("32", xyz, view)):
                raw, dx = DR.field(self.sd_dev, x, v, t, zero_canonical)
                out["raw" + tag], out["dx" + tag] = raw.double(), dx.double()
            self.cache[key] = out
        return self.cache[key]


@pytest.fixture(scope="module")
def model():
    return _Model()


def launch(module, t, B, *, xyz=None, xyz_stride=3, rays=None, z=None, spr=1, dir_emb=None, dir_stride=27, sigma_only=False,
           want=("sigma", "rgb", "dx")):
    """mnrf_dnerf_forward (raw rgb) into buffers with guard rows behind row B; an output that is not in `want` is null.
    -> name -> (B, ..) tensor on the device."""
    from mirror_nerf_amd import _lib, dnerf as DN
    pad = 5
    shape = {"sigma": (B + pad,), "rgb": (B + pad, 3), "dx": (B + pad, 3)}
    out = {k: torch.full(shape[k], GUARD, dtype=torch.float32, device=DEV) for k in want}
    flags = _lib.MNRF_DNERF_RAW_RGB | (_lib.MNRF_DNERF_SIGMA_ONLY if sigma_only else 0)
    if t == 0.0 and module.zero_canonical:
        flags |= _lib.MNRF_DNERF_CANONICAL
    p = _lib.ptr
    _lib.check(_lib.lib().mnrf_dnerf_forward(p(DN.packed_of(module)), flags, B, p(xyz), xyz_stride, p(rays), p(z), spr, p(dir_emb), dir_stride,
                                             float(t), p(out.get("sigma")), p(out.get("rgb")), p(out.get("dx")), _lib.stream()), "mnrf_dnerf_forward")
    for k, v in out.items():
        assert bool((v[B:] == GUARD).all()), f"{k}: a row behind B = {B} was written"
        if sigma_only and k == "rgb":
            assert bool((v == GUARD).all()), "sigma only: rgb was written"
    return {k: v[:B] for k, v in out.items()}


def _rows(a, ref):
    """(B,) float64: per sample, the largest |a - ref|."""
    return (a.double() - ref).abs().reshape(ref.shape[0], -1).amax(1)


def judge(key, tag, got, ref64, ref32, fails):
    """One output group of one launch per sample against the regime's bar; notes the restatement's and the kernel's figure."""
    assert bool(torch.isfinite(ref64).all()), (key, tag, "the float64 restatement is not finite")
    ek, er = _rows(got, ref64), _rows(ref32, ref64)
    fig = FIGS.setdefault(key, [0.0, 0.0])
    fig[0], fig[1] = max(fig[0], float(er.max())), max(fig[1], float(ek.max()) if bool(torch.isfinite(ek).all()) else math.inf)
    bar = _bar(key)
    print(f"FIG dnerf box={key[0]} {key[1]} {key[2]} {tag} rest={float(er.max()):.3e} kern={float(ek.max()):.3e} bar={bar}")
    if bar is None:
        fails.append(f"{key}: no bar recorded (4 x the restatement's figure {float(er.max()):.3e})")
        return
    bad = (~(ek <= bar)).nonzero().flatten().tolist()      # a NaN error is not <= bar
    if bad:
        fails.append(f"{key} {tag}: {len(bad)} samples beyond {bar:.0e}, the first: sample {bad[0]} off by {float(ek[bad[0]]):.3e}")


def two_stages(model, box, tname, t, zero_canonical, regime, B, got, x, view, tag):
    """Judges one launch's outputs (sigma, rgb, dx on the B points x) in the stages of its regime."""
    sd, fails = model.sd_dev, []
    if regime == "canonical":
        assert not bool(got["dx"].any()) and not bool(torch.signbit(got["dx"]).any()), "t = 0: dx is exactly zero"
        c64, c32 = DR.canonical(sd, x.double(), view.double()), DR.canonical(sd, x, view).double()
        judge((box, regime, "rgb2"), tag, got["rgb"], c64[:, :3], c32[:, :3], fails)
        judge((box, regime, "alpha2"), tag, got["sigma"], c64[:, 3], c32[:, 3], fails)
    else:
        w = model.whole(box, t, zero_canonical)
        judge((box, regime, "dx"), tag, got["dx"], w["dx64"][:B], w["dx32"][:B], fails)
        p = x + got["dx"]                                                            # the kernel's one fp32 add
        c64, c32 = DR.canonical(sd, p.double(), view.double()), DR.canonical(sd, p, view).double()
        judge((box, regime, "rgb2"), tag, got["rgb"], c64[:, :3], c32[:, :3], fails)
        judge((box, regime, "alpha2"), tag, got["sigma"], c64[:, 3], c32[:, 3], fails)
        judge((box, regime, "rgb1"), tag, got["rgb"], w["raw64"][:B, :3], w["raw32"][:B, :3], fails)
        judge((box, regime, "alpha1"), tag, got["sigma"], w["raw64"][:B, 3], w["raw32"][:B, 3], fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("B", SIZES)
@pytest.mark.parametrize("tname,t,zero_canonical,regime", TIMES, ids=[c[0] for c in TIMES])
@pytest.mark.parametrize("box", BOXES)
def test_two_stages(model, box, tname, t, zero_canonical, regime, B):
    """Explicit positions, the full launch: stage 1, stage 2 and the whole field, per sample."""
    xyz, view, de = model.inputs[box]
    got = launch(model.modules[zero_canonical], t, B, xyz=xyz[:B].contiguous(), dir_emb=de[:B].contiguous())
    if regime == "moving":
        assert float(got["dx"].abs().max()) > 1e-3, "the deformation net did not run"
    two_stages(model, box, tname, t, zero_canonical, regime, B, got, xyz[:B], view[:B], f"{tname} B={B}")


# ------------------------------------------------------------------------------------------------------------ ray mode
@pytest.mark.parametrize("t", [0.0, 0.37])
@pytest.mark.parametrize("spr", [1, 5, 64])
def test_ray_mode(model, spr, t):
    """o + d z from rays and depths (a multiply, then an add), the view row per ray (sample / spr): bit-equal to the launch on
    the explicit float32 positions, and both on the bars of test_two_stages.  With 5 samples per ray a ray straddles the
    16-sample groups and the workgroup seams.  The view encoding has B rows, NaN behind the n_rays that may be read."""
    n_rays = {1: 3 * WG + 17, 5: (3 * WG + 17) // 5 + 1, 64: 7}[spr]
    B = n_rays * spr
    xyz, view, de = model.inputs[8.0]
    rs = np.random.RandomState(spr)
    rays = torch.zeros(n_rays, 8, device=DEV)
    rays[:, :3], rays[:, 3:6], rays[:, 6], rays[:, 7] = xyz[:n_rays] * 0.25, view[:n_rays], 2.0, 6.0
    z = torch.from_numpy(np.sort(rs.uniform(2.0, 6.0, (n_rays, spr)).astype(np.float32), axis=1)).to(DEV)
    pts = (rays[:, None, :3] + rays[:, None, 3:6] * z[:, :, None]).reshape(-1, 3).contiguous()      # two float32 operations
    assert float(pts.abs().max()) <= 8.0
    de_rows = torch.full((B, 27), NAN, device=DEV)
    de_rows[:n_rays] = de[:n_rays]
    module = model.modules[True]
    got = launch(module, t, B, rays=rays, z=z, spr=spr, dir_emb=de_rows)
    same = launch(module, t, B, xyz=pts, spr=spr, dir_emb=de_rows)
    for k in got:
        assert torch.equal(got[k], same[k]) and bool(torch.isfinite(got[k]).all()), f"{k}: ray-generated and explicit positions differ"
    regime = "canonical" if t == 0.0 else "moving"
    v = view[:n_rays].repeat_interleave(spr, 0)
    # (the whole field of these points is not in the model's cache: stage 1 and the whole field are restated here)
    sd, fails = model.sd_dev, []
    if regime == "moving":
        judge((8.0, regime, "dx"), f"rays spr={spr}", got["dx"], DR.deformation(sd, pts.double(), t), DR.deformation(sd, pts, t).double(), fails)
        p = pts + got["dx"]
    else:
        assert not bool(got["dx"].any())
        p = pts
    c64, c32 = DR.canonical(sd, p.double(), v.double()), DR.canonical(sd, p, v).double()
    judge((8.0, regime, "rgb2"), f"rays spr={spr}", got["rgb"], c64[:, :3], c32[:, :3], fails)
    judge((8.0, regime, "alpha2"), f"rays spr={spr}", got["sigma"], c64[:, 3], c32[:, 3], fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------------------ strides
@pytest.mark.parametrize("xyz_stride,dir_stride", [(3, 32), (4, 27), (90, 32)])
def test_strides(model, xyz_stride, dir_stride):
    """Rows of xyz_stride and dir_stride floats with NaN in every column that must not be read: the outputs are the bytes of the
    dense launch."""
    B, t = WG + 33, 0.37
    xyz, _, de = model.inputs[1.5]
    module = model.modules[True]
    dense = launch(module, t, B, xyz=xyz[:B].contiguous(), dir_emb=de[:B].contiguous())
    wide_x = torch.full((B, xyz_stride), NAN, device=DEV)
    wide_x[:, :3] = xyz[:B]
    wide_d = torch.full((B, dir_stride), NAN, device=DEV)
    wide_d[:, :27] = de[:B]
    got = launch(module, t, B, xyz=wide_x, xyz_stride=xyz_stride, dir_emb=wide_d, dir_stride=dir_stride)
    for k in dense:
        assert bool(torch.isfinite(got[k]).all()) and torch.equal(got[k], dense[k]), k


# ------------------------------------------------------------------------------------------------------------ null outputs
@pytest.mark.parametrize("t", [0.0, 0.37])
@pytest.mark.parametrize("sigma_only", [False, True], ids=["full", "sigma_only"])
def test_null_outputs(model, sigma_only, t):
    """Each output null in turn, alone and under MNRF_DNERF_SIGMA_ONLY (where rgb is never written and the view encoding may be
    null): the outputs that remain are the bytes of the launch that writes all three."""
    B = 2 * WG + 17
    xyz, _, de = model.inputs[8.0]
    module = model.modules[True]
    x, d = xyz[:B].contiguous(), de[:B].contiguous()
    full = launch(module, t, B, xyz=x, dir_emb=d)
    names = ("sigma", "dx") if sigma_only else ("sigma", "rgb", "dx")
    if sigma_only:
        base = launch(module, t, B, xyz=x, dir_emb=None, sigma_only=True)          # its rgb buffer is checked to stay untouched
        for k in names:
            assert torch.equal(base[k], full[k]), f"sigma only: {k} differs from the full launch"
    for absent in names:
        want = tuple(k for k in names if k != absent)
        got = launch(module, t, B, xyz=x, dir_emb=None if sigma_only else d, sigma_only=sigma_only, want=want)
        assert set(got) == set(want)
        for k in want:
            assert torch.equal(got[k], full[k]), f"without {absent}: {k} differs from the full launch"


# ------------------------------------------------------------------------------------------------------------ the table
def test_bars_table():
    """Every bar is 4 x its restatement figure rounded up to one digit, and no recorded kernel figure exceeds its bar; prints
    what this session measured (empty when the test runs alone)."""
    for key, (rest, kern) in sorted(FIGS.items()):
        print(f'\n    ({key[0]}, "{key[1]}", "{key[2]}"): ({rest:.3e}, {round_up_one_digit(4.0 * rest):.0e}, {kern:.3e}),', end="")
    assert BARS, "no bars recorded"
    for key, (rest, bar, kern) in BARS.items():
        assert bar == round_up_one_digit(4.0 * rest), (key, rest, bar)
        assert kern <= bar, (key, kern, bar)
    regimes = {(box, "moving", g) for box in BOXES for g in ("dx", "rgb2", "alpha2", "rgb1", "alpha1")}
    regimes |= {(box, "canonical", g) for box in BOXES for g in ("rgb2", "alpha2")}
    assert set(BARS) == regimes
