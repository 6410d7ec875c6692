"""What the float64 tests of the field kernels share (tests/test_hip_backward_fp64.py, tests/test_hip_forward_fp64.py): the
layout of the rows the training forward saves, that launch itself, the error measure -- and the inputs of the forward tests,
drawn on the CPU so that the CPU suite can state conditions on them (tests/test_torch_ref_cpu.py).  Importing this needs no GPU."""
import math

import torch

from tests import torch_ref as TR

DEV = "cuda:0"
F64 = torch.float64

# ---------------------------------------------------------------------------------------------- layout (mnrf_layout.h)
SEC_ENC, SEC_H, SEC_FIN, SEC_DIRE, SEC_HD, SEC_HN, SEC_HM = 0, 64, 2112, 2368, 2400, 2528, 2656


def _enc_col(t, g):
    P, s = 8 * g + (t >> 1), t & 1
    if P < 30:
        return 3 + 6 * (P // 3) + 3 * s + (P % 3)
    if P == 30:
        return s
    return 2 if s == 0 else -1


ENCPOS = [0] * 63          # logical column of the 63-wide xyz encoding -> its position in the saved (sin,cos)-pair order
for _g in range(4):
    for _t in range(16):
        _c = _enc_col(_t, _g)
        if _c >= 0:
            ENCPOS[_c] = 16 * (_t >> 2) + 4 * _g + (_t & 3)


def _sec(buf, off, width, B):
    return buf[off * B:(off + width) * B].view(B, width)


def _rel(a, b):
    """max |a - b| over the largest |b|; a reference of exact zeros must be met by exact zeros."""
    a, b = a.double(), b.double()
    s = float(b.abs().max()) if b.numel() else 0.0
    d = float((a - b).abs().max()) if b.numel() else 0.0
    if s == 0.0:
        return 0.0 if d == 0.0 else math.inf
    return d / s


# ---------------------------------------------------------------------------------------------- the kernel's own forward
def _rows_forward(model, inp, split):
    """Rows-route mnrf_field_forward_train (fp32 rows of every Linear's input) with the arithmetic flag of `split`."""
    from mirror_nerf_amd import _lib
    from mirror_nerf_amd.weights import packed_of
    L, p = _lib.lib(), _lib.ptr
    B = inp["B"]
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=DEV)  # noqa: E731
    o = (f(B), f(B, 3), f(B, 3), f(B), f(B, 3))
    sx = f(L.mnrf_train_save_floats(B))
    sm = torch.zeros(L.mnrf_train_mask_words(B), dtype=torch.int64, device=DEV)
    si, sj = f(B), f(B)
    packed = packed_of(model)
    _lib.check(L.mnrf_field_forward_train(p(packed), B, p(inp["xyz"]), 3, p(inp["rays"]), p(inp["z"]), inp["spr"], p(inp["de"]), 27,
                                          *[p(t) for t in o], p(sx), p(sm), p(si), p(sj), _lib.MNRF_SPLIT_F16 if split else 0,
                                          _lib.stream()), "forward rows")
    return dict(packed=packed, out=o, sx=sx, sm=sm, si=si, sj=sj)


def _saved(sx, B, rows=None):
    """The saved Linear inputs (float64, logical column order), optionally of some samples only."""
    s = lambda off, w: _sec(sx, off, w, B) if rows is None else _sec(sx, off, w, B)[rows]  # noqa: E731
    d = {"enc": s(SEC_ENC, 64)[:, ENCPOS]}
    for i in range(8):
        d[f"h{i + 1}"] = s(SEC_H + 256 * i, 256)
    d.update(fin=s(SEC_FIN, 256), dire=s(SEC_DIRE, 32), hd=s(SEC_HD, 128), hn=s(SEC_HN, 128), hm=s(SEC_HM, 128))
    return {k: v.to(F64) for k, v in d.items()}


# ---------------------------------------------------------------------------------------------- weights of the forward tests
_STATE = {}


def state_dict(kind):
    """numpy state dicts by name.  "init": seeded, opaque (the model of test_hip_backward_fp64); "straddle": the fine model of
    mirror_nerf_amd.synthetic.build_models(seed 0) with the mirror head straddling 0.5; "trained": the fine model of fixture G11;
    "no_normal" / "no_mirror" / "no_heads": seeded models without the optional heads; "bands_6_2" / "bands_0_0":
    MirrorNeRF(39, 15) / MirrorNeRF(3, 3)."""
    from tests.golden import weights as GW
    if kind not in _STATE:
        if kind == "init":
            sd = GW.apply_tweaks(GW.make_state_dict(5, 1)[0], GW.OPAQUE)
        elif kind == "straddle":
            sd = GW.apply_tweaks(GW.make_state_dict(0, 2)[1], GW.STRADDLE)
        elif kind == "trained":
            from tests.golden import fixtures as FX
            sd = FX.Fixture("g11_trained_grads_full").state_dicts()[1]
        elif kind in ("no_normal", "no_mirror", "no_heads"):
            sd = GW.apply_tweaks(GW.make_state_dict(3, 1, predict_normal=kind == "no_mirror", predict_mirror_mask=kind == "no_normal")[0],
                                 GW.OPAQUE)
        elif kind in ("bands_6_2", "bands_0_0"):
            a, b = (39, 15) if kind == "bands_6_2" else (3, 3)
            sd = GW.apply_tweaks(GW.make_state_dict(4, 1, in_xyz=a, in_dir=b)[0], GW.OPAQUE)
        else:
            raise KeyError(kind)
        _STATE[kind] = sd
    return _STATE[kind]


def bands(kind):
    """(position bands, view bands) of a model of state_dict()."""
    return {"bands_6_2": (6, 2), "bands_0_0": (0, 0)}.get(kind, (10, 4))


def weights(kind, dtype, device="cpu"):
    return {k: torch.from_numpy(v).to(device, dtype) for k, v in state_dict(kind).items()}


# ---------------------------------------------------------------------------------------------- inputs of the forward tests
CLOUD_BOX = {"box": None, "wide": 63.9}      # "box": |x| <= 3, or 1.2 for the trained model (the box of test_hip_fold.py)


def cloud(kind, which, n, seed=0):
    """n positions (n, 3) fp32 uniform in the cube of `which` and n unit directions, drawn on the CPU; a prefix of a larger draw
    with the same arguments."""
    half = CLOUD_BOX[which] or (1.2 if kind == "trained" else 3.0)
    g = torch.Generator().manual_seed(1000 * seed + (7 if which == "wide" else 3))
    xyz = ((torch.rand(n, 3, generator=g) * 2 - 1) * half).contiguous()
    assert float(xyz.abs().max()) < 64.0
    d = TR.l2n(torch.randn(n, 3, generator=g))
    return xyz, d


def ray_inputs(n_rays, spr, seed=0):
    """Rays (n, 8) with unit directions that differ widely from ray to ray, and sorted depths (n, spr) in [0.2, 4.2]."""
    g = torch.Generator().manual_seed(77 + 1000 * seed + 13 * spr + n_rays)
    rays = torch.randn(n_rays, 8, generator=g)
    rays[:, :3] *= 0.5
    rays[:, 3:6] = TR.l2n(rays[:, 3:6])
    z = torch.sort(torch.rand(n_rays, spr, generator=g) * 4 + 0.2, 1)[0].contiguous()
    return rays.contiguous(), z


def ray_positions(rays, z):
    """rays[:, :3] + rays[:, 3:6] * z in the dtype of the inputs as two separate operations (rendering.py:302; the kernels use
    no FMA there): (n * spr, 3)."""
    prod = rays[:, None, 3:6] * z[:, :, None]
    pos = rays[:, None, :3] + prod
    return pos.reshape(-1, 3)


RAY_SPR = (1, 5, 47, 49, 64, 191, 192, 193, 256)
RAY_MODEL = "init"      # tests/test_torch_ref_cpu.py: its colour moves by >= 1e-3 (median) under another ray's direction


def neighbour_shift(kind, n_rays, spr):
    """The median over samples of the largest change of the float64 rgb when every ray takes its neighbour's direction."""
    rays, z = ray_inputs(n_rays, spr)
    w = weights(kind, F64)
    x = ray_positions(rays, z).double()
    de = TR.embed(rays[:, 3:6].double(), 4)
    with torch.no_grad():
        a = TR.field(w, x, de.repeat_interleave(spr, 0))[1]
        b = TR.field(w, x, de.roll(1, 0).repeat_interleave(spr, 0))[1]
    return float((a - b).abs().amax(1).median())


def fused_inputs(n_rays, seed=0):
    """Rays of the synthetic camera (the rays of test_hip_blended_level) and sorted depths in [2, 6], 192 per ray."""
    from oracle import mirror_nerf_oracle as O
    rays = torch.from_numpy(O.synthetic_rays(64, 64)[:n_rays].copy())
    g = torch.Generator().manual_seed(500 + seed)
    z = torch.sort(2.0 + 4.0 * torch.rand(n_rays, 192, generator=g), dim=1).values.contiguous()
    return rays.contiguous(), z


def adversarial_sincos_positions():
    """Arguments where a wrong range reduction shows: for 512 seeded integers k, a = fp32(k pi/2) and fp32((2k + 1) pi/4)
    with their two fp32 neighbours, as x = a / 2^9 (exact) on every axis: (3072, 3).  The kernel's range is |x| < 64, i.e.
    a < 2^15 at the highest band, so the quadrant index k is drawn from 1 <= k < 2^16 / pi - 1 = 20 860 (k up to 2^15 would put
    x at 100 and trip the range guard); the lower bands see the same positions as a / 2^(9 - f)."""
    import numpy as np
    k = np.random.RandomState(9).randint(1, 20860, 512).astype(np.float64)
    a = np.concatenate([k * np.pi / 2, (2 * k + 1) * np.pi / 4]).astype(np.float32)
    a = np.concatenate([a, np.nextafter(a, np.float32(np.inf)), np.nextafter(a, np.float32(-np.inf))])
    x = (a / np.float32(512.0)).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) * 512.0, a.astype(np.float64)) and float(np.abs(x).max()) < 64.0
    return torch.from_numpy(np.repeat(x[:, None], 3, 1).copy())
