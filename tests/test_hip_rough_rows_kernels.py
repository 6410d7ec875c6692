"""mnrf_rough_rows, mnrf_perturb_normals and mnrf_reflect_jitter_fan_rows (csrc/mnrf_rough.hip) against their numpy restatements
(tests/rough_rows_ref.py), bit for bit: below, at and past one wavefront and one workgroup, 0 to 8 mirrors, bases aligned to 16
and to 4 bytes only, sentinel words around every output, and the edge rows (index -1, K-1 and out of range; mask 0, 0.5 and 1;
std 0; a NaN normal; a NaN draw).  With one std on every row the new kernels are held to the launches of the uniform route:
mnrf_reflect_jitter_fan, and mnrf_reflect_compact with the noise and the std."""
import ctypes

import numpy as np
import pytest
import torch

from tests import rough_ref as RR
from tests import rough_rows_ref as RW

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEAR2 = 0.1
SIZES = [1, 63, 64, 65, 255, 256, 257, 321]
COUNTS = [0, 1, 3, 8]
PAD = 4                   # sentinel floats on either side of an output: 16 bytes, so a shift of 0 keeps the 16-byte alignment
SENT = -777.25
GUARD_WORD = 0x5A5A5A5A
F = np.float32


def _L():
    from mirror_nerf_amd import _lib
    return _lib


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(got, want, what):
    """Bit for bit; a NaN matches a NaN (payloads are not compared)."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaNs elsewhere"
    bad = np.argwhere(got.view(np.int32)[~nan] != want.view(np.int32)[~nan])
    assert bad.size == 0, f"{what}: {len(bad)} values differ, the first is number {bad[0].tolist()} of the non-NaN ones"


class Buf:
    """A float array on the device `shift` floats past a 16-byte boundary, with PAD sentinel floats on either side."""

    def __init__(self, a=None, shape=None, shift=0):
        a = np.full(shape, SENT, F) if a is None else np.ascontiguousarray(a, F)
        self.shape, self.lo = a.shape, PAD + shift
        self.flat = torch.full((self.lo + a.size + PAD,), SENT, device=DEV)
        self.flat[self.lo:self.lo + a.size] = _t(a).reshape(-1)
        self.ptr = ctypes.c_void_p(self.flat.data_ptr() + 4 * self.lo)
        assert (self.flat.data_ptr() + 4 * self.lo) % 16 == (4 * shift) % 16

    def get(self):
        """The array; the sentinels around it must be untouched."""
        flat = self.flat.cpu().numpy()
        n = int(np.prod(self.shape))
        assert (flat[:self.lo] == F(SENT)).all() and (flat[self.lo + n:] == F(SENT)).all(), "a sentinel word was written"
        return flat[self.lo:self.lo + n].reshape(self.shape)


def case(n, K, seed):
    """n rays with every kind of row; K mirrors, every other one polished."""
    rs = np.random.RandomState(seed)
    rays = rs.normal(size=(n, 8)).astype(F)
    xs = rs.normal(size=(n, 3)).astype(F)
    nrm = rs.normal(size=(n, 3)).astype(F)
    index = rs.randint(-1, max(K, 1), size=n).astype(np.int32)
    odd = np.array([K - 1, -1, K, K + 5, -2, -7, 2 ** 31 - 1, -2 ** 31], np.int32)      # the last six: out of range, count as -1
    index[rs.permutation(n)[:min(n, odd.size)]] = odd[:min(n, odd.size)]
    mask = rs.choice(np.array([0.0, 0.5, 1.0], F), size=n)
    noise = rs.normal(size=(3, n, 3)).astype(F)
    if n > 4:
        nrm[1] = 0.0                       # the eps clamp of l2_normalize
        nrm[2] = np.nan
        noise[:, 3, 1] = np.nan
        mask[1:4] = 1.0                    # ... on mirror rays
        nrm[4, 0] = -0.0                   # a -0 component stays -0 where the std is 0
    roughness = np.array([0.0 if k % 2 else 0.01 * (k + 1) for k in range(K)], F)
    return dict(rays=rays, xs=xs, nrm=nrm, index=index, mask=mask, noise=noise, roughness=roughness)


def hip_rough_rows(index, mask, roughness, scene, any_in=0, shift=0, null_flag=False):
    L, p = _L().lib(), _L().ptr
    n, K = mask.shape[0], len(roughness)
    d_index = None if index is None else torch.cat([torch.zeros(shift, dtype=torch.int32, device=DEV), _t(index)])[shift:]
    d_mask = Buf(mask, shift=shift)
    std, jm = Buf(shape=(n,), shift=shift), Buf(shape=(n,), shift=shift)
    flag = torch.tensor([GUARD_WORD, any_in, GUARD_WORD], dtype=torch.int32, device=DEV)
    row = (ctypes.c_float * max(K, 1))(*[float(v) for v in roughness])
    code = L.mnrf_rough_rows(None if d_index is None else ctypes.c_void_p(d_index.data_ptr()), d_mask.ptr, n, K, row if K else None,
                             float(scene), std.ptr, jm.ptr, None if null_flag else p(flag[1:2]), _L().stream())
    assert code == 0, L.mnrf_last_error()
    _same(d_mask.get(), mask, "mask (an input)")
    return dict(std_rows=std.get(), jitter_mask=jm.get(), any=flag.cpu().numpy().tolist())


def hip_perturb(nrm, noise, std_rows, shift=0):
    n = nrm.shape[0]
    a, b, s, out = Buf(nrm, shift=shift), Buf(noise, shift=shift), Buf(std_rows, shift=shift), Buf(shape=(n, 3), shift=shift)
    assert _L().lib().mnrf_perturb_normals(a.ptr, b.ptr, s.ptr, n, out.ptr, _L().stream()) == 0, _L().lib().mnrf_last_error()
    return out.get()


def hip_fan_rows(c, noise, std_rows, index, n_jit, shift=0):
    """noise: (n_jit, n, 3) or None for the null pointer."""
    p = _L().ptr
    n, m = c["rays"].shape[0], index.shape[0]
    rays, sec = Buf(c["rays"], shift=shift), Buf(shape=(n_jit * m, 8), shift=shift)
    d = [_t(c["xs"]), _t(c["nrm"]), None if noise is None else _t(noise), _t(std_rows), _t(index)]
    code = _L().lib().mnrf_reflect_jitter_fan_rows(rays.ptr, p(d[0]), p(d[1]), p(d[2]), p(d[3]), p(d[4]), m, n, n_jit, NEAR2, sec.ptr,
                                                   _L().stream())
    assert code == 0, _L().lib().mnrf_last_error()
    return sec.get()


# ------------------------------------------------------------------------------------------------ mnrf_rough_rows
@pytest.mark.parametrize("K", COUNTS)
@pytest.mark.parametrize("n", SIZES)
def test_rough_rows_bit_exact(n, K):
    c = case(n, K, 100 * n + K)
    for scene in (0.0, 0.02):
        for index in (c["index"], None):
            for shift in (0, 1):
                want = RW.rough_rows_ref(index, c["mask"], c["roughness"], scene, any_in=4)
                got = hip_rough_rows(index, c["mask"], c["roughness"], scene, any_in=4, shift=shift)
                tag = f"n={n} K={K} scene={scene} index={'given' if index is not None else 'null'} shift={shift}"
                _same(got["std_rows"], want["std_rows"], tag + " std_rows")
                _same(got["jitter_mask"], want["jitter_mask"], tag + " jitter_mask")
                assert got["any"] == [GUARD_WORD, want["any"], GUARD_WORD], tag
    # what the case holds: the rule's own statements on this case, independent of the restatement's code
    want = RW.rough_rows_ref(c["index"], c["mask"], c["roughness"], 0.02)
    outside = (c["index"] < 0) | (c["index"] >= K)
    assert (want["std_rows"][outside] == F(0.02)).all()
    if K and n >= 8:
        assert (c["index"] == K - 1).any() and (want["std_rows"][c["index"] == K - 1] == c["roughness"][K - 1]).all()
    assert set(np.unique(want["jitter_mask"]).tolist()) <= {0.0, 1.0}
    assert not want["jitter_mask"][c["mask"] == 0].any() and not want["jitter_mask"][want["std_rows"] == 0].any()


@pytest.mark.parametrize("idx", [None, 0, 63, 64, 255, 256, 320])
def test_any_flag(idx):
    """n = 321: the flag is the OR over J of every wave, the tail wave of the second block included -- untouched while J is empty,
    OR-ed with 1 for exactly one ray of J wherever it sits; the caller's other bits stay; a null flag is skipped."""
    n = 321
    index = np.zeros(n, np.int32)                      # every ray took mirror 0, which is polished ...
    mask = np.ones(n, F)
    if idx is not None:
        index[idx] = 1                                 # ... but one, which took the frosted mirror
    for any_in, flag in ((0, int(idx is not None)), (4, 4 | int(idx is not None))):
        got = hip_rough_rows(index, mask, [0.0, 0.03], 0.01, any_in=any_in)
        assert got["any"] == [GUARD_WORD, flag, GUARD_WORD], (idx, any_in, got["any"])
        assert int(got["jitter_mask"].sum()) == int(idx is not None) and (idx is None or got["jitter_mask"][idx] == 1.0)
    got = hip_rough_rows(index, mask, [0.0, 0.03], 0.01, any_in=6, null_flag=True)
    assert got["any"] == [GUARD_WORD, 6, GUARD_WORD]
    # a mirror ray of the scene's own with the mask alone deciding: mask 0 keeps a ray with std > 0 out of J
    mask[:] = 0.0
    assert hip_rough_rows(None, mask, [], 0.01)["any"][1] == 0


# ------------------------------------------------------------------------------------------------ mnrf_perturb_normals
@pytest.mark.parametrize("n", SIZES)
def test_perturb_normals_bit_exact(n):
    for K in COUNTS:
        c = case(n, K, 100 * n + K)
        std = RW.rough_rows_ref(c["index"], c["mask"], c["roughness"], 0.0 if K else 0.02)["std_rows"]
        want = RW.perturb_normals_ref(c["nrm"], c["noise"][0], std)
        for shift in (0, 1):
            _same(hip_perturb(c["nrm"], c["noise"][0], std, shift), want, f"n={n} K={K} shift={shift}")
        rows = std == 0
        _same(want[rows], c["nrm"][rows], "std 0: the normal itself, a -0 and a NaN draw's row included")
    if n > 4:
        all0 = hip_perturb(c["nrm"], c["noise"][0], np.zeros(n, F))
        _same(all0, c["nrm"], "every std 0")
        assert np.signbit(all0[4, 0]) and np.isnan(hip_perturb(c["nrm"], c["noise"][0], np.full(n, F(0.01)))[3, 1])


@pytest.mark.parametrize("n", SIZES)
def test_perturb_then_reflect_is_reflect_with_the_noise(n):
    """mnrf_perturb_normals and mnrf_reflect_compact without noise against mnrf_reflect_compact with the noise and the std:
    secondary rays, index and reflect_dir, compacted and not."""
    from mirror_nerf_amd import recursion as R
    c = case(n, 3, 7 * n)
    rays, xs, nrm, noise, mask = _t(c["rays"]), _t(c["xs"]), _t(c["nrm"]), _t(c["noise"][0]), _t(c["mask"])
    for std in (0.01, 0.3):
        pert = R._perturb_normals(nrm, noise, torch.full((n,), std, device=DEV))
        for compact in (True, False):
            a = R._reflect(rays, xs, pert, mask, compact)
            b = R._reflect(rays, xs, nrm, mask, compact, noise, std)
            for got, want, what in zip(a, b, ("sec", "index", "reflect_dir")):
                if want is None:
                    assert got is None
                elif want.dtype == torch.int32:
                    assert torch.equal(got, want), what
                else:
                    _same(got.cpu().numpy(), want.cpu().numpy(), f"n={n} std={std} compact={compact} {what}")


# ------------------------------------------------------------------------------------------------ mnrf_reflect_jitter_fan_rows
@pytest.mark.parametrize("n_jit", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_fan_rows_bit_exact(n, n_jit):
    L, p = _L().lib(), _L().ptr
    for K in COUNTS:
        c = case(n, K, 100 * n + K)
        rows = RW.rough_rows_ref(c["index"], c["mask"], c["roughness"], 0.02 if K != 1 else 0.0)
        std = rows["std_rows"]
        for name, index in (("J", np.nonzero(rows["jitter_mask"])[0].astype(np.int32)), ("every ray", np.arange(n, dtype=np.int32))):
            if index.size == 0:
                continue
            noise = c["noise"][:n_jit]
            for shift in (0, 1):
                for dn in (noise, None):
                    want = RW.reflect_jitter_fan_rows_ref(c["rays"], c["xs"], c["nrm"], noise if dn is not None else (n_jit, None), std, index, NEAR2)
                    _same(hip_fan_rows(c, dn, std, index, n_jit, shift), want, f"n={n} K={K} {name} n_jit={n_jit} shift={shift} noise={'given' if dn is not None else 'null'}")
            if index.size > 1:       # a row whose index is outside the chunk is not written
                bad = index.copy()
                bad[0], bad[-1] = -1, n
                got = hip_fan_rows(c, noise, std, bad, n_jit).reshape(n_jit, index.size, 8)
                want = RW.reflect_jitter_fan_rows_ref(c["rays"], c["xs"], c["nrm"], noise, std, index, NEAR2).reshape(n_jit, index.size, 8).copy()
                want[:, [0, -1]] = SENT
                _same(got, want, f"n={n} K={K} {name}: rows outside the chunk")
    # one std on every row: the uniform fan, bit for bit
    index = np.arange(0, n, 2, dtype=np.int32)
    d = [_t(c[k]) for k in ("rays", "xs", "nrm")] + [_t(c["noise"][:n_jit]), _t(index)]
    for s in (0.05, 0.0):
        sec = torch.full((n_jit * index.size, 8), SENT, device=DEV)
        assert L.mnrf_reflect_jitter_fan(p(d[0]), p(d[1]), p(d[2]), p(d[3]), s, p(d[4]), index.size, n, n_jit, NEAR2, p(sec), _L().stream()) == 0
        _same(hip_fan_rows(c, c["noise"][:n_jit], np.full(n, F(s)), index, n_jit), sec.cpu().numpy(), f"n={n} n_jit={n_jit} std={s}: the uniform fan")
        _same(sec.cpu().numpy(), RR.reflect_jitter_fan_ref(c["rays"], c["xs"], c["nrm"], c["noise"][:n_jit], s, index, NEAR2), "the uniform fan's own restatement")


def test_fan_rows_with_no_row_touches_nothing():
    """m == 0 returns 0 without a launch, whatever the pointers are."""
    L = _L().lib()
    sec = Buf(shape=(4, 8))
    assert L.mnrf_reflect_jitter_fan_rows(None, None, None, None, None, None, 0, 65, 3, NEAR2, sec.ptr, _L().stream()) == 0
    torch.cuda.synchronize()
    assert (sec.get() == F(SENT)).all()
    assert L.mnrf_rough_rows(None, None, 0, 0, None, 0.0, None, None, None, _L().stream()) == 0
    assert L.mnrf_perturb_normals(None, None, None, 0, None, _L().stream()) == 0
