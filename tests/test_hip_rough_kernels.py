"""mnrf_reflect_jitter_fan and mnrf_jitter_mean (csrc/mnrf_rough.hip) against their numpy restatements (tests/rough_ref.py), bit
for bit: below, at and past one wavefront and one workgroup, every kind of mask, and the edge rows.  The fan is also held to
the kernel it replaces -- block j is mnrf_reflect_compact(compact=1) with draw j -- and the finish of the mean to torch's own
`tensor / (times + 1)` on the device, which is what settles how the kernel ends."""
import numpy as np
import pytest
import torch

from tests import rough_ref as RR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEAR2 = 0.1


def _L():
    from mirror_nerf_amd import _lib
    return _lib


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(got, want):
    """Bit for bit; a NaN matches a NaN (payloads are not compared)."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.int32)[~nan], want.view(np.int32)[~nan]))


def _fan(rays, xs, nrm, noise, std, index, n_jit):
    L, p = _L().lib(), _L().ptr
    m = index.shape[0]
    sec = torch.full((n_jit * m, 8), -7.0, device=DEV)
    code = L.mnrf_reflect_jitter_fan(p(rays), p(xs), p(nrm), p(noise), float(std), p(index), m, rays.shape[0], n_jit, NEAR2, p(sec),
                                     _L().stream())
    assert code == 0, L.mnrf_last_error()
    return sec


def _compact(rays, xs, nrm, noise, std, mask):
    from mirror_nerf_amd import recursion as R
    sec, index, _ = R._reflect(rays, xs, nrm, mask, True, noise, std, want_dir=False)
    return sec, index


def _inputs(n, seed):
    rs = np.random.RandomState(seed)
    rays = rs.normal(size=(n, 8)).astype(np.float32)
    xs = rs.normal(size=(n, 3)).astype(np.float32)
    nrm = rs.normal(size=(n, 3)).astype(np.float32)
    if n > 2:
        nrm[1] = 0.0           # the eps clamp of l2_normalize
        nrm[2] = np.nan
    return rs, rays, xs, nrm


def _masks(n, rs):
    first, last, every = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    first[0] = 1
    last[-1] = 1
    every[::2] = 1
    return {"first": first, "last": last, "all": np.ones(n, np.float32), "every_other": every,
            "about_40": (rs.uniform(size=n) < 0.4).astype(np.float32)}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025])
def test_fan_against_restatement_and_compaction(n):
    rs, rays, xs, nrm = _inputs(n, n)
    d_rays, d_xs, d_nrm = _t(rays), _t(xs), _t(nrm)
    for name, mask in _masks(n, rs).items():
        idx = np.nonzero(mask)[0].astype(np.int32)
        if idx.size == 0:
            continue
        d_idx, d_mask = _t(idx), _t(mask)
        for n_jit in (1, 2, 3, 5):
            noise = rs.normal(size=(n_jit, n, 3)).astype(np.float32)
            d_noise = _t(noise)
            for kind, dn, std in (("given", d_noise, 0.05), ("null", None, 0.05), ("std0", d_noise, 0.0)):
                got = _fan(d_rays, d_xs, d_nrm, dn, std, d_idx, n_jit)
                want = RR.reflect_jitter_fan_ref(rays, xs, nrm, noise if dn is not None else (n_jit, None), std, idx, NEAR2)
                assert _same(got.cpu().numpy(), want), (n, name, n_jit, kind)
                blocks = got.view(n_jit, idx.size, 8)
                for j in range(n_jit):                                   # the kernel it replaces
                    sec, index = _compact(d_rays, d_xs, d_nrm, dn[j].contiguous() if dn is not None else None, std, d_mask)
                    assert torch.equal(index, d_idx)
                    assert _same(blocks[j].cpu().numpy(), sec.cpu().numpy()), (n, name, n_jit, kind, j)
    if n > 2:          # the edge rows were among the selected ones: the clamp gave a finite direction, the NaN normal NaNs
        got = _fan(d_rays, d_xs, d_nrm, None, 0.0, _t(np.array([1, 2], np.int32)), 1).cpu().numpy()
        assert np.isfinite(got[0]).all() and np.isnan(got[1, 3:6]).all() and np.isfinite(got[1, [0, 1, 2, 6, 7]]).all()


def test_fan_unaligned_rows_take_the_scalar_path():
    """A ray buffer or a destination that is not 16-byte aligned (a view at a 4-byte offset): the same rows."""
    rs, rays, xs, nrm = _inputs(130, 7)
    idx = np.arange(0, 130, 3).astype(np.int32)
    noise = rs.normal(size=(2, 130, 3)).astype(np.float32)
    want = RR.reflect_jitter_fan_ref(rays, xs, nrm, noise, 0.05, idx, NEAR2)
    L, p = _L().lib(), _L().ptr
    flat = torch.zeros(130 * 8 + 1, device=DEV)
    flat[1:] = _t(rays).reshape(-1)
    out = torch.full((2 * idx.size * 8 + 1,), -7.0, device=DEV)
    import ctypes
    d_xs, d_nrm, d_noise, d_idx = _t(xs), _t(nrm), _t(noise), _t(idx)
    code = L.mnrf_reflect_jitter_fan(ctypes.c_void_p(flat.data_ptr() + 4), p(d_xs), p(d_nrm), p(d_noise), 0.05, p(d_idx),
                                     idx.size, 130, 2, NEAR2, ctypes.c_void_p(out.data_ptr() + 4), _L().stream())
    assert code == 0
    assert float(out[0]) == -7.0 and _same(out[1:].view(-1, 8).cpu().numpy(), want)


@pytest.mark.parametrize("m_n", [(1, 1), (1, 65), (63, 63), (64, 200), (65, 65), (257, 300), (1025, 1025), (410, 1025)])
def test_mean_against_restatement(m_n):
    m, n_acc = m_n
    rs = np.random.RandomState(m + n_acc)
    L, p = _L().lib(), _L().ptr
    for use_index in (False, True):
        rows = np.sort(rs.permutation(n_acc)[:m]).astype(np.int32) if use_index else None
        if rows is not None and m == 1:
            rows[:] = n_acc - 1                                          # a single row, the last
        for n_jit in (1, 2, 3, 5):
            acc = rs.normal(size=(n_acc, 3)).astype(np.float32)
            pieces = rs.normal(size=(n_jit, m, 3)).astype(np.float32)
            if m > 3:
                pieces[0, 1, 0] = np.inf
                pieces[n_jit - 1, 2, 1] = np.nan
            named = np.zeros(n_acc, bool)
            named[rows if rows is not None else np.arange(m)] = True
            acc[~named] = -12345.0                                       # sentinel rows: neither read nor written
            for mode, value in ((RR.MEAN_NONE, 0.0), (RR.MEAN_DIVIDE, float(n_jit + 1)),
                                (RR.MEAN_MULTIPLY, float(RR.finish_value(n_jit, RR.MEAN_MULTIPLY)))):
                d_acc, d_pieces = _t(acc), _t(pieces)
                d_rows = _t(rows) if rows is not None else None
                assert L.mnrf_jitter_mean(p(d_acc), p(d_pieces), p(d_rows), m, n_jit, n_acc, mode, value, _L().stream()) == 0
                got = d_acc.cpu().numpy()
                want = RR.jitter_mean_ref(acc, pieces, rows, mode, value)
                assert _same(got, want), (m_n, use_index, n_jit, mode)
                assert (got[~named] == -12345.0).all()
                if m > 3:
                    r1, r2 = (rows[1], rows[2]) if rows is not None else (1, 2)
                    assert np.isinf(got[r1, 0]) and np.isnan(got[r2, 1])
            if n_jit >= 2:                                               # two group calls, the last one finishing = one call
                value = float(RR.finish_value(n_jit, RR.DEVICE_FINISH))
                k = n_jit // 2
                one, two, d_all, d_head, d_tail = _t(acc), _t(acc), _t(pieces), _t(pieces[:k]), _t(pieces[k:])
                d_rows = _t(rows) if rows is not None else None
                assert L.mnrf_jitter_mean(p(one), p(d_all), p(d_rows), m, n_jit, n_acc, RR.DEVICE_FINISH, value, _L().stream()) == 0
                assert L.mnrf_jitter_mean(p(two), p(d_head), p(d_rows), m, k, n_acc, RR.MEAN_NONE, 0.0, _L().stream()) == 0
                assert L.mnrf_jitter_mean(p(two), p(d_tail), p(d_rows), m, n_jit - k, n_acc, RR.DEVICE_FINISH, value,
                                          _L().stream()) == 0
                assert _same(one.cpu().numpy(), two.cpu().numpy())


@pytest.mark.parametrize("count", [2, 3, 5, 65])
def test_finish_is_torchs_own_division(count):
    """`rgb / (trace_ray_times + 1)` as torch evaluates it on the device, against the kernel's finish as the driver asks for it
    (recursion.ROUGH_FINISH with the float the driver forms): torch.equal.  This comparison decides between a division and a
    multiplication by the reciprocal; the answer is written into include/mnrf.h and rough_ref.DEVICE_FINISH."""
    from mirror_nerf_amd import recursion as R
    L, p = _L().lib(), _L().ptr
    assert R.ROUGH_FINISH == RR.DEVICE_FINISH
    torch.manual_seed(count)
    n = 4099
    acc = torch.rand(n, 3, device=DEV) * (count - 1)
    piece = torch.rand(1, n, 3, device=DEV)
    want = (acc + piece[0]) / count
    value = float(RR.finish_value(count - 1, RR.DEVICE_FINISH))
    got = acc.clone()
    assert L.mnrf_jitter_mean(p(got), p(piece), None, n, 1, n, R.ROUGH_FINISH, value, _L().stream()) == 0
    assert torch.equal(got, want)
    want_np = RR.jitter_mean_ref(acc.cpu().numpy(), piece.cpu().numpy(), None, RR.DEVICE_FINISH, value)
    assert _same(got.cpu().numpy(), want_np)


def test_nothing_to_do_and_argument_errors():
    L, p = _L().lib(), _L().ptr
    E = _L().MNRF_ERR_ARG
    s = _L().stream()
    one = torch.zeros(8, device=DEV)
    idx = torch.zeros(1, dtype=torch.int32, device=DEV)
    # m == 0: nothing is launched, whatever the pointers are
    assert L.mnrf_reflect_jitter_fan(None, None, None, None, 0.0, None, 0, 5, 3, NEAR2, None, s) == 0
    assert L.mnrf_jitter_mean(None, None, None, 0, 1, 5, RR.MEAN_NONE, 0.0, s) == 0
    fan_ok = [p(one), p(one), p(one), None, 0.0, p(idx), 1, 1, 1, NEAR2, p(one)]
    for pos in (0, 1, 2, 5, 10):                                         # a null pointer (noise alone may be null)
        a = list(fan_ok)
        a[pos] = None
        assert L.mnrf_reflect_jitter_fan(*a, s) == E
        assert b"mnrf_reflect_jitter_fan" in L.mnrf_last_error()
    for pos, bad in ((6, -1), (7, -1), (8, 0), (8, -2), (6, 2)):         # negative sizes, n_jit < 1, m > n_rays
        a = list(fan_ok)
        a[pos] = bad
        assert L.mnrf_reflect_jitter_fan(*a, s) == E
    mean_ok = [p(one), p(one), None, 1, 1, 1, RR.MEAN_NONE, 0.0]
    for pos, bad in ((0, None), (1, None), (3, -1), (4, 0), (5, -1), (3, 2), (6, 3), (6, -1)):
        a = list(mean_ok)
        a[pos] = bad
        assert L.mnrf_jitter_mean(*a, s) == E
        assert b"mnrf_jitter_mean" in L.mnrf_last_error()
    torch.cuda.synchronize()
    assert float(one.abs().sum()) == 0.0
