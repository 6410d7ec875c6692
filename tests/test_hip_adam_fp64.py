"""csrc/mnrf_optim.hip against tests/adam_ref.py (torch.optim.Adam's update in float64): all four entry points -- mnrf_adam_step,
mnrf_adam_prep, mnrf_adam_step_dev, mnrf_adam_step_dev_n -- and training.FlatAdam's device-state path over them.

A block of the kernel takes 256 threads x 4 = 1024 elements; the sizes (adam_ref.SIZES) are the ragged tails of one float4, one
block less and more than a float4, and a fourth block of two elements.  Every tensor sits at a 16-byte aligned offset inside a
larger buffer of sentinels, which must survive on both sides.

Bounds of one step (adam_ref.bounds; u = 2^-24, G = |g| / grad_scale + weight_decay |p|), from the count of float32 roundings on
each path of adam_body (written out in adam_ref's docstring: 8, 13 and 16 at most, rounded up):
    exp_avg     8 u (|m| + (1 - beta1)(G + |m|)) + 2^-149
    exp_avg_sq  16 u (beta2 v + (1 - beta2) G^2) + 2^-149
    param       16 u (|p'| + |update|) + 2^-149
The float32 emulation of the kernel's operation order reaches 3.4, 5.9 and 8.4 of those units on these cases
(tests/test_adam_ref_cpu.py); with 1.f - (float)beta in place of (float)(1 - beta) it reaches 220 in exp_avg_sq and 109 in param.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import adam_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 8                                            # sentinel floats on either side (the tail up to the next float4 as well)
SENTINELS = {"p": -724001.0, "g": -724002.0, "m": -724003.0, "v": -724004.0}
NAMES = ("param", "exp_avg", "exp_avg_sq")


def _lib():
    from mirror_nerf_amd import _lib as B
    return B, B.lib()


class Box:
    """p, g, m, v of n floats, each inside its own buffer of sentinels at a 16-byte aligned offset."""

    def __init__(self, arrays, shift=0):
        self.n = len(arrays[0])
        self.buf, self.t = {}, {}
        for k, a in zip("pgmv", arrays):
            buf = torch.full((PAD + self.n + (-self.n) % 4 + PAD,), SENTINELS[k], dtype=torch.float32, device=DEV)
            buf[PAD:PAD + self.n].copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
            self.buf[k], self.t[k] = buf, buf[PAD + shift:PAD + shift + self.n]
            assert (self.t[k].data_ptr() - 4 * shift) % 16 == 0
        self.g0 = np.ascontiguousarray(arrays[1], dtype=np.float32)

    def ptrs(self):
        return [ctypes.c_void_p(self.t[k].data_ptr()) for k in "pgmv"]

    def read(self):
        """(p, m, v) as numpy float32 after checking that every sentinel, and the gradient, are as they were."""
        out = {}
        for k in "pgmv":
            h = self.buf[k].cpu().numpy()
            s = np.float32(SENTINELS[k])
            assert np.all(h[:PAD] == s), f"{k}: the sentinel in front was overwritten ({h[:PAD]})"
            assert np.all(h[PAD + self.n:] == s), f"{k}: the sentinel behind was overwritten ({h[PAD + self.n:]})"
            out[k] = h[PAD:PAD + self.n].copy()
        assert _same_bits(out["g"], self.g0), "the gradient was written to"
        return out["p"], out["m"], out["v"]


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))


def _dev(value, dtype):
    return torch.tensor([value], dtype=dtype, device=DEV)


def _scalar(value):
    return None if value is None else _dev(value, torch.float32)


def _hyper_dev(hyper):
    return torch.tensor([hyper[k] for k in ("lr", "beta1", "beta2", "eps", "weight_decay")], dtype=torch.float64, device=DEV)


def _adam_step(box, hyper, calls, skipped=0, grad_scale=None, found_inf=None):
    """mnrf_adam_step on the box -> *skipped afterwards."""
    B, L = _lib()
    sk = _dev(skipped, torch.int32)
    gs, fi = _scalar(grad_scale), _scalar(found_inf)
    B.check(L.mnrf_adam_step(*box.ptrs(), box.n, hyper["lr"], hyper["beta1"], hyper["beta2"], hyper["eps"], hyper["weight_decay"],
                             calls, B.ptr(sk), B.ptr(gs), B.ptr(fi), B.stream()), "mnrf_adam_step")
    return int(sk.item())


def _prep(hyper, calls, skipped=0, grad_scale=None, found_inf=None, guards=(), n_guards=None):
    """mnrf_adam_prep for the call that makes the device count `calls` -> (return code, state tensor, step tensor, skipped tensor)."""
    B, L = _lib()
    hy = None if hyper is None else _hyper_dev(hyper)
    step, sk = _dev(calls - 1, torch.int64), _dev(skipped, torch.int32)
    gs, fi = _scalar(grad_scale), _scalar(found_inf)
    state = torch.full((B.MNRF_ADAM_STATE_FLOATS + 2,), -1.0, dtype=torch.float32, device=DEV)
    gw = (ctypes.c_void_p * len(guards))(*[None if w is None else w.data_ptr() for w in guards]) if guards else None
    rc = L.mnrf_adam_prep(B.ptr(hy), B.ptr(step), B.ptr(sk), B.ptr(gs), B.ptr(fi), gw,
                          len(guards) if n_guards is None else n_guards, B.ptr(state), B.stream())
    torch.cuda.synchronize()
    return rc, state, step, sk, (hy, gs, fi, guards)


def _step_dev(box, state, skipped_t):
    B, L = _lib()
    B.check(L.mnrf_adam_step_dev(*box.ptrs(), box.n, B.ptr(state), B.ptr(skipped_t), B.stream()), "mnrf_adam_step_dev")


def _step_dev_n(boxes, state, skipped_ts, n_tensors=None):
    B, L = _lib()
    k = len(boxes)
    arr = lambda i: (ctypes.c_void_p * max(k, 1))(*[b.t["pgmv"[i]].data_ptr() for b in boxes])  # noqa: E731
    return L.mnrf_adam_step_dev_n(k if n_tensors is None else n_tensors, arr(0), arr(1), arr(2), arr(3),
                                  (ctypes.c_int64 * max(k, 1))(*[b.n for b in boxes]), B.ptr(state),
                                  (ctypes.c_void_p * max(k, 1))(*[t.data_ptr() for t in skipped_ts]), B.stream())


@pytest.mark.parametrize("n", R.SIZES)
def test_one_step_against_float64(n):
    """mnrf_adam_step, one step from adam_ref.inputs(n), for every weight decay, gradient scale and step of adam_ref.cases() -- the
    steps 1 .. 2^31 + 5, a count that advanced past skipped calls and the clamp of calls - skipped at 1 -- param, exp_avg and
    exp_avg_sq each inside adam_ref.bounds of step64, sentinels and gradient untouched, *skipped unchanged."""
    arrays = R.inputs(n)
    worst, failed = {k: 0.0 for k in NAMES}, []
    for wd, gs, calls, skipped in R.cases():
        hyper, t = R.hyper_of(wd), R.effective_step(calls, skipped)
        box = Box(arrays)
        assert _adam_step(box, hyper, calls, skipped, gs) == skipped
        got = dict(zip(NAMES, box.read()))
        want = dict(zip(NAMES, R.step64(*arrays, hyper, t, gs)))
        sc, bd = R.scales(*arrays, hyper, t, gs), R.bounds(*arrays, hyper, t, gs)
        for k in NAMES:
            e = R.in_units(got[k], want[k], sc[k])
            worst[k] = max(worst[k], e)
            if not np.all(np.abs(got[k].astype(np.float64) - want[k]) <= bd[k]):
                failed.append((k, wd, gs, calls, skipped, round(e, 1)))
    print(f"n={n}: worst error in units of u * scale (bounds {R.FACTORS}): {worst}")
    assert not failed, failed[:12]


@pytest.mark.parametrize("n", R.SIZES)
def test_veto_changes_nothing_and_counts_once(n):
    """found_inf = 1 leaves p, m and v bit for bit and raises *skipped by exactly one however many blocks run; found_inf = 0 is the
    step that a null found_inf takes."""
    arrays = R.inputs(n)
    hyper = R.hyper_of(1e-3)
    box = Box(arrays)
    assert _adam_step(box, hyper, 4, 2, 3.0, found_inf=1.0) == 3
    for got, was in zip(box.read(), (arrays[0], arrays[2], arrays[3])):
        assert _same_bits(got, was)
    a, b = Box(arrays), Box(arrays)
    assert _adam_step(a, hyper, 4, 2, 3.0, found_inf=0.0) == 2 and _adam_step(b, hyper, 4, 2, 3.0) == 2
    ra, rb = a.read(), b.read()
    bd = R.bounds(*arrays, hyper, 2, 3.0)
    for k, x, y, w in zip(NAMES, ra, rb, R.step64(*arrays, hyper, 2, 3.0)):
        assert _same_bits(x, y), k
        assert np.all(np.abs(x.astype(np.float64) - w) <= bd[k]), k


def _ulps(a, b):
    return np.abs(np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64) - np.asarray(b, dtype=np.float32).view(np.int32).astype(np.int64))


def test_prep_publishes_the_scalars_of_the_step():
    """state[0..8) of mnrf_adam_prep = adam_ref.state64 rounded to float32, exactly -- but for lr / bias correction 1 and sqrt(bias
    correction 2), which may be one float32 ulp off (the device's double pow may differ from the host's in its last bit, and the
    kernel divides in float) -- nothing written behind them; *step grows by one per call, vetoed or not, *skipped is only read."""
    B, _ = _lib()
    K = B.MNRF_ADAM_STATE_FLOATS
    assert K == 8
    for wd in R.WEIGHT_DECAYS:
        for gs in R.GRAD_SCALES:
            for calls, skipped in [(t, 0) for t in R.STEPS] + list(R.SKIPPED_CASES):
                for found in (None, 0.0, 1.0):
                    hyper = R.hyper_of(wd, lr=3.3e-4 if wd else 5e-4)
                    rc, state, step, sk, _keep = _prep(hyper, calls, skipped, gs, found)
                    assert rc == 0
                    got = state.cpu().numpy()
                    want = R.state64(hyper, R.effective_step(calls, skipped), gs, veto=found == 1.0).astype(np.float32)
                    d = _ulps(got[:K], want)
                    assert np.all(d[[0, 3, 4, 5, 6, 7]] == 0) and d[1] <= 1 and d[2] <= 1, (wd, gs, calls, skipped, found, got, want)
                    assert np.all(got[K:] == -1.0)
                    assert int(step.item()) == calls and int(sk.item()) == skipped
    # the same count tensor through three calls, the middle one vetoed
    B, L = _lib()
    hy = _hyper_dev(R.hyper_of())
    step, sk, state = _dev(0, torch.int64), _dev(0, torch.int32), torch.zeros(K, device=DEV)
    for i, found in enumerate((0.0, 1.0, 0.0)):
        fi = _scalar(found)
        B.check(L.mnrf_adam_prep(B.ptr(hy), B.ptr(step), B.ptr(sk), None, B.ptr(fi), None, 0, B.ptr(state), B.stream()), "mnrf_adam_prep")
        assert int(step.item()) == i + 1 and float(state[0].item()) == found


def test_prep_guard_words_and_refusals():
    """Each of one to four guard words vetoes when it alone is non-zero, none does when all are zero; five words, a null word and a
    null hyper are refused (and nothing is launched: the count stays)."""
    hyper = R.hyper_of()
    for k in range(1, 5):
        for hot in [None] + list(range(k)):
            words = [torch.tensor([0 if i != hot else 1 << (3 * i)], dtype=torch.int32, device=DEV) for i in range(k)]
            rc, state, step, _sk, _keep = _prep(hyper, 7, 0, guards=words)
            assert rc == 0 and float(state[0].item()) == (0.0 if hot is None else 1.0), (k, hot)
            assert int(step.item()) == 7
    words = [torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(5)]
    rc, state, step, _sk, _keep = _prep(hyper, 7, 0, guards=words)
    assert rc != 0 and int(step.item()) == 6 and float(state[0].item()) == -1.0
    rc, state, step, _sk, _keep = _prep(hyper, 7, 0, guards=[words[0], None, words[2]])
    assert rc != 0 and int(step.item()) == 6
    rc, state, step, _sk, _keep = _prep(hyper, 7, 0, guards=(), n_guards=2)          # a count without the array
    assert rc != 0 and int(step.item()) == 6
    rc, state, step, _sk, _keep = _prep(None, 7, 0)
    assert rc != 0 and int(step.item()) == 6


DEV_CASES = ((0.0, None, 1, 0), (1e-3, 3.0, 10, 0), (1e-3, 65536.0, 2 ** 31 + 5, 0), (0.0, 3.0, 10, 3), (1e-3, 65536.0, 3, 5))


@pytest.mark.parametrize("n", R.SIZES)
def test_step_dev_after_prep_is_step_bit_for_bit(n):
    """mnrf_adam_prep + mnrf_adam_step_dev against mnrf_adam_step given the same scalars on the host: both form the scalars of the
    step on the device with the same expressions, so the results are the same bits.  With and without a gradient scale."""
    arrays = R.inputs(n)
    for wd, gs, calls, skipped in DEV_CASES:
        hyper = R.hyper_of(wd)
        a, b = Box(arrays), Box(arrays)
        assert _adam_step(a, hyper, calls, skipped, gs) == skipped
        rc, state, _step, sk, _keep = _prep(hyper, calls, skipped, gs)
        assert rc == 0
        _step_dev(b, state, sk)
        for k, x, y in zip(NAMES, a.read(), b.read()):
            assert _same_bits(x, y), (k, wd, gs, calls, skipped)
        assert int(sk.item()) == skipped


@pytest.mark.parametrize("sizes", [(1027, 5, 4096), (3, 1025)])
def test_step_dev_n_with_tensors_of_unequal_length(sizes):
    """One launch over tensors of unequal length (blockIdx.x runs past the shorter ones) = mnrf_adam_step_dev one tensor at a time,
    bit for bit, sentinels intact; a veto raises each tensor's own skip count by exactly one and changes nothing."""
    hyper = R.hyper_of(1e-3)
    inputs = [R.inputs(n, seed=j + 1) for j, n in enumerate(sizes)]
    rc, state, _step, sk0, _keep = _prep(hyper, 10, 3, 3.0)
    assert rc == 0
    together, single = [Box(a) for a in inputs], [Box(a) for a in inputs]
    sks = [_dev(3 + j, torch.int32) for j in range(len(sizes))]
    assert _step_dev_n(together, state, sks) == 0
    for j, (bt, bs) in enumerate(zip(together, single)):
        _step_dev(bs, state, sk0)
        rt, rs = bt.read(), bs.read()
        bd = R.bounds(*inputs[j], hyper, 7, 3.0)
        for k, x, y, w in zip(NAMES, rt, rs, R.step64(*inputs[j], hyper, 7, 3.0)):
            assert _same_bits(x, y), (j, k)
            assert np.all(np.abs(x.astype(np.float64) - w) <= bd[k]), (j, k)
    assert [int(t.item()) for t in sks] == [3 + j for j in range(len(sizes))]
    # vetoed
    rc, vetoed, _step, _sk, _keep = _prep(hyper, 10, 3, 3.0, found_inf=1.0)
    boxes = [Box(a) for a in inputs]
    assert rc == 0 and _step_dev_n(boxes, vetoed, sks) == 0
    assert [int(t.item()) for t in sks] == [4 + j for j in range(len(sizes))]
    for b, a in zip(boxes, inputs):
        for got, was in zip(b.read(), (a[0], a[2], a[3])):
            assert _same_bits(got, was)


def test_step_dev_n_refusals():
    """No tensor is a no-op, five are refused, and so is a tensor 4 bytes off its 16-byte alignment -- in either entry point, before
    anything is launched."""
    B, L = _lib()
    hyper = R.hyper_of()
    rc, state, _step, sk, _keep = _prep(hyper, 1)
    arrays = R.inputs(1027)
    assert L.mnrf_adam_step_dev_n(0, None, None, None, None, None, B.ptr(state), None, B.stream()) == 0
    boxes = [Box(arrays) for _ in range(5)]
    sks = [_dev(0, torch.int32) for _ in range(5)]
    assert _step_dev_n(boxes, state, sks) != 0
    assert _step_dev_n(boxes[:4], state, sks[:4], n_tensors=-1) != 0
    off = [Box(arrays), Box(arrays, shift=1)]
    assert _step_dev_n(off, state, sks[:2]) != 0
    assert L.mnrf_adam_step_dev(*off[1].ptrs(), off[1].n, B.ptr(state), B.ptr(sk), B.stream()) != 0
    assert L.mnrf_adam_step(*off[1].ptrs(), off[1].n, 5e-4, 0.9, 0.999, 1e-8, 0.0, 1, B.ptr(sk), None, None, B.stream()) != 0
    torch.cuda.synchronize()
    for b in boxes + off[:1]:
        for got, was in zip(b.read(), (arrays[0], arrays[2], arrays[3])):
            assert _same_bits(got, was)
    assert [int(t.item()) for t in sks] == [0] * 5


def _twenty_steps(weight_decay):
    """-> {"kernel" | "torch": {quantity: largest deviation from the float64 run over twenty steps, in units of u * scale}}."""
    n = 20 * R.BLOCK + 3
    hyper = R.hyper_of(weight_decay)
    p0 = R.inputs(n)[0]
    a = torch.nn.Parameter(torch.from_numpy(p0.copy()).to(DEV))
    opt = torch.optim.Adam([a], lr=R.f32(hyper["lr"]), betas=(hyper["beta1"], hyper["beta2"]), eps=R.f32(hyper["eps"]),
                           weight_decay=R.f32(hyper["weight_decay"]), fused=True)
    zeros = np.zeros(n, dtype=np.float32)
    box = Box((p0, zeros, zeros, zeros))
    ref = (p0.astype(np.float64), np.zeros(n), np.zeros(n))
    worst = {"kernel": {k: 0.0 for k in NAMES}, "torch": {k: 0.0 for k in NAMES}}
    for t in range(1, 21):
        g = R.fresh_gradient(n, t)
        gd = torch.from_numpy(g).to(DEV)
        a.grad = gd.clone()
        opt.step()
        box.t["g"].copy_(gd)
        box.g0 = g
        assert _adam_step(box, hyper, t) == 0
        sc = R.scales(ref[0], g, ref[1], ref[2], hyper, t)
        ref = R.step64(ref[0], g, ref[1], ref[2], hyper, t)
        st = opt.state[a]
        got = {"kernel": box.read(), "torch": (a.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy())}
        for who, arrs in got.items():
            for k, x, w in zip(NAMES, arrs, ref):
                worst[who][k] = max(worst[who][k], R.in_units(x, w, sc[k], steps=t))
    return worst


def test_twenty_steps_beside_torch_fused_adam():
    """Twenty steps with fresh gradients, moments from zero: the kernel carries its float32 state, step64 its float64 state.  No
    tolerance fixed in advance: torch's fused Adam takes the same steps on the same device, and the kernel's largest deviation from
    the float64 run -- over the steps, in the units of the one-step test, for param, exp_avg and exp_avg_sq each -- may be at most
    twice torch's: both are float32 implementations with different, equally valid rounding orders.
    Weight decay is off here, so that the moments are functions of the gradients alone.  With it on, G = g + weight_decay p, and
    where g is small the moments inherit p's RELATIVE error -- which the one-step bound does not hold small: it allows 16 u
    |update|, and these inputs have parameters that start at exactly zero and consist of nothing but their updates.  There
    exp_avg_sq sits at (weight_decay p)^2 and deviates by p's relative error twice over, for which its unit has no term: measured
    with weight_decay = 1e-3, exp_avg_sq 170 (kernel) and 64 (torch, which forms the update in double), against 10.0 and 11.2
    without; param 93 and 124.
    The largest exp_avg deviation is in either case an element whose exp_avg has just cancelled against its gradient to a
    hundredth of what it was, and kept the rounding error of what it was: 2394 and 6591 units here, 10090 and 3952 with weight decay.
    Measured on an MI355X (units of u * scale; kernel, torch): param 102, 154; exp_avg 2394, 6591; exp_avg_sq 10.0, 11.2."""
    worst = _twenty_steps(0.0)
    print("twenty steps, largest deviation from float64 in units of u * scale:", worst)
    for k in NAMES:
        assert worst["kernel"][k] <= 2.0 * worst["torch"][k], (k, worst)


def _system():
    import mirror_nerf_amd as M
    from mirror_nerf_amd import training
    torch.manual_seed(0)
    return M.NeRFSystem(training.default_hparams(perturb=0.0, noise_std=0.0)).to(DEV)


def _set_grads(opt, grads):
    from mirror_nerf_amd.weights import params_of
    for m, flat in zip(opt.modules, grads):
        off = 0
        for q in params_of(m):
            q.grad = flat[off:off + q.numel()].view(q.shape).clone()
            off += q.numel()


def _step_dev_counted(opt, guard_words=()):
    """step_dev() with the host counts kept as GraphedTrainStep.__call__ keeps them."""
    opt.sync_hyper()
    opt.step_dev(guard_words)
    opt._calls += 1
    for i in opt._live_dev:
        opt._steps[i] += 1


def _same_optimizer_state(a, b):
    for i in range(len(a.flats)):
        assert torch.equal(a.flats[i].data, b.flats[i].data), ("param", i)
        assert torch.equal(a._m[i], b._m[i]), ("exp_avg", i)
        assert torch.equal(a._v[i], b._v[i]), ("exp_avg_sq", i)
        assert int(a._skipped[i].item()) == int(b._skipped[i].item()), ("skipped", i)


def test_flat_adam_step_dev_is_step_and_follows_a_loaded_state():
    """training.FlatAdam over a NeRFSystem's two models: three eager step_dev() calls (mnrf_adam_prep + mnrf_adam_step_dev_n) with
    hand-set gradients, the learning rate changed through param_groups[0] between the first two and the second vetoed by a guard
    word, against three step() calls (mnrf_adam_step, found_inf) on a twin: parameters, moments and skip counts bit for bit.  Then
    the state saved after the twin's first step is loaded into the optimizer that HAS device state (its device count stands at 3):
    its next step_dev() is the step of an optimizer built fresh from that state, the second step and not the fourth."""
    from mirror_nerf_amd import training
    sys_a, sys_b = _system(), _system()
    a = training.FlatAdam(list(sys_a.models.values()), lr=5e-4, weight_decay=1e-3)
    b = training.FlatAdam(list(sys_b.models.values()), lr=5e-4, weight_decay=1e-3)
    assert len(a.flats) == 2
    a.enable_device_state()
    gen = torch.Generator(device=DEV)
    gen.manual_seed(11)
    grads = [[torch.randn(fp.numel(), device=DEV, generator=gen) * 10.0 ** (torch.rand(fp.numel(), device=DEV, generator=gen) * 8 - 8)
              for fp in a.flats] for _ in range(4)]
    hot, cold = torch.tensor([4], dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    saved = None
    for k in range(3):
        if k == 1:
            a.param_groups[0]["lr"] = 2.5e-4
            b.param_groups[0]["lr"] = 2.5e-4
        _set_grads(a, grads[k])
        _set_grads(b, grads[k])
        _step_dev_counted(a, [cold, hot] if k == 1 else [cold, cold])
        if k == 1:
            b.found_inf = torch.ones((), device=DEV)
        b.step()
        _same_optimizer_state(a, b)
        if k == 0:
            saved = (b.state_dict(), [fp.data.clone() for fp in b.flats])
    assert [int(t.item()) for t in a._skipped] == [1, 1] and a._calls == b._calls == 3 and a._steps == b._steps == [3, 3]
    assert int(a._step_dev.item()) == 3
    assert not torch.equal(a.flats[0].data, saved[1][0])
    # resume from the state after the first step: into the optimizer with device state, and into a fresh one
    fresh = training.FlatAdam(list(sys_b.models.values()), lr=1e-3, weight_decay=0.0)
    for opt in (a, fresh):
        opt.load_state_dict(saved[0])
        for fp, src in zip(opt.flats, saved[1]):
            fp.data.copy_(src)
    fresh.enable_device_state()
    assert a.param_groups[0]["lr"] == 5e-4 and a._calls == 1
    for opt in (a, fresh):
        _set_grads(opt, grads[3])
        _step_dev_counted(opt, [cold])
    assert int(fresh._step_dev.item()) == 2
    assert int(a._step_dev.item()) == 2
    _same_optimizer_state(a, fresh)
