"""The SGD and RAdam kernels of csrc/mnrf_optim.hip against tests/optim_ref.py (torch.optim.SGD's and torch.optim.RAdam's updates
in float64): all six entry points -- mnrf_sgd_step, mnrf_sgd_prep, mnrf_sgd_step_dev_n, mnrf_radam_step, mnrf_radam_prep,
mnrf_radam_step_dev_n -- and training.FlatSGD's / FlatRAdam's device-state path over them.

A block takes 256 threads x 4 = 1024 elements; the sizes (adam_ref.SIZES) are the ragged tails of one float4, one block less and
more than a float4, and a fourth block of two elements.  Every tensor sits at a 16-byte aligned offset inside a larger buffer of
sentinels, which must survive on both sides.

Bounds of one step (optim_ref.sgd_bounds / radam_bounds; u = 2^-24; the count of float32 roundings on each path is written out
in optim_ref's doc string), with G = |g| / grad_scale + weight_decay |p|:
    momentum_buffer  8 u (|momentum buf| + G) + 2^-147
    SGD param        2 u (|p'| + |update|) + lr * (the buffer's bound) + 2^-147
    exp_avg          8 u (|m| + (1 - beta1)(G + |m|)) + 2^-147
    exp_avg_sq       16 u (beta2 v + (1 - beta2) G^2) + 2^-147
    RAdam param      16 u (|p'| + |update|) rectified, 4 u not, + K * (exp_avg's bound) + 2^-147, K = d update / d exp_avg
The float32 emulations of the kernels' operation order reach 0.37 / 0.49 (SGD) and 0.42 / 0.37 / 0.27 (RAdam) of these bounds on
the same cases (tests/test_optim_ref_cpu.py).  RAdam's steps are 1, the last unrectified and the first rectified step for beta2 =
0.999 (computed from rho_t's formula: 5 and 6), 10, 1000, 100000 and 2^31 + 5."""
import ctypes

import numpy as np
import pytest
import torch

from tests import optim_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 8                                            # sentinel floats on either side (the tail up to the next float4 as well)
SENTINEL = {"p": -724001.0, "g": -724002.0, "m": -724003.0, "v": -724004.0, "b": -724005.0}


def _lib():
    from mirror_nerf_amd import _lib as B
    return B, B.lib()


class Box:
    """Tensors of n floats named by `keys` ("pgb" for SGD, "pgmv" for RAdam), each inside its own buffer of sentinels at a
    16-byte aligned offset."""

    def __init__(self, keys, arrays, shift=0):
        self.keys, self.n = keys, len(arrays[0])
        self.buf, self.t = {}, {}
        for k, a in zip(keys, arrays):
            buf = torch.full((PAD + self.n + (-self.n) % 4 + PAD,), SENTINEL[k], dtype=torch.float32, device=DEV)
            buf[PAD:PAD + self.n].copy_(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
            self.buf[k], self.t[k] = buf, buf[PAD + shift:PAD + shift + self.n]
            assert (self.t[k].data_ptr() - 4 * shift) % 16 == 0
        self.g0 = np.ascontiguousarray(arrays[1], dtype=np.float32)

    def ptrs(self):
        return [ctypes.c_void_p(self.t[k].data_ptr()) for k in self.keys]

    def read(self):
        """The tensors but the gradient, as numpy float32, after checking that every sentinel and the gradient are as they were."""
        out = {}
        for k in self.keys:
            h = self.buf[k].cpu().numpy()
            s = np.float32(SENTINEL[k])
            assert np.all(h[:PAD] == s), f"{k}: the sentinel in front was overwritten ({h[:PAD]})"
            assert np.all(h[PAD + self.n:] == s), f"{k}: the sentinel behind was overwritten ({h[PAD + self.n:]})"
            out[k] = h[PAD:PAD + self.n].copy()
        assert _same_bits(out["g"], self.g0), "the gradient was written to"
        return tuple(out[k] for k in self.keys if k != "g")


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.uint32), np.asarray(b, dtype=np.float32).view(np.uint32))


def _ulps(a, b):
    return np.abs(np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64) - np.asarray(b, dtype=np.float32).view(np.int32).astype(np.int64))


def _dev(value, dtype):
    return torch.tensor([value], dtype=dtype, device=DEV)


def _scalar(value):
    return None if value is None else _dev(value, torch.float32)


class Kind:
    """One optimizer's entry points, reference and inputs behind one face, so that every test below runs for both."""

    def __init__(self, name):
        self.name = name
        sgd = name == "sgd"
        self.keys = "pgb" if sgd else "pgmv"
        self.names = ("param", "momentum_buffer") if sgd else ("param", "exp_avg", "exp_avg_sq")
        self.hyper_keys = ("lr", "momentum", "weight_decay") if sgd else ("lr", "beta1", "beta2", "eps", "weight_decay")
        self.state_floats = "MNRF_SGD_STATE_FLOATS" if sgd else "MNRF_RADAM_STATE_FLOATS"
        self.hyper = R.sgd_hyper if sgd else R.radam_hyper
        self.cases = R.sgd_cases if sgd else R.radam_cases

    def inputs(self, n, seed=0):
        p, g, m, v = R.inputs(n, seed)
        return (p, g, m) if self.name == "sgd" else (p, g, m, v)

    def zeros(self, p0):
        z = np.zeros_like(p0)
        return (p0, z, z) if self.name == "sgd" else (p0, z, z, z)

    def box(self, arrays, shift=0):
        return Box(self.keys, arrays, shift)

    def want(self, arrays, hyper, t, gs):
        return R.sgd64(*arrays, hyper, gs) if self.name == "sgd" else R.radam64(*arrays, hyper, t, gs)

    def bounds(self, arrays, hyper, t, gs):
        return R.sgd_bounds(*arrays, hyper, gs) if self.name == "sgd" else R.radam_bounds(*arrays, hyper, t, gs)

    def scales(self, arrays, hyper, t, gs):
        return R.sgd_scales(*arrays, hyper, gs) if self.name == "sgd" else R.radam_scales(*arrays, hyper, t, gs)

    def state64(self, hyper, t, gs, veto):
        return R.sgd_state64(hyper, gs, veto) if self.name == "sgd" else R.radam_state64(hyper, t, gs, veto)

    def step(self, box, hyper, calls, skipped=0, grad_scale=None, found_inf=None):
        """The host-scalar entry point on the box -> *skipped afterwards."""
        B, L = _lib()
        sk = _dev(skipped, torch.int32)
        gs, fi = _scalar(grad_scale), _scalar(found_inf)
        fn = getattr(L, f"mnrf_{self.name}_step")
        B.check(fn(*box.ptrs(), box.n, *[hyper[k] for k in self.hyper_keys], calls, B.ptr(sk), B.ptr(gs), B.ptr(fi), B.stream()), self.name)
        return int(sk.item())

    def prep(self, hyper, calls, skipped=0, grad_scale=None, found_inf=None, guards=(), n_guards=None):
        """The prep launch for the call that makes the device count `calls` -> (return code, state, step, skipped, keep-alive)."""
        B, L = _lib()
        hy = None if hyper is None else torch.tensor([hyper[k] for k in self.hyper_keys], dtype=torch.float64, device=DEV)
        step, sk = _dev(calls - 1, torch.int64), _dev(skipped, torch.int32)
        gs, fi = _scalar(grad_scale), _scalar(found_inf)
        state = torch.full((getattr(B, self.state_floats) + 2,), -1.0, dtype=torch.float32, device=DEV)
        gw = (ctypes.c_void_p * len(guards))(*[None if w is None else w.data_ptr() for w in guards]) if guards else None
        rc = getattr(L, f"mnrf_{self.name}_prep")(B.ptr(hy), B.ptr(step), B.ptr(sk), B.ptr(gs), B.ptr(fi), gw,
                                                  len(guards) if n_guards is None else n_guards, B.ptr(state), B.stream())
        torch.cuda.synchronize()
        return rc, state, step, sk, (hy, gs, fi, guards)

    def step_dev_n(self, boxes, state, skipped_ts, n_tensors=None):
        B, L = _lib()
        k = len(boxes)
        arr = lambda key: (ctypes.c_void_p * max(k, 1))(*[b.t[key].data_ptr() for b in boxes])  # noqa: E731
        return getattr(L, f"mnrf_{self.name}_step_dev_n")(k if n_tensors is None else n_tensors, *[arr(key) for key in self.keys],
                                                          (ctypes.c_int64 * max(k, 1))(*[b.n for b in boxes]), B.ptr(state),
                                                          (ctypes.c_void_p * max(k, 1))(*[t.data_ptr() for t in skipped_ts]), B.stream())


KINDS = {"sgd": Kind("sgd"), "radam": Kind("radam")}
both = pytest.mark.parametrize("kind", list(KINDS.values()), ids=list(KINDS))


@both
@pytest.mark.parametrize("n", R.SIZES)
def test_one_step_against_float64(kind, n):
    """The host-scalar entry point, one step from adam_ref.inputs(n), for every weight decay, gradient scale, step and skipped count
    of the kind's cases: every quantity inside its bound of the float64 update, sentinels and gradient untouched, *skipped
    unchanged."""
    arrays = kind.inputs(n)
    worst, failed = {k: 0.0 for k in kind.names}, []
    for wd, gs, calls, skipped in kind.cases():
        hyper, t = kind.hyper(wd), R.effective_step(calls, skipped)
        box = kind.box(arrays)
        assert kind.step(box, hyper, calls, skipped, gs) == skipped
        got = dict(zip(kind.names, box.read()))
        want = dict(zip(kind.names, kind.want(arrays, hyper, t, gs)))
        bd = kind.bounds(arrays, hyper, t, gs)
        for k in kind.names:
            e = R.in_bound_units(got[k], want[k], bd[k])
            worst[k] = max(worst[k], e)
            if not np.all(np.abs(got[k].astype(np.float64) - want[k]) <= bd[k]):
                failed.append((k, wd, gs, calls, skipped, round(e, 2)))
    print(f"{kind.name} n={n}: worst error as a fraction of its bound: {worst}")
    assert not failed, failed[:12]


@both
@pytest.mark.parametrize("n", R.SIZES)
def test_veto_changes_nothing_and_counts_once(kind, n):
    """found_inf = 1 leaves every tensor bit for bit and raises *skipped by exactly one however many blocks run; found_inf = 0 is
    the step that a null found_inf takes."""
    arrays = kind.inputs(n)
    hyper = kind.hyper(1e-3)
    box = kind.box(arrays)
    assert kind.step(box, hyper, 9, 2, 3.0, found_inf=1.0) == 3
    for got, was in zip(box.read(), (arrays[0],) + tuple(arrays[2:])):
        assert _same_bits(got, was)
    a, b = kind.box(arrays), kind.box(arrays)
    assert kind.step(a, hyper, 9, 2, 3.0, found_inf=0.0) == 2 and kind.step(b, hyper, 9, 2, 3.0) == 2
    bd = kind.bounds(arrays, hyper, 7, 3.0)
    for k, x, y, w in zip(kind.names, a.read(), b.read(), kind.want(arrays, hyper, 7, 3.0)):
        assert _same_bits(x, y), k
        assert np.all(np.abs(x.astype(np.float64) - w) <= bd[k]), k


@both
def test_prep_publishes_the_scalars_of_the_step(kind):
    """The state block of the prep launch = the kind's state64 rounded to float32, exactly -- but for RAdam's lr / bias correction 1
    and sqrt(bias correction 2) r_t, which may be one float32 ulp off (the device's double pow may differ from the host's in its
    last bit, and the kernel divides in float), as Adam's test allows; RAdam's branch flag is exact at every step, the two threshold
    steps included; nothing is written behind the block; *step grows by one per call, vetoed or not, *skipped is only read."""
    B, L = _lib()
    K = getattr(B, kind.state_floats)
    loose = [] if kind.name == "sgd" else [1, 2]
    steps = (1, 2 ** 31 + 5) if kind.name == "sgd" else R.radam_steps()
    for wd in R.WEIGHT_DECAYS:
        for gs in R.GRAD_SCALES:
            for calls, skipped in [(t, 0) for t in steps] + list(R.SKIPPED_CASES) + [(9, 3), (9, 4)]:      # (effective steps 6 and 5)
                for found in (None, 0.0, 1.0):
                    hyper = kind.hyper(wd, lr=3.3e-4 if wd else 5e-4)
                    rc, state, step, sk, _keep = kind.prep(hyper, calls, skipped, gs, found)
                    assert rc == 0
                    got = state.cpu().numpy()
                    want = kind.state64(hyper, R.effective_step(calls, skipped), gs, found == 1.0).astype(np.float32)
                    d = _ulps(got[:K], want)
                    assert all(d[i] <= (1 if i in loose else 0) for i in range(K)), (wd, gs, calls, skipped, found, got, want)
                    assert np.all(got[K:] == -1.0)
                    assert int(step.item()) == calls and int(sk.item()) == skipped
    # the same count tensor through three calls, the middle one vetoed
    hy = torch.tensor([kind.hyper()[k] for k in kind.hyper_keys], dtype=torch.float64, device=DEV)
    step, sk, state = _dev(0, torch.int64), _dev(0, torch.int32), torch.zeros(K, device=DEV)
    for i, found in enumerate((0.0, 1.0, 0.0)):
        fi = _scalar(found)
        B.check(getattr(L, f"mnrf_{kind.name}_prep")(B.ptr(hy), B.ptr(step), B.ptr(sk), None, B.ptr(fi), None, 0, B.ptr(state), B.stream()), "prep")
        assert int(step.item()) == i + 1 and float(state[0].item()) == found


@both
def test_prep_guard_words_and_refusals(kind):
    """Each of one to four guard words vetoes when it alone is non-zero, none does when all are zero; five words, a null word and a
    null hyper block are refused (and nothing is launched: the count stays)."""
    hyper = kind.hyper()
    for k in range(1, 5):
        for hot in [None] + list(range(k)):
            words = [torch.tensor([0 if i != hot else 1 << (3 * i)], dtype=torch.int32, device=DEV) for i in range(k)]
            rc, state, step, _sk, _keep = kind.prep(hyper, 7, 0, guards=words)
            assert rc == 0 and float(state[0].item()) == (0.0 if hot is None else 1.0), (k, hot)
            assert int(step.item()) == 7
    words = [torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(5)]
    rc, state, step, _sk, _keep = kind.prep(hyper, 7, 0, guards=words)
    assert rc != 0 and int(step.item()) == 6 and float(state[0].item()) == -1.0
    rc, state, step, _sk, _keep = kind.prep(hyper, 7, 0, guards=[words[0], None, words[2]])
    assert rc != 0 and int(step.item()) == 6
    rc, state, step, _sk, _keep = kind.prep(hyper, 7, 0, guards=(), n_guards=2)
    assert rc != 0 and int(step.item()) == 6
    rc, state, step, _sk, _keep = kind.prep(None, 7, 0)
    assert rc != 0 and int(step.item()) == 6


# (weight decay, gradient scale, calls, skipped): the first step, both sides of RAdam's threshold (effective steps 5 and 6), a large count
DEV_CASES = ((0.0, None, 1, 0), (1e-3, 3.0, 5, 0), (1e-3, 65536.0, 9, 3), (0.0, 3.0, 10, 3), (1e-3, 65536.0, 2 ** 31 + 5, 0), (1e-3, 65536.0, 3, 5))


@both
@pytest.mark.parametrize("n", R.SIZES)
def test_step_dev_after_prep_is_step_bit_for_bit(kind, n):
    """The prep launch + the device-state update against the host-scalar entry point given the same scalars: both form the scalars
    of the step on the device with the same expressions, so the results are the same bits."""
    arrays = kind.inputs(n)
    for wd, gs, calls, skipped in DEV_CASES:
        hyper = kind.hyper(wd)
        a, b = kind.box(arrays), kind.box(arrays)
        assert kind.step(a, hyper, calls, skipped, gs) == skipped
        rc, state, _step, sk, _keep = kind.prep(hyper, calls, skipped, gs)
        assert rc == 0 and kind.step_dev_n([b], state, [sk]) == 0
        for k, x, y in zip(kind.names, a.read(), b.read()):
            assert _same_bits(x, y), (k, wd, gs, calls, skipped)
        assert int(sk.item()) == skipped


@both
@pytest.mark.parametrize("sizes", [(1027, 5, 4096), (3, 1025)])
def test_step_dev_n_with_tensors_of_unequal_length(kind, sizes):
    """One launch over tensors of unequal length (blockIdx.x runs past the shorter ones) = one tensor at a time, bit for bit,
    inside the bounds, sentinels intact; a veto raises each tensor's own skip count by exactly one and changes nothing."""
    hyper = kind.hyper(1e-3)
    inputs = [kind.inputs(n, seed=j + 1) for j, n in enumerate(sizes)]
    rc, state, _step, sk0, _keep = kind.prep(hyper, 10, 3, 3.0)
    assert rc == 0
    together, single = [kind.box(a) for a in inputs], [kind.box(a) for a in inputs]
    sks = [_dev(3 + j, torch.int32) for j in range(len(sizes))]
    assert kind.step_dev_n(together, state, sks) == 0
    for j, (bt, bs) in enumerate(zip(together, single)):
        assert kind.step_dev_n([bs], state, [sk0]) == 0
        bd = kind.bounds(inputs[j], hyper, 7, 3.0)
        for k, x, y, w in zip(kind.names, bt.read(), bs.read(), kind.want(inputs[j], hyper, 7, 3.0)):
            assert _same_bits(x, y), (j, k)
            assert np.all(np.abs(x.astype(np.float64) - w) <= bd[k]), (j, k)
    assert [int(t.item()) for t in sks] == [3 + j for j in range(len(sizes))] and int(sk0.item()) == 3
    rc, vetoed, _step, _sk, _keep = kind.prep(hyper, 10, 3, 3.0, found_inf=1.0)
    boxes = [kind.box(a) for a in inputs]
    assert rc == 0 and kind.step_dev_n(boxes, vetoed, sks) == 0
    assert [int(t.item()) for t in sks] == [4 + j for j in range(len(sizes))]
    for b, a in zip(boxes, inputs):
        for got, was in zip(b.read(), (a[0],) + tuple(a[2:])):
            assert _same_bits(got, was)


@both
def test_step_dev_n_refusals(kind):
    """No tensor is a no-op, five are refused, and so is a tensor 4 bytes off its 16-byte alignment -- in either entry point, before
    anything is launched."""
    B, L = _lib()
    hyper = kind.hyper()
    rc, state, _step, sk, _keep = kind.prep(hyper, 1)
    arrays = kind.inputs(1027)
    assert kind.step_dev_n([], state, []) == 0
    boxes = [kind.box(arrays) for _ in range(5)]
    sks = [_dev(0, torch.int32) for _ in range(5)]
    assert kind.step_dev_n(boxes, state, sks) != 0
    assert kind.step_dev_n(boxes[:4], state, sks[:4], n_tensors=-1) != 0
    off = [kind.box(arrays), kind.box(arrays, shift=1)]
    assert kind.step_dev_n(off, state, sks[:2]) != 0
    fn = getattr(L, f"mnrf_{kind.name}_step")
    assert fn(*off[1].ptrs(), off[1].n, *[hyper[k] for k in kind.hyper_keys], 1, B.ptr(sk), None, None, B.stream()) != 0
    torch.cuda.synchronize()
    for b in boxes + off[:1]:
        for got, was in zip(b.read(), (arrays[0],) + tuple(arrays[2:])):
            assert _same_bits(got, was)
    assert [int(t.item()) for t in sks] == [0] * 5


def _twenty_steps(kind):
    """-> {"kernel" | "torch": {quantity: largest deviation from the float64 run over twenty steps, in units of u * scale}}."""
    n = 20 * 1024 + 3
    hyper = kind.hyper(0.0)
    p0 = R.inputs(n)[0]
    a = torch.nn.Parameter(torch.from_numpy(p0.copy()).to(DEV))
    if kind.name == "sgd":
        opt = torch.optim.SGD([a], lr=R.f32(hyper["lr"]), momentum=R.f32(hyper["momentum"]), weight_decay=0.0, fused=True)
        state_keys = ("momentum_buffer",)
    else:
        opt = torch.optim.RAdam([a], lr=R.f32(hyper["lr"]), betas=(hyper["beta1"], hyper["beta2"]), eps=R.f32(hyper["eps"]), weight_decay=0.0,
                                foreach=True)
        state_keys = ("exp_avg", "exp_avg_sq")
    box = kind.box(kind.zeros(p0))
    ref = (p0.astype(np.float64),) + tuple(np.zeros(n) for _ in state_keys)
    worst = {"kernel": {k: 0.0 for k in kind.names}, "torch": {k: 0.0 for k in kind.names}}
    for t in range(1, 21):
        g = R.fresh_gradient(n, t)
        gd = torch.from_numpy(g).to(DEV)
        a.grad = gd.clone()
        opt.step()
        box.t["g"].copy_(gd)
        box.g0 = g
        assert kind.step(box, hyper, t) == 0
        before = (ref[0], g) + ref[1:]
        sc = kind.scales(before, hyper, t, None)
        ref = kind.want(before, hyper, t, None)
        st = opt.state[a]
        got = {"kernel": box.read(), "torch": (a.detach().cpu().numpy(),) + tuple(st[k].cpu().numpy() for k in state_keys)}
        for who, arrs in got.items():
            for k, x, w in zip(kind.names, arrs, ref):
                worst[who][k] = max(worst[who][k], R.in_units(x, w, sc[k], steps=4 * t))
    return worst


@both
def test_twenty_steps_beside_torchs_own_optimizer(kind):
    """Twenty steps with fresh gradients, state from zero (RAdam crosses its threshold at step 6): the kernel carries its float32
    state, the reference its float64 state.  No tolerance fixed in advance: torch's own float32 optimizer -- SGD fused, RAdam
    foreach -- takes the same steps on the same device, and the kernel's largest deviation from the float64 run, over the steps, in
    units of u * scale for each quantity, may be at most twice torch's (the rule of test_twenty_steps_beside_torch_fused_adam;
    weight decay off for the reason given there).
    Measured on an MI355X (units of u * scale; kernel, torch): SGD param 109.2, 109.2; momentum_buffer 1300.4, 1300.4 -- the same
    figures: with its two fused multiply-adds the kernel rounds where torch's fused SGD does (with momentum * buf rounded apart
    from the sum the buffer stood at 9577: an element whose buffer cancels against its gradient keeps the product's rounding
    error).  RAdam param 948, 947; exp_avg 2394, 2280; exp_avg_sq 10.0, 13.8."""
    worst = _twenty_steps(kind)
    print(f"{kind.name}: twenty steps, largest deviation from float64 in units of u * scale:", worst)
    for k in kind.names:
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
        for (key, _attr), la, lb in zip(a.STATE, a._state_lists(), b._state_lists()):
            assert torch.equal(la[i], lb[i]), (key, i)
        assert int(a._skipped[i].item()) == int(b._skipped[i].item()), ("skipped", i)


@pytest.mark.parametrize("name", ["FlatSGD", "FlatRAdam"])
def test_flat_optimizer_step_dev_is_step_and_follows_a_loaded_state(name):
    """training.FlatSGD / FlatRAdam over a NeRFSystem's two models: seven eager step_dev() calls (prep + the four-tensor update) with
    hand-set gradients -- the learning rate changed through param_groups[0] before the second, the second vetoed by a guard word,
    so that RAdam's effective step 6, the first rectified one, is the seventh call -- against seven step() calls (the host-scalar
    entry point, found_inf) on a twin: parameters, state and skip counts bit for bit.  Then the state saved after the twin's first
    step is loaded into the optimizer that HAS device state (its device count stands at 7): its next step_dev() is the step of an
    optimizer built fresh from that state, the second step and not the eighth.  A state of another class is refused."""
    from mirror_nerf_amd import training
    cls = getattr(training, name)
    sys_a, sys_b = _system(), _system()
    a = cls(list(sys_a.models.values()), lr=5e-4, weight_decay=1e-3)
    b = cls(list(sys_b.models.values()), lr=5e-4, weight_decay=1e-3)
    assert len(a.flats) == 2 and training._takes_found_inf(a)
    a.enable_device_state()
    gen = torch.Generator(device=DEV)
    gen.manual_seed(11)
    grads = [[torch.randn(fp.numel(), device=DEV, generator=gen) * 10.0 ** (torch.rand(fp.numel(), device=DEV, generator=gen) * 8 - 8)
              for fp in a.flats] for _ in range(8)]
    hot, cold = torch.tensor([4], dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    saved = None
    for k in range(7):
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
    assert [int(t.item()) for t in a._skipped] == [1, 1] and a._calls == b._calls == 7 and a._steps == b._steps == [7, 7]
    assert int(a._step_dev.item()) == 7
    if name == "FlatRAdam":
        assert float(a._state_dev[8].item()) == 1.0 and R.rectified(0.999, 7 - 1) and not R.rectified(0.999, 6 - 1)
    fresh = cls(list(sys_b.models.values()), lr=1e-3, weight_decay=0.0)
    for opt in (a, fresh):
        opt.load_state_dict(saved[0])
        for fp, src in zip(opt.flats, saved[1]):
            fp.data.copy_(src)
    fresh.enable_device_state()
    assert a.param_groups[0]["lr"] == 5e-4 and a._calls == 1
    for opt in (a, fresh):
        _set_grads(opt, grads[7])
        _step_dev_counted(opt, [cold])
    assert int(fresh._step_dev.item()) == 2 and int(a._step_dev.item()) == 2
    _same_optimizer_state(a, fresh)
    other = training.FlatSGD if name == "FlatRAdam" else training.FlatRAdam
    with pytest.raises(ValueError, match="cannot continue"):
        other(list(_system().models.values())).load_state_dict(saved[0])
