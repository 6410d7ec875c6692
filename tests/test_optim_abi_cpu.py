"""The SGD and RAdam entry points of the C ABI without a GPU: every argument check comes before the launch, so refusals (and the
no-ops of empty work) can be called on a machine that has no device.  In the manner of tests/test_abi_cpu.py."""
import ctypes as C
import os

import pytest


@pytest.fixture(scope="module")
def L():
    from mirror_nerf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _aligned(n_floats=8, off=0):
    """A host buffer and an address inside it that is `off` bytes past a 16-byte boundary (never dereferenced: the call is refused)."""
    buf = (C.c_float * (n_floats + 8))()
    base = C.addressof(buf)
    return buf, C.c_void_p(base + (-base) % 16 + off)


def test_state_block_sizes():
    from mirror_nerf_amd import _lib
    assert (_lib.MNRF_SGD_STATE_FLOATS, _lib.MNRF_RADAM_STATE_FLOATS, _lib.MNRF_ADAM_STATE_FLOATS) == (5, 9, 8)
    for name in ("mnrf_sgd_step", "mnrf_sgd_prep", "mnrf_sgd_step_dev_n", "mnrf_radam_step", "mnrf_radam_prep", "mnrf_radam_step_dev_n"):
        assert name in _lib.SIGNATURES


def test_sgd_refusals(L):
    keep, ok = _aligned()
    keep2, off = _aligned(off=4)
    null = None
    assert L.mnrf_sgd_step(null, ok, ok, 4, 5e-4, 0.9, 0.0, 1, ok, null, null, null) < 0
    assert b"mnrf_sgd_step: null pointer" in L.mnrf_last_error()
    assert L.mnrf_sgd_step(ok, ok, ok, 4, 5e-4, 0.9, 0.0, 1, null, null, null, null) < 0            # the skip counter is required
    assert L.mnrf_sgd_step(ok, ok, ok, -1, 5e-4, 0.9, 0.0, 1, ok, null, null, null) < 0
    assert L.mnrf_sgd_step(ok, ok, ok, 4, 5e-4, 0.9, 0.0, 0, ok, null, null, null) < 0              # step >= 1
    assert b"step >= 1" in L.mnrf_last_error()
    for args in ((off, ok, ok), (ok, off, ok), (ok, ok, off)):
        assert L.mnrf_sgd_step(*args, 4, 5e-4, 0.9, 0.0, 1, ok, null, null, null) < 0
        assert b"16-byte aligned" in L.mnrf_last_error()
    assert L.mnrf_sgd_step(ok, ok, ok, 0, 5e-4, 0.9, 0.0, 1, ok, null, null, null) == 0             # nothing to do: no launch
    # prep
    assert L.mnrf_sgd_prep(null, ok, ok, null, null, null, 0, ok, null) < 0
    assert b"mnrf_sgd_prep: null pointer" in L.mnrf_last_error()
    assert L.mnrf_sgd_prep(ok, ok, ok, null, null, null, 5, ok, null) < 0
    assert L.mnrf_sgd_prep(ok, ok, ok, null, null, null, 2, ok, null) < 0                           # a count without the array
    assert b"0..4 guard words" in L.mnrf_last_error()
    words = (C.c_void_p * 2)(ok, None)
    assert L.mnrf_sgd_prep(ok, ok, ok, null, null, words, 2, ok, null) < 0
    assert b"null guard word" in L.mnrf_last_error()
    # the update of up to four tensors
    one = lambda p: (C.c_void_p * 1)(p)  # noqa: E731
    n1 = (C.c_int64 * 1)(4)
    assert L.mnrf_sgd_step_dev_n(0, null, null, null, null, ok, null, null) == 0
    assert L.mnrf_sgd_step_dev_n(5, one(ok), one(ok), one(ok), n1, ok, one(ok), null) < 0
    assert b"0..4 tensors" in L.mnrf_last_error()
    assert L.mnrf_sgd_step_dev_n(-1, one(ok), one(ok), one(ok), n1, ok, one(ok), null) < 0
    assert L.mnrf_sgd_step_dev_n(1, one(ok), one(ok), one(ok), n1, null, one(ok), null) < 0         # no state block
    assert L.mnrf_sgd_step_dev_n(1, one(ok), one(None), one(ok), n1, ok, one(ok), null) < 0
    assert L.mnrf_sgd_step_dev_n(1, one(ok), one(ok), one(off), n1, ok, one(ok), null) < 0
    assert b"16-byte aligned" in L.mnrf_last_error()
    assert L.mnrf_sgd_step_dev_n(1, one(ok), one(ok), one(ok), (C.c_int64 * 1)(-4), ok, one(ok), null) < 0
    assert L.mnrf_sgd_step_dev_n(1, one(ok), one(ok), one(ok), (C.c_int64 * 1)(0), ok, one(ok), null) == 0
    del keep, keep2


def test_radam_refusals(L):
    keep, ok = _aligned()
    keep2, off = _aligned(off=8)
    null = None
    tail = (5e-4, 0.9, 0.999, 1e-8, 0.0)
    assert L.mnrf_radam_step(ok, ok, ok, null, 4, *tail, 1, ok, null, null, null) < 0
    assert b"mnrf_radam_step: null pointer" in L.mnrf_last_error()
    assert L.mnrf_radam_step(ok, ok, ok, ok, 4, *tail, 1, null, null, null, null) < 0
    assert L.mnrf_radam_step(ok, ok, ok, ok, -1, *tail, 1, ok, null, null, null) < 0
    assert L.mnrf_radam_step(ok, ok, ok, ok, 4, *tail, 0, ok, null, null, null) < 0
    for args in ((off, ok, ok, ok), (ok, off, ok, ok), (ok, ok, off, ok), (ok, ok, ok, off)):
        assert L.mnrf_radam_step(*args, 4, *tail, 1, ok, null, null, null) < 0
        assert b"16-byte aligned" in L.mnrf_last_error()
    assert L.mnrf_radam_step(ok, ok, ok, ok, 0, *tail, 1, ok, null, null, null) == 0
    assert L.mnrf_radam_prep(ok, null, ok, null, null, null, 0, ok, null) < 0
    assert b"mnrf_radam_prep: null pointer" in L.mnrf_last_error()
    assert L.mnrf_radam_prep(ok, ok, ok, null, null, null, -1, ok, null) < 0
    assert L.mnrf_radam_prep(ok, ok, ok, null, null, (C.c_void_p * 1)(None), 1, ok, null) < 0
    one = lambda p: (C.c_void_p * 1)(p)  # noqa: E731
    n1 = (C.c_int64 * 1)(4)
    assert L.mnrf_radam_step_dev_n(0, null, null, null, null, null, ok, null, null) == 0
    assert L.mnrf_radam_step_dev_n(5, one(ok), one(ok), one(ok), one(ok), n1, ok, one(ok), null) < 0
    assert b"mnrf_radam_step_dev_n: 0..4 tensors" in L.mnrf_last_error()
    assert L.mnrf_radam_step_dev_n(1, one(ok), one(ok), one(ok), one(ok), n1, ok, null, null) < 0
    assert L.mnrf_radam_step_dev_n(1, one(ok), one(ok), one(ok), one(ok), n1, ok, one(None), null) < 0
    assert L.mnrf_radam_step_dev_n(1, one(ok), one(ok), one(ok), one(off), n1, ok, one(ok), null) < 0
    assert b"16-byte aligned" in L.mnrf_last_error()
    assert L.mnrf_radam_step_dev_n(1, one(ok), one(ok), one(ok), one(ok), (C.c_int64 * 1)(0), ok, one(ok), null) == 0
    del keep, keep2


def test_the_flat_optimizers_share_one_surface():
    """Built without a device nothing can be constructed (the modules' parameters decide the device), but the classes are there,
    name their entry points, and GraphedTrainStep's refusal names all three."""
    from mirror_nerf_amd import _lib, training as T
    assert T.FLAT_OPTIMIZERS == {"adam": T.FlatAdam, "sgd": T.FlatSGD, "radam": T.FlatRAdam}
    for cls in T.FLAT_OPTIMIZERS.values():
        assert issubclass(cls, T._FlatOptimizer) and cls.NAME == cls.__name__
        assert all(name in _lib.SIGNATURES for name in cls.ENTRY[:3]) and cls.ENTRY[3] in _lib.CONSTANTS
        for method in ("step", "step_dev", "enable_device_state", "sync_hyper", "zero_grad", "state_dict", "load_state_dict"):
            assert callable(getattr(cls, method))
    assert [k for k, _ in T.FlatSGD.STATE] == ["momentum_buffer"] and [k for k, _ in T.FlatRAdam.STATE] == ["exp_avg", "exp_avg_sq"]
    with pytest.raises(ValueError, match="FlatAdam, training.FlatSGD or training.FlatRAdam"):
        T.GraphedTrainStep(None, object(), 128)
