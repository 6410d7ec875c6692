"""The Python-to-kernel boundary without a GPU: include/mnrf.h declares an element type for every device pointer, the reader
(_abi.py) keeps it as a class per prototype and position, and the checked mode of the binding (_lib.checked()) holds the dtype of
every _lib.ptr(t) against it.  Pointers here are built by hand (a dtype and an address into a ctypes buffer) and go to entry
points that return before they touch memory: a zero-sized call, or an argument error."""
import collections
import ctypes
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mnrf.h")

DTYPES = [torch.float16, torch.bfloat16, torch.float32, torch.float64, torch.int8, torch.uint8, torch.bool, torch.int32, torch.int64]
# the element classes and the dtypes that may stand behind them ("The Python-to-kernel boundary")
ACCEPTS = {"float": {torch.float32}, "double": {torch.float64}, "int32": {torch.int32}, "int64": {torch.int64},
           "byte": {torch.uint8, torch.int8, torch.bool}, "void": set(DTYPES)}
# one early-returning call per class: name, arguments with "@" where the pointer under test goes, position of "@" (from 1),
# the header's own spelling of the type there
CALLS = {
    "float": ("mnrf_jitter_mean", ["@", None, None, 0, 1, 0, 0, 0.0, None], 1, "float*"),
    "int32": ("mnrf_jitter_mean", [None, None, "@", 0, 1, 0, 0, 0.0, None], 3, "int32_t*"),
    "byte": ("mnrf_rgb_to_uint8", [None, 0, "@", None], 3, "uint8_t*"),
    "double": ("mnrf_accumulate_colors", [None, "@", None, 0.2, 0, None, None, None], 2, "double*"),
    "void": ("mnrf_vertex_normals", [None, 0, None, 0, "@", None, None], 5, "void*"),
    "int64": ("mnrf_adam_prep", [None, "@", None, None, None, None, 0, None, None], 2, "int64_t*"),      # (refused: hyper is null)
}


@pytest.fixture(scope="module")
def L():
    from mirror_nerf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _hand_built(dtype, buf):
    from mirror_nerf_amd import _lib
    q = _lib.DevicePtr(ctypes.addressof(buf))
    q.dtype = dtype
    return q


def test_every_device_pointer_of_the_header_is_classified():
    from mirror_nerf_amd import _abi, _lib
    assert set(_lib.POINTEES) == set(_lib.SIGNATURES)
    counts, unclassified = collections.Counter(), []
    for name, classes in _lib.POINTEES.items():
        argtypes = _lib.SIGNATURES[name][1]
        assert len(classes) == len(argtypes)
        for i, (c, a) in enumerate(zip(classes, argtypes)):
            if a is ctypes.c_void_p:                   # a single-level device pointer (or a stream, a struct)
                if c is None or c[0] not in _lib.CLASS_DTYPES:
                    unclassified.append((name, i, c))
                    continue
                assert c[0] == ("struct" if c[1] in _lib.STRUCTS else _abi.POINTEE_CLASS[c[1]]), (name, i, c)
                counts[c[0]] += 1
            else:                                      # scalars, T* const*, MNRF_HOST pointers: as they were
                assert c is None, (name, i, c)
    print("device pointers per class:", dict(counts))
    assert len(unclassified) == 0, unclassified
    assert set(counts) == {"float", "double", "int32", "int64", "byte", "void", "struct"} and counts["float"] > 400
    assert set(_abi.POINTEE_CLASS.values()) | {"struct"} == set(_lib.CLASS_DTYPES)
    for c, want in ACCEPTS.items():
        have = _lib.CLASS_DTYPES[c]
        assert (set(DTYPES) if have is None else set(have)) == want
    # spot checks against the header's text
    F, V = ("float", "float"), ("void", "void")
    assert _lib.POINTEES["mnrf_jitter_mean"] == [F, F, ("int32", "int32_t"), None, None, None, None, None, V]
    assert _lib.POINTEES["mnrf_rgb_to_uint8"] == [F, None, ("byte", "uint8_t"), V]
    assert _lib.POINTEES["mnrf_accumulate_colors"][:3] == [F, ("double", "double"), F]
    assert _lib.POINTEES["mnrf_total_loss"][0] == ("struct", "MnrfLossArgs")


SYNTHETIC = """
#define MNRF_HOST
typedef struct { int a; } MnrfArgs;
int mnrf_all(const float* f, double* d, const int32_t* i, uint32_t* u, int* n, const int64_t* l, uint64_t* w,
             const uint8_t* b, int8_t* s, const unsigned char* c, void* v, const MnrfArgs* a,
             const float* const* pp, MNRF_HOST const float* h, MNRF_HOST int64_t* hl, int k, float x);
"""


def test_classes_of_a_synthetic_header():
    from mirror_nerf_amd._abi import parse_header
    pointees = {}
    out = parse_header(SYNTHETIC, pointees=pointees)
    assert len(out) == 3 and out[2] == parse_header(SYNTHETIC)[2]      # the return is the one of a call without the dict
    signatures = out[2]
    assert pointees == {"mnrf_all": [("float", "float"), ("double", "double"), ("int32", "int32_t"), ("int32", "uint32_t"), ("int32", "int"),
                                     ("int64", "int64_t"), ("int64", "uint64_t"), ("byte", "uint8_t"), ("byte", "int8_t"),
                                     ("byte", "unsigned char"), ("void", "void"), ("struct", "MnrfArgs"), None, None, None, None, None]}
    C = ctypes
    assert signatures["mnrf_all"][1] == [C.c_void_p] * 12 + [C.POINTER(C.c_void_p), C.POINTER(C.c_float), C.POINTER(C.c_int64),
                                                             C.c_int, C.c_float]
    with pytest.raises(ValueError, match=r"mnrf\.h: no element class .*mnrf_bad\(const char\* text\)"):
        parse_header("int mnrf_bad(const char* text);")
    parse_header("int mnrf_ok(MNRF_HOST const char* text);")      # host memory: not classified, as before


@pytest.mark.parametrize("cls", list(CALLS))
def test_accept_and_refuse_matrix(L, cls):
    from mirror_nerf_amd import _lib
    name, args, pos, declared = CALLS[cls]
    buf = (ctypes.c_double * 64)()
    fn = getattr(L, name)

    def call(value):
        return fn(*[value if a == "@" else a for a in args])
    with _lib.checked():
        assert _lib.POINTEES[name][pos - 1] == (cls, declared[:-1])
        for dtype in DTYPES:
            q = _hand_built(dtype, buf)
            if dtype in ACCEPTS[cls]:
                code = call(q)                         # entered, and returned early
                assert (code == 0) if cls != "int64" else (code < 0 and b"mnrf_adam_prep: null pointer" in L.mnrf_last_error()), (cls, dtype)
            else:
                with pytest.raises(ctypes.ArgumentError) as e:
                    call(q)
                msg = str(e.value)
                assert f"argument {pos}" in msg and name in msg and declared in msg and str(dtype) in msg, msg
        # what carries no dtype passes unchecked
        for untyped in (None, ctypes.addressof(buf), ctypes.c_void_p(ctypes.addressof(buf)), ctypes.cast(buf, ctypes.c_void_p)):
            call(untyped)
    assert all(v == 0.0 for v in buf)                  # nobody wrote through the pointers
    q = _hand_built(torch.float16, buf)
    call(q)                                            # outside the mode the same pointer is a plain address again


def test_leaving_the_mode_restores_the_binding(L):
    from mirror_nerf_amd import _lib
    before = {name: getattr(L, name).argtypes for name in _lib.SIGNATURES}
    ptr_before = _lib.ptr
    with _lib.checked():
        assert _lib.ptr is not ptr_before
        inside = L.mnrf_jitter_mean.argtypes
        assert issubclass(inside[0], ctypes.c_void_p) and inside[0] is not ctypes.c_void_p and inside[3] is ctypes.c_int64
        with _lib.checked():                           # nests
            assert L.mnrf_jitter_mean.argtypes[0] is inside[0]
        assert L.mnrf_jitter_mean.argtypes[0] is inside[0] and _lib.ptr is not ptr_before
    assert _lib.ptr is ptr_before
    for name in _lib.SIGNATURES:
        now = getattr(L, name).argtypes
        assert len(now) == len(before[name]) and all(a is b for a, b in zip(now, before[name])), name
    with pytest.raises(RuntimeError):
        with _lib.checked():
            raise RuntimeError("leaves through an exception")
    assert _lib.ptr is ptr_before and all(a is ctypes.c_void_p for a in L.mnrf_jitter_mean.argtypes[:3])


def test_the_default_path_is_the_path_of_before(L):
    """Outside the mode ptr returns exactly c_void_p and the argtypes are what parse_header gives for the header."""
    from mirror_nerf_amd import _abi, _lib
    assert _lib._checked == 0 and _lib.ptr is _lib._ptr_plain and _lib.ptr.__name__ == "ptr"
    _, _, signatures = _abi.parse_header(open(HEADER).read())
    assert signatures == _lib.SIGNATURES
    for name, (res, args) in signatures.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
        assert all(a is ctypes.c_void_p or not issubclass(a, ctypes.c_void_p) for a in fn.argtypes), name

    class FakeTensor:                                  # what ptr looks at, without a GPU
        is_cuda, dtype = True, torch.float16
        device = type("D", (), {"index": 0})()

        def is_contiguous(self):
            return True

        def data_ptr(self):
            return 4096
    import unittest.mock
    with unittest.mock.patch.object(_lib, "_cur_device", lambda: 0):
        got = _lib.ptr(FakeTensor())
        assert type(got) is ctypes.c_void_p and got.value == 4096 and not hasattr(got, "dtype")
        assert _lib.ptr(None) is None
        with _lib.checked():
            got = _lib.ptr(FakeTensor())
            assert type(got) is _lib.DevicePtr and got.value == 4096 and got.dtype is torch.float16
            assert _lib.ptr(None) is None
    assert "dtype" in _lib.ptr.__doc__ and "fp32/int32" not in _lib.ptr.__doc__


def test_the_environment_turns_the_mode_on_for_a_process():
    import subprocess
    import sys
    code = ("import ctypes, os, torch\nfrom mirror_nerf_amd import _lib\nL = _lib.lib()\non = os.environ['MNRF_CHECK_ABI'] == '1'\n"
            "assert (_lib.ptr is _lib._ptr_checked) == on and (L.mnrf_jitter_mean.argtypes[0] is not ctypes.c_void_p) == on\n"
            "buf = (ctypes.c_double * 8)()\nq = _lib.DevicePtr(ctypes.addressof(buf)); q.dtype = torch.float64\n"
            "try:\n    L.mnrf_jitter_mean(q, None, None, 0, 1, 0, 0, 0.0, None)\nexcept ctypes.ArgumentError as e:\n    print('refused', e)\n")
    for value, want in (("1", True), ("0", False), ("", False)):
        env = dict(os.environ, MNRF_CHECK_ABI=value, PYTHONPATH=ROOT)
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        assert ("refused" in r.stdout) == want, r.stdout
