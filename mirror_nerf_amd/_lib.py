"""ctypes binding of libmnrf_hip.so, read from include/mnrf.h: the header is the only place where the C ABI is declared.

There is no CPU fallback: if the shared library is missing, or a call fails,
a RuntimeError is raised.  torch is imported first so that the HIP runtime
already loaded by torch (same SONAME libamdhip64.so.7) is the one the library
binds to -- device pointers and streams then belong to one runtime.
"""
import contextlib
import ctypes
import os
import subprocess

import torch  # noqa: F401  (must precede CDLL, see module docstring)

from . import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MNRF_LIB", os.path.join(_HERE, "libmnrf_hip.so"))   # MNRF_LIB: tuning experiments
CSRC = os.path.join(_HERE, "csrc")

HEADER = os.path.join(os.path.dirname(_HERE), "include", "mnrf.h")


def _read_header():
    if not os.path.exists(HEADER):
        raise RuntimeError(f"{HEADER} not found: the binding of libmnrf_hip.so is read from the header, there is no other copy")
    with open(HEADER) as f:
        return _abi.parse_header(f.read(), pointees=POINTEES)


# Once per process: every `#define MNRF_*` integer, the argument structs as ctypes.Structure classes, and
# name -> (restype, argtypes) of every prototype (see _abi.py for the typing rule), and, filled in the same pass, POINTEES: name ->
# (element class, declared base type) of each single-level device pointer by argument position (None elsewhere), which only
# the checked mode below looks at.
POINTEES = {}
CONSTANTS, STRUCTS, SIGNATURES = _read_header()
globals().update(CONSTANTS)          # _lib.MNRF_SPLIT_F16, ...
N_PARAMS = CONSTANTS["MNRF_N_PARAMS"]
DNERF_N_PARAMS = CONSTANTS["MNRF_DNERF_N_PARAMS"]

_lib = None


def build(verbose=False):
    """Compile csrc/*.hip for gfx950 into libmnrf_hip.so (hipcc cross-compiles without a GPU)."""
    r = subprocess.run(["make", "-j4", "-C", CSRC], capture_output=True, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout + r.stderr)
    if r.returncode != 0:
        raise RuntimeError("building libmnrf_hip.so failed")
    return LIB_PATH


def lib():
    """The loaded library with typed entry points; raises if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: the HIP extension must be built "
                "(python -c 'import __graft_entry__ as g; g.build()'); there is no CPU fallback")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
        if _checked:
            _set_argtypes(True)
    return _lib


def check(code, what):
    if code != 0:
        msg = lib().mnrf_last_error()
        raise RuntimeError(f"{what} failed ({code}): {msg.decode() if msg else ''}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL) as a plain c_void_p.  Checked here: the tensor is on the GPU, on the current
    device, and contiguous.  NOT checked: its dtype and its extent -- the element type the kernel reads is the one mnrf.h
    declares for that argument, and holding a tensor to it is the caller's business (the public entry points convert or refuse
    a tensor of another precision where it enters).  `with checked():` makes a mismatch of the element type an ArgumentError."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("mirror_nerf_amd runs on the GPU only (tensor is on %s)" % t.device)
    if not t.is_contiguous():
        raise RuntimeError("tensor must be contiguous")
    if t.device.index != _cur_device():
        # kernels are launched on the CURRENT device's current stream (stream()): one process per GPU binds it once with
        # torch.cuda.set_device(LOCAL_RANK) (dist.init_from_env); anything else must wrap calls in torch.cuda.device(...)
        raise RuntimeError(f"tensor lives on cuda:{t.device.index} but the current device is cuda:{_cur_device()}; "
                           "call torch.cuda.set_device / use `with torch.cuda.device(t.device)`")
    return ctypes.c_void_p(t.data_ptr())


# ---- the checked mode: the element types of mnrf.h held against the dtypes of the tensors behind the pointers.  Off by default:
# a from_param written in Python costs ~0.2 us per pointer argument, and a step makes some hundred launches of 10-20 pointers each.

CLASS_DTYPES = {"float": (torch.float32,), "double": (torch.float64,), "int32": (torch.int32,), "int64": (torch.int64,),
                "byte": (torch.uint8, torch.int8, torch.bool), "void": None, "struct": None}      # None: anything


class DevicePtr(ctypes.c_void_p):
    """What ptr() returns in the checked mode: the address, and the dtype of the tensor it came from."""
    dtype = None


class _TypedPtr(ctypes.c_void_p):
    """argtypes entry of one device pointer in the checked mode (one subclass per function and position).  ctypes calls
    from_param for every argument before it enters the C function; what it raises surfaces as ctypes.ArgumentError."""
    _where, _declared, _accepts = "", "void", None

    @classmethod
    def from_param(cls, value):
        dtype = getattr(value, "dtype", None)          # None, ints and a plain c_void_p carry none: passed on unchecked
        if dtype is not None and cls._accepts is not None and dtype not in cls._accepts:
            raise TypeError(f"{cls._where}: mnrf.h declares {cls._declared}*, the tensor is {dtype}")
        return ctypes.c_void_p.from_param(value)


_checked = 0
_typed = {}          # name -> argtypes with a _TypedPtr subclass at every classified pointer, made on first use


def _typed_argtypes(name):
    if name not in _typed:
        args = list(SIGNATURES[name][1])
        for i, c in enumerate(POINTEES[name]):
            if c is not None:
                args[i] = type(f"{name}_arg{i}", (_TypedPtr,), {
                    "_where": f"{name}, argument {i + 1}", "_declared": c[1], "_accepts": CLASS_DTYPES[c[0]]})
        _typed[name] = args
    return _typed[name]


def _set_argtypes(typed):
    if _lib is not None:
        for name, (_, args) in SIGNATURES.items():
            getattr(_lib, name).argtypes = _typed_argtypes(name) if typed else args


def _ptr_checked(t):
    """ptr() of the checked mode: the same checks, and the pointer remembers the tensor's dtype."""
    p = _ptr_plain(t)
    if p is None:
        return None
    q = DevicePtr(p.value)
    q.dtype = t.dtype
    return q


_ptr_plain = ptr


def _enter_checked():
    global _checked, ptr
    _checked += 1
    if _checked == 1:
        ptr = _ptr_checked
        _set_argtypes(True)


def _leave_checked():
    global _checked, ptr
    _checked -= 1
    if _checked == 0:
        ptr = _ptr_plain
        _set_argtypes(False)


@contextlib.contextmanager
def checked():
    """Inside, every entry point of lib() refuses a ptr(t) whose dtype is not in the class mnrf.h declares for that argument:
    ctypes.ArgumentError naming function, position, declared type and dtype, raised before the C function is entered.  Leaving
    restores ptr and the argtypes objects of the default path.  MNRF_CHECK_ABI=1 at import turns it on for the whole process."""
    _enter_checked()
    try:
        yield
    finally:
        _leave_checked()


if os.environ.get("MNRF_CHECK_ABI", "") == "1":
    _enter_checked()


def preset(table, root_dir):
    """The first entry of a preset table ((key, dict), ...) whose key is a substring of root_dir (None: the reference's `else`)."""
    for key, value in table:
        if key is None or key in (root_dir or ""):
            return dict(value)
    raise AssertionError("preset tables end with a default entry")


# ---- the rule of the public entry points for a caller's tensor of another precision or layout: an input is converted, a tensor
# the call writes into is refused (DESIGN "The Python-to-kernel boundary").  Applied where a tensor enters, never per launch.

def f32_in(t):
    """An input the kernels read as float32 rows: the tensor itself, or its float32 contiguous copy (None stays None)."""
    if t is None or (t.dtype == torch.float32 and t.is_contiguous()):
        return t
    return t.float().contiguous()


def i32_in(t):
    """An input the kernels read as int32: the tensor itself, or its int32 contiguous copy (None stays None)."""
    if t is None or (t.dtype == torch.int32 and t.is_contiguous()):
        return t
    return t.int().contiguous()


def written(t, dtypes, name):
    """A tensor the call writes into: refused unless it is contiguous and of one of `dtypes` (None passes)."""
    if t is not None and (t.dtype not in dtypes or not t.is_contiguous()):
        raise ValueError(f"{name} is written in place: it must be a contiguous {' / '.join(str(d) for d in dtypes)} tensor, "
                         f"not {t.dtype}{'' if t.is_contiguous() else ' (not contiguous)'}")
    return t


F32, I32, BYTE = (torch.float32,), (torch.int32,), (torch.bool, torch.uint8, torch.int8)

_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None) or torch.cuda.current_device


def stream():
    """The current torch stream of the current device as a hipStream_t (every kernel is launched on it)."""
    if _raw_stream is not None:      # ~1 us; torch.cuda.current_stream() builds a Stream object (~13 us, 20 launches per step)
        return ctypes.c_void_p(_raw_stream(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
