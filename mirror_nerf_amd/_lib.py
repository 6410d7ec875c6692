"""ctypes binding of libmnrf_hip.so, read from include/mnrf.h: the header is the only place where the C ABI is declared.

There is no CPU fallback: if the shared library is missing, or a call fails,
a RuntimeError is raised.  torch is imported first so that the HIP runtime
already loaded by torch (same SONAME libamdhip64.so.7) is the one the library
binds to -- device pointers and streams then belong to one runtime.
"""
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
        return _abi.parse_header(f.read())


# Once per process: every `#define MNRF_*` integer, the argument structs as ctypes.Structure classes, and
# name -> (restype, argtypes) of every prototype (see _abi.py for the typing rule).
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
    return _lib


def check(code, what):
    if code != 0:
        msg = lib().mnrf_last_error()
        raise RuntimeError(f"{what} failed ({code}): {msg.decode() if msg else ''}")


def ptr(t):
    """Device pointer of a tensor (None -> NULL).  Tensors must be fp32/int32, contiguous, on the GPU."""
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


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None) or torch.cuda.current_device


def stream():
    """The current torch stream of the current device as a hipStream_t (every kernel is launched on it)."""
    if _raw_stream is not None:      # ~1 us; torch.cuda.current_stream() builds a Stream object (~13 us, 20 launches per step)
        return ctypes.c_void_p(_raw_stream(torch.cuda.current_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
