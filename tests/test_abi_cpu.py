"""CPU-side checks of the C-ABI library: it loads, exports every symbol include/mnrf.h declares,
and validates arguments before touching the GPU (no compute calls here)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mnrf.h")


@pytest.fixture(scope="module")
def L():
    from mirror_nerf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_exports_match_header(L):
    text = open(HEADER).read()
    declared = set(re.findall(r"\b(mnrf_[a-z0-9_]+)\s*\(", text))
    from mirror_nerf_amd import _lib
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    for name in declared:
        assert hasattr(L, name), f"libmnrf_hip.so lacks {name}"
    # ... and the reverse: the library defines no mnrf_ symbol that the header does not declare
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.split() and line.split()[-1].startswith("mnrf_")}
    assert exported == declared, exported ^ declared


def test_packed_size_matches_layout(L):
    # fp32 streams: forward tiles 2640 + bias block 3072 floats + backward tiles 1920 + head-backward tiles 704;
    # split-f16 streams: 1312 forward + 960 trunk-backward + 352 head-backward hi/lo tile pairs of 2 KiB (mnrf_layout.h)
    assert L.mnrf_packed_floats() == 2640 * 256 + 3072 + 1920 * 256 + 704 * 256 + (1312 + 960 + 352 + 1328) * 512 + 16384   # + tail pad
    assert L.mnrf_version() >= 1


def test_argument_validation_without_gpu(L):
    null = None
    assert L.mnrf_field_forward(null, 0, 128, null, 3, null, null, 1, null, 27, null, null, null, null, null,
                                null, null) < 0
    assert b"packed" in L.mnrf_last_error()
    assert L.mnrf_sample_fine(null, null, 4, 2, null, 0, 16, null, null) < 0      # S < 3
    assert L.mnrf_sample_fine(null, null, 4, 300, null, 0, 16, null, null) < 0    # S > 256
    assert L.mnrf_composite(null, 4, 64, null, null, null, null, null, null, null, 0, null, null, null, null,
                            null, null, null, null, null, null) < 0
    assert L.mnrf_embed(null, -1, 3, 4, null, null) < 0
    # loss reductions / metric: null argument block, missing outputs, bad sizes
    assert L.mnrf_total_loss(null, null, null) < 0
    assert b"mnrf_total_loss" in L.mnrf_last_error()
    from mirror_nerf_amd.losses import _Args
    import ctypes
    a = _Args()
    a.n_rays = 0
    ws = (ctypes.c_float * 64)()
    assert L.mnrf_total_loss(ctypes.byref(a), ctypes.cast(ws, ctypes.c_void_p), null) < 0      # n_rays must be positive
    a.n_rays = 4
    assert L.mnrf_total_loss(ctypes.byref(a), ctypes.cast(ws, ctypes.c_void_p), null) < 0      # out / targets / rays missing
    assert b"required" in L.mnrf_last_error()
    assert L.mnrf_mse_psnr(null, null, null, 10, 1, null, null, null) < 0
    assert L.mnrf_loss_workspace_floats(1024, 64, 192, 0) > 1024
    assert L.mnrf_mse_blocks() >= 1
    # round-3 entry points: the same contract (null pointers / sizes are refused with a message; sizes are plain arithmetic)
    import ctypes as C
    assert L.mnrf_field_composite_fused(null, 4, null, null, null, 27, 0, null, null, null, null, null, null, null, null) < 0
    assert b"mnrf_field_composite_fused" in L.mnrf_last_error()
    assert L.mnrf_fused_samples_per_ray() == 192
    assert L.mnrf_dw_planes(0, null, null, null, null, null, null, 0, null) < 0          # 1..8 evaluations
    assert L.mnrf_dw_planes(1, null, null, null, null, null, null, 0, null) < 0
    assert b"mnrf_dw_planes" in L.mnrf_last_error()
    assert L.mnrf_train_planes_bytes(128) == 4 * 174 * 2048 and L.mnrf_train_planes_bytes(129) == 8 * 174 * 2048
    assert L.mnrf_train_dy_planes_bytes(128) == 4 * 172 * 2048
    one = (C.c_int64 * 1)(4096)
    assert L.mnrf_dw_planes_workspace_floats(1, one) > 0
    assert L.mnrf_field_backward_planes(null, 4, null, 3, null, null, 1, null, null, null, null, null, null, null, null, null,
                                        null, null, null, null, null, 0, null) < 0
    offs = (C.c_int64 * 17)(*range(0, 17 * 1024, 1024))
    assert L.mnrf_tcnn_backward_workspace_floats2(offs, 16) == L.mnrf_tcnn_backward_workspace_floats(offs) + 16 * 1024 + 4      # (+ overflow word)
    assert L.mnrf_tcnn_backward_workspace_floats2(offs, 0) == L.mnrf_tcnn_backward_workspace_floats(offs)
    # zero-sized work is a no-op, not an error
    assert L.mnrf_field_composite_fused(null, 0, null, null, null, 27, 0, null, null, null, null, null, null, null, null) < 0   # (pointers are checked first)
    assert L.mnrf_embed(null, 0, 3, 4, null, null) == 0
    assert L.mnrf_threshold_mask(null, 0, null, null) == 0


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from mirror_nerf_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.lib()


def test_cpu_tensors_are_rejected():
    import torch
    import mirror_nerf_amd as M
    with pytest.raises(RuntimeError):
        M.render_rays({}, {"xyz": M.Embedding(10), "dir": M.Embedding(4)}, torch.zeros(4, 8))


def test_module_mirrors_reference_names():
    import torch
    import mirror_nerf_amd as M
    from mirror_nerf_amd.weights import PARAM_NAMES, PARAM_SHAPES
    from tests.golden import weights as GW
    torch.manual_seed(0)
    m = M.MirrorNeRF(in_channels_xyz=63, in_channels_dir=27, predict_normal=True, predict_mirror_mask=True)
    sd = m.state_dict()
    assert list(sd) == PARAM_NAMES
    ref = GW.make_state_dict(0, 1)[0]
    for k, v in sd.items():
        assert tuple(v.shape) == PARAM_SHAPES[k]
        assert (v.numpy() == ref[k]).all(), k     # same construction order => same init under a seed
    with pytest.raises(NotImplementedError):
        M.MirrorNeRF(W=128, predict_normal=True, predict_mirror_mask=True)
    with pytest.raises(NotImplementedError):
        M.MirrorNeRF(in_channels_xyz=75, in_channels_dir=27)      # Embedding(12): more bands than the kernels evaluate
    few = M.MirrorNeRF(in_channels_xyz=39, in_channels_dir=15, predict_normal=True, predict_mirror_mask=True)      # --N_emb_xyz 6 --N_emb_dir 2
    assert (few.n_freqs_xyz, few.n_freqs_dir) == (6, 2) and few.xyz_encoding_5[0].weight.shape == (256, 256 + 39)


def test_isa_invariants_of_the_built_field_kernels():
    """scripts/check_isa.py on the objects linked into libmnrf_hip.so: the counted s_waitcnt schemes of the field
    kernels require that no scalar load sits inside an MFMA range and that the forward kernels do not spill."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_isa.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "ISA check ok" in r.stdout


def test_the_shipped_objects_were_built_with_the_default_flags():
    """csrc/.cxxflags records the flags of the objects in the tree (every object depends on it): an experiment's -DMNRF_EXP_*
    must never be what the default library was linked from, and the library must not be older than any of its objects."""
    csrc = os.path.join(ROOT, "mirror_nerf_amd", "csrc")
    flags = os.path.join(csrc, ".cxxflags")
    if not os.path.exists(flags):
        pytest.skip("library not built by this Makefile here")
    assert "MNRF_EXP" not in open(flags).read()
    lib = os.path.join(ROOT, "mirror_nerf_amd", "libmnrf_hip.so")
    objs = [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".o")]
    assert objs and all(os.path.getmtime(o) <= os.path.getmtime(lib) + 1.0 for o in objs)
    assert all(os.path.getmtime(o) >= os.path.getmtime(flags) - 1.0 for o in objs)


def test_bench_refuses_a_world_size_that_contradicts_gpus():
    """`--gpus N` must equal the launched world size (a mismatch used to run one process labelled n_gpus 1)."""
    import subprocess
    import sys
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"], capture_output=True, text=True, env=env)
    assert r.returncode != 0 and "WORLD_SIZE=2" in (r.stderr + r.stdout)


def test_gradient_scale_policy():
    """mirror_nerf._lower_gradient_scale: only a trip that is nothing but a scaled gradient of the training backward lowers the
    module's gradient scale (2^4 at a time, 2^8 at most); anything else leaves the decision to the fp32 fall-back."""
    import warnings
    import torch
    from mirror_nerf_amd import mirror_nerf as MN
    m = torch.nn.Linear(1, 1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert not MN._lower_gradient_scale(m, 1)                 # saturated, but not tagged as the backward
        assert not MN._lower_gradient_scale(m, 1 | 128 | 256)     # the forward saturated too
        assert not MN._lower_gradient_scale(m, 1 | 256 | 512)     # ... or the second-order pass
        assert not MN._lower_gradient_scale(m, 2 | 1 | 256)       # ... or a weight is out of range
        for want in (4, 8):
            assert MN._lower_gradient_scale(m, 1 | 256) and m.__dict__["_mnrf_seed_reduction"] == want
        assert not MN._lower_gradient_scale(m, 1 | 256)           # exhausted: fp32 from here


# ---- the header reader (mirror_nerf_amd/_abi.py) on synthetic headers

SYNTHETIC = """
/* a comment with ( and ; and mnrf_x( inside */
#ifndef MNRF_H
#define MNRF_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define MNRF_HOST
#define MNRF_DEC 7
#define MNRF_HEX 0x100000u     // mnrf_y( ;
#define MNRF_SUFFIX 256u
#define MNRF_NEG (-3)
#define MNRF_BARE_NEG -2
#define MNRF_PAREN (12)
#define MNRF_EXPR (1 << 3)
#define MNRF_TEXT "no"
typedef struct {
    const float* rgb[2];      /* (N,3); */
    float a, b, c;
    int x[2];
    unsigned flags;
    const unsigned char* bytes;
    int64_t n;
} MnrfThing;
const char* mnrf_last_error(void);
int64_t mnrf_size(void);
int mnrf_many(float* packed, unsigned flags,
              int64_t n, const float* const* params,
              float* const* out /* (n) or null: mnrf_z( */,
              const MnrfThing* thing, uint64_t seed,
              unsigned int more, uint32_t word, double d, float f,
              void* stream);
int mnrf_host(MNRF_HOST const int* a, MNRF_HOST const unsigned* b, MNRF_HOST const int64_t* c, MNRF_HOST uint64_t* d,
              MNRF_HOST const float* e, MNRF_HOST double* f, MNRF_HOST const uint32_t* g, const int32_t* device);
#ifdef __cplusplus
}
#endif
#endif /* MNRF_H */
"""


def test_reader_on_a_synthetic_header():
    import ctypes as C
    from mirror_nerf_amd._abi import parse_header
    constants, structs, signatures = parse_header(SYNTHETIC)
    assert constants == {"MNRF_DEC": 7, "MNRF_HEX": 0x100000, "MNRF_SUFFIX": 256, "MNRF_NEG": -3, "MNRF_BARE_NEG": -2,
                         "MNRF_PAREN": 12}
    assert list(structs) == ["MnrfThing"] and issubclass(structs["MnrfThing"], C.Structure)
    assert structs["MnrfThing"]._fields_ == [("rgb", C.c_void_p * 2), ("a", C.c_float), ("b", C.c_float), ("c", C.c_float),
                                             ("x", C.c_int * 2), ("flags", C.c_uint), ("bytes", C.c_void_p), ("n", C.c_int64)]
    P = C.POINTER
    assert signatures == {
        "mnrf_last_error": (C.c_char_p, []),
        "mnrf_size": (C.c_int64, []),
        "mnrf_many": (C.c_int, [C.c_void_p, C.c_uint, C.c_int64, P(C.c_void_p), P(C.c_void_p), C.c_void_p, C.c_uint64,
                                C.c_uint, C.c_uint, C.c_double, C.c_float, C.c_void_p]),
        "mnrf_host": (C.c_int, [P(C.c_int), P(C.c_uint), P(C.c_int64), P(C.c_uint64), P(C.c_float), P(C.c_double), P(C.c_uint),
                                C.c_void_p]),
    }
    assert list(signatures) == ["mnrf_last_error", "mnrf_size", "mnrf_many", "mnrf_host"]


@pytest.mark.parametrize("bad", [
    "int mnrf_a(flot x);",                                   # an unknown type word
    "int mnrf_a(int n, const float*);",                      # a parameter without a name
    "int mnrf_a(int);",
    "long mnrf_a(int n);",                                   # ... an unknown return type
    "typedef struct { int a; float b;",                      # an unterminated struct
    "typedef struct { int a; } MnrfA;\n}",                   # an unbalanced body
    "typedef struct { wide a; } MnrfA;",
    "typedef struct { float* a, b; } MnrfA;",                # b would be a scalar: not guessed
    "int mnrf_a(int n);\nint mnrf_a(int n);",                # declared twice
    "int mnrf_a(MNRF_HOST const float* const* p);",          # the marker is for single-level pointers
    "int mnrf_a(MNRF_HOST int n);",
    "int mnrf_a(float*** p);",
    "int mnrf_a(int n)",                                     # no semicolon: runs into what follows
    "static int x = 3;",
], ids=lambda s: s[:32].replace("\n", " "))
def test_reader_refuses_what_it_does_not_recognise(bad):
    from mirror_nerf_amd._abi import parse_header
    with pytest.raises(ValueError, match="mnrf.h"):
        parse_header(bad + "\nint mnrf_ok(int n);\ntypedef struct { int a; } MnrfOk;\n")


def test_every_define_and_struct_of_the_header_is_read():
    """An independent regex over the raw header: the reader has skipped no integer constant and no struct."""
    from mirror_nerf_amd import _lib
    text = open(HEADER).read()
    defined = set(re.findall(r"#define\s+(MNRF_\w+)", text)) - {"MNRF_H", "MNRF_HOST"}
    assert defined == set(_lib.CONSTANTS) and len(defined) > 40
    for name, value in _lib.CONSTANTS.items():
        assert getattr(_lib, name) == value
    assert (_lib.N_PARAMS, _lib.DNERF_N_PARAMS) == (_lib.MNRF_N_PARAMS, _lib.MNRF_DNERF_N_PARAMS) == (32, 42)
    assert set(re.findall(r"\}\s*(Mnrf\w+)\s*;", text)) == set(_lib.STRUCTS) == {"MnrfLossArgs", "MnrfBank", "MnrfFrameMaps",
                                                                                "MnrfFrameImages"}
    from mirror_nerf_amd import data, frames, losses
    assert losses._Args is _lib.STRUCTS["MnrfLossArgs"] and data._Bank is _lib.STRUCTS["MnrfBank"]
    assert frames._Maps is _lib.STRUCTS["MnrfFrameMaps"] and frames._Images is _lib.STRUCTS["MnrfFrameImages"]
    assert tuple(n for n, _ in frames._Maps._fields_) == tuple(n for n, _ in frames._Images._fields_) == frames.STEMS
    assert losses.FLAG_GEOMETRY_STAGE == 1 and losses.FLAG_PLANE_ON_DEVICE == 256 == _lib.MNRF_LOSS_PLANE_ON_DEVICE


def test_the_header_is_read_once_per_process(L, monkeypatch, tmp_path):
    """lib() types the entry points from the dict made at import: it neither reads nor parses the header again."""
    from mirror_nerf_amd import _abi, _lib

    def refuse(*a, **k):
        raise AssertionError("the header was parsed again")
    monkeypatch.setattr(_abi, "parse_header", refuse)
    monkeypatch.setattr(_lib, "HEADER", str(tmp_path / "gone.h"))
    assert _lib.lib() is L
    monkeypatch.setattr(_lib, "_lib", None)          # even a fresh load of the library
    fresh = _lib.lib()
    assert fresh.mnrf_embed.argtypes == _lib.SIGNATURES["mnrf_embed"][1]


def test_missing_header_fails_loudly(monkeypatch, tmp_path):
    from mirror_nerf_amd import _lib
    monkeypatch.setattr(_lib, "HEADER", str(tmp_path / "nope.h"))
    with pytest.raises(RuntimeError, match="nope.h not found"):
        _lib._read_header()


# ---- the compiler as referee: the host C++ compiler reads the same header and states what it sees

REFEREE = r"""
#include <cstddef>
#include <cstdio>
#include <tuple>
#include <type_traits>
#include "mnrf.h"
template <class T> void code() {
    if constexpr (std::is_pointer_v<T>) std::printf(std::is_pointer_v<std::remove_pointer_t<T>> ? " pp" : " p");
    else if constexpr (std::is_floating_point_v<T>) std::printf(" f%zu", sizeof(T));
    else if constexpr (std::is_unsigned_v<T>) std::printf(" u%zu", sizeof(T));
    else { static_assert(std::is_integral_v<T>, "a type with no code"); std::printf(" i%zu", sizeof(T)); }
}
template <class F> struct Sig;
template <class R, class... A> struct Sig<R (*)(A...)> {
    static void print(const char* name) { std::printf("%s", name); code<R>(); std::printf(" <-"); (code<A>(), ...); std::printf("\n"); }
    template <int I> static void pointee(const char* name) {
        std::printf("%s#%d", name, I); code<std::remove_cv_t<std::remove_pointer_t<std::tuple_element_t<I, std::tuple<A...>>>>>();
        std::printf("\n");
    }
};
int main() {
"""


def _code(t):
    import ctypes as C
    if t in (C.c_void_p, C.c_char_p):
        return " p"
    if isinstance(t, type) and issubclass(t, C._Pointer):
        return " pp" if t._type_ is C.c_void_p else " p"
    kind = "f" if t in (C.c_float, C.c_double) else "u" if t(-1).value > 0 else "i"
    return f" {kind}{C.sizeof(t)}"


def test_the_compiler_agrees_with_the_generated_binding(tmp_path):
    """Return and argument types of every entry point (pointer / pointer to pointer / signed, unsigned or floating + size; for a
    MNRF_HOST pointer also its pointee), size and field offsets of every struct and the value of every constant, as g++ sees
    them in include/mnrf.h, against the ctypes objects the package generated from the same file."""
    import ctypes as C
    from mirror_nerf_amd import _lib
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    body, want = [], []
    for name, (res, args) in _lib.SIGNATURES.items():
        body.append(f'Sig<decltype(&{name})>::print("{name}");')
        want.append(name + _code(res) + " <-" + "".join(_code(a) for a in args))
        for i, a in enumerate(args):
            if issubclass(a, C._Pointer) and a._type_ is not C.c_void_p:
                body.append(f'Sig<decltype(&{name})>::pointee<{i}>("{name}");')
                want.append(f"{name}#{i}" + _code(a._type_))
    for name, cls in _lib.STRUCTS.items():
        body.append(f'std::printf("{name} %zu\\n", sizeof({name}));')
        want.append(f"{name} {C.sizeof(cls)}")
        for field, _ in cls._fields_:
            body.append(f'std::printf("{name}.{field} %zu %zu\\n", offsetof({name}, {field}), sizeof((({name}*)0)->{field}));')
            want.append(f"{name}.{field} {getattr(cls, field).offset} {getattr(cls, field).size}")
    for name, value in _lib.CONSTANTS.items():
        body.append(f'std::printf("{name} %lld\\n", (long long)({name}));')
        want.append(f"{name} {value}")
    assert len(_lib.SIGNATURES) > 100 and len(_lib.STRUCTS) == 4 and len(want) == len(body)
    src = tmp_path / "referee.cpp"
    src.write_text(REFEREE + "\n".join("    " + line for line in body) + "\n    return 0;\n}\n")
    exe = tmp_path / "referee"
    r = subprocess.run([gxx, "-std=c++17", "-O0", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
