"""Embedding and MirrorNeRF with the reference's constructor/forward signatures
(models/mirror_nerf.py:6-38, 41-212), evaluated by the fused HIP field kernel.

The modules own ordinary `nn.Linear` parameters under the reference's names, built in the
reference's construction order (so a given `torch.manual_seed` yields the same weights and
reference checkpoints load with `load_state_dict`).  `forward` does no arithmetic in
Python: it hands pointers to `mnrf_field_forward`.  Outputs carry no autograd history
(inference / forward path; see DESIGN.md "out of scope this round").
"""
import os

import torch
from torch import nn

from . import _lib
from .weights import folded_of, packed_of


class Embedding(nn.Module):
    """models/mirror_nerf.py:6-38.  x (B, f) -> (B, f*(2*N_freqs+1))."""

    def __init__(self, N_freqs, logscale=True):
        super().__init__()
        if not logscale:
            raise NotImplementedError("only logscale=True (the reference default) is implemented")
        self.N_freqs = N_freqs
        self.freq_bands = 2 ** torch.linspace(0, N_freqs - 1, N_freqs) if N_freqs > 0 else torch.zeros(0)

    def forward(self, x):
        x = x.float().contiguous()
        n, c = x.shape
        out = torch.empty(n, c * (2 * self.N_freqs + 1), dtype=torch.float32, device=x.device)
        if n:
            _lib.check(_lib.lib().mnrf_embed(_lib.ptr(x), n, c, self.N_freqs, _lib.ptr(out), _lib.stream()),
                       "mnrf_embed")
        return out


# Arithmetic of the field kernel's Linears:
#   "split" -- every fp32 operand carried as a hi/lo f16 pair on the f16 matrix pipe with fp32 accumulation
#              (MNRF_SPLIT_F16; agrees with the fp32 chain to ~3e-6, 3.2x faster; default; see
#              csrc/mnrf_field_split.inc);
#   "fp32"  -- v_mfma_f32_16x16x4_f32, bit-for-bit an fp32 fmaf chain.
# The training path (forward with saved activations, activation gradients, second-order pass) follows the same switch.
PRECISION = os.environ.get("MNRF_PRECISION", "split")


def set_precision(mode):
    """Select the arithmetic of the inference field kernel: "fp32" or "split"."""
    global PRECISION
    if mode not in ("fp32", "split"):
        raise ValueError("precision must be 'fp32' or 'split'")
    PRECISION = mode


# ---- range guard of the split arithmetic (include/mnrf.h MNRF_GUARD_*, csrc/mnrf_field_split.inc "range guard")
# The split kernels raise a sticky flag in the last word of the module's packed weight image when an operand of a Linear
# reaches the f16 maximum (65504: the hi/lo pair stops carrying fp32 there), a weight is out of range, or a position has
# |x| >= 64 (sin/cos arguments beyond the fast exact reduction).  The flag costs the kernels one VALU per converted pair;
# the HOST reads it at the natural sync points -- the end of a frame (batched_inference), of a training forward
# (NeRFSystem.forward), of a training step (training.train_step), of a stand-alone render_rays / MirrorNeRF.forward call
# -- and when it is set the module is switched to the exact fp32 kernels for good and the work is repeated, so a result
# computed outside the range of the fast arithmetic is never returned.  The one exception is training.train_step, which
# reads the flag asynchronously and learns about a trip one step late (that step's update used saturated values; every
# later step runs on fp32): a synchronous read there drains the queue before the optimizer step and costs 6 % of the step.
# MNRF_GUARD=0 disables the host side.
GUARD = os.environ.get("MNRF_GUARD", "1") != "0"
GUARD_NAMES = {_lib.MNRF_GUARD_SATURATED: "an activation reached the f16 maximum (65504)",
               _lib.MNRF_GUARD_WEIGHT: "a weight is non-finite or >= 65504",
               _lib.MNRF_GUARD_ENC_RANGE: "a sample position has |x| >= 64 (encoding argument >= 2^15)",
               _lib.MNRF_GUARD_IN_FORWARD: "in a forward evaluation",
               _lib.MNRF_GUARD_IN_BACKWARD: "in the training backward: a scaled activation gradient",
               _lib.MNRF_GUARD_IN_SECOND_ORDER: "in the second-order pass: a scaled tangent or signal"}


def precision_of(module):
    """The arithmetic `module` is evaluated in: the global PRECISION unless the range guard pinned it to fp32."""
    return module.__dict__.get("_mnrf_precision") or PRECISION


def reset_guard(module):
    """Undo the guard's switch to fp32 (e.g. after loading other weights into the same module)."""
    module.__dict__.pop("_mnrf_precision", None)
    module.__dict__.pop("_mnrf_transient", None)
    module.__dict__.pop("_mnrf_range_trips", None)


def guard_words(modules):
    """The guard words of `modules` (0 = clean) with ONE device->host read."""
    packs = [m.__dict__["_mnrf_packed"].packed for m in modules
             if m.__dict__.get("_mnrf_packed") is not None and m.__dict__["_mnrf_packed"].packed is not None]
    if not packs:
        return [0] * len(list(modules))
    words = torch.cat([p[-1:] for p in packs]).view(torch.int32).tolist()
    it = iter(words)
    return [next(it) if (m.__dict__.get("_mnrf_packed") is not None and m.__dict__["_mnrf_packed"].packed is not None) else 0
            for m in modules]


def check_guard(modules):
    """Read the range-guard flags of `modules` (an iterable of MirrorNeRF modules, or one NeRFSystem-like object with a
    `.models` dict).  Returns True when a module running the split arithmetic tripped: it has then been switched to the
    fp32 kernels (sticky, see reset_guard) and the caller must repeat the work whose results it was about to use.
    Custom training loops call it after `loss.backward()`; the drivers of this package call it themselves."""
    if not GUARD or PRECISION != "split":
        return False
    if hasattr(modules, "models"):
        modules = list(modules.models.values())
    modules = [m for m in dict.fromkeys(modules) if isinstance(m, MirrorNeRF) and precision_of(m) == "split"]
    if not modules:
        return False
    tripped = False
    for m, w in zip(modules, guard_words(modules)):
        if w:
            import warnings
            why = "; ".join(v for k, v in GUARD_NAMES.items() if w & k)
            m.__dict__["_mnrf_guard_trips"] = m.__dict__.get("_mnrf_guard_trips", 0) + 1
            if _range_only(w) and m.__dict__.get("_mnrf_range_trips", 0) < RANGE_TRIPS_BEFORE_PIN:
                # positions beyond the fast sin/cos range and nothing else (round 5): a property of THIS call's rays, not of the
                # model -- the work is repeated on the exact kernels and the model returns to the split arithmetic afterwards
                # (release_transient, called by the drivers behind the repeated work); a model that keeps meeting such rays is
                # pinned after RANGE_TRIPS_BEFORE_PIN calls
                m.__dict__["_mnrf_range_trips"] = m.__dict__.get("_mnrf_range_trips", 0) + 1
                m.__dict__["_mnrf_transient"] = True
                m.__dict__["_mnrf_packed"].packed[-1:].zero_()      # the sticky word: the next split launch starts clean
                warnings.warn(f"mirror_nerf_amd: the split-f16 arithmetic left its range ({why}); this call is repeated with the "
                              "exact fp32 kernels", RuntimeWarning, stacklevel=2)
            else:
                warnings.warn(f"mirror_nerf_amd: the split-f16 arithmetic left its range ({why}); this model is evaluated with "
                              "the exact fp32 kernels from now on and the affected work is repeated", RuntimeWarning, stacklevel=2)
            m.__dict__["_mnrf_precision"] = "fp32"
            tripped = True
    return tripped


RANGE_TRIPS_BEFORE_PIN = 3


def _range_only(w):
    """A guard word that says nothing but "a position was beyond the fast sin/cos range" (MNRF_GUARD_ENC_RANGE)."""
    return bool(w & _lib.MNRF_GUARD_ENC_RANGE) and not (w & (_lib.MNRF_GUARD_SATURATED | _lib.MNRF_GUARD_WEIGHT))


def _backward_saturation_only(w):
    """A guard word that says nothing but "a scaled activation gradient of the training backward reached the f16 maximum".  (The
    kernels set a MNRF_GUARD_IN_* bit only together with MNRF_GUARD_SATURATED.)"""
    return bool((w & _lib.MNRF_GUARD_SATURATED) and (w & _lib.MNRF_GUARD_IN_BACKWARD)) and not (
        w & (_lib.MNRF_GUARD_WEIGHT | _lib.MNRF_GUARD_ENC_RANGE | _lib.MNRF_GUARD_IN_FORWARD | _lib.MNRF_GUARD_IN_SECOND_ORDER))


def release_transient(modules):
    """Behind the repeated work of a range-only trip: the modules check_guard moved to fp32 for that call only return to the split
    arithmetic."""
    if hasattr(modules, "models"):
        modules = list(modules.models.values())
    for m in modules:
        if m.__dict__.pop("_mnrf_transient", None):
            m.__dict__.pop("_mnrf_precision", None)


def guard_async_begin(modules):
    """Training: start an asynchronous read of the guard words (device -> pinned host memory on the current stream) and
    return a token for guard_async_end.  Unlike check_guard this does not drain the GPU queue: the host keeps running ahead
    of the device across the optimizer step (a synchronous read costs ~0.5 ms of an 8 ms step)."""
    if not GUARD or PRECISION != "split":
        return None
    if hasattr(modules, "models"):
        modules = list(modules.models.values())
    modules = [m for m in dict.fromkeys(modules) if isinstance(m, MirrorNeRF) and precision_of(m) == "split"
               and m.__dict__.get("_mnrf_packed") is not None and m.__dict__["_mnrf_packed"].packed is not None]
    if not modules:
        return None
    dev_words = torch.cat([m.__dict__["_mnrf_packed"].packed[-1:] for m in modules]).view(torch.int32)
    host = torch.empty(len(modules), dtype=torch.int32, pin_memory=True)
    host.copy_(dev_words, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    # (dev_words: the flags on the device, for a device-side decision -- training.train_step; the gradient-scale reductions the
    #  step was ISSUED with: guard_async_end ignores a backward overflow that a reduction made since has already answered)
    return modules, host, ev, dev_words, [m.__dict__.get("_mnrf_seed_reduction", 0) for m in modules]


def pin_fp32(modules):
    """Switch `modules` (or a NeRFSystem-like object's models) to the exact fp32 kernels, as a tripped guard does."""
    if hasattr(modules, "models"):
        modules = list(modules.models.values())
    for m in modules:
        if isinstance(m, MirrorNeRF):
            m.__dict__["_mnrf_precision"] = "fp32"
            m.__dict__.pop("_mnrf_transient", None)      # (for good: release_transient leaves it alone)


GRAD_SCALE_STEP, GRAD_SCALE_MAX = 4, 8       # bits per adaptation / in total (mnrf_field_backward_planes takes r <= 15)


def _lower_gradient_scale(m, w):
    """A trip that was ONLY a scaled activation gradient of the training backward outgrowing the f16 range (trained weights
    amplify gradients on their way down the trunk; the per-sample scale puts the largest seed at 2^6 and the planes hold up to
    2^12): lower that scale by 2^4 for this module instead of giving up the split arithmetic -- the loss-scaling move, downwards.
    Returns True when it did."""
    if _backward_saturation_only(w):
        r = m.__dict__.get("_mnrf_seed_reduction", 0)
        if r + GRAD_SCALE_STEP <= GRAD_SCALE_MAX:
            import warnings
            m.__dict__["_mnrf_seed_reduction"] = r + GRAD_SCALE_STEP
            warnings.warn(f"mirror_nerf_amd: scaled activation gradients outgrew the f16 range in the previous training step (its update "
                          f"was skipped); this model's gradient scale is lowered by 2^{GRAD_SCALE_STEP} (now 2^-{r + GRAD_SCALE_STEP} of "
                          "the default) and it stays on the split arithmetic", RuntimeWarning, stacklevel=4)
            return True
    return False


def guard_async_end(token, adapt=False):
    """Finish guard_async_begin (waits for that copy only -- it completed long ago when called one step later).  Returns
    True when a module tripped; it is then pinned to the fp32 kernels like check_guard does -- unless `adapt` and the trip was
    a gradient-scale matter (_lower_gradient_scale): then the module stays on the split arithmetic and nothing is reported."""
    if token is None:
        return False
    modules, host, ev = token[:3]
    issued_with = token[4] if len(token) > 4 else [None] * len(modules)
    ev.synchronize()
    tripped = False
    for m, w, r0 in zip(modules, host.tolist(), issued_with):
        if w and precision_of(m) == "split":
            if adapt and r0 is not None and m.__dict__.get("_mnrf_seed_reduction", 0) > r0 and _backward_saturation_only(w):
                # the step behind this token was queued before the previous trip's adaptation took effect (flags are settled one
                # step late): its backward overflowed at the OLD scale -- the update was vetoed on the device like the first one's,
                # but it says nothing about the new scale.  Without this one overflow cost two adaptations.
                continue
            m.__dict__["_mnrf_guard_trips"] = m.__dict__.get("_mnrf_guard_trips", 0) + 1
            if adapt and _lower_gradient_scale(m, w):
                continue
            if adapt and _range_only(w) and m.__dict__.get("_mnrf_range_trips", 0) < RANGE_TRIPS_BEFORE_PIN:
                # one rank, skip mode: the step's update was vetoed on the device; a batch whose rays leave the fast sin/cos range
                # costs that batch, not the model's arithmetic (a scene that keeps doing it is pinned after a few)
                m.__dict__["_mnrf_range_trips"] = m.__dict__.get("_mnrf_range_trips", 0) + 1
                import warnings
                warnings.warn("mirror_nerf_amd: a training batch held positions beyond the fast sin/cos range (|x| >= 64); its update "
                              "was skipped, the model stays on the split arithmetic", RuntimeWarning, stacklevel=3)
                continue
            import warnings
            why = "; ".join(v for k, v in GUARD_NAMES.items() if w & k)
            warnings.warn(f"mirror_nerf_amd: the split-f16 arithmetic left its range in the previous training step ({why}); "
                          "this model is evaluated with the exact fp32 kernels from now on", RuntimeWarning, stacklevel=3)
            m.__dict__["_mnrf_precision"] = "fp32"
            tripped = True
    return tripped


def verify_split(module, n=8192, bound=4.0, seed=0):
    """Evaluate `module` on n random positions of [-bound, bound]^3 with both arithmetics and return the largest
    difference of each output relative to max(1, |fp32 output|).  ~3e-6 is normal; a large value means some activation
    left the range the f16 hi/lo pairs carry (> 1.3e5) -- use set_precision("fp32") for that model."""
    global PRECISION
    dev = next(module.parameters()).device
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    x = (torch.rand(n, 3, device=dev, generator=g) * 2 - 1) * bound
    d = torch.nn.functional.normalize(torch.randn(n, 3, device=dev, generator=g), dim=1)
    de = Embedding(4)(d)
    old, old_pin, out = PRECISION, module.__dict__.pop("_mnrf_precision", None), {}
    try:
        for mode in ("fp32", "split"):
            PRECISION = mode
            out[mode] = field_forward(module, n, xyz=x.contiguous(), xyz_stride=3, spr=1, dir_emb=de, dir_stride=27)
    finally:
        PRECISION = old
        if old_pin is not None:
            module.__dict__["_mnrf_precision"] = old_pin
    return {k: float((out["fp32"][k] - out["split"][k]).abs().max() / max(1.0, float(out["fp32"][k].abs().max())))
            for k in out["fp32"]}


# When a list is installed here, every field-kernel launch is bracketed by two events on the
# launching stream and (flags, B, start, end) is appended -- bench.py reads kernel time from it.
LAUNCH_LOG = None

# algorithmic work per sample (SURVEY 8d / BASELINE.md section 3), FLOP = 2*MAC
FLOP_FULL = 1318912
FLOP_SIGMA = 982528
FLOP_GRAD = 982528      # density-gradient pass: the trunk GEMMs once more, transposed


def field_forward(module, B, *, xyz=None, xyz_stride=3, rays=None, z_vals=None, spr=1, dir_emb=None,
                  dir_stride=27, sigma_only=False, grad_normal=False, want_geo=False, device=None):
    """Run the fused field kernel; returns flat per-sample tensors (sigma (B,), rgb (B,3), ...)."""
    # (the full forward-only split launches read the image's folded head stream: weights.folded_of)
    packed = folded_of(module) if precision_of(module) == "split" and not sigma_only and not grad_normal else packed_of(module)
    dev = packed.device
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
    out = {"sigma": f(B)}
    # optional heads (mirror_nerf.py:80-99): an absent head is packed as zeros and its output is simply not requested
    if getattr(module, "predict_normal", True) and not sigma_only:
        out["pred_normal"] = f(B, 3)
    if not sigma_only:
        out["rgb"] = f(B, 3)
        if getattr(module, "predict_mirror_mask", True):
            out["is_mirror"] = f(B)
    if grad_normal:
        out["normal"] = f(B, 3)
    if want_geo:
        out["geo_feat"] = f(B, 256)
    flags = (_lib.MNRF_SIGMA_ONLY if sigma_only else 0) | (_lib.MNRF_GRAD_NORMAL if grad_normal else 0)
    prec = precision_of(module)
    if prec == "split":
        flags |= _lib.MNRF_SPLIT_F16
    p = _lib.ptr
    if LAUNCH_LOG is not None:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    _lib.check(_lib.lib().mnrf_field_forward(
        p(packed), flags, B, p(xyz), xyz_stride, p(rays), p(z_vals), spr, p(dir_emb), dir_stride,
        p(out["sigma"]), p(out.get("rgb")), p(out.get("pred_normal")), p(out.get("is_mirror")),
        p(out.get("normal")), p(out.get("geo_feat")), _lib.stream()), "mnrf_field_forward")
    if LAUNCH_LOG is not None:
        e1.record()
        LAUNCH_LOG.append((flags, B, e0, e1))
    return out


class MirrorNeRF(nn.Module):
    """models/mirror_nerf.py:41-212 (same constructor, parameter names and forward contract)."""

    def __init__(self, D=8, W=256, in_channels_xyz=63, in_channels_dir=27, skips=[4], **kwargs):
        super().__init__()
        self.D, self.W = D, W
        self.in_channels_xyz, self.in_channels_dir = in_channels_xyz, in_channels_dir
        self.skips = skips
        for i in range(D):
            if i == 0:
                layer = nn.Linear(in_channels_xyz, W)
            elif i in skips:
                layer = nn.Linear(W + in_channels_xyz, W)
            else:
                layer = nn.Linear(W, W)
            setattr(self, f"xyz_encoding_{i+1}", nn.Sequential(layer, nn.ReLU(True)))
        self.geo_feat_dim = W
        self.xyz_encoding_final = nn.Linear(W, W)
        self.dir_encoding = nn.Sequential(nn.Linear(W + in_channels_dir, W // 2), nn.ReLU(True))
        self.sigma = nn.Linear(W, 1)
        self.rgb = nn.Sequential(nn.Linear(W // 2, 3), nn.Sigmoid())
        self.predict_normal = kwargs.get("predict_normal", False)
        if self.predict_normal:
            self.hidden_dim_normal = W // 2
            self.normal_net = nn.Sequential(nn.Linear(W, W // 2), nn.Linear(W // 2, 3))
        self.predict_mirror_mask = kwargs.get("predict_mirror_mask", False)
        if self.predict_mirror_mask:
            self.hidden_dim_is_mirror = W // 2
            self.is_mirror_net = nn.Sequential(nn.Linear(W, W // 2), nn.LeakyReLU(inplace=True),
                                               nn.Linear(W // 2, 1), nn.Sigmoid())
        # --N_emb_xyz / --N_emb_dir (opt.py:35-46) below the defaults run on the same kernels: the kernel always evaluates
        # 10 / 4 frequency bands and the weight columns of the bands this model does not have are packed as zeros
        # (weights.pack_state), so every value and every gradient is the reference's.  More bands, another depth / width
        # / skip layout do not fit the kernels' register and weight-stream layout.
        ok_in = (in_channels_xyz - 3) % 6 == 0 and 3 <= in_channels_xyz <= 63 and \
            (in_channels_dir - 3) % 6 == 0 and 3 <= in_channels_dir <= 27
        if (D, W, list(skips)) != (8, 256, [4]) or not ok_in:
            raise NotImplementedError(
                "the HIP field kernel covers the reference's trunk: D=8, W=256, skips=[4], Embedding(N <= 10) for positions "
                "(3 + 6 N <= 63 input channels) and Embedding(N <= 4) for directions (<= 27), with or without the normal / "
                "mirror-mask heads")
        self.n_freqs_xyz, self.n_freqs_dir = (in_channels_xyz - 3) // 6, (in_channels_dir - 3) // 6

    def forward(self, x, compute_normal=True, sigma_only=False, embedding_xyz=None, embedding_dir=None,
                mirror_mask=None, detach_density_outside_mirror_for_mask_loss=False,
                detach_density_for_mask_loss=False, detach_density_for_normal_loss=False):
        """x: (B,3) when sigma_only else (B, 3+27) = [raw xyz, embedded dir] (mirror_nerf.py:130-133).
        The three detach_* flags only alter gradients in the reference; values are identical."""
        if embedding_xyz is None or getattr(embedding_xyz, "N_freqs", None) != self.n_freqs_xyz:
            raise NotImplementedError(f"embedding_xyz must be Embedding({self.n_freqs_xyz}) ({self.in_channels_xyz} input channels)")
        x = x.float().contiguous()
        B = x.shape[0]
        if sigma_only:
            if x.shape[1] != 3:
                raise RuntimeError(f"sigma_only expects (B,3), got {tuple(x.shape)}")
        elif x.shape[1] != 3 + self.in_channels_dir:
            raise RuntimeError(f"expected (B,{3 + self.in_channels_dir}), got {tuple(x.shape)}")
        elif self.in_channels_dir != 27:      # the kernel reads 27 view-encoding channels per sample: the absent bands as zeros
            x = torch.cat([x, torch.zeros(B, 27 - self.in_channels_dir, device=x.device)], 1).contiguous()
        ld = x.shape[1]
        o = field_forward(self, B, xyz=x, xyz_stride=ld, spr=1,
                          dir_emb=None if sigma_only else x.view(-1)[3:], dir_stride=ld,
                          sigma_only=sigma_only, grad_normal=compute_normal, want_geo=True) if B else None
        if B and check_guard([self]):      # range guard: the module is on the fp32 kernels now (a range-only trip: for this call), evaluate again
            try:
                return self.forward(x, compute_normal, sigma_only, embedding_xyz, embedding_dir)
            finally:
                release_transient([self])
        out = {}
        dev = x.device
        z = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
        if compute_normal:
            out["normal"] = o["normal"] if B else z(0, 3)
        out["sigma"] = o["sigma"].view(B, 1) if B else z(0, 1)
        out["geo_feat"] = o["geo_feat"] if B else z(0, 256)
        if sigma_only:
            # the reference evaluates normal_net here as well (mirror_nerf.py:154-161)
            if self.predict_normal:
                if B:
                    xx = torch.cat([x, torch.zeros(B, 27, device=dev)], 1).contiguous()
                    o2 = field_forward(self, B, xyz=xx, xyz_stride=30, spr=1, dir_emb=xx.view(-1)[3:], dir_stride=30)
                    out["pred_normal"] = o2["pred_normal"]
                else:
                    out["pred_normal"] = z(0, 3)
        else:
            if self.predict_normal:
                out["pred_normal"] = o["pred_normal"] if B else z(0, 3)
            out["rgb"] = o["rgb"] if B else z(0, 3)
            if self.predict_mirror_mask:
                out["is_mirror"] = o["is_mirror"].view(B, 1) if B else z(0, 1)
        return out
