"""The D-NeRF object field of app_reflect_newly_placed_objects (the reference's default --obj_model_type, eval.py:108,
233-259, 1062-1077): DirectTemporalNeRF (models/d_nerf/run_dnerf_helpers.py:70-253) behind the reference's own parameter
names, its render_rays (models/d_nerf/run_dnerf.py:441-597) and the loader of its checkpoints.

The field runs in ONE HIP launch per evaluation (csrc/mnrf_dnerf.hip, exact fp32 matrix instructions): deformation net,
x + dx, canonical net.  `set_precision("split")` does not reach it.  Sampling and compositing are the kernels render_rays
uses for the scene (mnrf_sample_coarse / mnrf_sample_fine / mnrf_composite): the reference's raw2outputs is the same
computation up to `dists * norm(rays_d)`, a factor within an ulp of 1 for the unit directions every ray producer here makes.
"""
import ctypes
import os

import torch
from torch import nn

from . import _lib
from .weights import _GENERATION, param_refs

__all__ = ["DirectTemporalNeRF", "NeRFOriginal", "render_rays_dnerf", "load_dnerf_object", "read_config", "dnerf_field"]

PARAM_NAMES = []
for _i in range(8):
    PARAM_NAMES += [f"_occ.pts_linears.{_i}.weight", f"_occ.pts_linears.{_i}.bias"]
for _n in ("views_linears.0", "feature_linear", "alpha_linear", "rgb_linear"):
    PARAM_NAMES += [f"_occ.{_n}.weight", f"_occ.{_n}.bias"]
for _i in range(8):
    PARAM_NAMES += [f"_time.{_i}.weight", f"_time.{_i}.bias"]
PARAM_NAMES += ["_time_out.weight", "_time_out.bias"]

PARAM_SHAPES = {}
for _net, _extra in (("_occ.pts_linears", 0), ("_time", 21)):
    for _i in range(8):
        _in = 63 + _extra if _i == 0 else (319 if _i == 5 else 256)
        PARAM_SHAPES[f"{_net}.{_i}.weight"] = (256, _in)
        PARAM_SHAPES[f"{_net}.{_i}.bias"] = (256,)
PARAM_SHAPES.update({
    "_occ.views_linears.0.weight": (128, 283), "_occ.views_linears.0.bias": (128,),
    "_occ.feature_linear.weight": (256, 256), "_occ.feature_linear.bias": (256,),
    "_occ.alpha_linear.weight": (1, 256), "_occ.alpha_linear.bias": (1,),
    "_occ.rgb_linear.weight": (3, 128), "_occ.rgb_linear.bias": (3,),
    "_time_out.weight": (3, 256), "_time_out.bias": (3,),
})

N_FREQS_XYZ, N_FREQS_DIR = 10, 4
CH_XYZ, CH_DIR, CH_TIME = 63, 27, 21


def _covered(D, W, input_ch, input_ch_views, input_ch_time, skips, use_viewdirs, memory):
    if (D, W, input_ch, input_ch_views, input_ch_time, list(skips), bool(use_viewdirs), list(memory)) != \
            (8, 256, CH_XYZ, CH_DIR, CH_TIME, [4], True, []):
        raise NotImplementedError(
            "the HIP D-NeRF field is built for D=8, W=256, skips=[4], multires 10 (63 position / 21 time channels), "
            f"multires_views 4 (27 channels) and use_viewdirs; got D={D}, W={W}, input_ch={input_ch}, "
            f"input_ch_views={input_ch_views}, input_ch_time={input_ch_time}, skips={list(skips)}, use_viewdirs={use_viewdirs}")


class NeRFOriginal(nn.Module):
    """The canonical network (run_dnerf_helpers.py:171-253): parameter names and construction order of the reference.  It is
    evaluated as part of DirectTemporalNeRF only."""

    def __init__(self, D=8, W=256, input_ch=CH_XYZ, input_ch_views=CH_DIR, input_ch_time=CH_TIME, output_ch=4, skips=(4,),
                 use_viewdirs=True, memory=(), embed_fn=None, output_color_ch=3, zero_canonical=True):
        super().__init__()
        _covered(D, W, input_ch, input_ch_views, input_ch_time, skips, use_viewdirs, memory)
        if output_color_ch != 3:
            raise NotImplementedError("output_color_ch must be 3")
        self.D, self.W, self.input_ch, self.input_ch_views, self.skips, self.use_viewdirs = D, W, input_ch, input_ch_views, list(skips), True
        layers = [nn.Linear(input_ch, W)]
        for i in range(D - 1):
            layers += [nn.Linear(W + (input_ch if i in self.skips else 0), W)]
        self.pts_linears = nn.ModuleList(layers)
        self.views_linears = nn.ModuleList([nn.Linear(input_ch_views + W, W // 2)])
        self.feature_linear = nn.Linear(W, W)
        self.alpha_linear = nn.Linear(W, 1)
        self.rgb_linear = nn.Linear(W // 2, output_color_ch)

    def forward(self, x, ts):
        raise NotImplementedError("the canonical network runs inside DirectTemporalNeRF's launch (time 0 is the canonical frame)")


class _PackedCache:
    """The packed image of one DirectTemporalNeRF, rebuilt when a parameter changed (the key of weights.PackedCache)."""

    def __init__(self):
        self.key, self.packed = None, None

    def get(self, module):
        key = [_GENERATION[0]]
        for sub, pname, _ in param_refs(module):
            q = sub._parameters[pname]
            key += [q.data_ptr(), q._version]
        if key != self.key or self.packed is None:
            self.packed = pack_state({full: sub._parameters[pname] for sub, pname, full in param_refs(module)}, self.packed)
            self.key = key
        return self.packed


def pack_state(tensors, out=None):
    """{parameter name: fp32 CUDA tensor} in the reference's naming -> the packed image of mnrf_dnerf_pack_weights."""
    L = _lib.lib()
    missing = [n for n in PARAM_NAMES if n not in tensors]
    if missing:
        raise RuntimeError(f"D-NeRF state: missing parameters {missing}")
    arr = (ctypes.c_void_p * _lib.DNERF_N_PARAMS)()
    keep = []
    for i, n in enumerate(PARAM_NAMES):
        t = tensors[n].detach()
        if tuple(t.shape) != PARAM_SHAPES[n]:
            raise RuntimeError(f"{n}: shape {tuple(t.shape)} != {PARAM_SHAPES[n]} (D=8, W=256, multires 10/4 only)")
        if t.dtype != torch.float32 or not t.is_cuda:
            raise RuntimeError(f"{n}: need a float32 CUDA tensor")
        t = t.contiguous()
        keep.append(t)
        arr[i] = t.data_ptr()
    if out is None:
        out = torch.empty(L.mnrf_dnerf_packed_floats(), dtype=torch.float32, device=keep[0].device)
    _lib.check(L.mnrf_dnerf_pack_weights(arr, _lib.ptr(out), _lib.stream()), "mnrf_dnerf_pack_weights")
    return out


def packed_of(module):
    cache = module.__dict__.get("_mnrf_dnerf_packed")
    if cache is None:
        cache = module.__dict__["_mnrf_dnerf_packed"] = _PackedCache()
    return cache.get(module)


def dnerf_field(module, B, t, *, xyz=None, xyz_stride=3, rays=None, z_vals=None, spr=1, dir_emb=None, sigma_only=False,
                raw_rgb=False, want_dx=True):
    """One mnrf_dnerf_forward launch of `module` on B samples at time t -> dict(sigma (B) raw, rgb (B,3), dx (B,3))."""
    packed = packed_of(module)
    dev = packed.device
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
    out = {"sigma": f(B)}
    if not sigma_only:
        out["rgb"] = f(B, 3)
    if want_dx:
        out["dx"] = f(B, 3)
    t = float(t)
    flags = (_lib.MNRF_DNERF_SIGMA_ONLY if sigma_only else 0) | (_lib.MNRF_DNERF_RAW_RGB if raw_rgb else 0)
    if t == 0.0 and module.zero_canonical:                      # run_dnerf_helpers.py:147-148
        flags |= _lib.MNRF_DNERF_CANONICAL
    p = _lib.ptr
    dir_ptr, dir_stride = None, CH_DIR
    if dir_emb is not None:
        # rows of 27 floats, possibly a column slice of wider rows (the view encoding inside forward's x): read in place
        if dir_emb.device != dev or dir_emb.dtype != torch.float32 or dir_emb.stride(1) != 1 or dir_emb.shape[1] < CH_DIR:
            raise RuntimeError("dir_emb: need fp32 rows of at least 27 contiguous floats on the model's device")
        dir_ptr, dir_stride = ctypes.c_void_p(dir_emb.data_ptr()), dir_emb.stride(0)
    _lib.check(_lib.lib().mnrf_dnerf_forward(
        p(packed), flags, B, p(xyz), xyz_stride, p(rays), p(z_vals), spr, dir_ptr, dir_stride,
        t, p(out["sigma"]), p(out.get("rgb")), p(out.get("dx")), _lib.stream()), "mnrf_dnerf_forward")
    return out


class DirectTemporalNeRF(nn.Module):
    """run_dnerf_helpers.py:70-154 behind the same constructor, parameter names and construction order (`_occ`, then `_time`,
    `_time_out`): the same seed gives the reference's initial weights, and its `network_fn_state_dict` loads directly."""

    def __init__(self, D=8, W=256, input_ch=CH_XYZ, input_ch_views=CH_DIR, input_ch_time=CH_TIME, output_ch=4, skips=(4,),
                 use_viewdirs=True, memory=(), embed_fn=None, zero_canonical=True):
        super().__init__()
        _covered(D, W, input_ch, input_ch_views, input_ch_time, skips, use_viewdirs, memory)
        self.D, self.W, self.input_ch, self.input_ch_views, self.input_ch_time = D, W, input_ch, input_ch_views, input_ch_time
        self.skips, self.use_viewdirs, self.memory, self.zero_canonical = list(skips), True, [], bool(zero_canonical)
        self.embed_fn = embed_fn          # kept for the reference's signature: the kernel encodes x + dx itself
        self._occ = NeRFOriginal(D=D, W=W, input_ch=input_ch, input_ch_views=input_ch_views, input_ch_time=input_ch_time,
                                 output_ch=output_ch, skips=skips, use_viewdirs=use_viewdirs, memory=memory, embed_fn=embed_fn,
                                 output_color_ch=3)
        layers = [nn.Linear(input_ch + input_ch_time, W)]
        for i in range(D - 1):
            layers += [nn.Linear(W + (input_ch if i in self.skips else 0), W)]
        self._time, self._time_out = nn.ModuleList(layers), nn.Linear(W, 3)

    @torch.no_grad()
    def forward(self, x, ts):
        """x = cat[embed(xyz) (63), embed(viewdir) (27)], ts = [embed(t), embed(t)] (B, 21) each, one time for all rows ->
        (cat[rgb raw, alpha raw] (B,4), dx (B,3)).  The position is x[:, :3], the time ts[0][0, 0]: the encodings' first
        channels are the raw inputs."""
        x = x.float().contiguous()
        B = x.shape[0]
        if x.shape[1] != CH_XYZ + CH_DIR:
            raise ValueError(f"x has {x.shape[1]} channels, not {CH_XYZ} + {CH_DIR}")
        if B == 0:
            return x.new_zeros(0, 4), x.new_zeros(0, 3)
        t = ts[0]
        if bool((t[:, :1] != t[0, 0]).any()):
            raise AssertionError("Only accepts all points from same time")          # run_dnerf_helpers.py:143-145
        o = dnerf_field(self, B, float(t[0, 0]), xyz=x, xyz_stride=x.shape[1], spr=1, dir_emb=x[:, CH_XYZ:], raw_rgb=True)
        return torch.cat([o["rgb"], o["sigma"][:, None]], 1), o["dx"]


@torch.no_grad()
def render_rays_dnerf(ray_batch, **render_kwargs):
    """The reference's render_rays (run_dnerf.py:441-597) for (N, 9) rows [o, d, near, far, frame_time] or (N, 12) rows with
    the unit view direction appended (eval.py:234-247), on the device.  Keys honoured: network_fn, network_fine, N_samples,
    N_importance, white_bkgd, use_two_models_for_fine, lindisp, perturb (0 / False only), raw_noise_std (0 only); everything
    else (network_query_fn, near, far ...) is ignored, as `**kwargs` swallows it there.  (N, 9) rows take d / |d| as the view
    direction, as the reference's `render` does in front of this function.  -> rgb_map, disp_map, acc_map, depth_map, z_vals,
    position_delta."""
    from .rendering import _embed, _linspace01, sample_pdf
    kw = render_kwargs
    net = kw["network_fn"]
    fine = kw.get("network_fine")
    N_samples, N_importance = int(kw["N_samples"]), int(kw.get("N_importance", 0))
    if kw.get("perturb", 0) not in (0, 0.0, False):
        raise NotImplementedError("render_rays_dnerf: perturb > 0 (stratified sampling) is a training feature")
    if kw.get("raw_noise_std", 0) not in (0, 0.0):
        raise NotImplementedError("render_rays_dnerf: raw_noise_std > 0 is a training feature")
    if not isinstance(net, DirectTemporalNeRF) or not (fine is None or isinstance(fine, DirectTemporalNeRF)):
        raise NotImplementedError("render_rays_dnerf: network_fn / network_fine must be DirectTemporalNeRF modules")
    if ray_batch.dim() != 2 or ray_batch.shape[1] not in (9, 12):
        raise ValueError(f"ray_batch must be (N, 9) or (N, 12), not {tuple(ray_batch.shape)}")
    if not ray_batch.is_cuda:
        raise RuntimeError("render_rays_dnerf needs CUDA (ROCm) tensors; there is no CPU path")
    ray_batch = ray_batch.float()
    dev = ray_batch.device
    N = ray_batch.shape[0]
    L, p = _lib.lib(), _lib.ptr
    f = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)  # noqa: E731
    S_fine = N_samples + max(N_importance, 0)
    if N == 0:
        return {"rgb_map": f(0, 3), "disp_map": f(0), "acc_map": f(0), "depth_map": f(0), "z_vals": f(0, S_fine),
                "position_delta": f(0, S_fine, 3)}
    rays = ray_batch[:, :8].contiguous()
    t = kw.get("_frame_time")                     # (batched_inference knows the time: no device -> host read)
    if t is None:
        if bool((ray_batch[:, 8] != ray_batch[0, 8]).any()):
            raise AssertionError("Only accepts all points from same time")          # run_dnerf.py:61
        t = float(ray_batch[0, 8])
    if ray_batch.shape[1] > 9:
        view = ray_batch[:, -3:]
    else:
        view = ray_batch[:, 3:6] / torch.norm(ray_batch[:, 3:6], dim=-1, keepdim=True)
    dir_emb = _embed(view, N_FREQS_DIR)
    white = int(bool(kw.get("white_bkgd", False)))

    z = f(N, N_samples)
    _lib.check(L.mnrf_sample_coarse_n(p(rays), N, p(_linspace01(N_samples, dev)), N_samples, int(bool(kw.get("lindisp", False))),
                                      0.0, None, p(z), None, _lib.stream()), "mnrf_sample_coarse")
    if N_importance > 0:
        # run_dnerf.py:536-560: only the coarse pass's weights go on (with two models its maps are rgb0 / disp0 / acc0, which this
        # function does not return), and they depend on the density alone
        o = dnerf_field(net, N * N_samples, t, rays=rays, z_vals=z, spr=N_samples, sigma_only=True, want_dx=False)
        weights = f(N, N_samples)
        _lib.check(L.mnrf_composite(p(rays), N, N_samples, p(o["sigma"]), p(z), None, None, None, None, None, white,
                                    p(weights), None, None, None, None, None, None, None, None, _lib.stream()), "mnrf_composite")
        z = sample_pdf(z, weights, N_importance, det=True)
    S = z.shape[1]
    run = net if fine is None else fine                                              # run_dnerf.py:565
    o = dnerf_field(run, N * S, t, rays=rays, z_vals=z, spr=S, dir_emb=dir_emb)
    weights, acc, rgb_map, depth = f(N, S), f(N), f(N, 3), f(N)
    _lib.check(L.mnrf_composite(p(rays), N, S, p(o["sigma"]), p(z), None, p(o["rgb"]), None, None, None, white,
                                p(weights), p(acc), p(rgb_map), p(depth), None, None, None, None, None, _lib.stream()), "mnrf_composite")
    disp = 1.0 / torch.max(1e-10 * torch.ones_like(depth), depth / acc)              # run_dnerf.py:429-431
    return {"rgb_map": rgb_map, "disp_map": disp, "acc_map": acc, "depth_map": depth, "z_vals": z,
            "position_delta": o["dx"].view(N, S, 3)}


# ---------------------------------------------------------------------------------------------------------- checkpoints
_CONFIG_KEYS = {        # key -> (type, default of the reference's config_parser, run_dnerf.py:600-860)
    "netdepth": (int, 8), "netwidth": (int, 256), "netdepth_fine": (int, 8), "netwidth_fine": (int, 256),
    "multires": (int, 10), "multires_views": (int, 4), "i_embed": (int, 0), "N_samples": (int, 64), "N_importance": (int, 0),
    "use_viewdirs": (bool, False), "use_two_models_for_fine": (bool, False), "white_bkgd": (bool, False),
    "nerf_type": (str, "original"), "not_zero_canonical": (bool, False), "lindisp": (bool, False),
}


def read_config(path):
    """The keys of a D-NeRF `config.txt` this package reads (`key = value` lines, `#` / `;` comments; a store_true flag is
    `key = True`), with the reference's defaults for the absent ones.  Other keys of the file are not looked at."""
    cfg = {k: d for k, (_, d) in _CONFIG_KEYS.items()}
    with open(path) as fh:
        for no, line in enumerate(fh, 1):
            line = line.split("#", 1)[0].split(";", 1)[0].strip()
            if not line or line.startswith("["):
                continue
            key, sep, val = line.partition("=")
            if not sep:
                key, _, val = line.partition(":")
            key, val = key.strip().lstrip("-"), val.strip().strip("'\"")
            if key not in _CONFIG_KEYS:
                continue
            typ = _CONFIG_KEYS[key][0]
            try:
                if typ is bool:
                    low = val.lower()
                    if low not in ("true", "false", "1", "0", "yes", "no", ""):
                        raise ValueError(val)
                    cfg[key] = low in ("true", "1", "yes", "")
                else:
                    cfg[key] = typ(val)
            except ValueError:
                raise ValueError(f"{path}:{no}: {key} = {val!r} is not {'a flag' if typ is bool else typ.__name__}") from None
    return cfg


def _check_config(cfg, path):
    bad = []
    want = dict(netdepth=8, netwidth=256, multires=10, multires_views=4, i_embed=0, use_viewdirs=True, nerf_type="direct_temporal")
    if cfg["use_two_models_for_fine"]:
        want.update(netdepth_fine=8, netwidth_fine=256)
    for k, v in want.items():
        if cfg[k] != v:
            bad.append(f"{k} = {cfg[k]!r} (covered: {v!r})")
    if cfg["N_samples"] < 3 or cfg["N_importance"] < 0:
        bad.append(f"N_samples = {cfg['N_samples']}, N_importance = {cfg['N_importance']} (N_samples >= 3, N_importance >= 0)")
    if bad:
        raise NotImplementedError(f"{path}: this D-NeRF configuration is not covered by the HIP field: " + "; ".join(bad))


def load_dnerf_object(ckpt_path, device, trusted=False):
    """The D-NeRF object of app_reflect_newly_placed_objects (eval.py:1062-1077): `config.txt` beside the checkpoint says how
    the object was trained, the `.tar` checkpoint holds `network_fn_state_dict` and, with use_two_models_for_fine,
    `network_fine_state_dict`.  -> the render_kwargs_test_d_nerf dict batched_inference / render_rays_dnerf take.
    `trusted` as in checkpoint.load_ckpt."""
    from .checkpoint import _load_file
    ckpt_path = os.fspath(ckpt_path)
    cfg_path = os.path.join(os.path.split(ckpt_path)[0], "config.txt")
    if not os.path.exists(cfg_path):
        raise FileNotFoundError(f"{cfg_path}: a D-NeRF checkpoint is read with the config.txt beside it (eval.py:1069-1072)")
    cfg = read_config(cfg_path)
    _check_config(cfg, cfg_path)
    ckpt = _load_file(ckpt_path, trusted)

    def model(key):
        if key not in ckpt:
            raise KeyError(f"{ckpt_path}: no '{key}' in the checkpoint")
        m = DirectTemporalNeRF(zero_canonical=not cfg["not_zero_canonical"])
        m.load_state_dict(ckpt[key])
        return m.to(device).eval()
    net = model("network_fn_state_dict")
    fine = model("network_fine_state_dict") if cfg["use_two_models_for_fine"] else None
    kwargs = {"network_query_fn": None, "perturb": False, "N_importance": cfg["N_importance"], "network_fine": fine,
              "N_samples": cfg["N_samples"], "network_fn": net, "use_viewdirs": True, "white_bkgd": cfg["white_bkgd"],
              "raw_noise_std": 0.0, "use_two_models_for_fine": cfg["use_two_models_for_fine"], "ndc": False,
              "lindisp": cfg["lindisp"]}
    kwargs.update({"near": 2.0, "far": 6.0})       # eval.py:1077; never read: near and far are columns 6 and 7 of the rays
    return kwargs
