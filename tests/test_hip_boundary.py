"""A tour of the public entry points with mistyped inputs, inside the checked mode of the binding (_lib.checked()).

THE RULE: a floating-point or integer input of another precision, or a non-contiguous view, is either CONVERTED -- the result
is bit-identical (NaN positions included) to the call with its `.float().contiguous()` / `.int().contiguous()` copy -- or
REFUSED with ValueError, RuntimeError or TypeError.  A tensor the call writes into is refused, never converted.
ctypes.ArgumentError never surfaces: inside the mode it would mean that a mistyped pointer got as far as the binding (the
controls at the end show that the mode was on).

Variants of a float32 / int32 original: float64, float16, bfloat16, a non-contiguous view cut out of a wider buffer, int64 and
bool.  Every 16-bit and 8-bit tensor is a contiguous view at the start of an allocation of four times its size (_backed), so
that even a reinterpreting read of it as float32 rows would stay inside memory this module owns.

Drivers: the 96 rays of fixture g7_eval_l1 (STRADDLE, 39 mirror rays), 64 + 64 samples, chunk 32 and 96; helpers: 33 to 65 rows.

    converts                                                          refuses
    ----------------------------------------------------------------  ----------------------------------------------------------
    render_rays (rays; eval and with gradients)                       batched_inference: object_used= that is not int32
    sample_pdf (bins_z, weights, u)                                   place_mirrors: depth, mask, normal, x_surface, mask_bool,
    Embedding.forward, MirrorNeRF.forward                                 flag, index (written in place)
    batched_inference (rays, _normal_noise) on every route            merge_objects: rgb, depth, mask, n_used (written in place)
    NeRFSystem.forward, render_rays_chunk_recursively                 ObjectBounds(bits=) that is not int32
    render_rays_dnerf (ray_batch), DirectTemporalNeRF.forward         finish_frame, colormap_depth, val_panel (every map)
    place_mirrors (rays), cull_objects (rays), ObjectBounds.cull      mesh: marching_cubes, vertex_normals, normal_rays,
    merge_objects (the objects' maps, slot, counts)                       rgb_to_uint8, component_labels
    metrics.mse / psnr / ssim / structural_similarity /               RayBank.gather (indices), RayBank.draw (out=, step_dev=)
        frame_metrics (images, valid_mask)                            TotalLoss: a predicted mirror mask (thresholded in place)
    TotalLoss (rgbs, rays, mirror_mask of the batch)
    mesh.occlusion_opacity (rays), synthetic.generate_rays (pose)
    training.train_step (rays, target, gt_mask)
    validation_step (rays, rgbs, mirror_mask of the batch; validate reads a RayBank and takes no tensor of the caller's)
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests.golden import fixtures as FX

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REFUSALS = (ValueError, RuntimeError, TypeError)
FLOATS = ("float64", "float16", "bfloat16", "strided")
MASKS = ("float64", "int64", "bool")


@pytest.fixture(scope="module", autouse=True)
def checked_mode():
    from mirror_nerf_amd import _lib
    with _lib.checked():
        yield


# ----------------------------------------------------------------------------------------------- variants
def _backed(t, dtype):
    """`t` as `dtype`: a contiguous view at the start of an allocation four times its size."""
    buf = torch.zeros(4 * max(t.numel(), 1), dtype=dtype, device=t.device)
    v = buf[:t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() == buf.data_ptr() and v.untyped_storage().nbytes() >= 4 * v.numel() * v.element_size()
    return v


def _strided(t):
    """`t` as a non-contiguous view cut out of a wider buffer (same dtype)."""
    if t.dim() >= 2:
        wide = torch.zeros(t.shape[:-1] + (t.shape[-1] + 3,), dtype=t.dtype, device=t.device)
        v = wide[..., 2:2 + t.shape[-1]]
    else:
        wide = torch.zeros(t.shape[0], 3, dtype=t.dtype, device=t.device)
        v = wide[:, 1]
    v.copy_(t)
    assert not v.is_contiguous() or t.numel() <= 1
    return v


def _variant(t, kind):
    if kind == "float64":
        return t.double()
    if kind in ("float16", "bfloat16"):
        return _backed(t, getattr(torch, kind))
    if kind == "strided":
        return _strided(t)
    if kind == "int64":
        return t.long()
    if kind == "int32":
        return t.int()
    if kind == "bool":
        return _backed(t != 0, torch.bool)
    if kind == "uint8":
        return _backed((t * 255).round() if t.is_floating_point() else t, torch.uint8)
    raise KeyError(kind)


def _back(v, like):
    """What THE RULE compares a converted call with."""
    return (v.int() if like.dtype == torch.int32 else v.float()).contiguous()


def _assert_same(a, b, what):
    if isinstance(a, dict):
        assert set(a) == set(b), (what, set(a) ^ set(b))
        for k in a:
            _assert_same(a[k], b[k], what + (k,))
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            _assert_same(x, y, what + (i,))
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
        if a.is_floating_point():
            assert torch.equal(torch.isnan(a), torch.isnan(b)), what
            a, b = torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0)
        assert torch.equal(a, b), what
    else:
        assert a == b or (a != a and b != b), what


def _rule(name, call, kinds, expect):
    """call(conv) runs the entry point with conv applied to the tensors under test; conv mistypes them (then the call converts
    or refuses) or makes the copies THE RULE compares with.  expect: "convert" / "refuse", or a dict by variant."""
    for kind in kinds:
        try:
            got = call(lambda t: _variant(t, kind))
        except REFUSALS as e:
            outcome = "refuse"
            print(f"  {name} [{kind}]: refused -- {type(e).__name__}: {str(e)[:100]}")
        else:
            _assert_same(got, call(lambda t: _back(_variant(t, kind), t)), (name, kind))
            outcome = "convert"
        want = expect[kind] if isinstance(expect, dict) else expect
        assert outcome == want, (name, kind, outcome)


# ----------------------------------------------------------------------------------------------- the shared scene
_S = {}


def _scene():
    """Fixture g7_eval_l1 once: the two scene models, the 96 rays, the arguments; the objects of G26 / G27 on first use."""
    if not _S:
        import mirror_nerf_amd as M
        from tests import test_hip_objects as TO
        fx = FX.Fixture("g7_eval_l1")
        sds = fx.state_dicts()
        _S.update(M=M, sds=sds, models={"coarse": TO._module(sds[0]), "fine": TO._module(sds[1])}, emb=TO._emb(),
                  rays=torch.from_numpy(fx.inputs["rays"]).to(DEV), args=dict(fx.meta["args"], near=0.05, root_dir="data/office"))
        assert _S["rays"].shape == (96, 8) and _S["rays"].dtype == torch.float32
    return SimpleNamespace(**_S)


def _objects():
    _scene()
    if "field_a" not in _S:
        from tests import test_hip_dnerf as TD
        from tests import test_hip_objects as TO
        g26, g27 = FX.Fixture("g26_object_office_l2"), FX.Fixture("g27_dnerf_office_l2")
        _S.update(field_a=TO._object_system(g26.meta), place_a=g26.meta["new_object"], field_b=TD._object_kwargs(g27.meta),
                  place_b=g27.meta["new_object"], time_b=g27.meta["frame_time"])
    return _scene()


def _draws(n_rays, chunk, per_chunk, seed=5):
    rs = np.random.RandomState(seed)
    return [torch.from_numpy(rs.normal(size=(min(chunk, n_rays - s), 3)).astype(np.float32)).to(DEV)
            for s in range(0, n_rays, chunk) for _ in range(per_chunk)]


def _infer(conv, chunk, args=None, draws=None, **kw):
    S = _scene()
    noise = None if draws is None else [conv(d) for d in draws]
    torch.manual_seed(0)                                              # (the draws of a route that is not given any)
    return S.M.batched_inference(S.models, S.emb, conv(S.rays), 64, 64, False, chunk, args=dict(S.args, **(args or {})),
                                 trace_secondary_rays=True, to_cpu=False, _normal_noise=noise, **kw)


# ----------------------------------------------------------------------------------------------- render_rays and its parts
def test_render_rays_in_eval_and_with_gradients():
    S = _scene()

    def eval_call(conv):
        with torch.no_grad():
            return S.M.render_rays(S.models, S.emb, conv(S.rays), 64, False, 0, 0, 64, 32768, False, test_time=True)
    _rule("render_rays eval", eval_call, FLOATS, "convert")

    def train_call(conv):
        for m in S.models.values():
            m.zero_grad(set_to_none=True)
        r = S.M.render_rays(S.models, S.emb, conv(S.rays[:33]), 64, False, 0, 0, 64, 32768, False)
        assert r["rgb_fine"].requires_grad
        (r["rgb_fine"].sum() + r["rgb_coarse"].sum()).backward()
        assert all(bool(torch.isfinite(q.grad).all()) for q in S.models["fine"].parameters() if q.grad is not None)
        return {k: v.detach() for k, v in r.items()}
    _rule("render_rays train", train_call, FLOATS, "convert")


def test_sample_pdf():
    M = _scene().M
    rs = np.random.RandomState(1)
    N, S, NI = 65, 16, 8
    bins = torch.from_numpy(np.sort(rs.uniform(2.0, 6.0, (N, S)), 1).astype(np.float32)).to(DEV)
    weights = torch.from_numpy(rs.uniform(0.0, 1.0, (N, S)).astype(np.float32)).to(DEV)
    u = torch.from_numpy(rs.uniform(0.0, 0.999, (N, NI)).astype(np.float32)).to(DEV)
    _rule("sample_pdf bins_z", lambda c: M.sample_pdf(c(bins), weights, NI, u=u), FLOATS, "convert")
    _rule("sample_pdf weights", lambda c: M.sample_pdf(bins, c(weights), NI, u=u), FLOATS, "convert")
    _rule("sample_pdf u", lambda c: M.sample_pdf(bins, weights, NI, u=c(u)), FLOATS, "convert")
    _rule("sample_pdf all", lambda c: M.sample_pdf(c(bins), c(weights), NI, u=c(u)), FLOATS, "convert")
    assert M.sample_pdf(bins, weights, NI, u=u).shape == (N, S + NI)


def test_embedding_and_field_forward():
    S = _scene()
    rs = np.random.RandomState(2)
    x = torch.from_numpy(rs.uniform(-1.0, 1.0, (65, 3)).astype(np.float32)).to(DEV)
    _rule("Embedding.forward", lambda c: S.emb["xyz"](c(x)), FLOATS, "convert")
    d = torch.from_numpy(rs.normal(size=(65, 3)).astype(np.float32)).to(DEV)
    with torch.no_grad():
        xd = torch.cat([x, S.emb["dir"](d / d.norm(dim=1, keepdim=True))], 1).contiguous()
        _rule("MirrorNeRF.forward", lambda c: S.models["fine"](c(xd), embedding_xyz=S.emb["xyz"], embedding_dir=S.emb["dir"]),
              FLOATS, "convert")
        _rule("MirrorNeRF.forward sigma_only", lambda c: S.models["fine"](c(x), sigma_only=True, embedding_xyz=S.emb["xyz"],
                                                                         embedding_dir=S.emb["dir"]), FLOATS, "convert")


# ----------------------------------------------------------------------------------------------- batched_inference
def _mirrors(roughness=0.0):
    import mirror_nerf_amd as M
    S = _scene()
    o, d = S.rays[48, :3].cpu().numpy().astype(np.float64), S.rays[48, 3:6].cpu().numpy().astype(np.float64)
    d /= np.linalg.norm(d)
    up = np.cross(d, [1.0, 0.0, 0.0])
    if np.linalg.norm(up) < 1e-3:
        up = np.cross(d, [0.0, 1.0, 0.0])
    # two mirrors across the view of ray 48, one behind the other: every chunk has rays that take one
    return [M.PlacedMirror(tuple(o + 1.0 * d), tuple(-d), tuple(up), (0.6, 0.6), roughness=roughness),
            M.PlacedMirror(tuple(o + 1.5 * d), tuple(-d), tuple(up), (3.0, 3.0), shape="ellipse")]


BIG_BOX = ((-50.0, -50.0, -50.0), (50.0, 50.0, 50.0))


def _bits_box():
    """BIG_BOX cut into 4 x 4 x 4 cells, every cell set: the occupancy words of the object on the device."""
    import mirror_nerf_amd as M
    return M.ObjectBounds(*BIG_BOX, (4, 4, 4), torch.full((4, 4, 1), 15, dtype=torch.int32, device=DEV))


def _placed(bounded):
    import mirror_nerf_amd as M
    S = _objects()
    box = None if not bounded else _bits_box() if bounded == "bits" else M.ObjectBounds(*BIG_BOX)
    return [M.PlacedObject(S.field_a, S.place_a, bounds=box), M.PlacedObject(S.field_b, S.place_b, bounds=box, time=0.8)]


ON = dict(app_reflect_newly_placed_objects=True)
CONFIGS = {
    "plain": lambda c, chunk: _infer(c, chunk),
    "rough_fan": lambda c, chunk: _infer(c, chunk, dict(app_control_mirror_roughness=True, trace_ray_times=3, normal_noise_std=0.01),
                                         _draws(96, chunk, 4), normal_noise_std=0.01, batch_jitter=True),
    "rough_loop": lambda c, chunk: _infer(c, chunk, dict(app_control_mirror_roughness=True, trace_ray_times=3, normal_noise_std=0.01),
                                          _draws(96, chunk, 4), normal_noise_std=0.01, batch_jitter=False),
    "place_new_mirror": lambda c, chunk: _infer(c, chunk, dict(app_place_new_mirror=True),
                                                new_mirror=dict(axis="x", position=-1.0, normal=(1.0, 0.0, 0.0), rect=(-1.0, 1.0, -0.5, 0.5))),
    "new_mirrors": lambda c, chunk: _infer(c, chunk, new_mirrors=_mirrors()),
    "new_mirrors_rough": lambda c, chunk: _infer(c, chunk, new_mirrors=_mirrors(0.02), rough_times=2, scene_roughness=0.01),
    "placed_objects_bounds": lambda c, chunk: _infer(c, chunk, ON, placed_objects=_placed(True)),
    "placed_objects_bits": lambda c, chunk: _infer(c, chunk, ON, placed_objects=_placed("bits")),
    "placed_objects": lambda c, chunk: _infer(c, chunk, ON, placed_objects=_placed(False)),
    "single_object_bounds": lambda c, chunk: _infer(c, chunk, dict(ON, obj_model_type="nerf_pl"), system_obj=_objects().field_a,
                                                    new_object=_objects().place_a, object_bounds=_bits_box()),
    "single_dnerf_bounds": lambda c, chunk: _infer(c, chunk, dict(ON, obj_model_type="d_nerf"), render_kwargs_test_d_nerf=_objects().field_b,
                                                   new_object=_objects().place_b, frame_time=_objects().time_b, args_d_nerf=SimpleNamespace(use_viewdirs=True),
                                                   object_bounds=_scene().M.ObjectBounds(*BIG_BOX)),
    "substitution": lambda c, chunk: _infer(c, chunk, dict(app_reflection_substitution=True),
                                            system_substitution=SimpleNamespace(models=_scene().models, embeddings=_scene().emb)),
}


@pytest.mark.parametrize("chunk", [32, 96])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_batched_inference_converts_its_rays(config, chunk):
    _rule(f"batched_inference {config} chunk {chunk}", lambda c: CONFIGS[config](c, chunk), FLOATS, "convert")
    if chunk == 96:                                                   # the configuration does what its name says
        got, plain = CONFIGS[config](lambda t: t, 96), CONFIGS["plain"](lambda t: t, 96)
        assert int((plain["mirror_mask_fine"] != 0).sum()) == 39
        if config != "plain" and "object" not in config:             # (an object shows only where a ray meets it)
            assert any(k not in plain or got[k].dtype != plain[k].dtype or not torch.equal(got[k], plain[k]) for k in got), \
                "the application changed nothing"


def test_batched_inference_refuses_an_object_used_it_cannot_write():
    S = _objects()
    for placed_kw, n in ((dict(placed_objects=_placed(True)), 2), (dict(placed_objects=_placed(True)), 1),
                         (dict(args=dict(obj_model_type="nerf_pl"), system_obj=S.field_a, new_object=S.place_a), 1)):
        extra = dict(placed_kw)
        args = dict(ON, **extra.pop("args", {}))
        for dtype in (torch.int64, torch.float32):                    # (nothing narrower than the int32 the kernels would add into)
            used = torch.full((n,), 77, dtype=dtype, device=DEV)
            with pytest.raises(ValueError, match="object_used must be an int32"):
                _infer(lambda t: t, 96, args, object_used=used, **extra)
            assert bool((used == 77).all())                           # refused before anything was written
        used = torch.full((n,), 77, dtype=torch.int32, device=DEV)
        _infer(lambda t: t.double(), 96, args, object_used=used, **extra)
        want = torch.full((n,), 77, dtype=torch.int32, device=DEV)
        _infer(lambda t: t, 96, args, object_used=want, **extra)
        assert torch.equal(used, want) and bool((used != 77).all())


# ----------------------------------------------------------------------------------------------- NeRFSystem, training
def _system(**over):
    from mirror_nerf_amd import training as T
    S = _scene()
    hp = T.default_hparams(chunk=32, perturb=0.0, noise_std=0.0, **over)
    system = S.M.NeRFSystem(hp)
    system.nerf_coarse.load_state_dict({k: torch.from_numpy(v) for k, v in S.sds[0].items()})
    system.nerf_fine.load_state_dict({k: torch.from_numpy(v) for k, v in S.sds[1].items()})
    return system.to(DEV), hp


def _gt_mask():
    return (torch.arange(96, device=DEV) % 3 == 0).float()


def test_nerf_system_forward():
    from mirror_nerf_amd import training as T
    S = _scene()
    system, hp = _system()
    gt = _gt_mask()

    def eval_call(conv_rays, conv_mask):
        with torch.no_grad():
            return system(conv_rays(S.rays), dict(T.extra_info(hp, conv_mask(gt)), is_eval=True))

    def train_call(conv_rays, conv_mask):
        system.zero_grad(set_to_none=True)
        r = system(conv_rays(S.rays), T.extra_info(hp, conv_mask(gt)))
        assert r["rgb_fine"].requires_grad and "rgb_fine_direct" in r
        r["rgb_fine"].sum().backward()
        return {k: v.detach() for k, v in r.items()}
    same = lambda t: t  # noqa: E731
    for name, call in (("eval", eval_call), ("train", train_call)):
        _rule(f"NeRFSystem.forward {name} rays", lambda c: call(c, same), FLOATS, "convert")
        _rule(f"NeRFSystem.forward {name} mirror_mask", lambda c: call(same, c), MASKS + ("strided",), "convert")
        _rule(f"NeRFSystem.forward {name} both", lambda c: call(c, c), ("float64",), "convert")
    out = eval_call(same, same)
    assert bool((out["rgb_fine_reflect"] != 0).any()) and out["rgb_fine"].shape == (96, 3)      # reflections were traced

    def level_call(conv):                                             # the level function itself, as a direct caller reaches it
        with torch.no_grad():
            return S.M.render_rays_chunk_recursively(system.models, system.embeddings, hp, conv(S.rays[:32].contiguous()), None, 0,
                                                     dict(T.extra_info(hp, gt[:32].contiguous()), is_eval=True))
    _rule("render_rays_chunk_recursively", level_call, FLOATS, "convert")


def test_train_step_on_a_float64_batch():
    from mirror_nerf_amd import training as T
    S = _scene()
    rs = np.random.RandomState(3)
    target = torch.from_numpy(rs.uniform(0, 1, (96, 3)).astype(np.float32)).to(DEV)
    gt = _gt_mask()

    def call(conv):
        torch.manual_seed(0)
        system, _ = _system()
        opt = torch.optim.Adam(system.parameters(), lr=5e-4)
        loss = T.train_step(system, opt, conv(S.rays), conv(target), conv(gt))
        after = next(iter(system.nerf_fine.parameters())).detach().clone()
        assert bool(torch.isfinite(after).all())
        return loss.detach()
    _rule("train_step", call, ("float64",), "convert")


def test_validation_step():
    S = _scene()
    system, hp = _system()
    rs = np.random.RandomState(12)
    target = torch.from_numpy(rs.uniform(0, 1, (96, 3)).astype(np.float32)).to(DEV)
    crit = S.M.get_loss(hp)

    def call(conv):
        batch = {"rays": conv(S.rays), "rgbs": conv(target), "mirror_mask": conv(_gt_mask()),
                 "valid_mask": torch.ones(96, dtype=torch.bool, device=DEV)}
        return S.M.validation_step(system, batch, crit, 5, hp)
    _rule("validation_step", call, ("float64", "strided"), "convert")
    assert bool(torch.isfinite(call(lambda t: t)["val_psnr"]))


def test_total_loss():
    from mirror_nerf_amd import training as T
    S = _scene()
    system, hp = _system()
    rs = np.random.RandomState(4)
    target = torch.from_numpy(rs.uniform(0, 1, (96, 3)).astype(np.float32)).to(DEV)
    gt = _gt_mask()
    res = {k: v.detach().clone() for k, v in system(S.rays, T.extra_info(hp, gt)).items()}      # the training route's keys
    crit = S.M.TotalLoss(SimpleNamespace())

    def call(conv_batch, conv_res=lambda t: t, conv_mask=lambda t: t):
        inputs = {k: (conv_mask(v.clone()) if k.startswith("mirror_mask") else conv_res(v)) for k, v in res.items()}
        batch = {"rgbs": conv_batch(target), "rays": conv_batch(S.rays), "mirror_mask": conv_batch(gt),
                 "valid_mask": torch.ones(96, dtype=torch.bool, device=DEV)}
        return crit(inputs, batch, epoch=5)
    _rule("TotalLoss batch", lambda c: call(c), ("float64", "strided"), "convert")
    _rule("TotalLoss inputs", lambda c: call(lambda t: t, c), ("float64", "strided"), "convert")
    _rule("TotalLoss predicted mirror mask", lambda c: call(lambda t: t, lambda t: t, c), ("float64", "strided"), "refuse")


# ----------------------------------------------------------------------------------------------- D-NeRF
def test_render_rays_dnerf():
    S = _objects()
    d = S.rays[:, 3:6]
    batch = torch.cat([S.rays, torch.full_like(S.rays[:, :1], 0.37), d / d.norm(dim=1, keepdim=True)], 1)[:65].contiguous()
    _rule("render_rays_dnerf", lambda c: S.M.render_rays_dnerf(c(batch), **S.field_b), FLOATS, "convert")
    # the module itself: x = [embedded position (63) | embedded view direction (27)], ts = the embedded time twice
    x = torch.cat([S.emb["xyz"](batch[:, :3].contiguous()), S.emb["dir"](batch[:, 9:12].contiguous())], 1).contiguous()
    ts = torch.cat([torch.full((65, 1), 0.37, device=DEV), torch.zeros(65, 20, device=DEV)], 1)
    net = S.field_b["network_fn"]
    _rule("DirectTemporalNeRF.forward x", lambda c: net(c(x), [ts, ts]), FLOATS, "convert")
    _rule("DirectTemporalNeRF.forward ts", lambda c: net(x, [c(ts), c(ts)]), ("float64", "strided"), "convert")


# ----------------------------------------------------------------------------------------------- the per-launch helpers
def _level_maps(n, seed):
    rs = np.random.RandomState(seed)
    f = lambda *s: torch.from_numpy(rs.uniform(0.1, 3.0, s).astype(np.float32)).to(DEV)  # noqa: E731
    return dict(depth=f(n), mask=(f(n) > 1.5).float(), normal=f(n, 3), x_surface=f(n, 3))


def test_place_mirrors():
    from mirror_nerf_amd import placed_mirrors as PM
    S = _scene()
    packed = PM.pack(_mirrors())
    rays = S.rays[:65].contiguous()

    def call(conv_rays, out_conv=None, which=None):
        m = _level_maps(65, 7)
        outs = dict(m, mask_bool=torch.zeros(65, dtype=torch.bool, device=DEV), flag=torch.zeros(1, dtype=torch.int32, device=DEV),
                    index=torch.full((65,), -1, dtype=torch.int32, device=DEV))
        if which is not None:
            outs[which] = out_conv(outs[which])
        PM.place_mirrors(conv_rays(rays), packed, 0.05, outs["depth"], outs["mask"], outs["normal"], outs["x_surface"], outs["mask_bool"],
                         outs["flag"], outs["index"])
        return outs
    same = lambda t: t  # noqa: E731
    _rule("place_mirrors rays", lambda c: call(c), FLOATS, "convert")
    assert bool((call(same)["index"] >= 0).any())
    for which in ("depth", "mask", "normal", "x_surface"):
        _rule(f"place_mirrors {which}", lambda c: call(same, c, which), FLOATS, "refuse")
    _rule("place_mirrors mask_bool", lambda c: call(same, c, "mask_bool"), ("float64", "int32", "int64"), "refuse")
    for which in ("flag", "index"):
        _rule(f"place_mirrors {which}", lambda c: call(same, c, which), ("int64", "float64", "bool"), "refuse")
    _rule("place_mirrors index strided", lambda c: call(same, c, "index"), ("strided",), "refuse")


def test_cull_and_merge_objects():
    from mirror_nerf_amd import placed_objects as PO
    from mirror_nerf_amd import recursion as R
    S = _objects()
    rays = S.rays[:65].contiguous()
    placed = [o.resolve(SimpleNamespace(**S.args), 0.37, torch.device(DEV)) for o in _placed(True)]
    _rule("cull_objects", lambda c: PO.cull_objects(c(rays), placed), FLOATS, "convert")
    box = S.M.ObjectBounds(*BIG_BOX)
    xform = R.resolve_new_object(None, S.place_a)

    def cull(conv):
        out, index, count = box.cull(conv(rays), xform)
        n = int(count.item())
        return out[:n], index[:n], n
    _rule("ObjectBounds.cull", cull, FLOATS, "convert")
    assert cull(lambda t: t)[2] > 0
    # the object's own tensor: occupancy words of another type are refused where they enter, on the host and on the device
    words = torch.full((4, 4, 1), 15, dtype=torch.int32, device=DEV)
    for bad in (torch.zeros(16, dtype=torch.int64), words.long(), words.float(), _backed(words, torch.uint8)):
        with pytest.raises(ValueError, match="bits must be int32"):
            S.M.ObjectBounds(*BIG_BOX, (4, 4, 4), bad)
    bits_box = _bits_box()
    _rule("ObjectBounds.cull with bits", lambda c: bits_box.cull(c(rays), xform)[2], FLOATS, "convert")
    assert int(bits_box.cull(rays, xform)[2].item()) == cull(lambda t: t)[2]

    _, _, slot, counts = PO.cull_objects(rays, placed)
    rs = np.random.RandomState(8)
    maps = [tuple(torch.from_numpy(rs.uniform(0.2, 1.0, s).astype(np.float32)).to(DEV) for s in ((65, 3), (65,), (65,))) for _ in placed]

    def merge(conv_in, out_conv=None, which=None):
        m = _level_maps(65, 9)
        outs = dict(rgb=m["normal"], depth=m["depth"], mask=m["mask"], n_used=torch.zeros(2, dtype=torch.int32, device=DEV))
        if which is not None:
            outs[which] = out_conv(outs[which])
        PO.merge_objects([tuple(conv_in(t) for t in mp) for mp in maps], placed, conv_in(slot), conv_in(counts), 65, 0.05, outs["rgb"],
                         outs["depth"], outs["mask"], outs["n_used"])
        return outs
    same = lambda t: t  # noqa: E731
    _rule("merge_objects inputs", lambda c: merge(lambda t: c(t) if t.is_floating_point() else t), FLOATS, "convert")
    _rule("merge_objects slot and counts", lambda c: merge(lambda t: t if t.is_floating_point() else c(t)), ("int64", "strided"), "convert")
    assert int(merge(same)["n_used"].sum()) > 0
    for which in ("rgb", "depth", "mask"):
        _rule(f"merge_objects {which}", lambda c: merge(same, c, which), FLOATS, "refuse")
    _rule("merge_objects n_used", lambda c: merge(same, c, "n_used"), ("int64", "float64", "strided"), "refuse")


def test_estimate_object_bounds_runs_inside_the_mode():
    S = _objects()
    b = S.M.estimate_object_bounds(S.field_a, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), res=4)
    assert b.res == (4, 4, 4) and b.bits.dtype == torch.int32
    b = S.M.estimate_object_bounds(S.field_b, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), res=4, frame_time=0.37)
    assert b.res == (4, 4, 4)


# ----------------------------------------------------------------------------------------------- metrics, frames, mesh, data
def test_metrics():
    from mirror_nerf_amd import metrics as MT
    rs = np.random.RandomState(10)
    a = torch.from_numpy(rs.uniform(0, 1, (2, 3, 13, 17)).astype(np.float32)).to(DEV)
    b = torch.from_numpy(rs.uniform(0, 1, (2, 3, 13, 17)).astype(np.float32)).to(DEV)
    valid = (torch.from_numpy(rs.uniform(0, 1, (2, 3, 13, 17))).to(DEV) > 0.3).float()
    images = ("float64", "float16", "strided", "uint8")
    for fn in (MT.mse, MT.psnr, MT.ssim):
        _rule(f"metrics.{fn.__name__}", lambda c: fn(c(a), c(b)), images, "convert")
    _rule("metrics.ssim map", lambda c: MT.ssim(c(a), c(b), reduction="none"), images, "convert")
    for fn in (MT.mse, MT.psnr):
        _rule(f"metrics.{fn.__name__} valid_mask", lambda c: fn(a, b, valid_mask=c(valid)),
              ("bool", "uint8", "int64"), "convert")
    last_a, last_b = a.permute(0, 2, 3, 1).contiguous(), b.permute(0, 2, 3, 1).contiguous()
    for fn in (MT.structural_similarity, MT.frame_metrics):
        _rule(f"metrics.{fn.__name__}", lambda c: fn(c(last_a), c(last_b)), images, "convert")


def test_frames():
    S = _scene()
    res = {k: v for k, v in _infer(lambda t: t, 96, maps_only=True).items()}
    assert res["mirror_mask_fine"].dtype == torch.float32
    finish = lambda c: S.M.finish_frame({k: c(v) for k, v in res.items()}, "fine")  # noqa: E731
    assert len(finish(lambda t: t)) >= 5
    _rule("finish_frame", finish, ("float64", "float16"), "refuse")
    depth = torch.stack([res["depth_fine"], res["depth_fine_reflect"]])
    _rule("colormap_depth", lambda c: S.M.colormap_depth(c(depth)), ("float64", "float16"), "refuse")
    _rule("colormap_depth strided", lambda c: S.M.colormap_depth(c(depth)), ("strided",), "convert")
    _rule("colormap_depth mask", lambda c: S.M.colormap_depth(depth, mask_stack=c(torch.stack([res["mirror_mask_fine"]] * 2))),
          ("float64", "bool"), "refuse")
    H, W = 8, 12
    batch = {"rgbs": res["rgb_fine"].clone(), "mirror_mask": _gt_mask()}
    panel = lambda cb, cr: S.M.val_panel((W, H), {k: cb(v) for k, v in batch.items()}, {k: cr(v) for k, v in res.items()})  # noqa: E731
    same = lambda t: t  # noqa: E731
    assert panel(same, same)[0].shape[1:] == (3, H, W)
    _rule("val_panel batch", lambda c: panel(c, same), ("float64", "bool"), "refuse")
    _rule("val_panel results", lambda c: panel(same, c), ("float64", "float16"), "refuse")


def test_mesh_entry_points():
    from mirror_nerf_amd import mesh as ME
    S = _scene()
    rs = np.random.RandomState(11)
    volume = torch.from_numpy(rs.uniform(0, 2, (5, 6, 7)).astype(np.float32)).to(DEV)
    _rule("mesh.marching_cubes", lambda c: ME.marching_cubes(c(volume), 1.0), ("float64", "float16"), "refuse")
    vertices, triangles = ME.marching_cubes(volume, 1.0)[:2]
    assert vertices.dtype == torch.float32 and triangles.dtype == torch.int32 and triangles.shape[0] > 0
    _rule("mesh.vertex_normals vertices", lambda c: ME.vertex_normals(c(vertices), triangles), ("float64", "float16"), "refuse")
    _rule("mesh.vertex_normals triangles", lambda c: ME.vertex_normals(vertices, c(triangles)), ("int64",), "refuse")
    _rule("mesh.component_labels", lambda c: ME.component_labels(vertices, c(triangles)), ("int64",), "refuse")
    normals = ME.vertex_normals(vertices, triangles)
    _rule("mesh.normal_rays", lambda c: ME.normal_rays(c(vertices), c(normals), 0.05, 8.0), ("float64", "float16"), "refuse")
    _rule("mesh.rgb_to_uint8", lambda c: ME.rgb_to_uint8(c(normals)), ("float64", "float16"), "refuse")
    with torch.no_grad():
        _rule("mesh.occlusion_opacity", lambda c: ME.occlusion_opacity(S.models["fine"], S.emb, c(S.rays[:65].contiguous())), FLOATS, "convert")


def test_raybank_and_generate_rays():
    from mirror_nerf_amd import synthetic as SY
    from tests import test_hip_raybank as TB
    b, (poses, _, _, focal) = TB._bank(F=2, H=5, W=7)
    idx = torch.arange(b.n_rays, device=DEV)
    assert b.gather(idx)[0].shape == (70, 8)
    _rule("RayBank.gather indices", lambda c: b.gather(c(idx)), ("int32", "float64"), "refuse")

    def draw(conv, which):
        out = [torch.empty(16, 8, device=DEV), torch.empty(16, 3, device=DEV), torch.empty(16, device=DEV)]
        out[which] = conv(out[which])
        return b.draw(0, 16, 1, rank=0, world=1, out=tuple(out))
    for which in range(3):
        _rule(f"RayBank.draw out[{which}]", lambda c: draw(c, which), ("float64", "float16", "strided"), "refuse")
    word = torch.zeros(1, dtype=torch.int64, device=DEV)
    b.draw(0, 16, 1, rank=0, world=1, step_dev=word)
    _rule("RayBank.draw step_dev", lambda c: b.draw(0, 16, 1, rank=0, world=1, step_dev=c(word)), ("int32", "float64"), "refuse")
    pose64 = np.asarray(poses[0], np.float64) + 1e-9
    got = SY.generate_rays(5, 7, focal, pose64, 0.05, 8.0, DEV)
    assert torch.equal(got, SY.generate_rays(5, 7, focal, pose64.astype(np.float32), 0.05, 8.0, DEV)) and got.dtype == torch.float32
    assert torch.equal(got, SY.generate_rays(5, 7, focal, torch.from_numpy(pose64), 0.05, 8.0, DEV))


# ----------------------------------------------------------------------------------------------- the controls
def test_the_mode_was_on_a_mistyped_pointer_at_the_binding_is_an_argument_error():
    """One control per element class of mnrf.h, on entry points that return before they launch (a zero-sized call, or an
    argument error): hand-built pointers into device memory this test owns, and _lib.ptr of real tensors."""
    from mirror_nerf_amd import _lib
    L = _lib.lib()
    assert _lib._checked >= 1 and _lib.ptr is _lib._ptr_checked
    mem = torch.zeros(256, dtype=torch.float64, device=DEV)

    def hand(dtype):
        q = _lib.DevicePtr(mem.data_ptr())
        q.dtype = dtype
        return q
    controls = [
        ("float", lambda q: L.mnrf_jitter_mean(q, None, None, 0, 1, 0, 0, 0.0, None), torch.float32, torch.float64),
        ("int32", lambda q: L.mnrf_jitter_mean(None, None, q, 0, 1, 0, 0, 0.0, None), torch.int32, torch.int64),
        ("int32", lambda q: L.mnrf_rough_rows(q, None, 0, 0, None, 0.0, None, None, None, None), torch.int32, torch.int64),
        ("float", lambda q: L.mnrf_rough_rows(None, q, 0, 0, None, 0.0, None, None, None, None), torch.float32, torch.bool),
        ("byte", lambda q: L.mnrf_rgb_to_uint8(None, 0, q, None), torch.uint8, torch.int32),
        ("double", lambda q: L.mnrf_accumulate_colors(None, q, None, 0.2, 0, None, None, None), torch.float64, torch.float32),
        ("int64", lambda q: L.mnrf_adam_prep(None, q, None, None, None, None, 0, None, None), torch.int64, torch.int32),
    ]
    for cls, call, right, wrong in controls:
        code = call(hand(right))
        assert code == 0 or (cls == "int64" and code < 0)            # (mnrf_adam_prep refuses its null hyper-parameters)
        with pytest.raises(ctypes.ArgumentError, match="mnrf.h declares"):
            call(hand(wrong))
    assert L.mnrf_vertex_normals(None, 0, None, 0, hand(torch.float16), None, None) == 0      # void*: anything
    for dtype, cls in ((torch.float64, "float"), (torch.float16, "float"), (torch.int64, "float")):
        t = _backed(torch.zeros(8, device=DEV), dtype)
        with pytest.raises(ctypes.ArgumentError, match=str(dtype)):
            L.mnrf_jitter_mean(_lib.ptr(t), None, None, 0, 1, 0, 0, 0.0, None)
    assert L.mnrf_jitter_mean(_lib.ptr(torch.zeros(8, device=DEV)), None, None, 0, 1, 0, 0, 0.0, None) == 0
    torch.cuda.synchronize()
    assert bool((mem == 0).all())

