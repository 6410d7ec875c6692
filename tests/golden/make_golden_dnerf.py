#!/usr/bin/env python3
"""Fixtures G27: the reference's D-NeRF object (models/d_nerf/: DirectTemporalNeRF, render_rays) and the d_nerf arm of the
new-object branch of `eval.batched_inference` (eval.py:233-259), captured from the reference itself.

Build-container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dnerf.py [name ...]
                       PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dnerf.py --calibrate

models.d_nerf.run_dnerf is imported at run time (imageio and configargparse are absent from the container and not on the
arithmetic path: empty stand-in modules); the networks and the render kwargs come from its own create_nerf.  No text of the
reference is kept here.  Weights are not stored: seed + tweaks + checksums, and every case asserts that this package's
DirectTemporalNeRF under the same seed rebuilds the reference's state_dict bit for bit (tests/dnerf_ref.make_state_dicts).

G27-model (g27_dnerf_model): the reference module's forward on N_POINTS points of [-1.5, 1.5]^3 with unit view directions, at
t = 0.37 and t = 0 (the canonical frame), in fp32 and in float64.  meta.floor[key] = max |fp32 - float64| / max(1, max |float64|)
per output group (dx, rgb, alpha) and time: the reference's own rounding noise, relative to the size of the values.

G27-scene (g27_dnerf_*): `batched_inference` of the patched eval.py (make_golden_objects.patched_eval: `pose_align` set to a
matrix so that the branch runs) with obj_model_type="d_nerf", captured like G26: the same ray picking, the same edge-margin
rule (a candidate within MARGIN of the 0.8 opacity edge or of the depth tie at any level is dropped, at most 5 % may go), the
same class conditions (level 0: transparent / blocked / used each hold >= 15 % of the rays; level 1: some ray uses the object)
and floor / floor_frac from a float64 run of the same call.  The deformation gain stays at 1 (the reference's own fp32 noise
grows quickly with it: at `_time_out x 5` its depth floor is 1.8e-3 and 1.2 % of the rays sit beyond the depth bar); the
density head gets x 1000 and a bias literal per model and case from `--calibrate`.
"""
import copy
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

import make_golden as MG  # noqa: E402  (installs the reference import stubs)
import make_golden_apps as GA  # noqa: E402
import make_golden_objects as GO  # noqa: E402
import torch  # noqa: E402

W, R = MG.W, MG.R
R._stub("configargparse")
from models.d_nerf import run_dnerf as RD  # noqa: E402  (the reference)

from tests import dnerf_ref as DR  # noqa: E402

N_POINTS = 2048
MARGIN = GO.MARGIN
OBJ_SEED = DR.MODEL_SEED


def dnerf_args(two_models, white_bkgd=False, n_samples=64, n_importance=64):
    """The fields of the reference's config that create_nerf reads, with its parser's defaults."""
    return types.SimpleNamespace(
        multires=10, multires_views=4, i_embed=0, use_viewdirs=True, N_importance=n_importance, N_samples=n_samples,
        nerf_type="direct_temporal", netdepth=8, netwidth=256, netdepth_fine=8, netwidth_fine=256, not_zero_canonical=False,
        use_two_models_for_fine=two_models, netchunk=1024 * 64, lrate=5e-4, do_half_precision=False, ft_path="none.tar",
        no_reload=True, basedir=".", expname="g27", perturb=1.0, white_bkgd=white_bkgd, raw_noise_std=0.0,
        dataset_type="blender", no_ndc=False, lindisp=False)


def ref_object(seed, tweaks, two_models, white_bkgd=False):
    """The reference's render_kwargs_test for networks built under `seed` with per-model tweaks (eval.py:1076-1077); checks the
    rebuild by this package's module.  -> (kwargs, state dicts)."""
    args = dnerf_args(two_models, white_bkgd)
    torch.manual_seed(seed)
    _, kw, _, _, _ = RD.create_nerf(args)
    kw.update({"near": 2.0, "far": 6.0})
    mods = [kw["network_fn"]] + ([kw["network_fine"]] if two_models else [])
    sds = DR.make_state_dicts(seed, len(mods))
    from mirror_nerf_amd.dnerf import PARAM_NAMES
    for m, sd, tw in zip(mods, sds, tweaks):
        ref_sd = {k: v.detach().numpy() for k, v in m.state_dict().items()}
        assert list(ref_sd) == PARAM_NAMES == list(sd), "state_dict names / order differ from the reference's"
        for k in ref_sd:
            assert np.array_equal(ref_sd[k], sd[k]), f"seed rebuild mismatch: {k}"
        W.apply_tweaks(sd, tw)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        m.eval()
    return kw, sds


def _double_kwargs(kw):
    kw = dict(kw)
    for k in ("network_fn", "network_fine"):
        if kw.get(k) is not None:
            kw[k] = copy.deepcopy(kw[k]).double()
    return kw


# ------------------------------------------------------------------------------------------------------------ G27-model
def model_case(name="g27_dnerf_model"):
    kw, sds = ref_object(OBJ_SEED, [DR.MODEL_TWEAKS], two_models=False)
    net = kw["network_fn"]
    rs = np.random.RandomState(270)
    xyz = rs.uniform(-1.5, 1.5, (N_POINTS, 3)).astype(np.float32)
    v = rs.normal(size=(N_POINTS, 3))
    v = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    embed_fn, _ = RD.get_embedder(10, 3, 0)
    embeddirs_fn, _ = RD.get_embedder(4, 3, 0)
    embedtime_fn, _ = RD.get_embedder(10, 1, 0)
    out, floor, mine = {}, {}, {}
    for tag, t in (("t037", 0.37), ("t0", 0.0)):
        res = {}
        for dt, mod in ((torch.float32, net), (torch.float64, copy.deepcopy(net).double())):
            x = torch.cat([embed_fn(torch.from_numpy(xyz).to(dt)), embeddirs_fn(torch.from_numpy(v).to(dt))], -1)
            te = embedtime_fn(torch.full((N_POINTS, 1), t, dtype=torch.float32).to(dt))
            with torch.no_grad():
                raw, dx = mod(x, [te, te])
            res[dt] = (raw.numpy(), dx.numpy())
        (raw32, dx32), (raw64, dx64) = res[torch.float32], res[torch.float64]
        out.update({f"raw_{tag}": raw32, f"dx_{tag}": dx32, f"raw64_{tag}": raw64, f"dx64_{tag}": dx64})
        for key, a, b in (("dx", dx32, dx64), ("rgb", raw32[:, :3], raw64[:, :3]), ("alpha", raw32[:, 3], raw64[:, 3])):
            scale = max(1.0, float(np.abs(b).max(initial=0.0)))
            floor[f"{key}_{tag}"] = float(np.abs(a.astype(np.float64) - b).max()) / scale
        # the restatement the tests hold the kernel to reproduces the reference's float64 run
        r64, d64 = DR.field(sds[0], torch.from_numpy(xyz).double(), torch.from_numpy(v).double(), t)
        mine[tag] = (float(np.abs(r64.numpy() - raw64).max()), float(np.abs(d64.numpy() - dx64).max()))
    print(f"  {name}: floor (relative to max(1, |value|)) {{{', '.join(f'{k}: {v:.2e}' for k, v in floor.items())}}}")
    print(f"    |dx| <= {np.abs(out['dx64_t037']).max():.3f}, |alpha| <= {np.abs(out['raw64_t037'][:, 3]).max():.1f}; "
          f"float64 restatement vs reference float64 (raw, dx): {mine}")
    meta = dict(seed=OBJ_SEED, n_models=1, tweaks=DR.MODEL_TWEAKS, checksum=[W.checksum(sds[0])], times=dict(t037=0.37, t0=0.0),
                floor=floor)
    MG.save(name, meta, {"xyz": xyz, "viewdirs": v}, out)


# ------------------------------------------------------------------------------------------------------------ G27-scene
class _Levels(GO._Levels):
    """make_golden_objects._Levels for the d_nerf arm: the object render is called as render_rays_obj(rays, **kwargs) and
    returns rgb_map / depth_map / acc_map."""

    def __enter__(self):
        super().__enter__()

        def obj(rays, **k):
            out = self.orig_obj(rays, **k)
            assert "opacity" not in self.prev and rays.shape[0] == self.prev["index"].shape[0]
            self.prev["opacity"], self.prev["obj_depth"] = out["acc_map"].clone(), out["depth_map"].clone()
            return out
        self.mod.render_rays_obj = obj
        return self


def patched_eval(pose_literal):
    mod = GO.patched_eval(pose_literal)
    mod.render_rays_obj = RD.render_rays
    return mod


def _args(root_dir, max_level):
    args = GO._args(root_dir, max_level)
    args.obj_model_type = "d_nerf"
    return args


def _run(mod, args, mods, kw, frame_time, rays, chunk, double=False):
    models = {"coarse": mods[0], "fine": mods[1]}
    if double:
        models = {k: copy.deepcopy(v).double() for k, v in models.items()}
        kw = _double_kwargs(kw)
    t = torch.from_numpy(rays)
    return MG.to_np(mod.batched_inference(models, MG.EMB, t.double() if double else t, 64, 64, False, chunk, args=args,
                                          trace_secondary_rays=True, render_kwargs_test_d_nerf=kw,
                                          args_d_nerf=types.SimpleNamespace(use_viewdirs=True), frame_time=frame_time))


def obj_tweaks(case):
    two, _white = CASE_OBJECT[case]
    tw = [[["_occ.alpha_linear.weight", "mul", 1000.0], ["_occ.alpha_linear.bias", "set", OBJ_BIAS[case][i]]]
          for i in range(2 if two else 1)]
    return tw


def candidate_rays(case):
    GO.CASE_SEEDS[case], GO.CASE_SHORT[case] = CASE_SEEDS[case], CASE_SHORT[case]
    return GO.candidate_rays(case)


def scene_case(name, tweaks=W.STRADDLE):
    root_dir, max_level, pose_literal, chunk, frame_time = CASE_ARGS[name]
    two, white = CASE_OBJECT[name]
    mod = patched_eval(pose_literal)
    args = _args(root_dir, max_level)
    near = float(args.near)
    scale, translation = GO.PRESETS[root_dir]
    pose_scale0 = float(torch.norm(torch.FloatTensor(pose_literal)[:3, 0]))
    mods, sds = MG.ref_models(0, 2, tweaks)
    kw, obj_sds = ref_object(OBJ_SEED, obj_tweaks(name), two, white)

    cand = candidate_rays(name)
    with _Levels(mod, max_level) as lv:
        _run(mod, args, mods, kw, frame_time, cand, chunk)
    drop = np.zeros(cand.shape[0], bool)
    dropped_per_level = {}
    for level, idx, _t, _b, _u, edge in lv.classes(scale, pose_scale0, near):
        drop[idx[edge]] = True
        dropped_per_level[level] = dropped_per_level.get(level, 0) + int(edge.sum())
    assert drop.mean() <= 0.05, f"{name}: {int(drop.sum())} of {cand.shape[0]} candidates sit on a decision edge"
    rays = cand[~drop]

    with _Levels(mod, max_level) as lv, GA._Recorder(mod) as rec:
        ref = _run(mod, args, mods, kw, frame_time, rays, chunk)
    n = rays.shape[0]
    count, obj_maps = {}, None
    for level, idx, t, b, u, edge in lv.classes(scale, pose_scale0, near):
        assert not edge.any(), f"{name}: a kept ray sits on a decision edge at level {level}"
        c = count.setdefault(level, dict(rays=0, transparent=0, blocked=0, used=0))
        for k, v in (("rays", idx.shape[0]), ("transparent", t.sum()), ("blocked", b.sum()), ("used", u.sum())):
            c[k] += int(v)
    for k in ("transparent", "blocked", "used"):
        assert count[0][k] >= 0.15 * n, f"{name}: {count[0][k]} of {n} rays are {k} at level 0 ({count})"
    assert max_level < 1 or count.get(1, {}).get("used", 0) > 0, f"{name}: no ray uses the object at level 1"

    # the object alone on the level-0 rays in its own frame: what tests/test_dnerf_ref_cpu.py holds the restatement to
    batch = _object_batch(name, rays, frame_time)
    with torch.no_grad():
        alone = {dt: RD.render_rays(batch.to(dt), **(kw if dt == torch.float32 else _double_kwargs(kw))) for dt in (torch.float32, torch.float64)}
    obj_maps = {f"object_{k}{'64' if dt == torch.float64 else ''}": alone[dt][k].numpy()
                for dt in alone for k in ("rgb_map", "depth_map", "acc_map", "disp_map")}

    ft = torch.FloatTensor
    torch.FloatTensor = lambda x: torch.tensor(x, dtype=torch.float64)
    try:
        ref64 = _run(mod, args, mods, kw, frame_time, rays, chunk, double=True)
    finally:
        torch.FloatTensor = ft
    floor = {k: float(np.max(np.abs(ref64[k].astype(np.float64) - ref[k].astype(np.float64)), initial=0.0))
             for k in ref if ref64[k].shape == ref[k].shape}
    floor_frac = {k: MG.off_fraction(ref64[k], ref[k]) for k in ref if ref64[k].shape == ref[k].shape}
    print(f"  {name}: {n} of {cand.shape[0]} candidates kept, per level {count}, render_rays rows {rec.sizes}")
    print("    fp32-vs-fp64 floor:", {k: f"{v:.1e}" for k, v in floor.items() if v > 2e-5})
    print("    fraction off by more than 1e-4:", {k: round(v, 4) for k, v in floor_frac.items() if v > 0})
    args_o = dict(predict_normal=True, only_one_field=False, only_one_field_fine_epoch=2, max_recursive_level=max_level,
                  app_reflect_newly_placed_objects=True, obj_model_type="d_nerf", root_dir=root_dir, near=near)
    meta = dict(seed=0, n_models=2, tweaks=tweaks, checksum=[W.checksum(s) for s in sds], args=args_o, N_samples=64,
                N_importance=64, chunk=chunk, floor=floor, floor_frac=floor_frac, traced_per_level=rec.sizes,
                frame_time=frame_time, obj_seed=OBJ_SEED, obj_tweaks=obj_tweaks(name), obj_checksum=[W.checksum(s) for s in obj_sds],
                obj_config=dict(N_samples=64, N_importance=64, white_bkgd=white, use_two_models_for_fine=two, lindisp=False),
                new_object=dict(pose_align=pose_literal, scale=scale, translation=list(translation)),
                conditions=dict(candidates=int(cand.shape[0]), dropped=int(drop.sum()),
                                dropped_per_level={str(k): v for k, v in dropped_per_level.items()}, margin=MARGIN,
                                per_level={str(k): v for k, v in count.items()}))
    MG.save(name, meta, {"rays": rays, "object_batch": batch.numpy()}, dict(ref, **obj_maps), keep_per_sample=False)
    return ref


def _object_batch(case, rays, frame_time):
    """Rays of a case as the branch hands them to the object's render_rays (eval.py:192-247, restated for the calibration and
    for the object-only capture): moved into the object's frame, the time in column 8, the unit directions behind it."""
    root_dir, _level, pose, _chunk, _t = CASE_ARGS[case]
    r = torch.from_numpy(rays)
    scale, translation = GO.PRESETS[root_dir]
    m = torch.tensor(pose)[:3]
    o = r[:, :3] @ m[:, :3].T + m[:, 3]
    d = r[:, 3:6] @ m[:, :3].T
    d = d / d.norm(dim=1, keepdim=True)
    return torch.cat([o * scale + torch.tensor(translation), d, r[:, 6:8], torch.full_like(r[:, :1], frame_time),
                      d / torch.norm(d, dim=-1, keepdim=True)], 1)


def calibrate():
    """The alpha_linear.bias literals of OBJ_BIAS, per case.  Coarse (or only) model: 5 - 1000 x the median raw density (without
    the head's bias, which the tweak replaces) over the coarse sample points of the case's candidate rays in the object's
    frame at the case's time.  A two-model case's fine model -- and the single model itself, whose one bias serves both passes
    -- by bisection: the literal, to two decimals, at which the set share of the case's short rays is opaque (acc_map > 0.8)
    in the reference's render of the object alone; the opaque share grows with the bias."""
    for case in CASES:
        two, white = CASE_OBJECT[case]
        frame_time = CASE_ARGS[case][4]
        batch = _object_batch(case, candidate_rays(case), frame_time)
        step, share = CASE_SHORT[case][2], CASE_SHORT[case][3]
        short = batch[1::step]

        def kwargs(biases):
            tw = [[["_occ.alpha_linear.weight", "mul", 1000.0]] + ([["_occ.alpha_linear.bias", "set", b]] if b is not None else [])
                  for b in biases]
            return ref_object(OBJ_SEED, tw, two, white)[0]
        kw = kwargs([None] * (2 if two else 1))
        with torch.no_grad():
            z = batch[:, 6:7] * (1 - torch.linspace(0, 1, 64)) + batch[:, 7:8] * torch.linspace(0, 1, 64)
            pts = batch[:, None, :3] + batch[:, None, 3:6] * z[..., None]
            raw, _ = kw["network_query_fn"](pts, batch[:, 9:12], batch[:, 8:9], kw["network_fn"])
            raw = raw[..., 3] - kw["network_fn"]._occ.alpha_linear.bias
        coarse = round(5.0 - float(raw.median()), 2)
        print(f"  {case}: raw density median {float(raw.median()):.4f}, std {float(raw.std()):.4f} -> coarse bias {coarse}")

        def opaque_share(bias):
            k = kwargs([coarse, bias] if two else [bias])
            with torch.no_grad():
                r = RD.render_rays(short, **k)
            return float((r["acc_map"] > 0.8).float().mean())
        lo, hi = -200.0, 200.0
        for _ in range(18):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if opaque_share(mid) < share else (lo, mid)
        print(f"    {'fine' if two else 'single'} bias {round(hi, 2)} (opaque share of the short rays {opaque_share(round(hi, 2)):.3f})")


CASE_SEEDS = {"g27_dnerf_office_l2": 310, "g27_dnerf_office_canonical_l2": 310, "g27_dnerf_single_posed_l1": 312}
# as make_golden_objects.CASE_SHORT: (far of the short rays, origin spread, every n-th ray is short, opaque share aimed at)
CASE_SHORT = {"g27_dnerf_office_l2": (0.25, 0.0, 2, 0.5), "g27_dnerf_office_canonical_l2": (0.25, 0.0, 2, 0.5),
              "g27_dnerf_single_posed_l1": (0.25, 0.0, 2, 0.5)}
# name -> (root_dir, max_recursive_level, pose literal, chunk, frame_time)
CASE_ARGS = {
    # a two-model object in motion under the office preset, two levels below the primary one
    "g27_dnerf_office_l2": ("data/office", 2, GO.IDENTITY, 32768, 0.37),
    # the same object at the canonical time: the deformation net is not evaluated
    "g27_dnerf_office_canonical_l2": ("data/office", 2, GO.IDENTITY, 32768, 0.0),
    # one model for both passes (use_two_models_for_fine = False), a similarity as the pose, white background of the object
    "g27_dnerf_single_posed_l1": ("data/washroom", 1, GO.SIMILARITY, 32768, 0.37),
}
# name -> (use_two_models_for_fine, white_bkgd of the object)
CASE_OBJECT = {"g27_dnerf_office_l2": (True, False), "g27_dnerf_office_canonical_l2": (True, False),
               "g27_dnerf_single_posed_l1": (False, True)}
# alpha_linear.bias per model, from --calibrate
# (the canonical case renders the office case's networks; with that case's literals the undeformed field leaves only 12 % of the
# rays transparent, so it carries its own)
OBJ_BIAS = {"g27_dnerf_office_l2": [7.06, -5.08], "g27_dnerf_office_canonical_l2": [7.55, -8.74], "g27_dnerf_single_posed_l1": [-12.18]}
CASES = {name: scene_case for name in CASE_ARGS}


def main():
    if sys.argv[1:] == ["--calibrate"]:
        return calibrate()
    want = sys.argv[1:] or ["g27_dnerf_model"] + list(CASES)
    torch.manual_seed(0)
    for name in want:
        (model_case if name == "g27_dnerf_model" else CASES[name])(name)


if __name__ == "__main__":
    main()
