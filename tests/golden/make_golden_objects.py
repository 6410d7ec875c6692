#!/usr/bin/env python3
"""Fixtures G26: the reference's new-object branch of `eval.batched_inference` (app_reflect_newly_placed_objects,
eval.py:173-291) with a nerf_pl object (models/nerf_pl/nerf_nerfpl.py, rendered by models/nerf_pl/rendering_nerfpl.py),
captured from the reference itself.

Build-container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_objects.py [name ...]
                       PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_objects.py --calibrate

The reference cannot run the branch as it stands: `pose_align` is hard-coded to None (eval.py:177), so `pose_scale`
(eval.py:264) is never bound.  With `pose_align` set to a matrix the branch runs as written.  So the reference's eval.py is
read at run time, the single occurrence of `pose_align = None` is replaced by a matrix literal, and the result is executed as
a fresh module whose `dataset` and `render_rays_obj` are set as eval.py's `__main__` block sets them.  No text of the reference
is kept here.  Two cases use the 4x4 identity as the literal (the tests pass the same identity as `new_object=`, so both sides
perform the same operations); one uses a similarity -- a rotation about z, a uniform scale of 1.25, a translation -- which
exercises the rotation and `pose_scale[0]`.

The object: the reference's nerf_pl `NeRF` pair under seed OBJ_SEED, which weights.make_state_dict(OBJ_SEED, 2,
predict_normal=False, predict_mirror_mask=False) rebuilds bit for bit (checked here).  A random-init field is nearly constant
in space (its raw sigma has a standard deviation of ~0.004), so both models get sigma.weight x 1000 and a sigma.bias literal
found by `--calibrate` (see calibrate()): for the coarse model 5 - 1000 x its median raw sigma -- the density head without its
bias, which the tweak replaces -- over the coarse sample points of the office case's object rays; for the fine model, per
case, the value at which a set share of the case's short rays is opaque.  One common fine literal does not serve: the field is
smooth, the rays of a case cross a small region of it, and which classes exist there turns on a change of 1 in that literal.
The literals are stored per model in meta.obj_tweaks, with the rebuild checksums in meta.obj_checksum.

Rays: make_golden.pick_rays(256, seed) with far = 0.25 on every second ray (CASE_SHORT; the default-preset case: on every ray,
with the origins spread along the rays).  Full-length rays through this object are always opaque (the last sample of a ray
takes what is left wherever the density is positive there); the short ones are what makes it semi-transparent.  A candidate
ray is dropped when at ANY recursion level the object's opacity is within MARGIN of 0.8, or the object is opaque there and its
scaled depth is within MARGIN of the scene's: such a ray changes class under any perturbation of 1e-4.  At most 5 % of the
candidates may go.  Every case asserts, and stores in meta.conditions: at level 0 each of transparent / blocked by the scene /
used holds at least 15 % of the rays, and at level 1 some rays use the object (it is seen in the mirrors).
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
import torch  # noqa: E402

W, R = MG.W, MG.R

OBJ_SEED = 7
MARGIN = 1e-3
IDENTITY = [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]]
# rotation about z by 0.3 rad x 1.25, translation (0.1, -0.2, 0.05)
SIMILARITY = [[1.194171, -0.369400, 0.0, 0.1], [0.369400, 1.194171, 0.0, -0.2], [0.0, 0.0, 1.25, 0.05], [0.0, 0.0, 0.0, 1.0]]
# the object presets of the reference (eval.py:177-190), restated for meta.new_object only (what the tests pass as the
# override, so that they can add the pose); the expected values come from the reference's own branch code
PRESETS = {"data/office": (2.0, (0.0, 3.0, 0.5)), "data/washroom": (2.0, (-0.5, -0.5, 0.0)), "data/synthetic": (1.0, (0.0, 0.0, 0.0))}
# density tweaks of the object, per model: sigma.bias from --calibrate (the fine model's per case)
OBJ_COARSE_BIAS = 6.18
OBJ_FINE_BIAS = {"g26_object_office_l2": 44.94, "g26_object_default_chunk96": 36.57, "g26_object_posed_l1": 50.44}


def obj_tweaks(case):
    return [[["sigma.weight", "mul", 1000.0], ["sigma.bias", "set", OBJ_COARSE_BIAS]],
            [["sigma.weight", "mul", 1000.0], ["sigma.bias", "set", OBJ_FINE_BIAS[case]]]]


def patched_eval(pose_literal):
    """The reference's eval.py as a fresh module, with `pose_align = None` (eval.py:177) replaced by the literal."""
    import eval as _plain  # noqa: F401  (the stubs of _ref_import make its imports resolve; also proves the plain file imports)
    path = os.path.join(R.REF_ROOT, "eval.py")
    with open(path) as f:
        text = f.read()
    phrase = "pose_align = None"
    assert text.count(phrase) == 1, f"eval.py holds {text.count(phrase)} occurrences of {phrase!r}"
    text = text.replace(phrase, "pose_align = " + repr(pose_literal))
    mod = types.ModuleType("ref_eval_objects")
    mod.__file__ = path
    exec(compile(text, path, "exec"), mod.__dict__)
    from models.nerf_pl.rendering_nerfpl import render_rays as render_rays_obj
    mod.dataset = types.SimpleNamespace(white_back=False)
    mod.render_rays_obj = render_rays_obj
    return mod


def object_models(tweaks):
    """The reference's nerf_pl NeRF pair under OBJ_SEED with per-model tweaks; checks that tests/golden/weights.py rebuilds them."""
    from models.nerf_pl.nerf_nerfpl import NeRF
    torch.manual_seed(OBJ_SEED)
    mods = [NeRF() for _ in range(2)]
    sds = W.make_state_dict(OBJ_SEED, 2, predict_normal=False, predict_mirror_mask=False)
    for m, sd, tw in zip(mods, sds, tweaks):
        ref_sd = {k: v.detach().numpy() for k, v in m.state_dict().items()}
        assert list(ref_sd) == list(sd), "nerf_pl state_dict names differ from the plain MirrorNeRF's"
        for k in ref_sd:
            assert np.array_equal(ref_sd[k], sd[k]), f"seed rebuild mismatch: {k}"
        W.apply_tweaks(sd, tw)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        m.eval()
    return mods, sds


def object_system(mods):
    from models.nerf_pl.nerf_nerfpl import Embedding
    return types.SimpleNamespace(models=list(mods), embeddings=[Embedding(3, 10), Embedding(3, 4)])


def candidate_rays(case):
    rays = MG.pick_rays(256, CASE_SEEDS[case]).copy()
    far, spread, step, _share = CASE_SHORT[case]
    rays[1::step, 7] = far
    if spread:      # the short rays start up to `spread` further along their line (as reflected rays start anywhere)
        t = np.random.RandomState(CASE_SEEDS[case] + 1000).uniform(0.0, spread, rays[1::step].shape[0]).astype(np.float32)
        rays[1::step, :3] += rays[1::step, 3:6] * t[:, None]
    return rays


class _Levels:
    """Wraps the two render calls of the patched module and keeps, per call pair (one recursion level of one chunk): the
    indices of its rows in the fixture's ray set, the scene's depth before the branch edits it, and the object's opacity
    and depth.  The level of a call follows from the previous level's mirror mask, which the reference thresholds in place
    (eval.py:303-306) after the branch has cleared it (eval.py:291): level 0 traces every ray (eval.py:159), the deeper
    levels the rays of the mask."""

    def __init__(self, mod, max_level):
        self.mod, self.max_level = mod, max_level
        self.levels, self.prev, self.offset = [], None, 0
        self.orig, self.orig_obj = mod.render_rays, mod.render_rays_obj

    def __enter__(self):
        def scene(models, embeddings, rays, *a, **k):
            out = self.orig(models, embeddings, rays, *a, **k)
            n = int(rays.shape[0])
            p = self.prev
            if p is not None and p["level"] < self.max_level and bool((p["mask"] != 0).any()):
                idx = p["index"] if p["level"] == 0 else p["index"][(p["mask"] != 0).numpy()]
                level = p["level"] + 1
            else:
                idx, level = np.arange(self.offset, self.offset + n), 0
                self.offset += n
            assert idx.shape[0] == n, (idx.shape, n, level)
            self.prev = dict(level=level, index=idx, mask=out["mirror_mask_fine"], depth=out["depth_fine"].clone())
            self.levels.append(self.prev)
            return out

        def obj(models, embeddings, rays, *a, **k):
            out = self.orig_obj(models, embeddings, rays, *a, **k)
            assert "opacity" not in self.prev and rays.shape[0] == self.prev["index"].shape[0]
            self.prev["opacity"], self.prev["obj_depth"] = out["opacity_fine"].clone(), out["depth_fine"].clone()
            return out
        self.mod.render_rays, self.mod.render_rays_obj = scene, obj
        return self

    def __exit__(self, *exc):
        self.mod.render_rays, self.mod.render_rays_obj = self.orig, self.orig_obj

    def classes(self, scale, pose_scale0, near):
        """Per level: (index, transparent, blocked, used, on_edge) as eval.py:261-284 decides them."""
        out = []
        for lv in self.levels:
            d = (lv["obj_depth"] / scale / pose_scale0).numpy()
            o, s = lv["opacity"].numpy(), lv["depth"].numpy()
            is_obj = (d > 0) & (o > 0.8)
            blocked = (d > s) & (s > near)
            edge = (np.abs(o.astype(np.float64) - 0.8) < MARGIN) | (is_obj & (np.abs(d.astype(np.float64) - s) < MARGIN))
            out.append((lv["level"], lv["index"], ~is_obj, is_obj & blocked, is_obj & ~blocked, edge))
        return out


def _args(root_dir, max_level):
    hp = R.get_hparams()
    args = types.SimpleNamespace(**vars(hp))
    for k, v in dict(predict_normal=True, predict_mirror_mask=True, only_one_field=False, max_recursive_level=max_level,
                     app_control_mirror_roughness=False, app_reflection_substitution=False, app_place_new_mirror=False,
                     app_reflect_newly_placed_objects=True, obj_model_type="nerf_pl", root_dir=root_dir).items():
        setattr(args, k, v)
    return args


def _run(mod, args, mods, obj_mods, rays, chunk, double=False):
    models = {"coarse": mods[0], "fine": mods[1]}
    if double:
        models = {k: copy.deepcopy(v).double() for k, v in models.items()}
        obj_mods = [copy.deepcopy(m).double() for m in obj_mods]
    t = torch.from_numpy(rays)
    return MG.to_np(mod.batched_inference(models, MG.EMB, t.double() if double else t, 64, 64, False, chunk, args=args,
                                          trace_secondary_rays=True, system_obj=object_system(obj_mods)))


def object_case(name, tweaks=W.STRADDLE):
    root_dir, max_level, pose_literal, chunk = CASE_ARGS[name]
    mod = patched_eval(pose_literal)
    args = _args(root_dir, max_level)
    near = float(args.near)
    scale, translation = PRESETS[root_dir]
    pose_scale0 = float(torch.norm(torch.FloatTensor(pose_literal)[:3, 0]))
    mods, sds = MG.ref_models(0, 2, tweaks)
    obj_mods, obj_sds = object_models(obj_tweaks(name))

    # candidates -> kept rays: drop what sits on a decision edge at any level (per ray the result does not depend on the others)
    cand = candidate_rays(name)
    with _Levels(mod, max_level) as lv:
        _run(mod, args, mods, obj_mods, cand, chunk)
    drop = np.zeros(cand.shape[0], bool)
    dropped_per_level = {}
    for level, idx, _t, _b, _u, edge in lv.classes(scale, pose_scale0, near):
        drop[idx[edge]] = True
        dropped_per_level[level] = dropped_per_level.get(level, 0) + int(edge.sum())
    assert drop.mean() <= 0.05, f"{name}: {int(drop.sum())} of {cand.shape[0]} candidates sit on a decision edge"
    rays = cand[~drop]

    with _Levels(mod, max_level) as lv, GA._Recorder(mod) as rec:
        ref = _run(mod, args, mods, obj_mods, rays, chunk)
    n = rays.shape[0]
    count = {}
    for level, idx, t, b, u, edge in lv.classes(scale, pose_scale0, near):
        assert not edge.any(), f"{name}: a kept ray sits on a decision edge at level {level}"
        c = count.setdefault(level, dict(rays=0, transparent=0, blocked=0, used=0))
        for k, v in (("rays", idx.shape[0]), ("transparent", t.sum()), ("blocked", b.sum()), ("used", u.sum())):
            c[k] += int(v)
    for k in ("transparent", "blocked", "used"):
        assert count[0][k] >= 0.15 * n, f"{name}: {count[0][k]} of {n} rays are {k} at level 0"
    assert max_level < 1 or count.get(1, {}).get("used", 0) > 0, f"{name}: no ray uses the object at level 1"

    # the reference's own noise: the same call in float64 (the branch's FloatTensor constants, eval.py:193-217, made float64)
    ft = torch.FloatTensor
    torch.FloatTensor = lambda x: torch.tensor(x, dtype=torch.float64)
    try:
        ref64 = _run(mod, args, mods, obj_mods, rays, chunk, double=True)
    finally:
        torch.FloatTensor = ft
    floor = {k: float(np.max(np.abs(ref64[k].astype(np.float64) - ref[k].astype(np.float64)), initial=0.0))
             for k in ref if ref64[k].shape == ref[k].shape}
    floor_frac = {k: MG.off_fraction(ref64[k], ref[k]) for k in ref if ref64[k].shape == ref[k].shape}
    print(f"  {name}: {n} of {cand.shape[0]} candidates kept, per level {count}, render_rays rows {rec.sizes}")
    print("    fp32-vs-fp64 floor:", {k: f"{v:.1e}" for k, v in floor.items() if v > 2e-5})
    print("    fraction off by more than 1e-4:", {k: round(v, 4) for k, v in floor_frac.items() if v > 0})
    args_o = dict(predict_normal=True, only_one_field=False, only_one_field_fine_epoch=2, max_recursive_level=max_level,
                  app_reflect_newly_placed_objects=True, obj_model_type="nerf_pl", root_dir=root_dir, near=near)
    meta = dict(seed=0, n_models=2, tweaks=tweaks, checksum=[W.checksum(s) for s in sds], args=args_o, N_samples=64,
                N_importance=64, chunk=chunk, floor=floor, floor_frac=floor_frac, traced_per_level=rec.sizes,
                obj_seed=OBJ_SEED, obj_tweaks=obj_tweaks(name), obj_checksum=[W.checksum(s) for s in obj_sds],
                new_object=dict(pose_align=pose_literal, scale=scale, translation=list(translation)),
                conditions=dict(candidates=int(cand.shape[0]), dropped=int(drop.sum()),
                                dropped_per_level={str(k): v for k, v in dropped_per_level.items()}, margin=MARGIN,
                                per_level={str(k): v for k, v in count.items()}))
    MG.save(name, meta, {"rays": rays}, ref, keep_per_sample=False)
    return ref


def _object_rays(case):
    """The candidate rays of a case in its object's frame (eval.py:192-217, restated for the calibration only)."""
    root_dir, _level, pose, _chunk = CASE_ARGS[case]
    rays = torch.from_numpy(candidate_rays(case))
    scale, translation = PRESETS[root_dir]
    m = torch.tensor(pose)[:3]
    o = rays[:, :3] @ m[:, :3].T + m[:, 3]
    d = rays[:, 3:6] @ m[:, :3].T
    return torch.cat([o * scale + torch.tensor(translation), d / d.norm(dim=1, keepdim=True), rays[:, 6:]], 1)


def calibrate():
    """The sigma.bias literals of OBJ_TWEAKS.  Coarse model: 5 - 1000 x the median raw sigma (without the head's bias) over
    the coarse sample points (64 per ray, near .. far) of the office case's candidate rays in the object's frame.  Fine model,
    per case (the field is smooth, so the rays of a case see nearly one density and a common literal leaves some case without
    a class): the literal, to two decimals, at which half of the case's short rays are opaque (opacity_fine > 0.8) in the
    reference's nerf_pl render of the object alone -- found by bisection, the opaque share grows with the bias."""
    from models.nerf_pl.nerf_nerfpl import Embedding
    from models.nerf_pl.rendering_nerfpl import render_rays as render_rays_obj
    mods, _ = object_models([[], []])
    rays = _object_rays("g26_object_office_l2")
    z = rays[:, 6:7] * (1 - torch.linspace(0, 1, 64)) + rays[:, 7:8] * torch.linspace(0, 1, 64)
    xyz = (rays[:, None, :3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3)
    x = torch.cat([Embedding(3, 10)(xyz), Embedding(3, 4)(rays[:, 3:6]).repeat_interleave(64, 0)], 1)
    with torch.no_grad():
        raw = mods[0](x)[:, 3] - mods[0].sigma.bias      # the tweak SETS the bias: what x 1000 scales is the head without it
    coarse = round(5.0 - 1000.0 * float(raw.median()), 2)
    print(f"  coarse: raw sigma median {float(raw.median()):.6f}, std {float(raw.std()):.6f} -> sigma.bias {coarse}")
    for case in CASES:
        short = _object_rays(case)[1::CASE_SHORT[case][2]]

        def opaque_share(bias):
            mods, _ = object_models([[["sigma.weight", "mul", 1000.0], ["sigma.bias", "set", coarse]],
                                     [["sigma.weight", "mul", 1000.0], ["sigma.bias", "set", bias]]])
            with torch.no_grad():
                r = render_rays_obj(object_system(mods).models, object_system(mods).embeddings, short, 64, False, 0, 0, 64, 32768, False)
            return float((r["opacity_fine"] > 0.8).float().mean())
        lo, hi = 0.0, 120.0
        for _ in range(16):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if opaque_share(mid) < CASE_SHORT[case][3] else (lo, mid)
        print(f"  {case}: fine sigma.bias {round(hi, 2)} (opaque share of the short rays {opaque_share(round(hi, 2)):.3f})")


CASE_SEEDS = {"g26_object_office_l2": 300, "g26_object_default_chunk96": 301, "g26_object_posed_l1": 302}
# every second ray is short: (its far, how far along its line its origin may move).  Under the default preset the object's
# frame is the scene's (scale 1): the short rays of one camera then cross a region so small that the smooth object field is
# one density to all of them and a class stays empty, so their origins are spread along the rays
CASE_SHORT = {"g26_object_office_l2": (0.25, 0.0, 2, 0.5), "g26_object_default_chunk96": (0.25, 6.0, 1, 0.8),
              "g26_object_posed_l1": (0.25, 0.0, 2, 0.5)}
# name -> (root_dir, max_recursive_level, pose literal, chunk)
CASE_ARGS = {
    # office preset (scale 2, translation (0, 3, 0.5)), identity pose, two levels below the primary one
    "g26_object_office_l2": ("data/office", 2, IDENTITY, 32768),
    # default preset, several chunks (chunk < N): the pipelined level 0
    "g26_object_default_chunk96": ("data/synthetic", 1, IDENTITY, 96),
    # a similarity as the pose: rotation, pose translation between rotation and scale, pose_scale[0] in the depth
    "g26_object_posed_l1": ("data/washroom", 1, SIMILARITY, 32768),
}
CASES = {name: object_case for name in CASE_ARGS}


def main():
    if sys.argv[1:] == ["--calibrate"]:
        return calibrate()
    want = sys.argv[1:] or list(CASES)
    torch.manual_seed(0)
    for name in want:
        CASES[name](name)


if __name__ == "__main__":
    main()
