#!/usr/bin/env python3
"""Fixtures G19: the two scene-editing applications of the reference's `eval.batched_inference` that need only MirrorNeRF
fields -- a new planar mirror (app_place_new_mirror, eval.py:311-320, 364-504) and reflection substitution
(app_reflection_substitution, eval.py:550-613) -- captured from the reference itself.

Build-container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_apps.py [name ...]
Every fixture also records the reference's own fp32-vs-fp64 difference (meta.floor, meta.floor_frac, as make_golden.eval_case),
the rays rendered per recursion level (meta.traced_per_level: the sizes of the reference's render_rays calls, in call order
per chunk) and how many rays of each kind of the place-mirror ray set it holds (meta.ray_kinds).

Ray sets of the place-mirror cases, built around the preset's rectangle (the synthetic scene's depth is ~0.22 everywhere
under W.STRADDLE, so an intersection closer than that is in front of the foreground):
  hit       -- ahead of the origin, inside the rectangle, 0.02 .. 0.18 away: unoccluded
  occluded  -- the same, 0.4 .. 2 away: behind the foreground
  behind    -- the intersection lies behind the origin
  parallel  -- direction exactly parallel to the plane; half of them start IN the plane (t = 0/0: NaN coordinates, which the
               reference's rectangle test counts as inside), half off it (t = inf: outside)
  miss      -- ahead and unoccluded, but outside the rectangle
  camera    -- rays of the synthetic camera: ~40 % of them are scene mirrors (W.STRADDLE)
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
import torch  # noqa: E402

W, R = MG.W, MG.R

# the planes of the reference's presets (eval.py:369-433), restated for the ray sets only; the fixtures' expected values come
# from the reference's own branch code
PLANES = {
    ("plane_x", "default"): (0, -1.0, (-1.0, 1.0, -0.5, 0.5)),
    ("plane_x", "office"): (0, 1.0, (-1.0, 1.0, -1.0, 0.75)),
    ("plane_y", "livingroom"): (1, 1.65, (-0.3, 1.5, -0.5, 1.0)),
}
KINDS = ("hit", "occluded", "behind", "parallel", "miss")


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def plane_rays(axis, pos, rect, n_each, seed):
    """(rays (M,8) fp32, kinds (M,) str) around the plane `axis` = pos with rectangle rect on the other two axes."""
    rs = np.random.RandomState(seed)
    b = 1 - axis
    out, kinds = [], []

    def on_plane(n, outside=False):
        x = np.zeros((n, 3))
        x[:, axis] = pos
        if outside:      # beyond one of the four edges by 0.1 .. 0.5
            u = rs.uniform(rect[0] + 0.05, rect[1] - 0.05, n)
            w = rs.uniform(rect[2] + 0.05, rect[3] - 0.05, n)
            side = rs.randint(0, 4, n)
            off = rs.uniform(0.1, 0.5, n)
            u = np.where(side == 0, rect[0] - off, np.where(side == 1, rect[1] + off, u))
            w = np.where(side == 2, rect[2] - off, np.where(side == 3, rect[3] + off, w))
        else:
            u = rs.uniform(rect[0] + 0.05, rect[1] - 0.05, n)
            w = rs.uniform(rect[2] + 0.05, rect[3] - 0.05, n)
        x[:, b], x[:, 2] = u, w
        return x

    def towards(n):
        d = rs.normal(size=(n, 3))
        d[:, axis] = np.sign(rs.uniform(-1, 1, n)) * rs.uniform(0.6, 1.5, n)
        return _unit(d)

    for kind in KINDS:
        n = n_each
        if kind == "parallel":
            o = on_plane(n)
            o[n // 2:, axis] += rs.uniform(0.05, 0.5, n - n // 2) * np.sign(rs.uniform(-1, 1, n - n // 2))
            d = rs.normal(size=(n, 3))
            d[:, axis] = 0.0
            d = _unit(d)
            d[:, axis] = 0.0
            o32 = o.astype(np.float32)
            o32[: n // 2, axis] = np.float32(pos)            # exactly in the plane
        else:
            x = on_plane(n, outside=(kind == "miss"))
            d = towards(n)
            t = rs.uniform(0.4, 2.0, n) if kind == "occluded" else rs.uniform(0.02, 0.18, n)
            o = x - t[:, None] * d if kind != "behind" else x + rs.uniform(0.05, 1.0, n)[:, None] * d
            o32 = o.astype(np.float32)
        r = np.zeros((n, 8), np.float32)
        r[:, :3] = o32
        r[:, 3:6] = d.astype(np.float32)
        r[:, 6], r[:, 7] = 0.05, 8.0       # synthetic camera near / far (run.sh:14-15)
        out.append(r)
        kinds += [kind] * n
    return np.concatenate(out, 0), np.array(kinds)


class _Recorder:
    """Wraps the reference's render_rays (the name eval.py calls) to log the rows of every call: rays rendered per level."""

    def __init__(self, ref_eval):
        self.ref_eval, self.sizes, self.orig = ref_eval, [], ref_eval.render_rays

    def __enter__(self):
        def wrapped(models, embeddings, rays, *a, **k):
            self.sizes.append(int(rays.shape[0]))
            return self.orig(models, embeddings, rays, *a, **k)
        self.ref_eval.render_rays = wrapped
        return self

    def __exit__(self, *exc):
        self.ref_eval.render_rays = self.orig


def _system(mods):
    return types.SimpleNamespace(models={"coarse": mods[0], "fine": mods[1]}, embeddings=MG.EMB)


def app_case(name, rays, max_level, root_dir, place=False, plane_pos="plane_x", subst=False, chunk=32768, kinds=None,
             sub_seed=1, tweaks=W.STRADDLE):
    import eval as ref_eval

    ref_eval.dataset = types.SimpleNamespace(white_back=False)
    hp = R.get_hparams()
    args = types.SimpleNamespace(**vars(hp))
    args.predict_normal = True
    args.predict_mirror_mask = True
    args.only_one_field = False
    args.max_recursive_level = max_level
    args.app_control_mirror_roughness = False
    args.app_reflection_substitution = subst
    args.app_place_new_mirror = place
    args.app_reflect_newly_placed_objects = False
    args.plane_pos = plane_pos
    args.root_dir = root_dir
    mods, sds = MG.ref_models(0, 2, tweaks)
    sub_mods, sub_sds = MG.ref_models(sub_seed, 2, tweaks) if subst else (None, None)
    kw = dict(args=args, trace_secondary_rays=True)
    if subst:
        kw["system_substitution"] = _system(sub_mods)
    with _Recorder(ref_eval) as rec:
        ref = MG.to_np(ref_eval.batched_inference({"coarse": mods[0], "fine": mods[1]}, MG.EMB, torch.from_numpy(rays), 64, 64,
                                                  False, chunk, **kw))
    # the reference's own noise: the same call in float64 (the substitution's FloatTensor constants, eval.py:557-594, made
    # float64 for it: a float64 ray times a float32 matrix does not multiply)
    m64 = {k: copy.deepcopy(v).double() for k, v in (("coarse", mods[0]), ("fine", mods[1]))}
    kw64 = dict(kw)
    if subst:
        kw64["system_substitution"] = _system([copy.deepcopy(m).double() for m in sub_mods])
    ft = torch.FloatTensor
    torch.FloatTensor = lambda x: torch.tensor(x, dtype=torch.float64)
    try:
        ref64 = MG.to_np(ref_eval.batched_inference(m64, MG.EMB, torch.from_numpy(rays).double(), 64, 64, False, chunk, **kw64))
    finally:
        torch.FloatTensor = ft
    floor = {k: float(np.max(np.abs(ref64[k].astype(np.float64) - ref[k].astype(np.float64)), initial=0.0))
             for k in ref if ref64[k].shape == ref[k].shape}
    floor_frac = {k: MG.off_fraction(ref64[k], ref[k]) for k in ref if ref64[k].shape == ref[k].shape}
    mm = ref["mirror_mask_fine"]
    print(f"  {name}: mask dtype {mm.dtype}, mirror rays {int((mm != 0).sum())}/{rays.shape[0]}, render_rays rows {rec.sizes}")
    print("    fp32-vs-fp64 floor:", {k: f"{v:.1e}" for k, v in floor.items() if v > 2e-5})
    print("    fraction off by more than 1e-4:", {k: round(v, 4) for k, v in floor_frac.items() if v > 0})
    args_o = dict(predict_normal=True, only_one_field=False, only_one_field_fine_epoch=2, max_recursive_level=max_level,
                  app_place_new_mirror=place, app_reflection_substitution=subst, plane_pos=plane_pos, root_dir=root_dir,
                  near=float(args.near))
    meta = dict(seed=0, n_models=2, tweaks=tweaks, checksum=[W.checksum(s) for s in sds], args=args_o, N_samples=64,
                N_importance=64, chunk=chunk, floor=floor, floor_frac=floor_frac, traced_per_level=rec.sizes)
    if subst:
        meta["sub_seed"] = sub_seed
        meta["sub_checksum"] = [W.checksum(s) for s in sub_sds]
    if kinds is not None:
        meta["ray_kinds"] = {k: int((kinds == k).sum()) for k in KINDS + ("camera",)}
        if place and max_level > 0:
            meta["ray_kinds_in_mirror"] = {k: int((mm[kinds == k]).sum()) for k in KINDS + ("camera",)}
            print("    rays per kind in the merged mirror mask:", meta["ray_kinds_in_mirror"], "of", meta["ray_kinds"])
    MG.save(name, meta, {"rays": rays}, ref, keep_per_sample=False)
    return ref


def mixed_rays(key, n_each, n_camera, seed):
    axis, pos, rect = PLANES[key]
    pr, kinds = plane_rays(axis, pos, rect, n_each, seed)
    cam = MG.pick_rays(n_camera, seed + 100)
    return np.concatenate([pr, cam], 0), np.concatenate([kinds, np.array(["camera"] * n_camera)])


def _place(name, key, n_each, n_camera, seed, max_level, root_dir, **kw):
    rays, kinds = mixed_rays(key, n_each, n_camera, seed)
    return app_case(name, rays, max_level, root_dir, place=True, plane_pos=key[0], kinds=kinds, **kw)


CASES = {
    # the default plane_x preset, three levels below the primary one
    "g19_place_x_default_l3": lambda n: _place(n, ("plane_x", "default"), 24, 64, 190, 3, "data/synthetic"),
    # plane_y livingroom: position and rectangle assigned twice in the reference, the last assignment counts
    "g19_place_y_livingroom": lambda n: _place(n, ("plane_y", "livingroom"), 24, 64, 191, 2, "data/livingroom"),
    # office plane_x, deep: new-mirror hits reflected into scene mirrors and on
    "g19_place_x_office_deep": lambda n: _place(n, ("plane_x", "office"), 24, 64, 192, 5, "data/office"),
    # several chunks (chunk < N): the pipelined level 0
    "g19_place_x_default_chunk96": lambda n: _place(n, ("plane_x", "default"), 32, 160, 193, 2, "data/synthetic", chunk=96),
    # substitution, second weight seed: office (translation) and market (rotation, directions re-normalised)
    "g19_subst_office": lambda n: app_case(n, MG.pick_rays(160, 194), 1, "data/office", subst=True),
    "g19_subst_market": lambda n: app_case(n, MG.pick_rays(160, 195), 1, "data/market", subst=True),
    # both applications in one call
    "g19_place_subst_office": lambda n: _place(n, ("plane_x", "office"), 24, 64, 196, 2, "data/office", subst=True),
}


def main():
    want = sys.argv[1:] or list(CASES)
    torch.manual_seed(0)
    for name in want:
        CASES[name](name)


if __name__ == "__main__":
    main()
