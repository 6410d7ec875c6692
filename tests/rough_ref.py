"""numpy restatements for mirror roughness on partly mirrored chunks (include/mnrf.h "Mirror roughness").

reflect_jitter_fan_ref / jitter_mean_ref repeat the two kernels of csrc/mnrf_rough.hip one fp32 operation at a time, in their
order: the GPU tests compare bit for bit.  render_eval_rough is THE RULE as a recursion over the oracle's own render_rays,
reflect and l2_normalize: where every ray of a chunk is a mirror ray it is oracle.render_eval (tests/test_rough_ref_cpu.py holds
it to that bit for bit), and it also runs where the oracle, like the reference, cannot add (M,3) to (N,3)."""
import numpy as np

from oracle import mirror_nerf_oracle as O

F32 = np.float32
EPS32 = F32(np.finfo(np.float32).eps)
MEAN_NONE, MEAN_DIVIDE, MEAN_MULTIPLY = 0, 1, 2      # MNRF_MEAN_*
# The finish torch performs on the device for `tensor / (times + 1)`: a multiplication by the fp32 reciprocal (found by
# tests/test_hip_rough_kernels.py::test_finish_is_torchs_own_division); numpy, like torch on the CPU, divides.
DEVICE_FINISH = MEAN_MULTIPLY


def finish_value(times, mode=DEVICE_FINISH):
    """The one float the kernel needs: times + 1 for the division, its fp32 reciprocal for the multiplication."""
    return F32(times + 1) if mode == MEAN_DIVIDE else F32(1) / F32(times + 1)


def reflect_direction_ref(normal, noise, noise_std, d):
    """mnrf_reflect.h `direction` on rows: every line one fp32 operation per element, sums left to right."""
    with np.errstate(all="ignore"):
        nv = np.asarray(normal, F32).copy()
        if noise is not None:
            nv = (nv + (np.asarray(noise, F32) * F32(noise_std)).astype(F32)).astype(F32)
        wv = (-np.asarray(d, F32)).astype(F32)
        nsq = ((nv[:, 0] * nv[:, 0] + nv[:, 1] * nv[:, 1]).astype(F32) + nv[:, 2] * nv[:, 2]).astype(F32)
        wsq = ((wv[:, 0] * wv[:, 0] + wv[:, 1] * wv[:, 1]).astype(F32) + wv[:, 2] * wv[:, 2]).astype(F32)
        ninv = (F32(1) / np.sqrt(np.fmax(nsq, EPS32)).astype(F32)).astype(F32)      # fmaxf: a NaN sum gives eps
        winv = (F32(1) / np.sqrt(np.fmax(wsq, EPS32)).astype(F32)).astype(F32)
        nv = (nv * ninv[:, None]).astype(F32)
        wv = (wv * winv[:, None]).astype(F32)
        c = ((wv[:, 0] * nv[:, 0] + wv[:, 1] * nv[:, 1]).astype(F32) + wv[:, 2] * nv[:, 2]).astype(F32)
        return (((F32(2) * c)[:, None] * nv).astype(F32) - wv).astype(F32)


def reflect_jitter_fan_ref(rays, x_surface, normal, noise, noise_std, index, near2):
    """mnrf_reflect_jitter_fan: (n_jit * m, 8); noise (n_jit, n_rays, 3) or (n_jit, None) for the null pointer."""
    n_jit = noise[0] if isinstance(noise, tuple) else noise.shape[0]
    idx = np.asarray(index, np.int64)
    out = np.empty((n_jit, idx.size, 8), F32)
    for j in range(n_jit):
        nz = None if isinstance(noise, tuple) else noise[j][idx]
        out[j, :, 0:3] = x_surface[idx]
        out[j, :, 3:6] = reflect_direction_ref(normal[idx], nz, noise_std, rays[idx, 3:6])
        out[j, :, 6] = F32(near2)
        out[j, :, 7] = rays[idx, 7]
    return out.reshape(n_jit * idx.size, 8)


def jitter_mean_ref(acc, pieces, index, finish_mode=MEAN_NONE, value=None):
    """mnrf_jitter_mean on a copy of acc (n_acc,3); pieces (n_jit, m, 3); index (m) distinct rows or None."""
    acc = np.array(acc, F32, copy=True)
    rows = np.arange(pieces.shape[1]) if index is None else np.asarray(index, np.int64)
    with np.errstate(all="ignore"):
        a = acc[rows]
        for j in range(pieces.shape[0]):
            a = (a + pieces[j]).astype(F32)
        if finish_mode == MEAN_DIVIDE:
            a = (a / F32(value)).astype(F32)
        elif finish_mode == MEAN_MULTIPLY:
            a = (a * F32(value)).astype(F32)
    acc[rows] = a
    return acc


def render_eval_rough(models, embeddings, rays, N_samples, N_importance, use_disp, chunk, args, white_back=False,
                      trace_secondary_rays=True, test_time=True, normal_noise=None, finish_mode=MEAN_DIVIDE):
    """oracle.render_eval with THE RULE in the roughness branch.  finish_mode: MEAN_DIVIDE is the oracle's (and numpy's) `/`;
    MEAN_MULTIPLY what the device does (one ulp apart at most)."""
    pieces = {}
    for i in range(0, rays.shape[0], chunk):
        r = _recurse(models, embeddings, rays[i:i + chunk], 0, N_samples, N_importance, use_disp, chunk, args, white_back,
                     trace_secondary_rays, test_time, normal_noise, finish_mode)
        for k, v in r.items():
            pieces.setdefault(k, []).append(v)
    return {k: np.concatenate(v, 0) for k, v in pieces.items()}


def _recurse(models, embeddings, rays, level, N_samples, N_importance, use_disp, chunk, args, white_back, trace_flag, test_time,
             normal_noise, finish_mode):
    one_field = args.get("only_one_field", False)
    r = O.render_rays(models, embeddings, rays, N_samples, use_disp, 0, 0, N_importance, chunk, white_back, test_time=test_time,
                      compute_normal=trace_flag and (not args["predict_normal"]), only_one_field=one_field,
                      only_one_field_fine_epoch=args.get("only_one_field_fine_epoch", 2),
                      current_epoch=args.get("only_one_field_fine_epoch", 2) + 1)
    sel = "fine" if (N_importance > 0 and not one_field) else "coarse"
    only_in = not (level < 1)
    r[f"rgb_{sel}_reflect"] = np.zeros_like(r[f"rgb_{sel}"])
    r[f"depth_{sel}_reflect"] = np.zeros_like(r[f"depth_{sel}"])
    mask = None
    for key in (f"mirror_mask_{sel}", "mirror_mask_fine", "mirror_mask_coarse"):
        if key in r:
            mask = r[key]
            break
    mb = None
    if mask is not None:
        O._hard_threshold_inplace(mask)
        mb = mask.astype(bool)
    trace = bool(mb is not None and mb.any() and trace_flag)
    if level >= args["max_recursive_level"]:
        trace = False
    if not trace:
        return r
    far = rays[:, 7:8]
    sec_o = r[f"x_surface_{sel}"]
    normal = O._pick_normal(r, sel)
    rough = args.get("app_control_mirror_roughness", False)
    std = F32(args.get("normal_noise_std", 0))
    normal_bkp = normal.copy()
    if rough:
        normal = normal + (next(normal_noise) * std).astype(F32)
    refl, _, wv = O.reflect(rays[:, 3:6], normal)
    r["reflect_direction"] = refl
    near2 = np.full_like(far, 0.1)
    sec = np.concatenate([sec_o, refl, near2, far], -1).astype(F32)
    if only_in:
        sec = sec[mb]
    if sec.shape[0] == 0:
        return r
    rec = (N_samples, N_importance, use_disp, chunk, args, white_back, trace_flag, test_time, normal_noise, finish_mode)
    r2 = _recurse(models, embeddings, sec, level + 1, *rec)
    if rough:
        times = args["trace_ray_times"]
        index = np.nonzero(mb)[0]                                      # the level's one compaction
        rows = np.arange(index.size) if only_in else index             # row of R that ray index[p] has
        keys = [f"rgb_{typ}" for typ in ("coarse", "fine") if f"rgb_{typ}" in r2]
        for _ in range(times):
            nrm = O.l2_normalize(normal_bkp + (next(normal_noise) * std).astype(F32))
            rd = (F32(2) * np.sum(wv * nrm, -1, dtype=F32)[:, None] * nrm - wv).astype(F32)
            s2 = np.concatenate([sec_o, rd, near2, far], -1).astype(F32)[index]
            r3 = _recurse(models, embeddings, s2, level + 1, *rec)
            for k in keys:
                r2[k][rows] = (r2[k][rows] + r3[k]).astype(F32)         # S = ((R[row] + J_1[p]) + J_2[p]) + ...
        for k in keys:                                                 # a ray of level 0 that is no mirror ray keeps R[i]
            if finish_mode == MEAN_MULTIPLY:
                r2[k][rows] = (r2[k][rows] * finish_value(times, MEAN_MULTIPLY)).astype(F32)
            else:
                r2[k][rows] = (r2[k][rows] / F32(times + 1)).astype(F32)
    base = r[f"rgb_{sel}"]
    if only_in:
        part = base.copy()
        part[mb] = r2[f"rgb_{sel}"]
    else:
        part = r2[f"rgb_{sel}"]
    m3 = mb.astype(F32)[:, None]
    r[f"rgb_{sel}"] = (m3 * part + (F32(1) - m3) * base).astype(F32)
    if only_in:
        rr = np.zeros_like(r[f"rgb_{sel}"])
        rr[mb] = r2[f"rgb_{sel}"]
        r[f"rgb_{sel}_reflect"] = rr
        dd = np.zeros_like(r[f"depth_{sel}"])
        dd[mb] = r2[f"depth_{sel}"]
        r[f"depth_{sel}_reflect"] = dd
    else:
        r[f"rgb_{sel}_reflect"] = r2[f"rgb_{sel}"]
        r[f"depth_{sel}_reflect"] = r2[f"depth_{sel}"]
    return r
