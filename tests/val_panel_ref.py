"""numpy float32 restatement of the reference's validation panel, visualize_val_image(img_wh, batch, results, add_text=False)
(utils/visualization.py:26-184), the yardstick of tests/test_val_panel_cpu.py and tests/test_hip_val_panel.py, written from
reading it: every tile is the reference's own chain of float32 operations; the depth canvas is tests/frames_ref.py's
(`T[k]` in place of cv2.applyColorMap, float32 division by 255 in place of ToTensor).

Maps are flat, (n,) or (n, 3) float32 with n = H W; the panel is (N_pics, 3, H, W) float32 and `names` the reference's labels."""
import numpy as np

from . import frames_ref as FR

F32 = np.float32
TYPS = ("fine", "coarse")


def chw(v, H, W):
    """.view(H, W, 3).permute(2, 0, 1)"""
    return np.ascontiguousarray(np.asarray(v, F32).reshape(H, W, 3).transpose(2, 0, 1))


def mask_tile(m, H, W):
    """.squeeze().unsqueeze(-1).repeat(1, 3).view(H, W, 3).permute(2, 0, 1)"""
    return chw(np.repeat(np.asarray(m, F32).reshape(-1)[:, None], 3, axis=1), H, W)


def global_map(v):
    """visualize_rgb_map_global (visualization.py:208-221); torch.min / torch.max propagate a NaN, as np.min / np.max do"""
    v = np.asarray(v, F32)
    mn, mx = np.min(v), np.max(v)
    if mn == mx:
        return np.ones_like(v)
    with np.errstate(all="ignore"):
        return (v - mn) / (mx - mn)


def depth_tile(d, table, H, W):
    """visualize_depth(depth.view(H, W)) with vmin = vmax = None: (3, H, W)"""
    return chw(FR.depth_canvas(np.asarray(d, F32).reshape(-1), table), H, W)


def val_panel(img_wh, batch, results, table):
    W, H = img_wh
    tiles = [("gt_img", chw(batch["rgbs"], H, W))]
    for key, name in (("rgb_{}", "img_{}"), ("rgb_{}_reflect", "img_reflect_{}"), ("rgb_{}_direct", "img_direct_{}")):
        tiles += [(name.format(t), chw(results[key.format(t)], H, W)) for t in TYPS if key.format(t) in results]
    for key, name in (("depth_{}", "depth_{}"), ("depth_{}_reflect", "depth_reflect_{}")):
        tiles += [(name.format(t), depth_tile(results[key.format(t)], table, H, W)) for t in TYPS if key.format(t) in results]
    if "mirror_mask" in batch:
        tiles.append(("gt_mirror_mask", mask_tile(batch["mirror_mask"], H, W)))
    tiles += [(f"mirror_mask_pred_{t}", mask_tile(results[f"mirror_mask_{t}"], H, W)) for t in TYPS if f"mirror_mask_{t}" in results]
    for t in TYPS:
        for key, name in ((f"surface_normal_{t}", f"normal_pred_{t}"), (f"surface_normal_grad_{t}", f"normal_grad_{t}")):
            if key in results:
                tiles.append((name, chw((np.asarray(results[key], F32) + 1) / 2, H, W)))
    for key in ("secondary_rays_o", "reflect_direction"):
        if key in results:
            tiles += [(key, chw(results[key], H, W)), (f"{key}_vis", chw(global_map(results[key]), H, W))]
    tiles += [(f"x_surface_{t}", chw(global_map(results[f"x_surface_{t}"]), H, W)) for t in TYPS if f"x_surface_{t}" in results]
    return np.stack([t for _, t in tiles]), [n for n, _ in tiles]


RESULT_KEYS3 = ("rgb_{}", "rgb_{}_reflect", "rgb_{}_direct", "surface_normal_{}", "surface_normal_grad_{}", "x_surface_{}")
RESULT_KEYS1 = ("depth_{}", "depth_{}_reflect", "mirror_mask_{}")
VARIANTS = ("all", "coarse_only", "no_reflect", "nan_depth", "nan_global", "const_global", "const_depth", "depth_extremes_last")


def seeded_case(H, W, seed, variant="all"):
    """(batch, results) of numpy float32 maps carrying every key of visualization.py:32-179, then edited per `variant`."""
    assert variant in VARIANTS
    n = H * W
    rng = np.random.default_rng(seed)
    batch = {"rgbs": rng.uniform(0, 1, (n, 3)).astype(F32), "mirror_mask": (rng.uniform(0, 1, n) > 0.5).astype(F32)}
    res = {}
    for t in TYPS:
        for k in RESULT_KEYS3:
            res[k.format(t)] = rng.uniform(-1.2, 1.2, (n, 3)).astype(F32)
        res[f"x_surface_{t}"] = rng.normal(0, 3, (n, 3)).astype(F32)
        res[f"depth_{t}"] = rng.uniform(2, 6, n).astype(F32)
        res[f"depth_{t}_reflect"] = rng.uniform(0, 9, n).astype(F32)
        res[f"mirror_mask_{t}"] = rng.uniform(-0.1, 1.1, n).astype(F32)
    res["secondary_rays_o"] = rng.normal(0, 2, (n, 3)).astype(F32)
    res["reflect_direction"] = rng.uniform(-1, 1, (n, 3)).astype(F32)
    # an infinity in one depth map: nan_to_num makes it FLT_MAX, the map's maximum
    res["depth_coarse_reflect"][n // 3] = np.inf
    if variant == "coarse_only":
        res = {k: v for k, v in res.items() if "fine" not in k}
    elif variant == "no_reflect":
        res = {k: v for k, v in res.items() if "reflect" not in k and "direct" not in k and k != "secondary_rays_o"}
    elif variant == "nan_depth":
        res["depth_fine"][n // 2] = np.nan
        res["depth_coarse_reflect"][0] = np.nan
    elif variant == "nan_global":
        res["secondary_rays_o"][n - 1, 2] = np.nan
        res["x_surface_fine"][n // 2, 1] = np.nan
    elif variant == "const_global":
        res["reflect_direction"][:] = F32(0.25)
        res["x_surface_coarse"][:] = F32(-7.5)
    elif variant == "const_depth":
        res["depth_fine"][:] = F32(3.25)
        res["depth_fine_reflect"][:] = F32(0)
    elif variant == "depth_extremes_last":
        res["depth_fine"][n - 1] = F32(9.5)
        res["depth_coarse"][n - 1] = F32(-1.0)
        res["x_surface_fine"][n - 1, 2] = F32(40.0)
    return batch, res
