"""numpy restatements for a roughness per placed mirror (include/mnrf.h "A roughness per mirror").

rough_rows_ref, perturb_normals_ref and reflect_jitter_fan_rows_ref repeat the three kernels of csrc/mnrf_rough.hip one fp32
operation at a time, in their order: the GPU tests compare bit for bit.  The reflected direction is tests/rough_ref.py's
reflect_direction_ref, the restatement of csrc/mnrf_reflect.h that the uniform route's tests already use."""
import numpy as np

from tests.rough_ref import reflect_direction_ref

F32 = np.float32


def rough_rows_ref(index, mask, roughness, scene_roughness, any_in=0):
    """mnrf_rough_rows -> dict(std_rows, jitter_mask, any).  index: (n,) int32 or None (the null pointer: all -1); roughness: the K
    per-mirror values; an index outside [0, K) takes scene_roughness."""
    mask = np.asarray(mask, F32)
    n = mask.shape[0]
    idx = np.full(n, -1, np.int64) if index is None else np.asarray(index, np.int64)
    rough = np.asarray(roughness, F32).reshape(-1)
    std = np.full(n, F32(scene_roughness), F32)
    placed = (idx >= 0) & (idx < rough.size)
    std[placed] = rough[idx[placed]]
    with np.errstate(invalid="ignore"):
        in_j = (mask != 0) & (std > 0)                 # a NaN mask is != 0, as in mnrf_reflect_compact's selection
    return dict(std_rows=std, jitter_mask=in_j.astype(F32), any=int(any_in) | int(in_j.any()))


def perturb_normals_ref(normal, noise, std_rows):
    """mnrf_perturb_normals: normal + noise * std where std > 0 (one multiplication, one addition), the untouched value elsewhere."""
    normal, noise, std = np.asarray(normal, F32), np.asarray(noise, F32), np.asarray(std_rows, F32)
    with np.errstate(all="ignore"):
        scaled = (noise * std[:, None]).astype(F32)
        moved = (normal + scaled).astype(F32)
    out = normal.copy()
    rows = std > 0
    out[rows] = moved[rows]
    return out


def reflect_jitter_fan_rows_ref(rays, x_surface, normal, noise, std_rows, index, near2):
    """mnrf_reflect_jitter_fan_rows: (n_jit * m, 8); noise (n_jit, n_rays, 3) or (n_jit, None) for the null pointer.  The kernel
    evaluates mnrf_reflect.h's direction with the ray's own std: the addition is made on every row, a std of 0 included."""
    n_jit = noise[0] if isinstance(noise, tuple) else noise.shape[0]
    idx = np.asarray(index, np.int64)
    std = np.asarray(std_rows, F32)[idx]
    out = np.empty((n_jit, idx.size, 8), F32)
    for j in range(n_jit):
        nv = np.asarray(normal, F32)[idx]
        if not isinstance(noise, tuple):
            with np.errstate(all="ignore"):
                scaled = (np.asarray(noise[j], F32)[idx] * std[:, None]).astype(F32)
                nv = (nv + scaled).astype(F32)
        out[j, :, 0:3] = x_surface[idx]
        out[j, :, 3:6] = reflect_direction_ref(nv, None, 0.0, rays[idx, 3:6])
        out[j, :, 6] = F32(near2)
        out[j, :, 7] = rays[idx, 7]
    return out.reshape(n_jit * idx.size, 8)


def first_reflection_ref(normal, draw, std_rows, d):
    """The first reflection of THE RULE on every row: mnrf_perturb_normals, then mnrf_reflect_compact without noise."""
    return reflect_direction_ref(perturb_normals_ref(normal, draw, std_rows), None, 0.0, d)
