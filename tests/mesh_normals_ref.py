"""Plain numpy restatements for the tests of the colouring along the vertex normals (mirror_nerf_amd.mesh.vertex_normals,
normal_rays, rgb_to_uint8): float64 throughout, sums in the order of the triangle array (np.add.at).  Nothing is shared
with csrc/mnrf_mesh.hip, whose sums are 64-bit fixed point and free of any order.
"""
import numpy as np


def vertex_normals(vertices, triangles, dtype=np.float32):
    """The definition of DESIGN 4.6: per triangle (a, b, c) the unnormalised (v_b - v_a) x (v_c - v_a) in float64 from the
    float32 vertices, summed per vertex, normalised in float64, cast to `dtype`; (0, 0, 1) where the sum has zero or
    non-finite length."""
    v = np.asarray(vertices, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        cross = np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]]) if len(t) else np.zeros((0, 3))
        total = np.zeros_like(v)
        for corner in range(3):
            np.add.at(total, t[:, corner], cross)
        length = np.sqrt(total[:, 0] * total[:, 0] + total[:, 1] * total[:, 1] + total[:, 2] * total[:, 2])
        out = total / length[:, None]
    bad = ~(np.isfinite(length) & (length > 0))
    out[bad] = (0.0, 0.0, 1.0)
    return out.astype(dtype)


def normal_rays_torch(vertices, normals, near, far, near_t=1.0):
    """extract_color_mesh.py:250-253, 262 with torch on the CPU, float32: (V, 8) [o, d, near, far]."""
    import torch
    rays_d = torch.FloatTensor(np.asarray(normals, dtype=np.float32))
    near_ = near * torch.ones_like(rays_d[:, :1])
    far_ = far * torch.ones_like(rays_d[:, :1])
    rays_o = torch.FloatTensor(np.asarray(vertices, dtype=np.float32)) - rays_d * near_ * near_t
    return torch.cat([rays_o, rays_d, near_, far_], 1).numpy()


def rgb_to_uint8(rgb):
    """extract_color_mesh.py:359-362 for values whose product lies in [0, 256): (rgb * 255.0).astype(np.uint8)."""
    return (np.asarray(rgb, dtype=np.float32) * 255.0).astype(np.uint8)


def ray_error_stats(a, b):
    """Per ray the largest difference over the channels: (median, 95th percentile, share above 1e-4, the (V,) array)."""
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).reshape(len(a), -1).max(1)
    return float(np.median(d)), float(np.percentile(d, 95)), float((d > 1e-4).mean()), d
