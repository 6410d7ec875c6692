"""Plain numpy restatements for the tests of the colouring along the vertex normals (mirror_nerf_amd.mesh.vertex_normals,
normal_rays, rgb_to_uint8): float64 throughout, sums in the order of the triangle array (np.add.at).  Nothing is shared
with csrc/mnrf_mesh.hip, whose sums are 64-bit fixed point and free of any order.  `height_field_mesh` and `fan_mesh` build
the large meshes of the tests: more triangles than one sweep of the maximum kernel, and 100 000 triangles on one vertex.
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


def cross_products(vertices, triangles):
    """(T, 3) float64: (v_b - v_a) x (v_c - v_a) of every triangle, from the float32 vertices."""
    v = np.asarray(vertices, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return np.cross(v[t[:, 1]] - v[t[:, 0]], v[t[:, 2]] - v[t[:, 0]])


def height_field_mesh(n, seed=0):
    """An n x n grid of unit spacing with seeded heights in [0, 0.3): (vertices (n^2, 3) float32, triangles (2 (n - 1)^2, 3)
    int32), two triangles per square in row order, wound so that the normals point to +z.  The last two triangles are
    (n^2 - n - 2, n^2 - 1, n^2 - n - 1) and (n^2 - n - 2, n^2 - 2, n^2 - 1): the corner vertex n^2 - 1 belongs to them and to
    no other."""
    rs = np.random.RandomState(seed)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([i, j, rs.uniform(0, 0.3, (n, n))], -1).reshape(-1, 3).astype(np.float32)
    a = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1)
    lower = np.stack([a, a + n, a + n + 1], 1)          # (i, j), (i + 1, j), (i + 1, j + 1)
    upper = np.stack([a, a + n + 1, a + 1], 1)          # (i, j), (i + 1, j + 1), (i, j + 1)
    t = np.stack([upper, lower], 1).reshape(-1, 3).astype(np.int32)
    return v, t


def fan_mesh(n_triangles, radius=1.0, height=0.25):
    """A closed fan: hub 0 at (0, 0, height), n_triangles rim vertices on the circle of `radius` in z = 0, triangle k =
    (0, 1 + k, 1 + (k + 1) % n): every triangle holds the hub, all are congruent up to float32 rounding of the rim."""
    k = np.arange(n_triangles)
    ang = 2.0 * np.pi * k / n_triangles
    v = np.concatenate([[[0.0, 0.0, height]], np.stack([radius * np.cos(ang), radius * np.sin(ang), 0 * ang], 1)], 0).astype(np.float32)
    t = np.stack([0 * k, 1 + k, 1 + (k + 1) % n_triangles], 1).astype(np.int32)
    return v, t


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
