"""Mesh extraction on the device: the reference's third program, extract_color_mesh.py, behind plain functions.

    volume = density_grid(model, embedding_xyz, x_range, y_range, z_range, N)      # extract_color_mesh.py:146-185
    vertices, triangles = marching_cubes(volume, threshold)                       # :189 (mcubes.marching_cubes)
    vertices, triangles = largest_component(vertices, triangles)                  # :220-224 (open3d clustering)
    colors = fuse_vertex_colors(world_vertices, model, embeddings, images, poses, focal, near, ...)      # :269-355
    colors = normal_vertex_colors(world_vertices, triangles, models, embeddings, near, far)              # :247-267, 358-359
    normals = vertex_normals(world_vertices, triangles)                           # :249 (open3d compute_vertex_normals)
    write_ply(path, world_vertices, triangles, colors, normals)                   # :367-369 (plyfile)

`extract_mesh` chains the first three and maps the vertices to world coordinates.  The arithmetic runs in
csrc/mnrf_mesh.hip and the field kernels (include/mnrf.h); this module allocates, scans the per-block counts
(torch.cumsum), compacts (boolean indexing) and writes files.  Datasets are out of scope: the images and poses of `fuse_vertex_colors` come
from the caller; `normal_vertex_colors` (the reference's `--use_vertex_normal`) needs the two models only.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from . import mirror_nerf as _mn
from .mirror_nerf_tcnn import MirrorNeRFTcnn
from .weights import packed_of


def _range(r, name):
    r = [float(v) for v in r]
    if len(r) != 2:
        raise ValueError(f"{name} must hold two numbers (min, max)")
    return r


def _device_of(model):
    return next(model.parameters()).device


# ----------------------------------------------------------------------------------------------- density grid
def grid_points(x_range, y_range, z_range, N, start, count, out=None, device=None):
    """Rows [start, start + count) of the reference's (N^3, 3) float32 query tensor, generated on the device and
    bit-identical to `np.stack(np.meshgrid(x, y, z), -1).reshape(-1, 3)` of three float64 `np.linspace`s cast to float32
    (extract_color_mesh.py:146-152).  `out`: an optional (>= count, 3) float32 device buffer to write into."""
    (x0, x1), (y0, y1), (z0, z1) = _range(x_range, "x_range"), _range(y_range, "y_range"), _range(z_range, "z_range")
    if out is None:
        out = torch.empty(count, 3, dtype=torch.float32, device=device or "cuda")
    if out.dtype != torch.float32 or out.dim() != 2 or out.shape[1] != 3 or out.shape[0] < count:
        raise ValueError("out must be a float32 tensor of shape (>= count, 3)")
    with torch.cuda.device(out.device):
        _lib.check(_lib.lib().mnrf_grid_points(x0, x1, y0, y1, z0, z1, int(N), int(start), int(count), _lib.ptr(out),
                                               _lib.stream()), "mnrf_grid_points")
    return out[:count]


def density_grid(model, embedding_xyz, x_range, y_range, z_range, N, chunk=1 << 20):
    """The (N, N, N) float32 density volume `max(sigma, 0)` of extract_color_mesh.py:146-185 on the device.

    volume[a, b, c] is the density at (x[b], y[a], z[c]) -- the "xy" order of numpy.meshgrid, as in the reference.  The
    points of one chunk at a time are generated into a (chunk, 3) buffer and pushed through the sigma-only field launch
    (the model's current arithmetic, "split" or "fp32"), which writes into the volume; neither the N^3 x 3 point tensor nor
    the reference's zero directions and their encoding exist.  The reference runs the full forward; sigma does not depend
    on the direction.  `model`: a MirrorNeRF or a MirrorNeRFTcnn."""
    N = int(N)
    if N < 2:
        raise ValueError("N must be at least 2")
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be positive")
    hashgrid = isinstance(model, MirrorNeRFTcnn)
    if not hashgrid and getattr(embedding_xyz, "N_freqs", None) != model.n_freqs_xyz:
        raise NotImplementedError(f"embedding_xyz must be Embedding({model.n_freqs_xyz})")
    dev = _device_of(model)
    total = N * N * N
    chunk = min(chunk, total)
    L = _lib.lib()
    with torch.cuda.device(dev), torch.no_grad():
        volume = torch.empty(total, dtype=torch.float32, device=dev)
        xyz = torch.empty(chunk, 3, dtype=torch.float32, device=dev)
        while True:
            for start in range(0, total, chunk):
                n = min(chunk, total - start)
                grid_points(x_range, y_range, z_range, N, start, n, out=xyz)
                if hashgrid:      # (its launch wrapper allocates its outputs: one copy of the chunk's sigma)
                    volume[start:start + n] = model.field(n, xyz=xyz, xyz_stride=3, sigma_only=True)["sigma"]
                else:
                    split = _mn.precision_of(model) == "split"
                    flags = _lib.MNRF_SIGMA_ONLY | (_lib.MNRF_SPLIT_F16 if split else 0)
                    _lib.check(L.mnrf_field_forward(_lib.ptr(packed_of(model)), flags, n, _lib.ptr(xyz), 3, None, None, 1, None, 27,
                                                    ctypes.c_void_p(volume.data_ptr() + 4 * start), None, None, None, None, None,
                                                    _lib.stream()), "mnrf_field_forward")
            # range guard of the split arithmetic: a trip switches the model to the exact kernels; evaluate again
            if hashgrid or not _mn.check_guard([model]):
                break
        if not hashgrid:
            _mn.release_transient([model])
        _lib.check(L.mnrf_clamp_zero(_lib.ptr(volume), total, _lib.stream()), "mnrf_clamp_zero")
    return volume.view(N, N, N)


# ----------------------------------------------------------------------------------------------- marching cubes
def mc_table():
    """The 256 x 16 int8 triangle table of the marching-cubes kernels (mnrf_mc_table; a host call)."""
    out = np.empty((256, 16), dtype=np.int8)
    row = (ctypes.c_int8 * 16)()
    L = _lib.lib()
    for c in range(256):
        _lib.check(L.mnrf_mc_table(c, ctypes.cast(row, ctypes.c_void_p)), "mnrf_mc_table")
        out[c] = np.frombuffer(row, dtype=np.int8)
    return out


def marching_cubes(volume, threshold, timings=None):
    """Iso-surface of a (Nx, Ny, Nz) float32 device volume at `threshold`: (vertices (V, 3) float32 in index coordinates of
    the volume, triangles (T, 3) int32), both on the device, vertices welded (one per crossed grid edge).

    A corner is inside when its value >= threshold; triangles are wound so that the geometric normal points towards lower
    values.  The order of the output is deterministic (two runs are bit-identical).  `mcubes` itself cannot be compared
    with here: its handling of ties and its winding are not pinned.
    `timings`: an optional dict that receives the torch.cuda.Event pairs of the stages (scripts/bench_mesh.py)."""
    if not volume.is_cuda or volume.dtype != torch.float32 or volume.dim() != 3:
        raise RuntimeError("marching_cubes needs a 3-D float32 tensor on the GPU")
    volume = volume.contiguous()
    nx, ny, nz = (int(s) for s in volume.shape)
    L, p = _lib.lib(), _lib.ptr
    dev = volume.device

    def mark(name):
        if timings is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            timings.setdefault("events", []).append((name, e))

    with torch.cuda.device(dev):
        blocks = L.mnrf_mc_blocks(nx, ny, nz)
        if blocks < 0:
            _lib.check(int(blocks), "mnrf_mc_blocks")
        mark("start")
        counts = torch.empty(blocks, 2, dtype=torch.int32, device=dev)
        _lib.check(L.mnrf_mc_count(p(volume), nx, ny, nz, float(threshold), p(counts), _lib.stream()), "mnrf_mc_count")
        mark("count")
        # (scanned along the contiguous axis: torch's scan over the strided block axis of the (blocks, 2) array is ~30x slower)
        inclusive = torch.cumsum(counts.t().contiguous(), 1, dtype=torch.int64).t()
        n_vert, n_tri = (int(v) for v in inclusive[-1].tolist())
        if n_vert > (1 << 29) or n_tri > (1 << 31) // 3:
            raise RuntimeError(f"marching_cubes: {n_vert} vertices / {n_tri} triangles exceed the 32-bit index range")
        offsets = (inclusive - counts).to(torch.int32).contiguous()
        mark("scan")
        vertices = torch.empty(n_vert, 3, dtype=torch.float32, device=dev)
        triangles = torch.empty(n_tri, 3, dtype=torch.int32, device=dev)
        if n_vert or n_tri:
            base = torch.empty(nx * ny * nz, dtype=torch.int32, device=dev)
            _lib.check(L.mnrf_mc_emit(p(volume), nx, ny, nz, float(threshold), p(offsets), p(base), n_vert, n_tri,
                                      p(vertices) if n_vert else None, p(triangles) if n_tri else None, _lib.stream()),
                       "mnrf_mc_emit")
        mark("emit")
    return vertices, triangles


# ----------------------------------------------------------------------------------------------- connected components
def component_labels(vertices_or_count, triangles):
    """labels (V,) int32 on the device: the smallest vertex index of each vertex's connected component (vertices joined by
    a triangle are connected).  Union-find on the device: hooking by atomic min + pointer jumping, to the fixed point."""
    V = int(vertices_or_count) if isinstance(vertices_or_count, int) else int(vertices_or_count.shape[0])
    if not triangles.is_cuda or triangles.dtype != torch.int32 or triangles.dim() != 2 or triangles.shape[1] != 3:
        raise RuntimeError("triangles must be a (T, 3) int32 tensor on the GPU")
    triangles = triangles.contiguous()
    T = int(triangles.shape[0])
    dev = triangles.device
    L, p = _lib.lib(), _lib.ptr
    with torch.cuda.device(dev):
        labels = torch.empty(V, dtype=torch.int32, device=dev)
        _lib.check(L.mnrf_cc_init(p(labels), V, _lib.stream()), "mnrf_cc_init")
        changed = torch.zeros(1, dtype=torch.int32, device=dev)
        for _ in range(V + 2):      # (each round at least halves the number of trees that can still merge; V is a safe cap)
            if not (V and T):
                break
            changed.zero_()
            _lib.check(L.mnrf_cc_step(p(triangles), T, p(labels), V, p(changed), _lib.stream()), "mnrf_cc_step")
            if int(changed.item()) == 0:
                break
        else:
            raise RuntimeError("component_labels: no fixed point")
    return labels


def largest_component(vertices, triangles, return_info=False):
    """Keep the connected component with the most TRIANGLES, drop the vertices it does not reference and re-index
    (extract_color_mesh.py:220-224: open3d's cluster_connected_triangles + argmax + remove_unreferenced_vertices).
    Triangle order and vertex order are kept.  Between components of equal size the one with the smallest label wins,
    i.e. the one that holds the lowest-numbered vertex.  An empty mesh is returned unchanged.
    return_info: also return {"n_components", "largest_triangles"} (components that own at least one triangle)."""
    V, T = int(vertices.shape[0]), int(triangles.shape[0])
    info = {"n_components": 0, "largest_triangles": 0}
    if V == 0 or T == 0:
        out = (vertices[:0], triangles[:0]) if T == 0 else (vertices, triangles)
        return out + (info,) if return_info else out
    labels = component_labels(V, triangles)
    dev = triangles.device
    L, p = _lib.lib(), _lib.ptr
    with torch.cuda.device(dev):
        counts = torch.zeros(V, dtype=torch.int32, device=dev)
        _lib.check(L.mnrf_cc_count(p(triangles.contiguous()), T, p(labels), V, p(counts), _lib.stream()), "mnrf_cc_count")
        best = torch.argmax(counts)      # the first maximum: the smallest label
        keep_v = labels == best
        keep_t = keep_v[triangles[:, 0].long()]
        new_index = (torch.cumsum(keep_v, 0, dtype=torch.int32) - 1).to(torch.int32)
        out_t = new_index[triangles[keep_t].long()].contiguous()
        out_v = vertices[keep_v].contiguous()
        if return_info:
            info = {"n_components": int((counts > 0).sum().item()), "largest_triangles": int(counts[best].item())}
    return (out_v, out_t, info) if return_info else (out_v, out_t)


# ----------------------------------------------------------------------------------------------- world coordinates
def index_to_world(vertices, x_range, y_range, z_range, N, exact_spacing=False):
    """Index coordinates of the (N, N, N) volume -> world coordinates, float32, on the device the vertices live on.

    exact_spacing=False (default) restates extract_color_mesh.py:193-199 with its quirks: the index is divided by N
    although the samples are N - 1 steps apart (the mesh comes out (N - 1) / N too small, anchored at the box minimum),
    and after the x / y swap that the "xy" meshgrid calls for (volume axis 0 is y) the first two coordinates are scaled
    with each other's range -- harmless for the square boxes the reference is used with:
        v = float32(vertices / N);  x = (ymax - ymin) * v[:, 1] + ymin;  y = (xmax - xmin) * v[:, 0] + xmin;
        z = (zmax - zmin) * v[:, 2] + zmin
    exact_spacing=True divides by N - 1 and gives every axis its own range, so that a vertex on grid point (a, b, c) lands
    on the position that point was sampled at: x = (xmax - xmin) * v[:, 1] + xmin, y = (ymax - ymin) * v[:, 0] + ymin.
    The swap mirrors the mesh, so triangles that were wound outwards in index coordinates are wound inwards in world
    coordinates -- in both settings, as in the reference."""
    (x0, x1), (y0, y1), (z0, z1) = _range(x_range, "x_range"), _range(y_range, "y_range"), _range(z_range, "z_range")
    N = int(N)
    v = (vertices.double() / float(N - 1 if exact_spacing else N)).float()
    f32 = lambda a: torch.tensor(np.float32(a).item(), dtype=torch.float32, device=v.device)  # noqa: E731
    if exact_spacing:
        x = f32(x1 - x0) * v[:, 1] + f32(x0)
        y = f32(y1 - y0) * v[:, 0] + f32(y0)
    else:
        x = f32(y1 - y0) * v[:, 1] + f32(y0)
        y = f32(x1 - x0) * v[:, 0] + f32(x0)
    z = f32(z1 - z0) * v[:, 2] + f32(z0)
    return torch.stack([x, y, z], 1).contiguous()


def extract_mesh(model, embedding_xyz, x_range, y_range, z_range, N, sigma_threshold, keep_largest=True,
                 exact_spacing=False, chunk=1 << 20):
    """Density grid -> marching cubes -> (largest component) -> world coordinates: (vertices (V, 3) float32, triangles
    (T, 3) int32) on the device.  See density_grid, marching_cubes, largest_component and index_to_world."""
    volume = density_grid(model, embedding_xyz, x_range, y_range, z_range, N, chunk=chunk)
    vertices, triangles = marching_cubes(volume, sigma_threshold)
    if keep_largest:
        vertices, triangles = largest_component(vertices, triangles)
    return index_to_world(vertices, x_range, y_range, z_range, N, exact_spacing), triangles


# ----------------------------------------------------------------------------------------------- vertex colours
def project_view(vertices, image, pose, focal, near):
    """One view of the colouring: (colors (V, 3) float32 bilinear samples of `image`, depth (V,) float64, rays (V, 8)
    occlusion rays [camera origin, unit direction to the vertex, near, far = depth]).  `pose`: camera-to-world (3, 4);
    `image`: (H, W, 3) uint8 on the device.  Vertices that project outside the image (or lie behind the camera) are
    clipped to the border, not dropped, as in extract_color_mesh.py:297-298."""
    if not vertices.is_cuda or vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise RuntimeError("vertices must be a (V, 3) float32 tensor on the GPU")
    if not image.is_cuda or image.dtype != torch.uint8 or image.dim() != 3 or image.shape[2] != 3:
        raise RuntimeError("image must be a (H, W, 3) uint8 tensor on the GPU")
    vertices, image = vertices.contiguous(), image.contiguous()
    V, (H, W) = int(vertices.shape[0]), (int(image.shape[0]), int(image.shape[1]))
    pose = np.asarray(pose.detach().cpu() if torch.is_tensor(pose) else pose, dtype=np.float32).reshape(3, 4)
    c2w = np.concatenate([pose, np.array([0, 0, 0, 1]).reshape(1, 4)], 0)      # float64, as the reference builds it
    w2c = np.ascontiguousarray(np.linalg.inv(c2w)[:3], dtype=np.float64)
    dev = vertices.device
    with torch.cuda.device(dev):
        colors = torch.empty(V, 3, dtype=torch.float32, device=dev)
        depth = torch.empty(V, dtype=torch.float64, device=dev)
        rays = torch.empty(V, 8, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().mnrf_project_colors(
            _lib.ptr(vertices), V, _lib.ptr(image), H, W, (ctypes.c_double * 12)(*w2c.reshape(-1).tolist()),
            (ctypes.c_float * 3)(*pose[:, 3].tolist()), float(np.float32(focal)), float(near), _lib.ptr(colors),
            _lib.ptr(depth), _lib.ptr(rays), _lib.stream()), "mnrf_project_colors")
    return colors, depth, rays


def fuse_vertex_colors(vertices, model, embeddings, images, poses, focal, near, N_samples=64, occ_threshold=0.2,
                       white_back=False, chunk=32 * 1024, return_sums=False):
    """Vertex colours (V, 3) uint8 by the reference's default method (extract_color_mesh.py:269-355): every view projects
    the world-space vertices into its image, samples it bilinearly, and weights the sample with 0.1 / depth plus 1 when
    the vertex is not occluded in that view -- the opacity accumulated by `render_rays({"coarse": model}, ...,
    N_importance=0, test_time=True)` along the ray from the camera to the vertex stays below `occ_threshold`.

    images: (n_views, H, W, 3) uint8 on the device; poses: (n_views, 3, 4) camera-to-world; focal in pixels; near: the
    near bound of the occlusion rays (the reference's dataset.bounds.min()).
    Differences from the reference, both because the libraries are not available to compare with: the bilinear sample is
    evaluated in float (cv2.remap rounds its weights to 1/32 and its result to uint8 per view); the final cast truncates,
    as numpy's astype(uint8) does.  return_sums: also return the float64 (color_sum (V, 3), weight_sum (V,))."""
    if not images.is_cuda or images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
        raise RuntimeError("images must be a (n_views, H, W, 3) uint8 tensor on the GPU")
    poses = np.asarray(poses.detach().cpu() if torch.is_tensor(poses) else poses, dtype=np.float32).reshape(-1, 3, 4)
    if poses.shape[0] != images.shape[0]:
        raise ValueError(f"{images.shape[0]} images but {poses.shape[0]} poses")
    vertices = vertices.contiguous()
    V, dev = int(vertices.shape[0]), vertices.device
    L, p = _lib.lib(), _lib.ptr
    with torch.cuda.device(dev), torch.no_grad():
        color_sum = torch.zeros(V, 3, dtype=torch.float64, device=dev)
        weight_sum = torch.zeros(V, dtype=torch.float64, device=dev)
        for view in range(images.shape[0]):
            colors, depth, rays = project_view(vertices, images[view], poses[view], focal, near)
            opacity = occlusion_opacity(model, embeddings, rays, N_samples, white_back, chunk)
            _lib.check(L.mnrf_accumulate_colors(p(colors), p(depth), p(opacity), float(occ_threshold), V, p(color_sum),
                                                p(weight_sum), _lib.stream()), "mnrf_accumulate_colors")
        out = (color_sum / weight_sum[:, None]).to(torch.uint8)
    return (out, color_sum, weight_sum) if return_sums else out


def occlusion_opacity(model, embeddings, rays, N_samples=64, white_back=False, chunk=32 * 1024):
    """`opacity_coarse` (V,) of the occlusion rays: the reference's `f({"coarse": nerf_fine}, ..., N_importance=0)`
    (extract_color_mesh.py:89-115, 336-347), chunked the same way."""
    from .rendering import render_rays
    out = []
    with torch.no_grad():
        for i in range(0, rays.shape[0], chunk):
            r = render_rays({"coarse": model}, embeddings, rays[i:i + chunk], N_samples, False, 0, 0, 0, chunk, white_back,
                            test_time=True)
            out.append(r["opacity_coarse"])
    return torch.cat(out, 0).float().contiguous() if out else torch.empty(0, device=rays.device)


# ----------------------------------------------------------------------------------------------- colours along the normals
def _check_mesh(vertices, triangles):
    if not vertices.is_cuda or vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise RuntimeError("vertices must be a (V, 3) float32 tensor on the GPU")
    if not triangles.is_cuda or triangles.dtype != torch.int32 or triangles.dim() != 2 or triangles.shape[1] != 3:
        raise RuntimeError("triangles must be a (T, 3) int32 tensor on the GPU")


def vertex_normals(vertices, triangles):
    """Unit vertex normals (V, 3) float32 on the device: for every triangle (a, b, c) the unnormalised cross product
    (v_b - v_a) x (v_c - v_a) in float64, summed per vertex (so: weighted by area), normalised in float64, cast.  What
    open3d's compute_vertex_normals is believed to do (extract_color_mesh.py:249; open3d is not available to compare with).
    A vertex without a triangle, or with degenerate ones only, gets (0, 0, 1).  The direction follows the winding as
    given: for the meshes of `extract_mesh` it points towards HIGHER density, in both spacing modes.  Deterministic, and
    independent of the order of the triangle array (64-bit fixed-point sums, include/mnrf.h)."""
    _check_mesh(vertices, triangles)
    vertices, triangles = vertices.contiguous(), triangles.contiguous()
    V, T, dev = int(vertices.shape[0]), int(triangles.shape[0]), vertices.device
    L, p = _lib.lib(), _lib.ptr
    with torch.cuda.device(dev):
        nbytes = L.mnrf_vertex_normals_scratch_bytes(V)
        if nbytes < 0:
            _lib.check(int(nbytes), "mnrf_vertex_normals_scratch_bytes")
        scratch = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
        normals = torch.empty(V, 3, dtype=torch.float32, device=dev)
        _lib.check(L.mnrf_vertex_normals(p(vertices), V, p(triangles) if T else None, T, p(scratch) if V else None, p(normals),
                                         _lib.stream()), "mnrf_vertex_normals")
    return normals


def normal_rays(vertices, normals, near, far, near_t=1.0):
    """One ray per vertex along its normal, (V, 8) float32 [o, d, near, far] with d = n and o = v - (d * near) * near_t:
    extract_color_mesh.py:250-253, 262 as torch evaluates it in float32 (bit-equal to that expression on the CPU)."""
    if not vertices.is_cuda or vertices.dtype != torch.float32 or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise RuntimeError("vertices must be a (V, 3) float32 tensor on the GPU")
    if not normals.is_cuda or normals.dtype != torch.float32 or normals.shape != vertices.shape:
        raise RuntimeError("normals must be a float32 tensor of the vertices' shape on the GPU")
    vertices, normals = vertices.contiguous(), normals.contiguous()
    V, dev = int(vertices.shape[0]), vertices.device
    with torch.cuda.device(dev):
        rays = torch.empty(V, 8, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().mnrf_normal_rays(_lib.ptr(vertices), _lib.ptr(normals), V, float(near), float(far), float(near_t),
                                               _lib.ptr(rays), _lib.stream()), "mnrf_normal_rays")
    return rays


def rgb_to_uint8(rgb):
    """`(rgb * 255.0).astype(np.uint8)` of extract_color_mesh.py:359-362 on the device: the float32 product truncated
    towards zero.  Where numpy's cast is undefined the value saturates to [0, 255] and a NaN becomes 0."""
    if not rgb.is_cuda or rgb.dtype != torch.float32:
        raise RuntimeError("rgb must be a float32 tensor on the GPU")
    rgb = rgb.contiguous()
    with torch.cuda.device(rgb.device):
        out = torch.empty(rgb.shape, dtype=torch.uint8, device=rgb.device)
        _lib.check(_lib.lib().mnrf_rgb_to_uint8(_lib.ptr(rgb), rgb.numel(), _lib.ptr(out), _lib.stream()), "mnrf_rgb_to_uint8")
    return out


def normal_vertex_colors(vertices, triangles, models, embeddings, near, far, near_t=1.0, N_samples=64, N_importance=128,
                         white_back=False, chunk=32 * 1024, normals=None, return_rgb=False):
    """Vertex colours (V, 3) uint8 by the reference's `--use_vertex_normal` method (extract_color_mesh.py:247-267, 358-362):
    one ray per vertex that starts `near * near_t` in front of it and travels along the vertex normal, rendered by
    `render_rays(models, ..., N_samples, False, 0, 0, N_importance, chunk, white_back, test_time=True)` in chunks;
    `rgb_fine * 255`, truncated, is the colour.  Needs nothing but the two models.

    models: {"coarse": ..., "fine": ...}; near, far: the bounds of the rays (the reference's dataset.bounds).  The ray must
    run from the outside into the surface, so the normals must point towards higher density: the winding of `extract_mesh`.
    normals: None computes them with `vertex_normals`; a (V, 3) float32 tensor is used as it is.
    Of the render only `rgb_fine` is read, so MirrorNeRF models go through the ray-fused colour / depth pass of render_rays
    (nothing per sample reaches memory; the same map bit for bit as the two-kernel route); that pass, like every forward-only
    one, does not evaluate the density-gradient normals the reference's call computes and discards, whose kernel rounds
    rgb differently by ~1e-6.  The fused pass exists for N_samples + N_importance = 192 samples per ray
    (mnrf_fused_samples_per_ray) in the split arithmetic; any other sample count, and the fp32 arithmetic, take the
    two-kernel route of render_rays with the same values.  The range guard of the split arithmetic is checked once over all
    chunks.  MirrorNeRFTcnn models take render_rays as it is.  The Whitted recursion is not traced: a mirror's
    vertices get the mirror's direct colour, as in the reference.  return_rgb: also return the float32 `rgb_fine` (V, 3)."""
    from .rendering import render_rays
    if "coarse" not in models or "fine" not in models:
        raise ValueError('models must hold "coarse" and "fine"')
    if int(N_importance) < 1:
        raise ValueError("N_importance must be positive: the colour is rgb_fine")
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be positive")
    _check_mesh(vertices, triangles)
    if normals is None:
        normals = vertex_normals(vertices, triangles)
    rays = normal_rays(vertices, normals, near, far, near_t)
    V, dev = int(rays.shape[0]), rays.device
    hashgrid = isinstance(models["coarse"], MirrorNeRFTcnn)
    extra = {} if hashgrid else dict(compute_normal=False, _guard=False, _maps_only=True, _rgb_depth_only=True)
    with torch.cuda.device(dev), torch.no_grad():
        while True:
            out = [render_rays(models, embeddings, rays[i:i + chunk], N_samples, False, 0, 0, N_importance, chunk, white_back,
                               test_time=True, **extra)["rgb_fine"] for i in range(0, V, chunk)]
            # range guard of the split arithmetic: a trip switches the models to the exact kernels; render again
            if hashgrid or not V or not _mn.check_guard(list(models.values())):
                break
        if not hashgrid and V:
            _mn.release_transient(list(models.values()))
        rgb = torch.cat(out, 0).float().contiguous() if out else torch.empty(0, 3, dtype=torch.float32, device=dev)
        colors = rgb_to_uint8(rgb)
    return (colors, rgb) if return_rgb else colors


# ----------------------------------------------------------------------------------------------- PLY
def _host(a, dtype):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a.astype(dtype, copy=False))


def write_ply(path, vertices, triangles, colors=None, normals=None):
    """Binary little-endian PLY: vertex x y z (float) [nx ny nz (float)] [red green blue (uchar)], face vertex_indices
    (uchar count + 3 int).  The layout plyfile / open3d write for the reference's meshes; plain numpy."""
    v = _host(vertices, "<f4").reshape(-1, 3)
    t = _host(triangles, "<i4").reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}",
              "property float x", "property float y", "property float z"]
    if normals is not None:
        n = _host(normals, "<f4").reshape(-1, 3)
        if len(n) != len(v):
            raise ValueError(f"{len(v)} vertices but {len(n)} normals")
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        header += ["property float nx", "property float ny", "property float nz"]
    if colors is not None:
        c = _host(colors, "u1").reshape(-1, 3)
        if len(c) != len(v):
            raise ValueError(f"{len(v)} vertices but {len(c)} colours")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header += [f"element face {len(t)}", "property list uchar int vertex_indices", "end_header"]
    vert = np.empty(len(v), dtype=fields)
    vert["x"], vert["y"], vert["z"] = v[:, 0], v[:, 1], v[:, 2]
    if normals is not None:
        vert["nx"], vert["ny"], vert["nz"] = n[:, 0], n[:, 1], n[:, 2]
    if colors is not None:
        vert["red"], vert["green"], vert["blue"] = c[:, 0], c[:, 1], c[:, 2]
    face = np.empty(len(t), dtype=[("n", "u1"), ("vertex_indices", "<i4", (3,))])
    face["n"] = 3
    face["vertex_indices"] = t
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(vert.tobytes())
        f.write(face.tobytes())


def read_ply(path, return_normals=False):
    """Reads what write_ply wrote (binary little-endian, float xyz, optional float normals, optional uchar rgb, triangles as
    `uchar int` lists): (vertices (V, 3) float32, triangles (T, 3) int32, colors (V, 3) uint8 or None), and with
    return_normals=True the normals (V, 3) float32 or None as a fourth value."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError(f"{path}: not a binary little-endian PLY")
    counts, props, cur = {}, {}, None
    for ln in lines[2:]:
        w = ln.split()
        if w[:1] == ["element"]:
            cur = w[1]
            counts[cur], props[cur] = int(w[2]), []
        elif w[:1] == ["property"]:
            props[cur].append(tuple(w[1:]))
    want = [("float", "x"), ("float", "y"), ("float", "z")]
    nrm = [("float", "nx"), ("float", "ny"), ("float", "nz")]
    rgb = [("uchar", "red"), ("uchar", "green"), ("uchar", "blue")]
    layouts = [(want + (nrm if n else []) + (rgb if c else []), n, c) for n in (False, True) for c in (False, True)]
    found = [(n, c) for layout, n, c in layouts if props.get("vertex") == layout]
    if not found or props.get("face") != [("list", "uchar", "int", "vertex_indices")]:
        raise ValueError(f"{path}: unsupported PLY layout")
    has_normal, has_color = found[0]
    vdt = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")] if has_normal else [])
                   + ([("red", "u1"), ("green", "u1"), ("blue", "u1")] if has_color else []))
    fdt = np.dtype([("n", "u1"), ("vertex_indices", "<i4", (3,))])
    nv, nf = counts["vertex"], counts["face"]
    if len(data) != end + nv * vdt.itemsize + nf * fdt.itemsize:
        raise ValueError(f"{path}: size does not match the header")
    vert = np.frombuffer(data, dtype=vdt, count=nv, offset=end)
    face = np.frombuffer(data, dtype=fdt, count=nf, offset=end + nv * vdt.itemsize)
    if nf and not (face["n"] == 3).all():
        raise ValueError(f"{path}: only triangles are supported")
    vertices = np.stack([vert["x"], vert["y"], vert["z"]], 1).astype(np.float32)
    colors = np.stack([vert["red"], vert["green"], vert["blue"]], 1).astype(np.uint8) if has_color else None
    out = (vertices, face["vertex_indices"].astype(np.int32).reshape(-1, 3), colors)
    if return_normals:
        out += (np.stack([vert["nx"], vert["ny"], vert["nz"]], 1).astype(np.float32) if has_normal else None,)
    return out
