// mnrf_mesh.hip -- mesh extraction on the device (extract_color_mesh.py): the grid-point generator of the density volume,
// marching cubes with welded vertices, connected components of the mesh, the per-view colour projection, and the colouring
// along the vertex normals (area-weighted vertex normals, one ray per vertex, the uint8 cast).
//
// Marching cubes is memory-bound (one float of density per grid point, a few hundred thousand vertices out), so the kernels
// keep no per-point intermediate but one: a point OWNS its +x, +y and +z edges, a cell is owned by its lowest corner, and
// one thread handles one point in flat (z fastest) order.  The count launch leaves two numbers per block of 256 points; the
// caller scans those (64 K numbers at 256^3); the emit launches repeat the classification and scan inside the block.  The
// welded vertex index of an edge is `vertex_base[owner point]` + the edge's rank among the owner's crossed edges; that
// array (one int32 per point: 29 bits of index, 3 bits of crossed-edge flags) is the only per-point intermediate, written by
// the vertex launch and read by the triangle launch for active cells only.  Nothing is claimed with an atomic, so the
// order of the output is the flat order of the volume and two runs agree to the bit.
// Compiled with -ffp-contract=off: every expression below is evaluated as written.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdint.h>

#include "../../include/mnrf.h"
#include "mnrf_error.h"
#include "mnrf_fill.h"

namespace {

constexpr int MC_BLOCK = 256;
constexpr long long MC_MAX_POINTS = 1ll << 30;
constexpr long long MC_MAX_VERTICES = 1ll << 29;      // vertex_base keeps the index in 29 bits

const int8_t h_mc_table[256][16] = {
#include "mnrf_mc_table.inc"
};
__device__ const int8_t d_mc_table[256][16] = {
#include "mnrf_mc_table.inc"
};

inline unsigned blocks_for(long long n, int threads) { return (unsigned)((n + threads - 1) / threads); }

// ------------------------------------------------------------------------------------------------ grid points
struct GridArgs {
    double lo[3], hi[3], delta[3], step[3];      // per axis x, y, z
    int n;
    long long start, count;
    float* out;
};

// numpy.linspace(lo, hi, n) in float64: i * step + lo with step = (hi - lo) / (n - 1), the last sample set to hi, and
// (i / (n - 1)) * delta + lo when the step is zero
__device__ inline float linspace_at(const GridArgs& A, int axis, int i) {
    if (i == A.n - 1) return (float)A.hi[axis];
    const double di = (double)i;
    const double v = A.step[axis] != 0.0 ? di * A.step[axis] : (di / (double)(A.n - 1)) * A.delta[axis];
    return (float)(v + A.lo[axis]);
}

// numpy.meshgrid(x, y, z) in "xy" order, stacked and flattened: the flat index runs y, x, z from slow to fast
__global__ __launch_bounds__(256) void grid_points_kernel(GridArgs A) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= A.count) return;
    const long long f = A.start + t;
    const int iz = (int)(f % A.n);
    const long long q = f / A.n;
    const int ix = (int)(q % A.n);
    const int iy = (int)(q / A.n);
    float* o = A.out + t * 3;
    o[0] = linspace_at(A, 0, ix);
    o[1] = linspace_at(A, 1, iy);
    o[2] = linspace_at(A, 2, iz);
}

// sigma = max(sigma, 0) (extract_color_mesh.py:185); a NaN stays a NaN, as under numpy.maximum
__global__ __launch_bounds__(256) void clamp_zero_kernel(float* x, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    x[i] = v < 0.f ? 0.f : v;
}

// ------------------------------------------------------------------------------------------------ marching cubes
struct McArgs {
    const float* vol;
    int nx, ny, nz;
    float thr;
    long long npts;
};

struct McPoint {
    int i, j, k;
    float s0;
    bool in0;
};

__device__ inline McPoint mc_point(const McArgs& A, long long p) {
    McPoint P;
    P.k = (int)(p % A.nz);
    const long long q = p / A.nz;
    P.j = (int)(q % A.ny);
    P.i = (int)(q / A.ny);
    P.s0 = A.vol[p];
    P.in0 = P.s0 >= A.thr;
    return P;
}

// bit a set <=> the edge from this point to its +axis-a neighbour exists and its ends differ
__device__ inline unsigned mc_edge_flags(const McArgs& A, long long p, const McPoint& P, float s1[3]) {
    const long long sx = (long long)A.ny * A.nz, sy = A.nz;
    unsigned f = 0;
    if (P.i + 1 < A.nx) { s1[0] = A.vol[p + sx]; f |= ((s1[0] >= A.thr) != P.in0) ? 1u : 0u; }
    if (P.j + 1 < A.ny) { s1[1] = A.vol[p + sy]; f |= ((s1[1] >= A.thr) != P.in0) ? 2u : 0u; }
    if (P.k + 1 < A.nz) { s1[2] = A.vol[p + 1];  f |= ((s1[2] >= A.thr) != P.in0) ? 4u : 0u; }
    return f;
}

// case index of the cell whose lowest corner is this point (bit c <=> corner c inside); 0 where there is no cell
__device__ inline int mc_cell_case(const McArgs& A, long long p, const McPoint& P) {
    if (P.i + 1 >= A.nx || P.j + 1 >= A.ny || P.k + 1 >= A.nz) return 0;
    const long long sx = (long long)A.ny * A.nz, sy = A.nz;
    int c = P.in0 ? 1 : 0;
    c |= (A.vol[p + sx] >= A.thr) ? 2 : 0;
    c |= (A.vol[p + sy] >= A.thr) ? 4 : 0;
    c |= (A.vol[p + sx + sy] >= A.thr) ? 8 : 0;
    c |= (A.vol[p + 1] >= A.thr) ? 16 : 0;
    c |= (A.vol[p + sx + 1] >= A.thr) ? 32 : 0;
    c |= (A.vol[p + sy + 1] >= A.thr) ? 64 : 0;
    c |= (A.vol[p + sx + sy + 1] >= A.thr) ? 128 : 0;
    return c;
}

__device__ inline int mc_case_triangles(int c) {
    if (c == 0 || c == 255) return 0;
    int n = 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) n += d_mc_table[c][3 * t] >= 0 ? 1 : 0;
    return n;
}

// exclusive scan of x over the 256 threads of the block (4 waves of 64); *total = the block's sum
__device__ inline unsigned block_scan_exclusive(unsigned x, unsigned* total) {
    __shared__ unsigned wave_sum[MC_BLOCK / 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned inc = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned y = __shfl_up(inc, d);
        if (lane >= d) inc += y;
    }
    __syncthreads();      // (a second scan in the same kernel must not overwrite wave_sum early)
    if (lane == 63) wave_sum[w] = inc;
    __syncthreads();
    unsigned base = 0, tot = 0;
#pragma unroll
    for (int q = 0; q < MC_BLOCK / 64; ++q) {
        if (q < w) base += wave_sum[q];
        tot += wave_sum[q];
    }
    *total = tot;
    return base + inc - x;
}

// per block: [crossed owned edges, triangles]; the two counts share one scan (vertices in the low 16 bits: <= 768 a block)
__global__ __launch_bounds__(MC_BLOCK) void mc_count_kernel(McArgs A, int32_t* block_counts) {
    const long long p = (long long)blockIdx.x * MC_BLOCK + threadIdx.x;
    unsigned packed = 0;
    if (p < A.npts) {
        const McPoint P = mc_point(A, p);
        float s1[3];
        packed = __popc(mc_edge_flags(A, p, P, s1)) | ((unsigned)mc_case_triangles(mc_cell_case(A, p, P)) << 16);
    }
    unsigned total;
    block_scan_exclusive(packed, &total);
    if (threadIdx.x == 0) {
        block_counts[2 * (long long)blockIdx.x + 0] = (int32_t)(total & 0xffffu);
        block_counts[2 * (long long)blockIdx.x + 1] = (int32_t)(total >> 16);
    }
}

// vertices of the crossed edges this point owns, in axis order, at the block's scanned offset + the offset in the block
__global__ __launch_bounds__(MC_BLOCK) void mc_vertices_kernel(McArgs A, const int32_t* block_offsets, int32_t* vertex_base,
                                                              long long n_vertices, float* vertices) {
    const long long p = (long long)blockIdx.x * MC_BLOCK + threadIdx.x;
    unsigned flags = 0;
    McPoint P = {};
    float s1[3] = {0.f, 0.f, 0.f};
    if (p < A.npts) {
        P = mc_point(A, p);
        flags = mc_edge_flags(A, p, P, s1);
    }
    unsigned total;
    const unsigned local = block_scan_exclusive(__popc(flags), &total);
    if (p >= A.npts) return;
    const long long base = (long long)block_offsets[2 * (long long)blockIdx.x] + local;
    vertex_base[p] = (int32_t)(((unsigned)base & 0x1fffffffu) | (flags << 29));
    long long v = base;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!(flags & (1u << a))) continue;
        if (v >= 0 && v < n_vertices) {
            // from the lower-index end: both cells that share the edge read the vertex the owner wrote
            const float t = (A.thr - P.s0) / (s1[a] - P.s0);
            float pos[3] = {(float)P.i, (float)P.j, (float)P.k};
            pos[a] = pos[a] + t;
            vertices[v * 3 + 0] = pos[0];
            vertices[v * 3 + 1] = pos[1];
            vertices[v * 3 + 2] = pos[2];
        }
        ++v;
    }
}

// triangles of the cell this point owns: table order, each corner the welded index of its edge
__global__ __launch_bounds__(MC_BLOCK) void mc_triangles_kernel(McArgs A, const int32_t* block_offsets, const int32_t* vertex_base,
                                                               long long n_triangles, int32_t* triangles) {
    const long long p = (long long)blockIdx.x * MC_BLOCK + threadIdx.x;
    int c = 0, nt = 0;
    if (p < A.npts) {
        const McPoint P = mc_point(A, p);
        c = mc_cell_case(A, p, P);
        nt = mc_case_triangles(c);
    }
    unsigned total;
    const unsigned local = block_scan_exclusive((unsigned)nt, &total);
    if (nt == 0) return;
    const long long sx = (long long)A.ny * A.nz, sy = A.nz;
    const long long stride[3] = {sx, sy, 1};
    const long long base = (long long)block_offsets[2 * (long long)blockIdx.x + 1] + local;
    for (int t = 0; t < nt; ++t) {
        const long long out = base + t;
        if (out < 0 || out >= n_triangles) break;
        for (int q = 0; q < 3; ++q) {
            // edge e: axis a = e / 4; its lower end sits at offsets (k & 1, k >> 1), k = e % 4, along the two other axes
            const int e = d_mc_table[c][3 * t + q];
            const int a = e >> 2, k = e & 3;
            const int o0 = a == 0 ? 1 : 0, o1 = a == 2 ? 1 : 2;
            const long long owner = p + (k & 1) * stride[o0] + (k >> 1) * stride[o1];      // inside the cell: in bounds
            const unsigned w = (unsigned)vertex_base[owner];
            triangles[out * 3 + q] = (int32_t)((w & 0x1fffffffu) + __popc((w >> 29) & ((1u << a) - 1u)));
        }
    }
}

// ------------------------------------------------------------------------------------------------ connected components
// Union-find over the vertices.  labels[v] <= v always: a root is hooked under a smaller root with a (vector-memory)
// atomic min, so every chain descends and ends in a root, and the root of a finished component is its smallest vertex.
__device__ inline int cc_find(const int32_t* labels, int x) {
    for (;;) {
        const int p = __atomic_load_n(&labels[x], __ATOMIC_RELAXED);
        if (p == x) return x;
        x = p;
    }
}

__device__ inline void cc_hook_pair(int32_t* labels, int u, int v, int32_t* changed) {
    const int ru = cc_find(labels, u), rv = cc_find(labels, v);
    if (ru == rv) return;
    // a hook that loses the race against a smaller one leaves its two trees apart: the flag asks for another round
    atomicMin(&labels[ru > rv ? ru : rv], ru > rv ? rv : ru);
    *changed = 1;
}

__global__ __launch_bounds__(256) void cc_init_kernel(int32_t* labels, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) labels[i] = (int32_t)i;
}

__global__ __launch_bounds__(256) void cc_hook_kernel(const int32_t* tri, long long n_tri, int32_t* labels, long long n_vert,
                                                      int32_t* changed) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tri) return;
    const int a = tri[t * 3 + 0], b = tri[t * 3 + 1], c = tri[t * 3 + 2];
    if (a < 0 || b < 0 || c < 0 || a >= n_vert || b >= n_vert || c >= n_vert) return;      // (refused: never index out of bounds)
    cc_hook_pair(labels, a, b, changed);
    cc_hook_pair(labels, b, c, changed);
}

// pointer jumping: every vertex points at its root
__global__ __launch_bounds__(256) void cc_jump_kernel(int32_t* labels, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int r = cc_find(labels, (int)i);
    __atomic_store_n(&labels[i], r, __ATOMIC_RELAXED);
}

// triangles per label (the label of a triangle is the label of its first vertex); integer adds: the order is immaterial
__global__ __launch_bounds__(256) void cc_count_kernel(const int32_t* tri, long long n_tri, const int32_t* labels, long long n_vert,
                                                       int32_t* counts) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tri) return;
    const int a = tri[t * 3 + 0], b = tri[t * 3 + 1], c = tri[t * 3 + 2];
    if (a < 0 || b < 0 || c < 0 || a >= n_vert || b >= n_vert || c >= n_vert) return;      // (refused, as cc_hook_kernel refuses it)
    const int l = labels[a];
    if (l < 0 || l >= n_vert) return;
    atomicAdd(&counts[l], 1);
}

// ------------------------------------------------------------------------------------------------ vertex colours
struct ProjectArgs {
    const float* vertices;
    long long n;
    const uint8_t* image;
    int H, W;
    double w2c[12];
    float origin[3];
    float focal, near;
    float* colors;
    double* depth;
    float* rays;
};

// extract_color_mesh.py:285-301 (projection, in float64 as numpy evaluates it), 303-317 (bilinear sample; in float here),
// 326-335 (the occlusion ray from the camera to the vertex, far = the vertex's depth)
__global__ __launch_bounds__(256) void project_colors_kernel(ProjectArgs A) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const float vx = A.vertices[i * 3 + 0], vy = A.vertices[i * 3 + 1], vz = A.vertices[i * 3 + 2];
    double cam[3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
        cam[r] = A.w2c[r * 4 + 0] * (double)vx + A.w2c[r * 4 + 1] * (double)vy + A.w2c[r * 4 + 2] * (double)vz + A.w2c[r * 4 + 3];
    cam[1] = -cam[1];      // "right up back" -> "right down forward"
    cam[2] = -cam[2];
    const double f = (double)A.focal;
    const double u = f * cam[0] + (double)(0.5f * (float)A.W) * cam[2];
    const double v = f * cam[1] + (double)(0.5f * (float)A.H) * cam[2];
    const double depth = cam[2] + 1e-5;
    // clipped to the image, not dropped (a NaN coordinate, depth == 0, lands on pixel 0)
    const float px = fminf(fmaxf((float)(u / depth), 0.f), (float)(A.W - 1));
    const float py = fminf(fmaxf((float)(v / depth), 0.f), (float)(A.H - 1));
    const float x0f = floorf(px), y0f = floorf(py);
    const float fx = px - x0f, fy = py - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const int x1 = x0 + 1 < A.W ? x0 + 1 : A.W - 1, y1 = y0 + 1 < A.H ? y0 + 1 : A.H - 1;
    const uint8_t* p00 = A.image + ((long long)y0 * A.W + x0) * 3;
    const uint8_t* p01 = A.image + ((long long)y0 * A.W + x1) * 3;
    const uint8_t* p10 = A.image + ((long long)y1 * A.W + x0) * 3;
    const uint8_t* p11 = A.image + ((long long)y1 * A.W + x1) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float top = (1.f - fx) * (float)p00[c] + fx * (float)p01[c];
        const float bot = (1.f - fx) * (float)p10[c] + fx * (float)p11[c];
        A.colors[i * 3 + c] = (1.f - fy) * top + fy * bot;
    }
    A.depth[i] = depth;
    const float dx = vx - A.origin[0], dy = vy - A.origin[1], dz = vz - A.origin[2];
    const float len = sqrtf(dx * dx + dy * dy + dz * dz);
    float* r = A.rays + i * 8;
    r[0] = A.origin[0];
    r[1] = A.origin[1];
    r[2] = A.origin[2];
    r[3] = dx / len;
    r[4] = dy / len;
    r[5] = dz / len;
    r[6] = A.near;
    r[7] = (float)depth;
}

// extract_color_mesh.py:346-355: w = 0.1 / depth + (opacity < occ_threshold), sums of colour * w and w in float64.
// numpy.nan_to_num(opacity, 1) as the reference calls it: the second positional parameter is `copy`, so a NaN becomes 0
// (and counts as unoccluded) and +-inf the largest finite float.
__global__ __launch_bounds__(256) void accumulate_colors_kernel(const float* colors, const double* depth, const float* opacity,
                                                                float occ_threshold, long long n, double* color_sum,
                                                                double* weight_sum) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float op = opacity[i];
    if (op != op) op = 0.f;
    else if (isinf(op)) op = op > 0.f ? 3.4028234663852886e38f : -3.4028234663852886e38f;
    const double w = 0.1 / depth[i] + (op < occ_threshold ? 1.0 : 0.0);
#pragma unroll
    for (int c = 0; c < 3; ++c) color_sum[i * 3 + c] = color_sum[i * 3 + c] + (double)colors[i * 3 + c] * w;
    weight_sum[i] = weight_sum[i] + w;
}

// ------------------------------------------------------------------------------------------------ vertex normals
// normal(v) = normalise(sum over the triangles (a, b, c) that hold v of (v_b - v_a) x (v_c - v_a)), float64 from the float32
// vertices.  The sum is order-free because it is an integer sum: every cross-product component is rounded to a multiple of
// 2^-k and added as a 64-bit integer with a vector-memory atomic.  k comes from the mesh itself: M = the largest finite
// |component| of any cross product (a first pass, an integer atomic max over the bits of the non-negative doubles), M < 2^e,
// 3 T < 2^b contributions at most per accumulator, k = 62 - e - b, so |sum| < 2^62 and the rounding (half a step per
// contribution) keeps it below 2^63.  One step is at most M * 2^(b - 61): with T = 2 M triangles 2^-38 of the largest cross
// product.  A triangle with a non-finite corner marks its three vertices instead (finite float32 corners cannot overflow a
// float64 cross product); those, and vertices whose sum is zero, get (0, 0, 1).
struct NormalArgs {
    const float* vertices;
    long long n_vert;
    const int32_t* tri;
    long long n_tri;
    long long* sums;                 // (n_vert, 3), zeroed
    unsigned long long* max_bits;    // the bits of M, zeroed
    uint32_t* marked;                // (n_vert), zeroed
    int count_bits;                  // b
};

// false: the triangle indexes outside [0, n_vert) and is skipped
__device__ inline bool vn_cross(const NormalArgs& A, long long t, int idx[3], double c[3]) {
    idx[0] = A.tri[t * 3 + 0];
    idx[1] = A.tri[t * 3 + 1];
    idx[2] = A.tri[t * 3 + 2];
    for (int q = 0; q < 3; ++q)
        if (idx[q] < 0 || idx[q] >= A.n_vert) return false;
    double p[3][3];
    for (int q = 0; q < 3; ++q)
        for (int a = 0; a < 3; ++a) p[q][a] = (double)A.vertices[(long long)idx[q] * 3 + a];
    const double ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
    const double wx = p[2][0] - p[0][0], wy = p[2][1] - p[0][1], wz = p[2][2] - p[0][2];
    c[0] = uy * wz - uz * wy;
    c[1] = uz * wx - ux * wz;
    c[2] = ux * wy - uy * wx;
    return true;
}

__device__ inline bool vn_finite(const double c[3]) { return isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]); }

// M: grid-stride over the triangles, one atomic per block
__global__ __launch_bounds__(256) void vn_max_kernel(NormalArgs A) {
    __shared__ double wave_max[4];
    double m = 0.0;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < A.n_tri; t += (long long)gridDim.x * blockDim.x) {
        int idx[3];
        double c[3];
        if (!vn_cross(A, t, idx, c) || !vn_finite(c)) continue;
        m = fmax(m, fmax(fabs(c[0]), fmax(fabs(c[1]), fabs(c[2]))));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmax(m, __shfl_xor(m, d));
    if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmax(fmax(wave_max[0], wave_max[1]), fmax(wave_max[2], wave_max[3]));
        if (m > 0.0) atomicMax(A.max_bits, (unsigned long long)__double_as_longlong(m));
    }
}

__global__ __launch_bounds__(256) void vn_accumulate_kernel(NormalArgs A) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= A.n_tri) return;
    int idx[3];
    double c[3];
    if (!vn_cross(A, t, idx, c)) return;
    if (!vn_finite(c)) {
        for (int q = 0; q < 3; ++q) atomicOr(&A.marked[idx[q]], 1u);
        return;
    }
    const double M = __longlong_as_double((long long)*A.max_bits);
    if (!(M > 0.0)) return;      // every triangle is degenerate
    int e;
    frexp(M, &e);                // M = m * 2^e, 0.5 <= m < 1
    const int k = 62 - e - A.count_bits;
    for (int a = 0; a < 3; ++a) {
        const long long q = __double2ll_rn(ldexp(c[a], k));
        if (q == 0) continue;
        for (int v = 0; v < 3; ++v)
            atomicAdd((unsigned long long*)&A.sums[(long long)idx[v] * 3 + a], (unsigned long long)q);
    }
}

__global__ __launch_bounds__(256) void vn_finish_kernel(NormalArgs A, float* normals) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n_vert) return;
    const double sx = (double)A.sums[i * 3 + 0], sy = (double)A.sums[i * 3 + 1], sz = (double)A.sums[i * 3 + 2];
    const double len = sqrt(sx * sx + sy * sy + sz * sz);      // (|s| < 2^62: the squares cannot overflow)
    float n[3] = {0.f, 0.f, 1.f};
    if (!A.marked[i] && len > 0.0) {
        n[0] = (float)(sx / len);
        n[1] = (float)(sy / len);
        n[2] = (float)(sz / len);
    }
    normals[i * 3 + 0] = n[0];
    normals[i * 3 + 1] = n[1];
    normals[i * 3 + 2] = n[2];
}

// extract_color_mesh.py:250-253, 262 as torch evaluates it in float32: d = n, o = v - (d * near) * near_t, [o, d, near, far]
__global__ __launch_bounds__(256) void normal_rays_kernel(const float* vertices, const float* normals, long long n, float near,
                                                          float far, float near_t, float* rays) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float* r = rays + i * 8;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float d = normals[i * 3 + a];
        const float step = d * near;
        r[a] = vertices[i * 3 + a] - step * near_t;
        r[3 + a] = d;
    }
    r[6] = near;
    r[7] = far;
}

// extract_color_mesh.py:359-362: (rgb * 255.0).astype(uint8) -- the float32 product truncated towards zero.  Outside
// [0, 256) numpy's cast is undefined; here the value saturates and a NaN becomes 0.
__global__ __launch_bounds__(256) void rgb_to_uint8_kernel(const float* rgb, long long n, uint8_t* out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = rgb[i] * 255.0f;
    out[i] = v >= 255.f ? (uint8_t)255 : (v > 0.f ? (uint8_t)(int)v : (uint8_t)0);
}

int mc_check(const char* who, const float* volume, int nx, int ny, int nz, float threshold, long long* npts) {
    static thread_local char msg[160];
    if (nx < 2 || ny < 2 || nz < 2) {
        snprintf(msg, sizeof(msg), "%s: every side of the volume needs at least 2 points", who);
        return mnrf_fail(MNRF_ERR_ARG, msg);
    }
    *npts = (long long)nx * ny * nz;
    if (*npts > MC_MAX_POINTS) {
        snprintf(msg, sizeof(msg), "%s: more than 2^30 grid points", who);
        return mnrf_fail(MNRF_ERR_ARG, msg);
    }
    if (!(threshold == threshold)) {
        snprintf(msg, sizeof(msg), "%s: the threshold is NaN", who);
        return mnrf_fail(MNRF_ERR_ARG, msg);
    }
    if (!volume) {
        snprintf(msg, sizeof(msg), "%s: null volume", who);
        return mnrf_fail(MNRF_ERR_ARG, msg);
    }
    return MNRF_OK;
}

}  // namespace

extern "C" int mnrf_grid_points(double x0, double x1, double y0, double y1, double z0, double z1, int n, int64_t start,
                                int64_t count, float* out, void* stream) {
    if (n < 2) return mnrf_fail(MNRF_ERR_ARG, "mnrf_grid_points: N must be at least 2");
    if (n > 2048) return mnrf_fail(MNRF_ERR_ARG, "mnrf_grid_points: N must be at most 2048");
    const long long total = (long long)n * n * n;
    if (start < 0 || count < 0 || start > total || count > total - start)
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_grid_points: [start, start + count) must lie inside the N^3 points");
    if (count == 0) return MNRF_OK;
    if (!out) return mnrf_fail(MNRF_ERR_ARG, "mnrf_grid_points: null pointer");
    GridArgs A;
    const double lo[3] = {x0, y0, z0}, hi[3] = {x1, y1, z1};
    for (int a = 0; a < 3; ++a) {
        A.lo[a] = lo[a];
        A.hi[a] = hi[a];
        A.delta[a] = hi[a] - lo[a];
        A.step[a] = A.delta[a] / (double)(n - 1);
    }
    A.n = n;
    A.start = start;
    A.count = count;
    A.out = out;
    hipLaunchKernelGGL(grid_points_kernel, dim3(blocks_for(count, 256)), dim3(256), 0, (hipStream_t)stream, A);
    return mnrf_check_launch("mnrf_grid_points");
}

extern "C" int mnrf_clamp_zero(float* x, int64_t n, void* stream) {
    if (n < 0) return mnrf_fail(MNRF_ERR_ARG, "mnrf_clamp_zero: bad size");
    if (n == 0) return MNRF_OK;
    if (!x) return mnrf_fail(MNRF_ERR_ARG, "mnrf_clamp_zero: null pointer");
    hipLaunchKernelGGL(clamp_zero_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, x, (long long)n);
    return mnrf_check_launch("mnrf_clamp_zero");
}

extern "C" int mnrf_mc_table(int case_index, int8_t* out16) {
    if (case_index < 0 || case_index > 255) return mnrf_fail(MNRF_ERR_ARG, "mnrf_mc_table: the case index runs from 0 to 255");
    if (!out16) return mnrf_fail(MNRF_ERR_ARG, "mnrf_mc_table: null pointer");
    for (int k = 0; k < 16; ++k) out16[k] = h_mc_table[case_index][k];
    return MNRF_OK;
}

extern "C" int64_t mnrf_mc_blocks(int nx, int ny, int nz) {
    if (nx < 2 || ny < 2 || nz < 2) return mnrf_fail(MNRF_ERR_ARG, "mnrf_mc_blocks: every side of the volume needs at least 2 points");
    const long long npts = (long long)nx * ny * nz;
    if (npts > MC_MAX_POINTS) return mnrf_fail(MNRF_ERR_ARG, "mnrf_mc_blocks: more than 2^30 grid points");
    return (npts + MC_BLOCK - 1) / MC_BLOCK;
}

extern "C" int mnrf_mc_count(const float* volume, int nx, int ny, int nz, float threshold, int32_t* block_counts, void* stream) {
    long long npts = 0;
    const int rc = mc_check("mnrf_mc_count", volume, nx, ny, nz, threshold, &npts);
    if (rc != MNRF_OK) return rc;
    if (!block_counts) return mnrf_fail(MNRF_ERR_ARG, "mnrf_mc_count: null block_counts");
    const McArgs A{volume, nx, ny, nz, threshold, npts};
    hipLaunchKernelGGL(mc_count_kernel, dim3(blocks_for(npts, MC_BLOCK)), dim3(MC_BLOCK), 0, (hipStream_t)stream, A, block_counts);
    return mnrf_check_launch("mnrf_mc_count");
}

extern "C" int mnrf_mc_emit(const float* volume, int nx, int ny, int nz, float threshold, const int32_t* block_offsets,
                            int32_t* vertex_base, int64_t n_vertices, int64_t n_triangles, float* vertices, int32_t* triangles,
                            void* stream) {
    long long npts = 0;
    const int rc = mc_check("mnrf_mc_emit", volume, nx, ny, nz, threshold, &npts);
    if (rc != MNRF_OK) return rc;
    if (n_vertices < 0 || n_triangles < 0 || n_vertices > MC_MAX_VERTICES)
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_mc_emit: vertex / triangle count out of range (at most 2^29 vertices)");
    if (n_vertices == 0 && n_triangles == 0) return MNRF_OK;
    if (!block_offsets || !vertex_base) return mnrf_fail(MNRF_ERR_ARG, "mnrf_mc_emit: null block_offsets / vertex_base");
    if ((n_vertices > 0 && !vertices) || (n_triangles > 0 && !triangles))
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_mc_emit: null output");
    const McArgs A{volume, nx, ny, nz, threshold, npts};
    hipLaunchKernelGGL(mc_vertices_kernel, dim3(blocks_for(npts, MC_BLOCK)), dim3(MC_BLOCK), 0, (hipStream_t)stream, A,
                       block_offsets, vertex_base, (long long)n_vertices, vertices);
    if (n_triangles > 0)
        hipLaunchKernelGGL(mc_triangles_kernel, dim3(blocks_for(npts, MC_BLOCK)), dim3(MC_BLOCK), 0, (hipStream_t)stream, A,
                           block_offsets, (const int32_t*)vertex_base, (long long)n_triangles, triangles);
    return mnrf_check_launch("mnrf_mc_emit");
}

extern "C" int mnrf_cc_init(int32_t* labels, int64_t n_vertices, void* stream) {
    if (n_vertices < 0 || n_vertices > MC_MAX_VERTICES) return mnrf_fail(MNRF_ERR_ARG, "mnrf_cc_init: bad size");
    if (n_vertices == 0) return MNRF_OK;
    if (!labels) return mnrf_fail(MNRF_ERR_ARG, "mnrf_cc_init: null pointer");
    hipLaunchKernelGGL(cc_init_kernel, dim3(blocks_for(n_vertices, 256)), dim3(256), 0, (hipStream_t)stream, labels,
                       (long long)n_vertices);
    return mnrf_check_launch("mnrf_cc_init");
}

extern "C" int mnrf_cc_step(const int32_t* triangles, int64_t n_triangles, int32_t* labels, int64_t n_vertices, int32_t* changed,
                            void* stream) {
    if (n_triangles < 0 || n_vertices < 0 || n_vertices > MC_MAX_VERTICES) return mnrf_fail(MNRF_ERR_ARG, "mnrf_cc_step: bad size");
    if (n_triangles == 0 || n_vertices == 0) return MNRF_OK;
    if (!triangles || !labels || !changed) return mnrf_fail(MNRF_ERR_ARG, "mnrf_cc_step: null pointer");
    hipLaunchKernelGGL(cc_hook_kernel, dim3(blocks_for(n_triangles, 256)), dim3(256), 0, (hipStream_t)stream, triangles,
                       (long long)n_triangles, labels, (long long)n_vertices, changed);
    hipLaunchKernelGGL(cc_jump_kernel, dim3(blocks_for(n_vertices, 256)), dim3(256), 0, (hipStream_t)stream, labels,
                       (long long)n_vertices);
    return mnrf_check_launch("mnrf_cc_step");
}

extern "C" int mnrf_cc_count(const int32_t* triangles, int64_t n_triangles, const int32_t* labels, int64_t n_vertices,
                             int32_t* counts, void* stream) {
    if (n_triangles < 0 || n_vertices < 0 || n_vertices > MC_MAX_VERTICES) return mnrf_fail(MNRF_ERR_ARG, "mnrf_cc_count: bad size");
    if (n_triangles == 0 || n_vertices == 0) return MNRF_OK;
    if (!triangles || !labels || !counts) return mnrf_fail(MNRF_ERR_ARG, "mnrf_cc_count: null pointer");
    hipLaunchKernelGGL(cc_count_kernel, dim3(blocks_for(n_triangles, 256)), dim3(256), 0, (hipStream_t)stream, triangles,
                       (long long)n_triangles, labels, (long long)n_vertices, counts);
    return mnrf_check_launch("mnrf_cc_count");
}

extern "C" int mnrf_project_colors(const float* vertices, int64_t n_vertices, const uint8_t* image, int H, int W,
                                   const double* w2c_host12, const float* origin_host3, float focal, float near, float* colors,
                                   double* depth, float* rays, void* stream) {
    if (n_vertices < 0 || H < 1 || W < 1 || H > 32768 || W > 32768) return mnrf_fail(MNRF_ERR_ARG, "mnrf_project_colors: bad size");
    if (!w2c_host12 || !origin_host3) return mnrf_fail(MNRF_ERR_ARG, "mnrf_project_colors: null camera");
    if (n_vertices == 0) return MNRF_OK;
    if (!vertices || !image || !colors || !depth || !rays) return mnrf_fail(MNRF_ERR_ARG, "mnrf_project_colors: null pointer");
    ProjectArgs A;
    A.vertices = vertices;
    A.n = n_vertices;
    A.image = image;
    A.H = H;
    A.W = W;
    for (int k = 0; k < 12; ++k) A.w2c[k] = w2c_host12[k];
    for (int k = 0; k < 3; ++k) A.origin[k] = origin_host3[k];
    A.focal = focal;
    A.near = near;
    A.colors = colors;
    A.depth = depth;
    A.rays = rays;
    hipLaunchKernelGGL(project_colors_kernel, dim3(blocks_for(n_vertices, 256)), dim3(256), 0, (hipStream_t)stream, A);
    return mnrf_check_launch("mnrf_project_colors");
}

extern "C" int mnrf_accumulate_colors(const float* colors, const double* depth, const float* opacity, float occ_threshold,
                                      int64_t n_vertices, double* color_sum, double* weight_sum, void* stream) {
    if (n_vertices < 0) return mnrf_fail(MNRF_ERR_ARG, "mnrf_accumulate_colors: bad size");
    if (n_vertices == 0) return MNRF_OK;
    if (!colors || !depth || !opacity || !color_sum || !weight_sum)
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_accumulate_colors: null pointer");
    hipLaunchKernelGGL(accumulate_colors_kernel, dim3(blocks_for(n_vertices, 256)), dim3(256), 0, (hipStream_t)stream, colors, depth,
                       opacity, occ_threshold, (long long)n_vertices, color_sum, weight_sum);
    return mnrf_check_launch("mnrf_accumulate_colors");
}

extern "C" int64_t mnrf_vertex_normals_scratch_bytes(int64_t n_vertices) {
    if (n_vertices < 0 || n_vertices > MC_MAX_VERTICES)
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_vertex_normals_scratch_bytes: bad size (at most 2^29 vertices)");
    return ((24 * n_vertices + 8 + 4 * n_vertices + 7) / 8) * 8;
}

extern "C" int mnrf_vertex_normals(const float* vertices, int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                                   void* scratch, float* normals, void* stream) {
    if (n_vertices < 0 || n_vertices > MC_MAX_VERTICES || n_triangles < 0 || n_triangles > (1ll << 31) / 3)
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_vertex_normals: bad size (at most 2^29 vertices, 2^31 / 3 triangles)");
    if (n_vertices == 0) return MNRF_OK;
    if (!vertices || !scratch || !normals || (n_triangles > 0 && !triangles))
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_vertex_normals: null pointer");
    if (((uintptr_t)scratch & 7u) != 0) return mnrf_fail(MNRF_ERR_ARG, "mnrf_vertex_normals: scratch must be 8-byte aligned");
    NormalArgs A;
    A.vertices = vertices;
    A.n_vert = n_vertices;
    A.tri = triangles;
    A.n_tri = n_triangles;
    A.sums = (long long*)scratch;
    A.max_bits = (unsigned long long*)scratch + 3 * n_vertices;
    A.marked = (uint32_t*)((unsigned long long*)scratch + 3 * n_vertices + 1);
    A.count_bits = 0;
    for (long long c = 3 * (long long)n_triangles; c > 0; c >>= 1) ++A.count_bits;      // 3 T < 2^count_bits
    hipStream_t s = (hipStream_t)stream;
    mnrf::zero_fill(s, scratch, (size_t)(24 * n_vertices + 8 + 4 * n_vertices));
    if (n_triangles > 0) {
        unsigned blocks = blocks_for(n_triangles, 256);
        hipLaunchKernelGGL(vn_max_kernel, dim3(blocks > 1024u ? 1024u : blocks), dim3(256), 0, s, A);
        hipLaunchKernelGGL(vn_accumulate_kernel, dim3(blocks), dim3(256), 0, s, A);
    }
    hipLaunchKernelGGL(vn_finish_kernel, dim3(blocks_for(n_vertices, 256)), dim3(256), 0, s, A, normals);
    return mnrf_check_launch("mnrf_vertex_normals");
}

extern "C" int mnrf_normal_rays(const float* vertices, const float* normals, int64_t n_vertices, float near, float far,
                                float near_t, float* rays, void* stream) {
    if (n_vertices < 0) return mnrf_fail(MNRF_ERR_ARG, "mnrf_normal_rays: bad size");
    if (n_vertices == 0) return MNRF_OK;
    if (!vertices || !normals || !rays) return mnrf_fail(MNRF_ERR_ARG, "mnrf_normal_rays: null pointer");
    hipLaunchKernelGGL(normal_rays_kernel, dim3(blocks_for(n_vertices, 256)), dim3(256), 0, (hipStream_t)stream, vertices, normals,
                       (long long)n_vertices, near, far, near_t, rays);
    return mnrf_check_launch("mnrf_normal_rays");
}

extern "C" int mnrf_rgb_to_uint8(const float* rgb, int64_t n, uint8_t* out, void* stream) {
    if (n < 0) return mnrf_fail(MNRF_ERR_ARG, "mnrf_rgb_to_uint8: bad size");
    if (n == 0) return MNRF_OK;
    if (!rgb || !out) return mnrf_fail(MNRF_ERR_ARG, "mnrf_rgb_to_uint8: null pointer");
    hipLaunchKernelGGL(rgb_to_uint8_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, (hipStream_t)stream, rgb, (long long)n, out);
    return mnrf_check_launch("mnrf_rgb_to_uint8");
}
