// mnrf_frames.hip -- the output stage of eval.py on the device: the 8-bit images of a rendered frame and its depth colour
// maps (eval.py:743-978 with utils/visualization.py:10-23, 208-221), from the float32 maps batched_inference leaves there.
//
// Two launches per frame, no host read between them or after them:
//   frame_extrema_kernel   the extremes the images are normalised by, into the caller's stats block, and the frame's raw
//                          depth extremes folded into the caller's split-wide running block
//   frame_finish_kernel    every requested (n, 3) uint8 image, read in place from the float maps
// and one more for the second pass over a split (save_depth_unified_normalization):
//   depth_colormap_kernel  a stack of (F, n) resident depth maps coloured with one pair of extremes read from the device
// and two for the validation panel of the training loop (utils/visualization.py:26-184; stated where they are defined, below):
//   panel_extrema_kernel, panel_write_kernel    the (N_pics, 3, H, W) float32 stack of visualize_val_image(add_text=False)
//
// ARITHMETIC.  Every image is the reference's expression, one IEEE fp32 operation after the other in its order (compiled with
// -ffp-contract=off, hipcc's correctly rounded fp32 division, no fast-math), so the bytes are numpy's:
//   u8(v)          astype(np.uint8) of a value inside [0, 256): truncation.  Outside it numpy leaves the result to the
//                  platform; here NaN and anything below 0 give 0 and anything from 256 up gives 255.
//   clip(v, a, b)  np.minimum(np.maximum(v, a), b); a NaN stays a NaN (and becomes byte 0)
//   n2n(v)         np.nan_to_num: NaN -> 0, +inf -> FLT_MAX, -inf -> -FLT_MAX
//   rgb            u8(clip(rgb, 0, 1) * 255)
//   mirror_mask    u8(clip(m, 0, 1) * 255) in all three channels
//   normals        u8(clip((v + 1) / 2, 0, 1) * 255)
//   x_surface      mn == mx ? 255 : u8(clip((v - mn) / (mx - mn), 0, 1) * 255); mn, mx over all 3 n values, NaN propagating
//                  (torch.min / torch.max)
//   depth          x = clip(n2n(d), mi, ma); x = (x - mi) / (1e-8f > ma - mi ? 1e-8f : ma - mi); k = u8(255 * x);
//                  byte c = u8((float(T[k][c]) / 255.0f) * 255.0f)       (T: the caller's (256, 3) colour table)
//   depth_reflect  the same from the reflected depth and its extremes, byte c = u8(((float(T[k][c]) / 255.0f) * m) * 255.0f)
//                  with m = clip(mirror_mask, 0, 1)
// mi, ma are the frame's own min / max of n2n(d) (stats block), or the pair the caller points depth_colormap at.
//
// EXTREMES.  min and max do not depend on the order of reduction.  A float is mapped to an unsigned integer that orders as
// the float does (negative: all bits flipped; otherwise: sign bit set; -0 below +0; no non-NaN value maps to 0 or 2^32 - 1);
// a maximum is reduced as that key and a minimum as the key's complement, so that every accumulator is an integer maximum
// with 0 as "nothing seen".  A block reduces in registers and LDS and issues one vector-memory integer atomic per
// accumulator; the block that takes the last ticket reads the accumulators back (exchanging them for 0, so the block is ready
// for the next launch), decodes them into floats and folds the running block.  The three kinds of extremes:
//   stats[0..3]   min, max of n2n(depth), of n2n(depth_reflect)
//   stats[4..5]   min, max of x_surface; a NaN anywhere makes both NaN (torch.min / torch.max)
//   running[0..3] min, max over the frames folded so far of each frame's np.min / np.max of the RAW depth / reflected depth
//                 (infinities kept); a frame that holds a NaN has NaN extremes, and the `<` / `>` update skips them
// A null map leaves NaN in its stats entries and folds nothing.
//
// STORES.  The three-channel maps are flat arrays of 3 n floats whose bytes are an elementwise function: a thread takes 4
// consecutive floats (one 16-byte load when the map is 16-byte aligned) and stores one dword, so a wave reads 1 KiB and writes
// 256 B contiguously.  The per-pixel maps (mask, depths) give 3 bytes per float: a thread takes 4 pixels (one 16-byte load)
// and stores 12 bytes as three dwords, lane i at byte 12 i.  The tail (3 n or n not a multiple of 4) and any image whose
// address is not a multiple of 4 are written byte by byte.  Nothing is assumed about n.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "../../include/mnrf.h"
#include "mnrf_error.h"

namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int STATS_FLOATS = 32;     // [0..5] floats out, [8..17] accumulators, [18] ticket
constexpr int RUNNING_FLOATS = 4;
constexpr int ACC0 = 8, N_ACC = 10, TICKET = 18;
// accumulators: 0,1 n2n depth min/max  2,3 n2n reflect min/max  4,5 x_surface min/max  6,7 raw depth min/max  8,9 raw reflect

__device__ __forceinline__ uint32_t key_of(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float float_of(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ float n2n(float v) {
    if (v != v) return 0.f;
    if (v == __builtin_inff()) return FLT_MAX;
    if (v == -__builtin_inff()) return -FLT_MAX;
    return v;
}
__device__ __forceinline__ float np_max(float a, float b) { return (a != a) ? a : ((b != b) ? b : (a > b ? a : b)); }
__device__ __forceinline__ float np_min(float a, float b) { return (a != a) ? a : ((b != b) ? b : (a < b ? a : b)); }
__device__ __forceinline__ float clip(float v, float lo, float hi) { return np_min(np_max(v, lo), hi); }
__device__ __forceinline__ uint32_t u8(float v) { return v >= 0.f ? (v < 256.f ? (uint32_t)v : 255u) : 0u; }
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

// ---------------------------------------------------------------- extremes

struct ExtremaArgs {
    const float* depth;        // (F, n) or null
    const float* reflect;      // (F, n) or null
    const float* xs;           // (F, n, 3) or null
    long long n;
    float* stats;              // (F, STATS_FLOATS)
    float* running;            // RUNNING_FLOATS or null
};

__device__ __forceinline__ void depth_acc(float v, uint32_t* a, uint32_t* raw) {
    const uint32_t k = key_of(n2n(v));
    a[0] = umax(a[0], ~k);
    a[1] = umax(a[1], k);
    const uint32_t r = key_of(v);
    raw[0] = umax(raw[0], v != v ? 0xffffffffu : ~r);
    raw[1] = umax(raw[1], v != v ? 0xffffffffu : r);
}

__global__ __launch_bounds__(TPB) void frame_extrema_kernel(ExtremaArgs A) {
    __shared__ uint32_t red[WAVES][N_ACC];
    __shared__ int last;
    const long long f = blockIdx.y, n = A.n;
    const long long t0 = (long long)blockIdx.x * TPB + threadIdx.x, step = (long long)gridDim.x * TPB;
    uint32_t a[N_ACC];
#pragma unroll
    for (int i = 0; i < N_ACC; ++i) a[i] = 0u;
    if (A.depth) {
        const float* p = A.depth + f * n;
        for (long long i = t0; i < n; i += step) depth_acc(p[i], a + 0, a + 6);
    }
    if (A.reflect) {
        const float* p = A.reflect + f * n;
        for (long long i = t0; i < n; i += step) depth_acc(p[i], a + 2, a + 8);
    }
    if (A.xs) {
        const float* p = A.xs + f * n * 3;
        for (long long i = t0; i < 3 * n; i += step) {
            const float v = p[i];
            const uint32_t k = key_of(v);
            a[4] = umax(a[4], v != v ? 0xffffffffu : ~k);
            a[5] = umax(a[5], v != v ? 0xffffffffu : k);
        }
    }
#pragma unroll
    for (int i = 0; i < N_ACC; ++i)
        for (int o = 32; o > 0; o >>= 1) a[i] = umax(a[i], (uint32_t)__shfl_xor((int)a[i], o));
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int i = 0; i < N_ACC; ++i) red[threadIdx.x >> 6][i] = a[i];
    __syncthreads();
    uint32_t* acc = reinterpret_cast<uint32_t*>(A.stats + f * STATS_FLOATS);
    if (threadIdx.x == 0) {
        for (int i = 0; i < N_ACC; ++i) {
            uint32_t m = red[0][i];
            for (int w = 1; w < WAVES; ++w) m = umax(m, red[w][i]);
            if (m) atomicMax(acc + ACC0 + i, m);
        }
        __threadfence();
        last = atomicAdd(acc + TICKET, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last || threadIdx.x != 0) return;
    __threadfence();
    const float q = __builtin_nanf("");
    float out[N_ACC];
    for (int i = 0; i < N_ACC; ++i) {
        const uint32_t e = atomicExch(acc + ACC0 + i, 0u);       // read, and leave the accumulator ready for the next launch
        out[i] = (e == 0u || e == 0xffffffffu) ? q : float_of((i & 1) ? e : ~e);
    }
    atomicExch(acc + TICKET, 0u);
    float* s = A.stats + f * STATS_FLOATS;
    for (int i = 0; i < 6; ++i) s[i] = out[i];
    if (A.running) {                                             // launches on one stream follow each other: no atomics
        for (int i = 0; i < 4; ++i) {
            const float v = out[6 + i], r = A.running[i];
            if ((i & 1) ? v > r : v < r) A.running[i] = v;       // false for a NaN: the frame is skipped
        }
    }
}

// ---------------------------------------------------------------- images

__device__ __forceinline__ bool aligned(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1)) == 0; }

// v[0..3] = p[i .. i + 4), zeros past `total`
__device__ __forceinline__ void load4(const float* p, long long i, long long total, bool a16, float* v) {
    if (a16 && i + 4 <= total) {
        const float4 t = *reinterpret_cast<const float4*>(p + i);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = i + j < total ? p[i + j] : 0.f;
}

// out[i .. i + 4) = b[0..3], nothing past `total`
__device__ __forceinline__ void store4(uint8_t* out, long long i, long long total, bool a4, const uint32_t* b) {
    if (a4 && i + 4 <= total) {
        *reinterpret_cast<uint32_t*>(out + i) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (i + j < total) out[i + j] = (uint8_t)b[j];
}

// out[12 q .. 12 q + 3 cnt) = the 3 bytes of each of cnt pixels
__device__ __forceinline__ void store_pixels(uint8_t* out, long long q, int cnt, bool a4, const uint32_t (*b)[3]) {
    if (a4 && cnt == 4) {
        uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 12; ++j) w[j >> 2] |= b[j / 3][j % 3] << (8 * (j & 3));
        uint32_t* o = reinterpret_cast<uint32_t*>(out + 12 * q);
        o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
        return;
    }
    for (int j = 0; j < cnt; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) out[12 * q + 3 * j + c] = (uint8_t)b[j][c];
}

__device__ __forceinline__ void depth_pixel(float d, float mi, float ma, const uint8_t* __restrict__ T, bool masked, float m,
                                            uint32_t* b) {
    float x = clip(n2n(d), mi, ma);
    const float range = ma - mi;
    const float den = (1e-8f > range) ? 1e-8f : range;           // Python's max(ma - mi, 1e-8)
    x = (x - mi) / den;
    const uint32_t k = u8(255.0f * x);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float t = (float)T[k * 3 + c] / 255.0f;                  // ToTensor()
        if (masked) t = t * m;
        b[c] = u8(t * 255.0f);
    }
}

// one (n) depth map -> (n, 3) bytes; mask: (n) or null
__device__ __forceinline__ void depth_image(const float* d, const float* mask, long long n, float mi, float ma,
                                            const uint8_t* __restrict__ T, uint8_t* out, long long t0, long long step) {
    const bool da = aligned(d, 16), ma16 = mask && aligned(mask, 16), oa = aligned(out, 4);
    for (long long q = t0; 4 * q < n; q += step) {
        const int cnt = n - 4 * q < 4 ? (int)(n - 4 * q) : 4;
        float v[4], m[4] = {0.f, 0.f, 0.f, 0.f};
        uint32_t b[4][3];
        load4(d, 4 * q, n, da, v);
        if (mask) load4(mask, 4 * q, n, ma16, m);
#pragma unroll
        for (int j = 0; j < 4; ++j) depth_pixel(v[j], mi, ma, T, mask != nullptr, clip(m[j], 0.f, 1.f), b[j]);
        store_pixels(out, q, cnt, oa, b);
    }
}

struct FinishArgs {
    MnrfFrameMaps in;
    MnrfFrameImages out;
    long long n;
    const float* stats;
    const uint8_t* table;
};

__global__ __launch_bounds__(TPB) void frame_finish_kernel(FinishArgs A) {
    const long long n = A.n, total = 3 * n;
    const long long t0 = (long long)blockIdx.x * TPB + threadIdx.x, step = (long long)gridDim.x * TPB;

    // the three-channel maps as flat arrays: 4 floats in, 4 bytes out
    const float* src[3] = {A.in.rgb, A.in.surface_normal, A.in.surface_normal_grad};
    uint8_t* dst[3] = {A.out.rgb, A.out.surface_normal, A.out.surface_normal_grad};
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        if (!src[s] || !dst[s]) continue;
        const bool ia = aligned(src[s], 16), oa = aligned(dst[s], 4);
        for (long long g = t0; 4 * g < total; g += step) {
            float v[4];
            uint32_t b[4];
            load4(src[s], 4 * g, total, ia, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float x = s == 0 ? v[j] : (v[j] + 1.0f) / 2.0f;
                b[j] = u8(clip(x, 0.f, 1.f) * 255.0f);
            }
            store4(dst[s], 4 * g, total, oa, b);
        }
    }
    if (A.in.x_surface && A.out.x_surface) {
        const float mn = A.stats[4], mx = A.stats[5];
        const bool ia = aligned(A.in.x_surface, 16), oa = aligned(A.out.x_surface, 4);
        const bool flat = mn == mx;
        const float rg = mx - mn;
        for (long long g = t0; 4 * g < total; g += step) {
            float v[4];
            uint32_t b[4];
            load4(A.in.x_surface, 4 * g, total, ia, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j] = flat ? 255u : u8(clip((v[j] - mn) / rg, 0.f, 1.f) * 255.0f);
            store4(A.out.x_surface, 4 * g, total, oa, b);
        }
    }

    // the per-pixel maps: 4 pixels in, 12 bytes out
    if (A.in.mirror_mask && A.out.mirror_mask) {
        const bool ia = aligned(A.in.mirror_mask, 16), oa = aligned(A.out.mirror_mask, 4);
        for (long long q = t0; 4 * q < n; q += step) {
            const int cnt = n - 4 * q < 4 ? (int)(n - 4 * q) : 4;
            float v[4];
            uint32_t b[4][3];
            load4(A.in.mirror_mask, 4 * q, n, ia, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) b[j][0] = b[j][1] = b[j][2] = u8(clip(v[j], 0.f, 1.f) * 255.0f);
            store_pixels(A.out.mirror_mask, q, cnt, oa, b);
        }
    }
    if (A.in.depth && A.out.depth)
        depth_image(A.in.depth, nullptr, n, A.stats[0], A.stats[1], A.table, A.out.depth, t0, step);
    if (A.in.depth_reflect && A.out.depth_reflect)
        depth_image(A.in.depth_reflect, A.in.mirror_mask, n, A.stats[2], A.stats[3], A.table, A.out.depth_reflect, t0, step);
}

// frame blockIdx.y of a stack; extrema: 2 floats, every `extrema_stride` floats a frame's own pair (0: one pair for all)
__global__ __launch_bounds__(TPB) void depth_colormap_kernel(const float* depth, const float* mask, long long n,
                                                             const float* extrema, long long extrema_stride,
                                                             const uint8_t* table, uint8_t* out) {
    const long long f = blockIdx.y;
    const float* e = extrema + f * extrema_stride;
    depth_image(depth + f * n, mask ? mask + f * n : nullptr, n, e[0], e[1], table, out + f * n * 3,
                (long long)blockIdx.x * TPB + threadIdx.x, (long long)gridDim.x * TPB);
}

// ---------------------------------------------------------------- the validation panel (utils/visualization.py:26-184)
//
// The (N_pics, 3, H, W) float32 stack of visualize_val_image(..., add_text=False), two launches:
//   panel_extrema_kernel   min and max of every global and every depth tile into that tile's 8-float stats slot
//                          ([0] min, [1] max, [2] [3] accumulators, [4] ticket; zero before the first launch, left zero)
//   panel_write_kernel     the whole stack: a thread takes 4 consecutive pixels of one tile, reads its map in place and stores
//                          one 16-byte row piece per channel, so every output element is written once, along W
// Tile t of kind k from map m, n = H W pixels p, channel c:
//   copy    out[c][p] = m[3 p + c]                                        view(H, W, 3).permute(2, 0, 1)
//   mask    out[c][p] = m[p]                                              unsqueeze(-1).repeat(1, 3)
//   normal  out[c][p] = (m[3 p + c] + 1) / 2
//   global  out[c][p] = mn == mx ? 1 : (m[3 p + c] - mn) / (mx - mn)      mn, mx over all 3 n values, NaN propagating
//   depth   x = clip(n2n(m[p]), mi, ma); x = (x - mi) / max(ma - mi, 1e-8f); k = u8(255 x); out[c][p] = float(T[k][c]) / 255
//           with mi, ma the min and max of n2n(m)

constexpr int PANEL_MAX_TILES = 32;        // the reference's panel has at most 24
constexpr int PANEL_STATS = 8;

struct PanelExtremaArgs {
    const float* src[PANEL_MAX_TILES];     // the tiles that need extremes, compacted
    float* stats[PANEL_MAX_TILES];         // their slots
    unsigned char depth[PANEL_MAX_TILES];  // 1: n values through n2n; 0: 3 n values, a NaN poisons both extremes
    long long n;
};

__global__ __launch_bounds__(TPB) void panel_extrema_kernel(PanelExtremaArgs A) {
    __shared__ uint32_t red[WAVES][2];
    __shared__ int last;
    const int t = blockIdx.y;
    const float* p = A.src[t];
    const bool depth = A.depth[t] != 0;
    const long long total = depth ? A.n : 3 * A.n;
    const long long t0 = (long long)blockIdx.x * TPB + threadIdx.x, step = (long long)gridDim.x * TPB;
    uint32_t a[2] = {0u, 0u};
    for (long long i = t0; i < total; i += step) {
        const float raw = p[i];
        const bool poison = !depth && raw != raw;
        const uint32_t k = key_of(depth ? n2n(raw) : raw);
        a[0] = umax(a[0], poison ? 0xffffffffu : ~k);
        a[1] = umax(a[1], poison ? 0xffffffffu : k);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
        for (int o = 32; o > 0; o >>= 1) a[i] = umax(a[i], (uint32_t)__shfl_xor((int)a[i], o));
    if ((threadIdx.x & 63) == 0) {
        red[threadIdx.x >> 6][0] = a[0];
        red[threadIdx.x >> 6][1] = a[1];
    }
    __syncthreads();
    uint32_t* acc = reinterpret_cast<uint32_t*>(A.stats[t]);
    if (threadIdx.x == 0) {
        for (int i = 0; i < 2; ++i) {
            uint32_t m = red[0][i];
            for (int w = 1; w < WAVES; ++w) m = umax(m, red[w][i]);
            if (m) atomicMax(acc + 2 + i, m);
        }
        __threadfence();
        last = atomicAdd(acc + 4, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last || threadIdx.x != 0) return;
    __threadfence();
    for (int i = 0; i < 2; ++i) {
        const uint32_t e = atomicExch(acc + 2 + i, 0u);
        A.stats[t][i] = (e == 0u || e == 0xffffffffu) ? __builtin_nanf("") : float_of(i ? e : ~e);
    }
    atomicExch(acc + 4, 0u);
}

struct PanelWriteArgs {
    const float* src[PANEL_MAX_TILES];
    unsigned char kind[PANEL_MAX_TILES];
    long long n;
    const float* stats;                    // (tiles, PANEL_STATS)
    const uint8_t* table;
    float* out;                            // (tiles, 3, n)
};

__global__ __launch_bounds__(TPB) void panel_write_kernel(PanelWriteArgs A) {
    const int t = blockIdx.y, kind = A.kind[t];
    const long long n = A.n;
    const float* m = A.src[t];
    float* out = A.out + (long long)t * 3 * n;
    const bool pixel_map = kind == MNRF_PANEL_MASK || kind == MNRF_PANEL_DEPTH;
    const bool ia = aligned(m, 16);
    float lo = 0.f, hi = 0.f;
    if (kind == MNRF_PANEL_GLOBAL || kind == MNRF_PANEL_DEPTH) {
        lo = A.stats[t * PANEL_STATS];
        hi = A.stats[t * PANEL_STATS + 1];
    }
    const float range = hi - lo;
    const float den = (1e-8f > range) ? 1e-8f : range;               // Python's max(ma - mi, 1e-8)
    const long long q0 = (long long)blockIdx.x * TPB + threadIdx.x, step = (long long)gridDim.x * TPB;
    for (long long q = q0; 4 * q < n; q += step) {
        const long long p = 4 * q;
        const int cnt = n - p < 4 ? (int)(n - p) : 4;
        float o[3][4];
        if (pixel_map) {
            float v[4];
            load4(m, p, n, ia, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (kind == MNRF_PANEL_MASK) {
                    o[0][j] = o[1][j] = o[2][j] = v[j];
                } else {
                    const float x = (clip(n2n(v[j]), lo, hi) - lo) / den;
                    const uint32_t k = u8(255.0f * x);
#pragma unroll
                    for (int c = 0; c < 3; ++c) o[c][j] = (float)A.table[k * 3 + c] / 255.0f;     // ToTensor()
                }
            }
        } else {
            float v[12];
#pragma unroll
            for (int g = 0; g < 3; ++g) load4(m, 3 * p + 4 * g, 3 * n, ia, v + 4 * g);
#pragma unroll
            for (int j = 0; j < 12; ++j) {
                float x = v[j];
                if (kind == MNRF_PANEL_NORMAL) x = (x + 1.0f) / 2.0f;
                else if (kind == MNRF_PANEL_GLOBAL) x = (lo == hi) ? 1.0f : (x - lo) / range;
                o[j % 3][j / 3] = x;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* row = out + c * n + p;
            if (cnt == 4 && aligned(row, 16)) {
                *reinterpret_cast<float4*>(row) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < cnt) row[j] = o[c][j];
            }
        }
    }
}

// the checks the two panel entry points share; 0, or the error already recorded
int panel_check(const char* who, const float* const* maps, const int* kinds, int n_tiles, int H, int W, const void* stats) {
    char msg[160];
    const auto fail = [&](const char* what) {
        snprintf(msg, sizeof msg, "%s: %s", who, what);
        return mnrf_fail(MNRF_ERR_ARG, msg);
    };
    if (n_tiles < 0 || n_tiles > PANEL_MAX_TILES) return fail("bad tile count (0 .. 32)");
    if (H < 0 || W < 0) return fail("negative frame size");
    if (n_tiles == 0) return MNRF_OK;
    if (!maps || !kinds) return fail("null maps or kinds array");
    bool reduced = false;
    for (int t = 0; t < n_tiles; ++t) {
        if (kinds[t] < MNRF_PANEL_COPY || kinds[t] > MNRF_PANEL_DEPTH) return fail("unknown tile kind");
        if (!maps[t]) return fail("null map");
        reduced |= kinds[t] == MNRF_PANEL_GLOBAL || kinds[t] == MNRF_PANEL_DEPTH;
    }
    if (reduced && !stats) return fail("a global or depth tile needs the stats block");
    return MNRF_OK;
}

unsigned blocks_for(int64_t items, int per_thread, unsigned cap) {
    const int64_t b = (items + (int64_t)TPB * per_thread - 1) / ((int64_t)TPB * per_thread);
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

constexpr int64_t N_MAX = 0x7fffffffffffffffLL / 16;     // 3 n and 12 q stay inside 64 bits
constexpr int64_t FRAMES_MAX = 65535;                    // gridDim.y

}  // namespace

extern "C" int mnrf_frame_stats_floats(void) { return STATS_FLOATS; }
extern "C" int mnrf_split_extrema_floats(void) { return RUNNING_FLOATS; }

extern "C" int mnrf_frame_extrema(const float* depth, const float* depth_reflect, const float* x_surface, int64_t n,
                                  float* stats, float* running, void* stream) {
    if (!stats) return mnrf_fail(MNRF_ERR_ARG, "mnrf_frame_extrema: null stats block");
    if (n < 0 || n > N_MAX) return mnrf_fail(MNRF_ERR_ARG, "mnrf_frame_extrema: bad pixel count");
    if (n == 0) return MNRF_OK;
    const ExtremaArgs A{depth, depth_reflect, x_surface, (long long)n, stats, running};
    hipLaunchKernelGGL(frame_extrema_kernel, dim3(blocks_for(3 * n, 4, 1024)), dim3(TPB), 0, (hipStream_t)stream, A);
    return mnrf_check_launch("mnrf_frame_extrema");
}

extern "C" int mnrf_frame_finish(const MnrfFrameMaps* maps, const MnrfFrameImages* images, int64_t n, const float* stats,
                                 const uint8_t* table, void* stream) {
    if (!maps || !images) return mnrf_fail(MNRF_ERR_ARG, "mnrf_frame_finish: null maps or images block");
    if (!stats) return mnrf_fail(MNRF_ERR_ARG, "mnrf_frame_finish: null stats block");
    if (n < 0 || n > N_MAX) return mnrf_fail(MNRF_ERR_ARG, "mnrf_frame_finish: bad pixel count");
    const bool want_depth = (maps->depth && images->depth) || (maps->depth_reflect && images->depth_reflect);
    if (want_depth && !table) return mnrf_fail(MNRF_ERR_ARG, "mnrf_frame_finish: a depth image needs the colour table");
    if (images->depth_reflect && maps->depth_reflect && !maps->mirror_mask)
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_frame_finish: depth_reflect needs the mirror mask");
    if (n == 0) return MNRF_OK;
    const FinishArgs A{*maps, *images, (long long)n, stats, table};
    hipLaunchKernelGGL(frame_finish_kernel, dim3(blocks_for(3 * n, 4, 4096)), dim3(TPB), 0, (hipStream_t)stream, A);
    return mnrf_check_launch("mnrf_frame_finish");
}

extern "C" int mnrf_depth_colormap(const float* depth, const float* mask, int64_t frames, int64_t n, const float* extrema,
                                   float* stats, const uint8_t* table, uint8_t* out, void* stream) {
    if (!extrema && !stats)
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_depth_colormap: null extrema needs stats blocks for the frames' own extremes");
    if (n < 0 || n > N_MAX || frames < 0 || frames > FRAMES_MAX)
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_depth_colormap: bad pixel or frame count");
    if (!table) return mnrf_fail(MNRF_ERR_ARG, "mnrf_depth_colormap: null colour table");
    if (n == 0 || frames == 0) return MNRF_OK;
    if (!depth || !out) return mnrf_fail(MNRF_ERR_ARG, "mnrf_depth_colormap: null depth stack or output");
    if (!extrema) {
        const ExtremaArgs A{depth, nullptr, nullptr, (long long)n, stats, nullptr};
        hipLaunchKernelGGL(frame_extrema_kernel, dim3(blocks_for(n, 4, 1024), (unsigned)frames), dim3(TPB), 0,
                           (hipStream_t)stream, A);
    }
    hipLaunchKernelGGL(depth_colormap_kernel, dim3(blocks_for(n, 4, 4096), (unsigned)frames), dim3(TPB), 0, (hipStream_t)stream,
                       depth, mask, (long long)n, extrema ? extrema : (const float*)stats,
                       (long long)(extrema ? 0 : STATS_FLOATS), table, out);
    return mnrf_check_launch("mnrf_depth_colormap");
}

extern "C" int mnrf_val_panel_stats_floats(void) { return PANEL_STATS; }

extern "C" int mnrf_val_panel_extrema(const float* const* maps, const int* kinds, int n_tiles, int H, int W, float* stats,
                                      void* stream) {
    if (const int e = panel_check("mnrf_val_panel_extrema", maps, kinds, n_tiles, H, W, stats)) return e;
    const int64_t n = (int64_t)H * W;
    if (n_tiles == 0 || n == 0) return MNRF_OK;
    PanelExtremaArgs A;
    A.n = n;
    int r = 0;
    for (int t = 0; t < n_tiles; ++t) {
        if (kinds[t] != MNRF_PANEL_GLOBAL && kinds[t] != MNRF_PANEL_DEPTH) continue;
        A.src[r] = maps[t];
        A.stats[r] = stats + (int64_t)t * PANEL_STATS;
        A.depth[r++] = kinds[t] == MNRF_PANEL_DEPTH;
    }
    if (r == 0) return MNRF_OK;
    hipLaunchKernelGGL(panel_extrema_kernel, dim3(blocks_for(3 * n, 4, 256), (unsigned)r), dim3(TPB), 0, (hipStream_t)stream, A);
    return mnrf_check_launch("mnrf_val_panel_extrema");
}

extern "C" int mnrf_val_panel_write(const float* const* maps, const int* kinds, int n_tiles, int H, int W, const float* stats,
                                    const uint8_t* table, float* out, void* stream) {
    if (const int e = panel_check("mnrf_val_panel_write", maps, kinds, n_tiles, H, W, stats)) return e;
    const int64_t n = (int64_t)H * W;
    if (n_tiles == 0) return MNRF_OK;
    PanelWriteArgs A;
    for (int t = 0; t < n_tiles; ++t) {
        if (kinds[t] == MNRF_PANEL_DEPTH && !table)
            return mnrf_fail(MNRF_ERR_ARG, "mnrf_val_panel_write: a depth tile needs the colour table");
        A.src[t] = maps[t];
        A.kind[t] = (unsigned char)kinds[t];
    }
    if (n == 0) return MNRF_OK;
    if (!out) return mnrf_fail(MNRF_ERR_ARG, "mnrf_val_panel_write: null output stack");
    A.n = n;
    A.stats = stats;
    A.table = table;
    A.out = out;
    hipLaunchKernelGGL(panel_write_kernel, dim3(blocks_for(n, 4, 1024), (unsigned)n_tiles), dim3(TPB), 0, (hipStream_t)stream, A);
    return mnrf_check_launch("mnrf_val_panel_write");
}
