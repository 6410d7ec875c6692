// mnrf_objects.hip -- several placed objects at one recursion level of app_reflect_newly_placed_objects: the cull of one
// level's rays against K objects in two launches (mnrf_objects_cull) and the merge of the K objects' maps into the level's in
// one (mnrf_objects_merge).  Per object both evaluate the device functions of mnrf_object.h -- move_ray, keep_ray, merge_ray
// -- that the single-object kernels (mnrf_apps.hip, mnrf_object_cull.hip) evaluate, so the K-object result is, bit for bit,
// the chain of K single-object applications in list order.
//
// The per-object constants travel by value in the kernels' argument structs (160 B per object of the cull, 32 B of the merge,
// K <= 8): blockIdx.y / blockIdx.x selects the object, so reading them is a scalar load from the argument segment.  Both
// passes are memory-bound streams: a ray row is 32 B, read as two 16-B words per lane (a wave reads 2 KiB contiguous) and
// written as the lane's 32 contiguous bytes; the maps of the merge are read one lane per ray.  The mark pass runs one wave
// per workgroup -- 512 workgroups per object at 32768 rays, so that every CU has work at K = 1 and the divergent cell walk
// of keep_ray is not held back by a slow neighbour.
// Compiled with -ffp-contract=off and IEEE division, as the rest of the library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mnrf.h"
#include "mnrf_error.h"
#include "mnrf_object.h"

namespace {

constexpr int MARK_THREADS = 64;

inline unsigned blocks_for(long long n, int threads) { return (unsigned)((n + threads - 1) / threads); }

struct CullObject {
    mnrf_object::Move move; mnrf_object::Bounds bounds; int unbounded;
};

struct CullArgs {
    const float* rays; long long n; int K; CullObject obj[MNRF_OBJECTS_MAX];
    float* out_rays; int* index; int* slot; int* counts;      // (K, n, 8), (K, n), (K, n), (K)
};

__device__ inline void load_ray(const float* rays, long long i, float* r) {
    const float4* p = reinterpret_cast<const float4*>(rays) + i * 2;
    const float4 a = p[0], b = p[1];
    r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w;
    r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
}

__device__ inline void store_ray(float* rays, long long i, const float* q) {
    float4* p = reinterpret_cast<float4*>(rays) + i * 2;
    p[0] = make_float4(q[0], q[1], q[2], q[3]);
    p[1] = make_float4(q[4], q[5], q[6], q[7]);
}

// Pass 1, a grid over (ray tile, object): the decision of object k on ray i, as 0 / 1 in index[k][i].  An object without
// bounds keeps every ray.
__global__ __launch_bounds__(MARK_THREADS) void objects_mark_kernel(CullArgs A) {
    const long long i = (long long)blockIdx.x * MARK_THREADS + threadIdx.x;
    const int k = blockIdx.y;
    if (i >= A.n) return;
    const CullObject& O = A.obj[k];
    int keep = 1;
    if (!O.unbounded) {
        float r[8], q[8];
        load_ray(A.rays, i, r);
        mnrf_object::move_ray(O.move, r, q);
        keep = mnrf_object::keep_ray(O.bounds, q) ? 1 : 0;
    }
    A.index[(long long)k * A.n + i] = keep;
}

// Pass 2, one workgroup per object: cull_compact_kernel's walk of the marks in order (wave ballots, a scan over the 16 waves),
// so that the kept rows keep the source order and no atomic decides a position.  index[k] is compacted in place: a row is
// written at a position no larger than the one it was read from, and every mark of a round is read before the round's first
// write.  slot[k][i] = the row of ray i in object k's list, or -1.
__global__ __launch_bounds__(1024) void objects_compact_kernel(CullArgs A) {
    __shared__ int s_wave[16];
    __shared__ int s_base;
    const int k = blockIdx.x;
    const CullObject& O = A.obj[k];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int* index = A.index + (long long)k * A.n;
    int* slot = A.slot + (long long)k * A.n;
    float* out = A.out_rays + (long long)k * A.n * 8;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (long long start = 0; start < A.n; start += 1024) {
        const long long i = start + tid;
        const bool sel = i < A.n && index[i] != 0;
        const unsigned long long bal = __ballot(sel);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wv] = __popcll(bal);
        __syncthreads();
        int woff = 0, tot = 0;
        for (int w = 0; w < 16; ++w) { const int c = s_wave[w]; if (w < wv) woff += c; tot += c; }
        const int base = s_base;
        if (sel) {
            const long long p = base + woff + before;
            float r[8], q[8];
            load_ray(A.rays, i, r);
            mnrf_object::move_ray(O.move, r, q);
            store_ray(out, p, q);
            index[p] = (int)i;
            slot[i] = (int)p;
        } else if (i < A.n) {
            slot[i] = -1;
        }
        __syncthreads();
        if (tid == 0) s_base = base + tot;
        __syncthreads();
    }
    if (tid == 0) A.counts[k] = s_base;
}

struct MergeObject {
    const float* rgb; const float* depth; const float* opacity; float scale; float pose_scale0;
};

struct MergeArgs {
    MergeObject obj[MNRF_OBJECTS_MAX]; int K; const int* slot; const int* counts; long long n; long long cap;
    float near; float* rgb; float* depth; float* mask; int* n_used;
};

// One thread per ray of the level, the objects in list order: the ray's maps are read and written by this thread alone, so
// object k sees them as the scene and the objects 0 .. k-1 left them -- the chain of K single-object merges.
__global__ __launch_bounds__(256) void objects_merge_kernel(MergeArgs A) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (int k = 0; k < A.K; ++k) {
        const MergeObject& O = A.obj[k];
        if (!O.rgb) continue;                                              // (uniform: the object was not rendered)
        bool use = false;
        if (r < A.n) {
            const long long s = A.slot[(long long)k * A.n + r];
            const long long m = min((long long)max(A.counts[k], 0), A.cap);
            if (s >= 0 && s < m) {
                const mnrf_object::Merge M{O.scale, O.pose_scale0, A.near, A.rgb, A.depth, A.mask};
                use = mnrf_object::merge_ray(M, O.rgb, O.depth, O.opacity, s, r);
            }
        }
        if (A.n_used) {
            const unsigned long long b = __ballot(use);
            if (b != 0ull && (threadIdx.x & 63) == 0) atomicAdd(A.n_used + k, __popcll(b));
        }
    }
}

inline bool res_ok(int r) { return r >= 1 && r <= MNRF_OBJECT_MAX_RES; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int mnrf_objects_cull(const float* rays, int64_t n_rays, int n_objects, const int* posed, const float* poses,
                                 const float* scales, const float* translations, const int* unbounded, const float* box_lo,
                                 const float* box_hi, const int* res, const uint32_t* const* bits, float* out_rays,
                                 int32_t* index, int32_t* slot, int32_t* counts, void* stream) {
    if (n_objects < 1 || n_objects > MNRF_OBJECTS_MAX) return mnrf_fail(MNRF_ERR_ARG, "mnrf_objects_cull: n_objects must be in 1..8");
    if (n_rays < 0 || n_rays > 0x7fffffffLL) return mnrf_fail(MNRF_ERR_ARG, "mnrf_objects_cull: bad size");
    if (!posed || !poses || !scales || !translations || !unbounded || !box_lo || !box_hi || !res || !bits)
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_objects_cull: a per-object host array is null");
    CullArgs A{};
    for (int k = 0; k < n_objects; ++k) {
        CullObject& O = A.obj[k];
        O.move = mnrf_object::make_move(posed[k] ? poses + 12 * k : nullptr, scales[k], translations[3 * k], translations[3 * k + 1],
                                        translations[3 * k + 2]);
        O.unbounded = unbounded[k] != 0;
        if (O.unbounded) continue;
        const float *lo = box_lo + 3 * k, *hi = box_hi + 3 * k;
        for (int a = 0; a < 3; ++a)
            if (!(lo[a] < hi[a]) || !(hi[a] - lo[a] <= 3.4028234663852886e38f))
                return mnrf_fail(MNRF_ERR_ARG, "mnrf_objects_cull: a box needs finite lo < hi on every axis");
        if (bits[k] && (!res_ok(res[3 * k]) || !res_ok(res[3 * k + 1]) || !res_ok(res[3 * k + 2])))
            return mnrf_fail(MNRF_ERR_ARG, "mnrf_objects_cull: Rx, Ry, Rz must be in 1..1024");
        O.bounds = mnrf_object::make_bounds(lo, hi, res[3 * k], res[3 * k + 1], res[3 * k + 2], bits[k]);
    }
    if (n_rays == 0) return MNRF_OK;
    if (!rays || !out_rays || !index || !slot || !counts) return mnrf_fail(MNRF_ERR_ARG, "mnrf_objects_cull: null pointer");
    if (rays == out_rays) return mnrf_fail(MNRF_ERR_ARG, "mnrf_objects_cull: works out of place (out_rays must not be rays)");
    if (!aligned16(rays) || !aligned16(out_rays))
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_objects_cull: rays and out_rays must be aligned to 16 bytes (rows are moved as two 16-byte words)");
    A.rays = rays;
    A.n = (long long)n_rays;
    A.K = n_objects;
    A.out_rays = out_rays;
    A.index = index;
    A.slot = slot;
    A.counts = counts;
    hipLaunchKernelGGL(objects_mark_kernel, dim3(blocks_for(n_rays, MARK_THREADS), n_objects), dim3(MARK_THREADS), 0, (hipStream_t)stream, A);
    hipLaunchKernelGGL(objects_compact_kernel, dim3(n_objects), dim3(1024), 0, (hipStream_t)stream, A);
    return mnrf_check_launch("mnrf_objects_cull");
}

extern "C" int mnrf_objects_merge(const float* const* obj_rgb, const float* const* obj_depth, const float* const* obj_opacity,
                                  int n_objects, const int32_t* slot, const int32_t* counts, int64_t n_rays, int64_t capacity,
                                  const float* scales, const float* pose_scale0, float near, float* rgb, float* depth, float* mask,
                                  int32_t* n_used, void* stream) {
    if (n_objects < 1 || n_objects > MNRF_OBJECTS_MAX) return mnrf_fail(MNRF_ERR_ARG, "mnrf_objects_merge: n_objects must be in 1..8");
    if (n_rays < 0 || n_rays > 0x7fffffffLL || capacity < 0) return mnrf_fail(MNRF_ERR_ARG, "mnrf_objects_merge: bad size");
    if (!obj_rgb || !obj_depth || !obj_opacity || !scales || !pose_scale0)
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_objects_merge: a per-object host array is null");
    MergeArgs A{};
    bool any = false;
    for (int k = 0; k < n_objects; ++k) {
        const int given = (obj_rgb[k] != nullptr) + (obj_depth[k] != nullptr) + (obj_opacity[k] != nullptr);
        if (given != 0 && given != 3)
            return mnrf_fail(MNRF_ERR_ARG, "mnrf_objects_merge: an object's rgb, depth and opacity are given together or not at all");
        A.obj[k] = MergeObject{obj_rgb[k], obj_depth[k], obj_opacity[k], scales[k], pose_scale0[k]};
        any = any || given == 3;
    }
    if (n_rays == 0 || capacity == 0 || !any) return MNRF_OK;
    if (!slot || !counts || !rgb || !depth) return mnrf_fail(MNRF_ERR_ARG, "mnrf_objects_merge: null pointer");
    A.K = n_objects;
    A.slot = slot;
    A.counts = counts;
    A.n = (long long)n_rays;
    A.cap = (long long)capacity;
    A.near = near;
    A.rgb = rgb;
    A.depth = depth;
    A.mask = mask;
    A.n_used = n_used;
    hipLaunchKernelGGL(objects_merge_kernel, dim3(blocks_for(n_rays, 256)), dim3(256), 0, (hipStream_t)stream, A);
    return mnrf_check_launch("mnrf_objects_merge");
}
