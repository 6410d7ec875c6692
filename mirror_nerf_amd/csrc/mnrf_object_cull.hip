// mnrf_object_cull.hip -- object bounds for app_reflect_newly_placed_objects: a placed object is rendered only along the rays
// whose segment can touch it.  Bounds are a box in the object's frame cut into Rx x Ry x Rz cells with one bit per cell
// (mnrf_occupancy_bits makes the bits from a density volume); mnrf_object_cull keeps, compacted and in source order, the rays
// whose object-frame segment meets a set cell; mnrf_object_merge_indexed merges the object's maps of those rays back into
// the level's rows.  All three are memory-bound passes (about 32 B per ray in, at most 36 B out).
//
// The cull decision (mnrf_object.h keep_ray, shared with mnrf_objects.hip) is evaluated in float64 on the fp32 object-frame
// ray that mnrf_object_rays writes (mnrf_object.h move_ray, the same device function): against cells of extent c the margins below are 2^-12 c, far above the float64 rounding of
// the expressions and far below the one cell the rule allows (include/mnrf.h).
// Compiled with -ffp-contract=off and IEEE division, as the rest of the library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mnrf.h"
#include "mnrf_error.h"
#include "mnrf_object.h"

namespace {

inline unsigned blocks_for(long long n, int threads) { return (unsigned)((n + threads - 1) / threads); }

// ------------------------------------------------------------------------------------------------ occupancy bits
struct OccArgs {
    const float* volume; int Rx, Ry, Rz; float sigma_min; int dilate; uint32_t* bits; int* n_set; int words; long long n_words;
};

// One thread per output word (32 cells along x).  A cell is set when one of its 8 corners has !(sigma < sigma_min); grown by
// one cell over the 26-neighbourhood that is: one of the corners [i-1, i+2] x [j-1, j+2] x [k-1, k+2] (clipped to the volume)
// has it.  The thread ORs the corner flags of its rows into one 64-bit mask along x and folds neighbouring bits.
__global__ __launch_bounds__(256) void occupancy_bits_kernel(OccArgs A) {
    const long long w_id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    int cnt = 0;
    if (w_id < A.n_words) {
        const int w = (int)(w_id % A.words);
        const long long row = w_id / A.words;
        const int j = (int)(row % A.Ry), k = (int)(row / A.Ry);
        const int g = A.dilate;
        const int x_first = w * 32 - g;                       // corner of bit 0
        const int n_bits = 33 + 2 * g;                        // corners x_first .. x_first + n_bits - 1
        const int k0 = max(k - g, 0), k1 = min(k + 1 + g, A.Rz);
        const int j0 = max(j - g, 0), j1 = min(j + 1 + g, A.Ry);
        const int b0 = max(0, -x_first), b1 = min(n_bits - 1, A.Rx - x_first);
        unsigned long long c = 0ull;
        for (int kk = k0; kk <= k1; ++kk)
            for (int jj = j0; jj <= j1; ++jj) {
                const float* v = A.volume + ((long long)kk * (A.Ry + 1) + jj) * (A.Rx + 1);
                for (int b = b0; b <= b1; ++b)
                    if (!(v[x_first + b] < A.sigma_min)) c |= 1ull << b;       // a NaN corner sets the cell
            }
        unsigned long long cells = c | (c >> 1);                               // cell i: corners i, i + 1 (bits i + g ...)
        if (g) cells |= (c >> 2) | (c >> 3);                                   // ... or corners i - 1 .. i + 2 (bits i .. i + 3)
        const int valid = min(32, A.Rx - w * 32);                              // padding bits of the row's last word stay zero
        const uint32_t out = (uint32_t)cells & (valid >= 32 ? 0xffffffffu : ((1u << valid) - 1u));
        A.bits[w_id] = out;
        cnt = __popc(out);
    }
    if (A.n_set) {                                                             // integer sum: the same whatever the order
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) cnt += __shfl_xor(cnt, s);
        if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(A.n_set, cnt);
    }
}

// ------------------------------------------------------------------------------------------------ the cull
struct CullArgs {
    const float* rays; long long n; mnrf_object::Move move; mnrf_object::Bounds bounds;
    float* out_rays; int* index; int* count;
};

// Pass 1, one thread per ray over the whole chip: the decision, as 0 / 1 in index[i].
__global__ __launch_bounds__(256) void cull_mark_kernel(CullArgs A) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    float q[8];
    mnrf_object::move_ray(A.move, A.rays + i * 8, q);
    A.index[i] = mnrf_object::keep_ray(A.bounds, q) ? 1 : 0;
}

// Pass 2: one workgroup walks the marks in order (wave ballots, a scan over the 16 waves: reflect_compact_kernel's scheme), so
// that the kept rows keep the source order and no atomic decides a position.  index is compacted in place: a row is written
// at a position no larger than the one it was read from, and every mark of a round is read before the round's first write.
__global__ __launch_bounds__(1024) void cull_compact_kernel(CullArgs A) {
    __shared__ int s_wave[16];
    __shared__ int s_base;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (long long start = 0; start < A.n; start += 1024) {
        const long long i = start + tid;
        const bool sel = i < A.n && A.index[i] != 0;
        const unsigned long long bal = __ballot(sel);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wv] = __popcll(bal);
        __syncthreads();
        int woff = 0, tot = 0;
        for (int k = 0; k < 16; ++k) { const int c = s_wave[k]; if (k < wv) woff += c; tot += c; }
        const int base = s_base;
        if (sel) {
            const long long p = base + woff + before;
            mnrf_object::move_ray(A.move, A.rays + i * 8, A.out_rays + p * 8);
            A.index[p] = (int)i;
        }
        __syncthreads();
        if (tid == 0) s_base = base + tot;
        __syncthreads();
    }
    if (tid == 0) *A.count = s_base;
}

// ------------------------------------------------------------------------------------------------ the indexed merge
struct MergeIdxArgs {
    const float* obj_rgb; const float* obj_depth; const float* obj_opacity; const int* index; const int* count; long long cap;
    mnrf_object::Merge merge; int* n_used;
};

__global__ __launch_bounds__(256) void object_merge_indexed_kernel(MergeIdxArgs A) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long n = min((long long)max(*A.count, 0), A.cap);
    bool use = false;
    if (i < n) use = mnrf_object::merge_ray(A.merge, A.obj_rgb, A.obj_depth, A.obj_opacity, i, (long long)A.index[i]);
    if (A.n_used) {
        const unsigned long long b = __ballot(use);
        if (b != 0ull && (threadIdx.x & 63) == 0) atomicAdd(A.n_used, __popcll(b));
    }
}

inline bool res_ok(int r) { return r >= 1 && r <= MNRF_OBJECT_MAX_RES; }

}  // namespace

extern "C" int mnrf_occupancy_bits(const float* volume, int Rx, int Ry, int Rz, float sigma_min, int dilate, uint32_t* bits,
                                   int32_t* n_set, void* stream) {
    if (!res_ok(Rx) || !res_ok(Ry) || !res_ok(Rz)) return mnrf_fail(MNRF_ERR_ARG, "mnrf_occupancy_bits: Rx, Ry, Rz must be in 1..1024");
    if (dilate != 0 && dilate != 1) return mnrf_fail(MNRF_ERR_ARG, "mnrf_occupancy_bits: dilate must be 0 or 1");
    if (!volume || !bits) return mnrf_fail(MNRF_ERR_ARG, "mnrf_occupancy_bits: null pointer");
    const int words = (Rx + 31) / 32;
    const long long n_words = (long long)words * Ry * Rz;
    if (n_set && hipMemsetAsync(n_set, 0, sizeof(int32_t), (hipStream_t)stream) != hipSuccess)
        return mnrf_fail(MNRF_ERR_LAUNCH, "mnrf_occupancy_bits: clearing n_set failed");
    OccArgs A{volume, Rx, Ry, Rz, sigma_min, dilate, bits, n_set, words, n_words};
    hipLaunchKernelGGL(occupancy_bits_kernel, dim3(blocks_for(n_words, 256)), dim3(256), 0, (hipStream_t)stream, A);
    return mnrf_check_launch("mnrf_occupancy_bits");
}

extern "C" int mnrf_object_cull(const float* rays, int64_t n_rays, const float* pose, float scale, float tx, float ty, float tz,
                                const float* box_lo, const float* box_hi, int Rx, int Ry, int Rz, const uint32_t* bits,
                                float* out_rays, int32_t* index, int32_t* count, void* stream) {
    if (n_rays < 0 || n_rays > 0x7fffffffLL) return mnrf_fail(MNRF_ERR_ARG, "mnrf_object_cull: bad size");
    if (!box_lo || !box_hi) return mnrf_fail(MNRF_ERR_ARG, "mnrf_object_cull: box_lo / box_hi are null");
    for (int a = 0; a < 3; ++a)
        if (!(box_lo[a] < box_hi[a]) || !(box_hi[a] - box_lo[a] <= 3.4028234663852886e38f))
            return mnrf_fail(MNRF_ERR_ARG, "mnrf_object_cull: the box needs finite lo < hi on every axis");
    if (bits && (!res_ok(Rx) || !res_ok(Ry) || !res_ok(Rz)))
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_object_cull: Rx, Ry, Rz must be in 1..1024");
    if (n_rays == 0) return MNRF_OK;
    if (!rays || !out_rays || !index || !count) return mnrf_fail(MNRF_ERR_ARG, "mnrf_object_cull: null pointer");
    if (rays == out_rays) return mnrf_fail(MNRF_ERR_ARG, "mnrf_object_cull: works out of place (out_rays must not be rays)");
    CullArgs A{};
    A.rays = rays;
    A.n = (long long)n_rays;
    A.move = mnrf_object::make_move(pose, scale, tx, ty, tz);
    A.bounds = mnrf_object::make_bounds(box_lo, box_hi, Rx, Ry, Rz, bits);
    A.out_rays = out_rays;
    A.index = index;
    A.count = count;
    hipLaunchKernelGGL(cull_mark_kernel, dim3(blocks_for(n_rays, 256)), dim3(256), 0, (hipStream_t)stream, A);
    hipLaunchKernelGGL(cull_compact_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, A);
    return mnrf_check_launch("mnrf_object_cull");
}

extern "C" int mnrf_object_merge_indexed(const float* obj_rgb, const float* obj_depth, const float* obj_opacity,
                                         const int32_t* index, const int32_t* count, int64_t capacity, float scale,
                                         float pose_scale0, float near, float* rgb, float* depth, float* mask, int32_t* n_used,
                                         void* stream) {
    if (capacity < 0) return mnrf_fail(MNRF_ERR_ARG, "mnrf_object_merge_indexed: bad size");
    if (capacity == 0) return MNRF_OK;
    if (!obj_rgb || !obj_depth || !obj_opacity || !index || !count || !rgb || !depth)
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_object_merge_indexed: null pointer");
    MergeIdxArgs A{obj_rgb, obj_depth, obj_opacity, index, count, (long long)capacity, {scale, pose_scale0, near, rgb, depth, mask}, n_used};
    hipLaunchKernelGGL(object_merge_indexed_kernel, dim3(blocks_for(capacity, 256)), dim3(256), 0, (hipStream_t)stream, A);
    return mnrf_check_launch("mnrf_object_merge_indexed");
}
