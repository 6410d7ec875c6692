// mnrf_rough.hip -- mirror roughness (eval.batched_inference with app_control_mirror_roughness, eval.py:622-674) on chunks in
// which only SOME rays are mirror rays: THE RULE of include/mnrf.h ("Mirror roughness") in two launches.
//
// reflect_jitter_fan_kernel: the n_jit jittered reflections of the m mirror rays of a level, all of them in one launch.  Every
// jitter compacts through the same mask, so the compaction is not repeated: `index` (made once per chunk and level by
// mnrf_reflect_compact) names the source ray of row p, and row j*m + p of `sec` is that ray reflected about
// l2n(normal + noise[j] * std) -- mnrf_reflect.h's expressions, the ones mnrf_reflect_compact evaluates.  One thread per
// (j, p) across the chip: no order to establish, no count, no device state.  Per thread 32 B of ray row (two 16-byte words
// where the base allows it), 36 B of x_surface, normal and draw (gathered through index: the rows of a wave ascend, so they
// share cache lines) and one 32-byte row written as two 16-byte stores.  Memory-bound; 256 threads per workgroup as the other
// per-ray kernels.
//
// jitter_mean_kernel: acc[row(p)] = ((acc[row(p)] + pieces[0][p]) + pieces[1][p]) + ..., then the finish -- single fp32 additions
// in the order the reference adds its renders (eval.py:661-666).  One thread per (p, channel): the pieces are read coalesced,
// 12 B per row and jitter; rows of acc that index does not name are neither read nor written.
//
// A roughness per placed mirror (include/mnrf.h "A roughness per mirror", batched_inference rough_times=): the standard deviation
// becomes a per-ray row.  rough_rows_kernel forms it from the index mnrf_place_mirrors wrote (std_rows) together with the 0/1
// mask of the jitter set J = {mask != 0 and std > 0} and its "any" flag; perturb_normals_kernel adds draw * std to the normals
// of the rays with std > 0 and copies the others untouched (no `+ 0`: a -0 stays -0), so mnrf_reflect_compact without noise
// then evaluates mnrf_reflect.h's remaining operations on them; reflect_jitter_fan_rows_kernel is reflect_jitter_fan_kernel with
// std_rows[i] in place of the call's one std (one body, a template flag).  All three one thread per ray (or per 4 floats),
// 256 threads per workgroup, memory-bound.
// Compiled with -ffp-contract=off and IEEE division, as the rest of the library.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mnrf.h"
#include "mnrf_error.h"
#include "mnrf_reflect.h"

namespace {

struct FanArgs {
    const float* rays; const float* x_surface; const float* normal; const float* noise; float noise_std;
    const float* std_rows;                             // ROWS: the std of source ray i is std_rows[i], noise_std is not read
    const int* index; long long m, n_rays, total; float near2; float* sec; int wide;
};

template <bool ROWS>
__global__ __launch_bounds__(256) void reflect_jitter_fan_kernel(FanArgs A) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;      // row j * m + p of sec
    if (t >= A.total) return;
    const long long j = t / A.m, p = t - j * A.m;
    const long long i = A.index[p];
    if (i < 0 || i >= A.n_rays) return;                // not a row of the chunk (the precondition is broken): nothing is touched
    float d[3], far;
    if (A.wide) {                                      // (uniform) 16-byte aligned bases: the row as two 16-byte words
        const float4* q = reinterpret_cast<const float4*>(A.rays) + i * 2;
        const float4 a = q[0], b = q[1];
        d[0] = a.w; d[1] = b.x; d[2] = b.y; far = b.w;
    } else {
        const float* q = A.rays + i * 8;
        d[0] = q[3]; d[1] = q[4]; d[2] = q[5]; far = q[7];
    }
    float r[3];
    mnrf_reflect::direction(A.normal + i * 3, A.noise ? A.noise + (j * A.n_rays + i) * 3 : nullptr, ROWS ? A.std_rows[i] : A.noise_std,
                            d, r);
    const float* x = A.x_surface + i * 3;
    if (A.wide) {
        float4* o = reinterpret_cast<float4*>(A.sec) + t * 2;
        o[0] = make_float4(x[0], x[1], x[2], r[0]);
        o[1] = make_float4(r[1], r[2], A.near2, far);      // ray_forward_offset, absolute (eval.py:529)
    } else {
        float* o = A.sec + t * 8;
        o[0] = x[0]; o[1] = x[1]; o[2] = x[2];
        o[3] = r[0]; o[4] = r[1]; o[5] = r[2];
        o[6] = A.near2;
        o[7] = far;
    }
}

__global__ __launch_bounds__(256) void jitter_mean_kernel(float* __restrict__ acc, const float* __restrict__ pieces,
                                                          const int* __restrict__ index, long long m, int n_jit, long long n_acc,
                                                          int finish_mode, float finish_value) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;      // element p * 3 + channel of a piece
    if (e >= m * 3) return;
    const long long p = e / 3;
    const int ch = (int)(e - p * 3);
    const long long row = index ? (long long)index[p] : p;
    if (row < 0 || row >= n_acc) return;               // not a row of acc (the precondition is broken): nothing is touched
    float a = acc[row * 3 + ch];
    for (int j = 0; j < n_jit; ++j) a = a + pieces[(long long)j * m * 3 + e];
    if (finish_mode == MNRF_MEAN_DIVIDE) a = a / finish_value;
    else if (finish_mode == MNRF_MEAN_MULTIPLY) a = a * finish_value;
    acc[row * 3 + ch] = a;
}

struct RowsArgs {
    const int* index; const float* mask; long long n; int K; float rough[MNRF_MIRRORS_MAX]; float scene;
    float* std_rows; float* jitter_mask; int* any;
};

__global__ __launch_bounds__(256) void rough_rows_kernel(RowsArgs A) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool in_j = false;
    if (i < A.n) {
        const int idx = A.index ? A.index[i] : -1;
        float s = A.scene;                             // no placed mirror taken, or an index outside [-1, K): the scene's own
#pragma unroll
        for (int k = 0; k < MNRF_MIRRORS_MAX; ++k)     // (a select per mirror: the table stays in the argument registers)
            if (k < A.K && idx == k) s = A.rough[k];
        in_j = A.mask[i] != 0.f && s > 0.f;
        A.std_rows[i] = s;
        A.jitter_mask[i] = in_j ? 1.f : 0.f;
    }
    if (A.any && __ballot(in_j) != 0ull && (threadIdx.x & 63) == 0) atomicOr(A.any, 1);
}

// element e of the flat (n_rays * 3) arrays belongs to ray e / 3
__device__ __forceinline__ float perturbed(float nrm, float draw, float s) { return s > 0.f ? nrm + draw * s : nrm; }

__global__ __launch_bounds__(256) void perturb_normals_kernel(const float* __restrict__ normal, const float* __restrict__ noise,
                                                              const float* __restrict__ std_rows, long long total, int wide,
                                                              float* __restrict__ out) {
    const long long e0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;      // four consecutive floats per thread
    if (e0 >= total) return;
    if (wide && e0 + 4 <= total) {                     // 16-byte aligned bases and a whole word: one 16-byte access per array
        const float4 a = *reinterpret_cast<const float4*>(normal + e0), b = *reinterpret_cast<const float4*>(noise + e0);
        float4 o;
        o.x = perturbed(a.x, b.x, std_rows[(e0 + 0) / 3]);
        o.y = perturbed(a.y, b.y, std_rows[(e0 + 1) / 3]);
        o.z = perturbed(a.z, b.z, std_rows[(e0 + 2) / 3]);
        o.w = perturbed(a.w, b.w, std_rows[(e0 + 3) / 3]);
        *reinterpret_cast<float4*>(out + e0) = o;
    } else {
        for (long long e = e0; e < e0 + 4 && e < total; ++e) out[e] = perturbed(normal[e], noise[e], std_rows[e / 3]);
    }
}

}  // namespace

extern "C" int mnrf_reflect_jitter_fan(const float* rays, const float* x_surface, const float* normal, const float* noise,
                                       float noise_std, const int32_t* index, int64_t m, int64_t n_rays, int n_jit, float near2,
                                       float* sec, void* stream) {
    if (m < 0 || n_rays < 0 || n_rays > 0x7fffffffLL || m > n_rays) return mnrf_fail(MNRF_ERR_ARG, "mnrf_reflect_jitter_fan: bad size");
    if (n_jit < 1) return mnrf_fail(MNRF_ERR_ARG, "mnrf_reflect_jitter_fan: n_jit must be at least 1");
    if (m == 0) return MNRF_OK;
    if (!rays || !x_surface || !normal || !index || !sec) return mnrf_fail(MNRF_ERR_ARG, "mnrf_reflect_jitter_fan: null pointer");
    const long long total = (long long)m * n_jit;
    const long long blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return mnrf_fail(MNRF_ERR_ARG, "mnrf_reflect_jitter_fan: n_jit * m is too large for one launch");
    FanArgs A{};
    A.rays = rays; A.x_surface = x_surface; A.normal = normal; A.noise = noise; A.noise_std = noise_std;
    A.index = index; A.m = (long long)m; A.n_rays = (long long)n_rays; A.total = total; A.near2 = near2; A.sec = sec;
    A.wide = (((uintptr_t)rays | (uintptr_t)sec) & 15u) == 0;
    hipLaunchKernelGGL(reflect_jitter_fan_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, A);
    return mnrf_check_launch("mnrf_reflect_jitter_fan");
}

extern "C" int mnrf_reflect_jitter_fan_rows(const float* rays, const float* x_surface, const float* normal, const float* noise,
                                            const float* std_rows, const int32_t* index, int64_t m, int64_t n_rays, int n_jit,
                                            float near2, float* sec, void* stream) {
    if (m < 0 || n_rays < 0 || n_rays > 0x7fffffffLL || m > n_rays) return mnrf_fail(MNRF_ERR_ARG, "mnrf_reflect_jitter_fan_rows: bad size");
    if (n_jit < 1) return mnrf_fail(MNRF_ERR_ARG, "mnrf_reflect_jitter_fan_rows: n_jit must be at least 1");
    if (m == 0) return MNRF_OK;
    if (!rays || !x_surface || !normal || !std_rows || !index || !sec)
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_reflect_jitter_fan_rows: null pointer");
    const long long total = (long long)m * n_jit;
    const long long blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return mnrf_fail(MNRF_ERR_ARG, "mnrf_reflect_jitter_fan_rows: n_jit * m is too large for one launch");
    FanArgs A{};
    A.rays = rays; A.x_surface = x_surface; A.normal = normal; A.noise = noise; A.std_rows = std_rows;
    A.index = index; A.m = (long long)m; A.n_rays = (long long)n_rays; A.total = total; A.near2 = near2; A.sec = sec;
    A.wide = (((uintptr_t)rays | (uintptr_t)sec) & 15u) == 0;
    hipLaunchKernelGGL(reflect_jitter_fan_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, A);
    return mnrf_check_launch("mnrf_reflect_jitter_fan_rows");
}

extern "C" int mnrf_rough_rows(const int32_t* index, const float* mask, int64_t n_rays, int n_mirrors, const float* roughness,
                               float scene_roughness, float* std_rows, float* jitter_mask, int32_t* any, void* stream) {
    if (n_rays < 0 || n_rays > 0x7fffffffLL) return mnrf_fail(MNRF_ERR_ARG, "mnrf_rough_rows: bad size");
    if (n_mirrors < 0 || n_mirrors > MNRF_MIRRORS_MAX) return mnrf_fail(MNRF_ERR_ARG, "mnrf_rough_rows: n_mirrors must be in 0..8");
    if (n_mirrors > 0 && !roughness) return mnrf_fail(MNRF_ERR_ARG, "mnrf_rough_rows: the per-mirror host array is null");
    RowsArgs A{};
    for (int k = 0; k < n_mirrors; ++k) {
        if (!(roughness[k] >= 0.f) || roughness[k] > 3.402823466e+38f)
            return mnrf_fail(MNRF_ERR_ARG, "mnrf_rough_rows: a roughness must be finite and not negative");
        A.rough[k] = roughness[k];
    }
    if (!(scene_roughness >= 0.f) || scene_roughness > 3.402823466e+38f)
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_rough_rows: scene_roughness must be finite and not negative");
    if (n_rays == 0) return MNRF_OK;
    if (!mask || !std_rows || !jitter_mask) return mnrf_fail(MNRF_ERR_ARG, "mnrf_rough_rows: null pointer");
    A.index = index; A.mask = mask; A.n = (long long)n_rays; A.K = n_mirrors; A.scene = scene_roughness;
    A.std_rows = std_rows; A.jitter_mask = jitter_mask; A.any = any;
    hipLaunchKernelGGL(rough_rows_kernel, dim3((unsigned)((n_rays + 255) / 256)), dim3(256), 0, (hipStream_t)stream, A);
    return mnrf_check_launch("mnrf_rough_rows");
}

extern "C" int mnrf_perturb_normals(const float* normal, const float* noise, const float* std_rows, int64_t n_rays, float* out,
                                    void* stream) {
    if (n_rays < 0 || n_rays > 0x7fffffffLL) return mnrf_fail(MNRF_ERR_ARG, "mnrf_perturb_normals: bad size");
    if (n_rays == 0) return MNRF_OK;
    if (!normal || !noise || !std_rows || !out) return mnrf_fail(MNRF_ERR_ARG, "mnrf_perturb_normals: null pointer");
    const long long total = (long long)n_rays * 3;
    const int wide = (((uintptr_t)normal | (uintptr_t)noise | (uintptr_t)out) & 15u) == 0;
    hipLaunchKernelGGL(perturb_normals_kernel, dim3((unsigned)(((total + 3) / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       normal, noise, std_rows, total, wide, out);
    return mnrf_check_launch("mnrf_perturb_normals");
}

extern "C" int mnrf_jitter_mean(float* acc, const float* pieces, const int32_t* index, int64_t m, int n_jit, int64_t n_acc,
                                int finish_mode, float finish_value, void* stream) {
    if (m < 0 || n_acc < 0 || n_acc > 0x7fffffffLL || m > n_acc) return mnrf_fail(MNRF_ERR_ARG, "mnrf_jitter_mean: bad size");
    if (n_jit < 1) return mnrf_fail(MNRF_ERR_ARG, "mnrf_jitter_mean: n_jit must be at least 1");
    if (finish_mode != MNRF_MEAN_NONE && finish_mode != MNRF_MEAN_DIVIDE && finish_mode != MNRF_MEAN_MULTIPLY)
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_jitter_mean: finish_mode must be MNRF_MEAN_NONE, MNRF_MEAN_DIVIDE or MNRF_MEAN_MULTIPLY");
    if (m == 0) return MNRF_OK;
    if (!acc || !pieces) return mnrf_fail(MNRF_ERR_ARG, "mnrf_jitter_mean: null pointer");
    const long long blocks = ((long long)m * 3 + 255) / 256;
    hipLaunchKernelGGL(jitter_mean_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, acc, pieces, index,
                       (long long)m, n_jit, (long long)n_acc, finish_mode, finish_value);
    return mnrf_check_launch("mnrf_jitter_mean");
}
