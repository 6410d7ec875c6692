// mnrf_mirrors.hip -- several new mirrors at one recursion level (batched_inference(new_mirrors=[...]), placed_mirrors.py):
// 1..MNRF_MIRRORS_MAX mirrors, axis-aligned (the expressions of place_mirror_kernel, shared through mnrf_mirror.h) or on any
// plane given by a frame, rectangular or elliptic, in ONE launch.  Every mirror is tested against the level's depth as it is
// before the call; the nearest hit wins and it alone writes the ray's normal, so two mirrors never overwrite each other's
// normals the way a chain of mnrf_place_mirror calls would.
//
// The mirror descriptors travel by value in the kernel's argument struct (80 B per mirror, K <= 8): the loop over k reads
// them with scalar loads, and the kind and shape branches are uniform.  One thread per ray, one pass: the ray row (32 B) is
// read as two 16-byte words per lane where the pointer allows it (a wave reads 2 KiB contiguous), depth and mask one dword
// per lane; the K intersections live in registers; depth, the 12-byte rows of normal and x_surface are written only where
// a mirror is taken (neither is read), the two masks and the index for every ray.  About 45 B read and up to 41 B written
// per ray: a memory-bound stream, 256 threads per workgroup as the other per-ray kernels.
//
// mnrf_place_mirrors_from is the same kernel body with one more input, `source` (one coalesced dword per lane): the placed mirror
// the ray was reflected off at the level directly above, which cannot be hit (`k != source`, a compare against the uniform k: no
// branch is added to the loop).  The body is a template on "a source row is given", so mnrf_place_mirrors' instantiation is the
// code it was.  mnrf_mirror_sources builds that row for the next level: a gather of this level's index through the
// compaction's index, repeated per jitter block -- one thread per written element, 4 B read through each index and 4 B written.
// Compiled with -ffp-contract=off and IEEE division, as the rest of the library.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/mnrf.h"
#include "mnrf_error.h"
#include "mnrf_mirror.h"

namespace {

struct Mirror {
    int kind; int shape; int axis; float pos;      // axis, pos: kind MNRF_MIRROR_AXIS
    float c[3]; float eu[3]; float ew[3];          // centre and in-plane axes: kind MNRF_MIRROR_FRAME
    float n[3];                                    // the normal written to a ray that takes the mirror; the plane's normal of a frame
    float rect[4];
};

struct MirrorsArgs {
    const float* rays; long long n; int K; int wide; Mirror m[MNRF_MIRRORS_MAX]; float near;
    float* depth; float* mask; float* normal; float* x_surface; uint8_t* mask_bool; int* any; int* index;
    const int* source;                                 // FROM: the mirror ray i left at the level above, never hit; else not read
};

template <bool FROM>
__global__ __launch_bounds__(256) void place_mirrors_kernel(MirrorsArgs A) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool merged = false;
    if (i < A.n) {
        float o[3], d[3];
        if (A.wide) {                                  // (uniform) a 16-byte aligned base: the row as two 16-byte words
            const float4* p = reinterpret_cast<const float4*>(A.rays) + i * 2;
            const float4 a = p[0], b = p[1];
            o[0] = a.x; o[1] = a.y; o[2] = a.z;
            d[0] = a.w; d[1] = b.x; d[2] = b.y;
        } else {
            const float* r = A.rays + i * 8;
            o[0] = r[0]; o[1] = r[1]; o[2] = r[2];
            d[0] = r[3]; d[1] = r[4]; d[2] = r[5];
        }
        const float depth0 = A.depth[i];               // the depth every mirror is tested against
        const int src = FROM ? A.source[i] : -1;       // no range check: a value outside 0 .. K-1 equals no k
        int best = -1;
        float best_dist = 0.f, bx[3] = {0.f, 0.f, 0.f}, bn[3] = {0.f, 0.f, 0.f};
        for (int k = 0; k < A.K; ++k) {
            const Mirror& M = A.m[k];
            float x[3], u, w;
            if (M.kind == MNRF_MIRROR_AXIS) mnrf_mirror::axis_point(M.axis, M.pos, o, d, x, u, w);
            else mnrf_mirror::frame_point(M.c, M.n, M.eu, M.ew, o, d, x, u, w);
            const bool inside = M.shape == MNRF_MIRROR_ELLIPSE ? mnrf_mirror::in_ellipse(u, w, M.rect) : mnrf_mirror::in_rect(u, w, M.rect);
            const float dist = mnrf_mirror::distance(o, x);
            const float s = mnrf_mirror::side(o, d, x);
            const bool hit = inside && s > 0.f && !mnrf_mirror::blocked(dist, depth0, A.near) && !(FROM && k == src);
            if (hit && (best < 0 || dist <= best_dist)) {      // the nearest hit; a tie goes to the later mirror; a NaN never replaces
                best = k;
                best_dist = dist;
                bx[0] = x[0]; bx[1] = x[1]; bx[2] = x[2];
                bn[0] = M.n[0]; bn[1] = M.n[1]; bn[2] = M.n[2];
            }
        }
        merged = A.mask[i] != 0.f || best >= 0;
        if (best >= 0) {
            A.x_surface[i * 3 + 0] = bx[0];
            A.x_surface[i * 3 + 1] = bx[1];
            A.x_surface[i * 3 + 2] = bx[2];
            A.depth[i] = best_dist;
            A.normal[i * 3 + 0] = bn[0];
            A.normal[i * 3 + 1] = bn[1];
            A.normal[i * 3 + 2] = bn[2];
        }
        A.mask[i] = merged ? 1.f : 0.f;
        if (A.mask_bool) A.mask_bool[i] = merged ? 1 : 0;
        if (A.index) A.index[i] = best;
    }
    if (A.any && __ballot(merged) != 0ull && (threadIdx.x & 63) == 0) atomicOr(A.any, 1);
}

__global__ __launch_bounds__(256) void mirror_sources_kernel(const int* __restrict__ level_index, const int* __restrict__ compaction_index,
                                                            long long m, long long total, int* __restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;      // element j * m + p of out
    if (t >= total) return;
    const long long p = t % m;
    out[t] = level_index ? level_index[compaction_index ? (long long)compaction_index[p] : p] : -1;
}

int fail(const char* who, const char* what) {
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: %s", who, what);
    return mnrf_fail(MNRF_ERR_ARG, msg);
}

// both entry points: `source` null launches the instantiation without it
int place_mirrors(const char* who, const float* rays, int64_t n_rays, int n_mirrors, const int* kinds, const int* shapes, const int* axes,
                  const float* positions, const float* frames, const float* normals, const float* rects, float near, const int32_t* source,
                  float* depth, float* mask, float* normal, float* x_surface, uint8_t* mask_bool, int32_t* any, int32_t* index,
                  void* stream) {
    if (n_rays < 0 || n_rays > 0x7fffffffLL) return fail(who, "bad size");
    if (n_mirrors < 1 || n_mirrors > MNRF_MIRRORS_MAX) return fail(who, "n_mirrors must be in 1..8");
    if (!kinds || !shapes || !axes || !positions || !frames || !normals || !rects) return fail(who, "a per-mirror host array is null");
    MirrorsArgs A{};
    for (int k = 0; k < n_mirrors; ++k) {
        Mirror& M = A.m[k];
        if (kinds[k] != MNRF_MIRROR_AXIS && kinds[k] != MNRF_MIRROR_FRAME) return fail(who, "kind must be MNRF_MIRROR_AXIS or MNRF_MIRROR_FRAME");
        if (shapes[k] != MNRF_MIRROR_RECT && shapes[k] != MNRF_MIRROR_ELLIPSE)
            return fail(who, "shape must be MNRF_MIRROR_RECT or MNRF_MIRROR_ELLIPSE");
        if (kinds[k] == MNRF_MIRROR_AXIS && axes[k] != MNRF_PLANE_X && axes[k] != MNRF_PLANE_Y)
            return fail(who, "axis must be MNRF_PLANE_X or MNRF_PLANE_Y");
        M.kind = kinds[k];
        M.shape = shapes[k];
        M.axis = axes[k];
        M.pos = positions[k];
        for (int j = 0; j < 3; ++j) {
            M.c[j] = frames[9 * k + j];
            M.eu[j] = frames[9 * k + 3 + j];
            M.ew[j] = frames[9 * k + 6 + j];
            M.n[j] = normals[3 * k + j];
        }
        for (int j = 0; j < 4; ++j) M.rect[j] = rects[4 * k + j];
    }
    if (n_rays == 0) return MNRF_OK;
    if (!rays || !depth || !mask || !normal || !x_surface) return fail(who, "null pointer");
    A.rays = rays;
    A.n = (long long)n_rays;
    A.K = n_mirrors;
    A.wide = ((uintptr_t)rays & 15u) == 0;
    A.near = near;
    A.depth = depth;
    A.mask = mask;
    A.normal = normal;
    A.x_surface = x_surface;
    A.mask_bool = mask_bool;
    A.any = any;
    A.index = index;
    A.source = source;
    const dim3 grid((unsigned)((n_rays + 255) / 256));
    if (source) hipLaunchKernelGGL(place_mirrors_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, A);
    else hipLaunchKernelGGL(place_mirrors_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, A);
    return mnrf_check_launch(who);
}

}  // namespace

extern "C" int mnrf_place_mirrors(const float* rays, int64_t n_rays, int n_mirrors, const int* kinds, const int* shapes, const int* axes,
                                  const float* positions, const float* frames, const float* normals, const float* rects, float near,
                                  float* depth, float* mask, float* normal, float* x_surface, uint8_t* mask_bool, int32_t* any,
                                  int32_t* index, void* stream) {
    return place_mirrors("mnrf_place_mirrors", rays, n_rays, n_mirrors, kinds, shapes, axes, positions, frames, normals, rects, near, nullptr,
                         depth, mask, normal, x_surface, mask_bool, any, index, stream);
}

extern "C" int mnrf_place_mirrors_from(const float* rays, int64_t n_rays, int n_mirrors, const int* kinds, const int* shapes, const int* axes,
                                       const float* positions, const float* frames, const float* normals, const float* rects, float near,
                                       const int32_t* source, float* depth, float* mask, float* normal, float* x_surface,
                                       uint8_t* mask_bool, int32_t* any, int32_t* index, void* stream) {
    return place_mirrors("mnrf_place_mirrors_from", rays, n_rays, n_mirrors, kinds, shapes, axes, positions, frames, normals, rects, near,
                         source, depth, mask, normal, x_surface, mask_bool, any, index, stream);
}

extern "C" int mnrf_mirror_sources(const int32_t* level_index, const int32_t* compaction_index, int64_t m, int n_rep, int32_t* out,
                                   void* stream) {
    if (m < 0 || m > 0x7fffffffLL) return fail("mnrf_mirror_sources", "bad size");
    if (n_rep < 1) return fail("mnrf_mirror_sources", "n_rep must be at least 1");
    if (m == 0) return MNRF_OK;
    if (!out) return fail("mnrf_mirror_sources", "null pointer");
    const long long total = (long long)m * n_rep;
    const long long blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return fail("mnrf_mirror_sources", "n_rep * m is too large for one launch");
    hipLaunchKernelGGL(mirror_sources_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, level_index, compaction_index,
                       (long long)m, total, out);
    return mnrf_check_launch("mnrf_mirror_sources");
}
