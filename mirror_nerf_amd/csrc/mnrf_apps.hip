// mnrf_apps.hip -- the per-ray kernels of the scene-editing applications of eval.batched_inference that need only
// MirrorNeRF fields: placing a new planar mirror (eval.py:311-320, 364-504), the ray transform in front of a reflection
// substitution (eval.py:550-613), and the two steps around the object field of a newly placed object (eval.py:173-291): the
// move of a level's rays into the object's frame and the depth-ordered merge of the object's maps into the level's.  All are
// memory-bound (one thread per ray, ~70 B read and written per ray); they exist so that the application modes run no chain
// of framework ops per level.
// Compiled with -ffp-contract=off and IEEE division: the expressions below are the reference's, in its order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mnrf.h"
#include "mnrf_error.h"
#include "mnrf_mirror.h"
#include "mnrf_object.h"

namespace {

constexpr float EPS32 = 1.1920928955078125e-07f;  // torch.finfo(float32).eps, utils/func.py:5

struct PlaceArgs {
    const float* rays; long long n; int axis; float pos; float nrm[3]; float rect[4]; float near;
    float* depth; float* mask; float* normal; float* x_surface; uint8_t* mask_bool; int* any;
};

// One ray.  The order of the reference's edits matters and is kept:
//   in_rect  = not (u < r0 or w < r2 or u > r1 or w > r3)       (a NaN coordinate -- a ray parallel to the plane whose
//                                                                  origin lies in it -- counts as inside here)
//   normal[in_rect] = plane normal                               (before the two filters below: the returned normal map
//                                                                  changes on rays that do not end up in the mirror)
//   new = in_rect and sum((x - o) * d) > 0 and not (|o - x| > depth and depth > near)
//   x_surface[new] = x, depth[new] = |o - x|, mask |= new
__global__ __launch_bounds__(256) void place_mirror_kernel(PlaceArgs A) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool merged = false;
    if (i < A.n) {
        const float* r = A.rays + i * 8;
        const float o[3] = {r[0], r[1], r[2]};
        const float d[3] = {r[3], r[4], r[5]};
        float x[3], u, w;
        mnrf_mirror::axis_point(A.axis, A.pos, o, d, x, u, w);                                     // eval.py:391-398 / 435-442
        const bool in_rect = mnrf_mirror::in_rect(u, w, A.rect);                                   // eval.py:403-414 / 445-456
        const float depth = A.depth[i];
        if (in_rect) {                                                                             // eval.py:458-460
            A.normal[i * 3 + 0] = A.nrm[0];
            A.normal[i * 3 + 1] = A.nrm[1];
            A.normal[i * 3 + 2] = A.nrm[2];
        }
        const float dist = mnrf_mirror::distance(o, x);                                            // eval.py:461-463
        const float s = mnrf_mirror::side(o, d, x);                                                // eval.py:466-474
        const bool blocked = mnrf_mirror::blocked(dist, depth, A.near);                            // eval.py:477-483
        const bool hit = in_rect && s > 0.f && !blocked;
        merged = A.mask[i] != 0.f || hit;                                                          // eval.py:307, 490
        if (hit) {                                                                                 // eval.py:484-499
            A.x_surface[i * 3 + 0] = x[0];
            A.x_surface[i * 3 + 1] = x[1];
            A.x_surface[i * 3 + 2] = x[2];
            A.depth[i] = dist;
        }
        A.mask[i] = merged ? 1.f : 0.f;
        if (A.mask_bool) A.mask_bool[i] = merged ? 1 : 0;
    }
    if (A.any && __ballot(merged) != 0ull && (threadIdx.x & 63) == 0) atomicOr(A.any, 1);
}

struct XformArgs {
    float* rays; long long n; int rotate; float R[9]; float scale; float t[3];
};

// eval.py:551-594: o = R o, d = l2_normalize(R d) (utils/func.py:5-7), then o = o * scale + t
__global__ __launch_bounds__(256) void transform_rays_kernel(XformArgs A) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    float* r = A.rays + i * 8;
    float o[3] = {r[0], r[1], r[2]};
    if (A.rotate) {
        const float d[3] = {r[3], r[4], r[5]};
        float ro[3], rd[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ro[k] = A.R[k * 3 + 0] * o[0] + A.R[k * 3 + 1] * o[1] + A.R[k * 3 + 2] * o[2];
            rd[k] = A.R[k * 3 + 0] * d[0] + A.R[k * 3 + 1] * d[1] + A.R[k * 3 + 2] * d[2];
        }
        const float len = sqrtf(fmaxf(rd[0] * rd[0] + rd[1] * rd[1] + rd[2] * rd[2], EPS32));
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            o[k] = ro[k];
            r[3 + k] = rd[k] / len;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) r[k] = o[k] * A.scale + A.t[k];
}

struct ObjectRaysArgs {
    const float* rays; long long n; mnrf_object::Move move; float* out;
};

// eval.py:175-217, out of place (mnrf_object.h move_ray, shared with the cull of mnrf_object_cull.hip)
__global__ __launch_bounds__(256) void object_rays_kernel(ObjectRaysArgs A) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    mnrf_object::move_ray(A.move, A.rays + i * 8, A.out + i * 8);
}

struct ObjectMergeArgs {
    const float* obj_rgb; const float* obj_depth; const float* obj_opacity; long long n; mnrf_object::Merge merge; int* n_used;
};

// eval.py:261-291, one thread per ray (mnrf_object.h merge_ray, shared with mnrf_object_merge_indexed)
__global__ __launch_bounds__(256) void object_merge_kernel(ObjectMergeArgs A) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool use = false;
    if (i < A.n) use = mnrf_object::merge_ray(A.merge, A.obj_rgb, A.obj_depth, A.obj_opacity, i, i);
    if (A.n_used) {
        const unsigned long long b = __ballot(use);
        if (b != 0ull && (threadIdx.x & 63) == 0) atomicAdd(A.n_used, __popcll(b));
    }
}

inline unsigned blocks_for(long long n, int threads) { return (unsigned)((n + threads - 1) / threads); }

}  // namespace

extern "C" int mnrf_place_mirror(const float* rays, int64_t n_rays, int axis, float position, float normal_x, float normal_y,
                                 float normal_z, float rect_u0, float rect_u1, float rect_w0, float rect_w1, float near,
                                 float* depth, float* mask, float* normal, float* x_surface, uint8_t* mask_bool, int32_t* any,
                                 void* stream) {
    if (n_rays < 0) return mnrf_fail(MNRF_ERR_ARG, "mnrf_place_mirror: bad size");
    if (axis != MNRF_PLANE_X && axis != MNRF_PLANE_Y) return mnrf_fail(MNRF_ERR_ARG, "mnrf_place_mirror: axis must be MNRF_PLANE_X or MNRF_PLANE_Y");
    if (n_rays == 0) return MNRF_OK;
    if (!rays || !depth || !mask || !normal || !x_surface) return mnrf_fail(MNRF_ERR_ARG, "mnrf_place_mirror: null pointer");
    PlaceArgs A{rays, (long long)n_rays, axis, position, {normal_x, normal_y, normal_z}, {rect_u0, rect_u1, rect_w0, rect_w1}, near,
                depth, mask, normal, x_surface, mask_bool, any};
    hipLaunchKernelGGL(place_mirror_kernel, dim3(blocks_for(n_rays, 256)), dim3(256), 0, (hipStream_t)stream, A);
    return mnrf_check_launch("mnrf_place_mirror");
}

extern "C" int mnrf_transform_rays(float* rays, int64_t n_rays, const float* rotation, float scale, float tx, float ty, float tz,
                                   void* stream) {
    if (n_rays < 0) return mnrf_fail(MNRF_ERR_ARG, "mnrf_transform_rays: bad size");
    if (n_rays == 0) return MNRF_OK;
    if (!rays) return mnrf_fail(MNRF_ERR_ARG, "mnrf_transform_rays: null pointer");
    XformArgs A{rays, (long long)n_rays, rotation != nullptr, {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, scale, {tx, ty, tz}};
    if (rotation)
        for (int k = 0; k < 9; ++k) A.R[k] = rotation[k];
    hipLaunchKernelGGL(transform_rays_kernel, dim3(blocks_for(n_rays, 256)), dim3(256), 0, (hipStream_t)stream, A);
    return mnrf_check_launch("mnrf_transform_rays");
}

extern "C" int mnrf_object_rays(const float* rays, int64_t n_rays, const float* pose, float scale, float tx, float ty, float tz,
                                float* out, void* stream) {
    if (n_rays < 0) return mnrf_fail(MNRF_ERR_ARG, "mnrf_object_rays: bad size");
    if (n_rays == 0) return MNRF_OK;
    if (!rays || !out) return mnrf_fail(MNRF_ERR_ARG, "mnrf_object_rays: null pointer");
    if (rays == out) return mnrf_fail(MNRF_ERR_ARG, "mnrf_object_rays: works out of place (out must not be rays)");
    ObjectRaysArgs A{rays, (long long)n_rays, mnrf_object::make_move(pose, scale, tx, ty, tz), out};
    hipLaunchKernelGGL(object_rays_kernel, dim3(blocks_for(n_rays, 256)), dim3(256), 0, (hipStream_t)stream, A);
    return mnrf_check_launch("mnrf_object_rays");
}

extern "C" int mnrf_object_merge(const float* obj_rgb, const float* obj_depth, const float* obj_opacity, int64_t n_rays, float scale,
                                 float pose_scale0, float near, float* rgb, float* depth, float* mask, int32_t* n_used,
                                 void* stream) {
    if (n_rays < 0) return mnrf_fail(MNRF_ERR_ARG, "mnrf_object_merge: bad size");
    if (n_rays == 0) return MNRF_OK;
    if (!obj_rgb || !obj_depth || !obj_opacity || !rgb || !depth) return mnrf_fail(MNRF_ERR_ARG, "mnrf_object_merge: null pointer");
    ObjectMergeArgs A{obj_rgb, obj_depth, obj_opacity, (long long)n_rays, {scale, pose_scale0, near, rgb, depth, mask}, n_used};
    hipLaunchKernelGGL(object_merge_kernel, dim3(blocks_for(n_rays, 256)), dim3(256), 0, (hipStream_t)stream, A);
    return mnrf_check_launch("mnrf_object_merge");
}
