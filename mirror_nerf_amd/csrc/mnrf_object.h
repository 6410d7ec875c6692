// mnrf_object.h -- the per-ray device functions of app_reflect_newly_placed_objects (eval.py:173-291) that more than one
// kernel evaluates: the move of a ray into the object's frame (mnrf_object_rays, mnrf_object_cull) and the depth-ordered merge
// of the object's maps (mnrf_object_merge, mnrf_object_merge_indexed).  One definition each: the kernels that share them give
// the same bits.  Compiled with -ffp-contract=off and IEEE division: the expressions are the reference's, in its order.
#pragma once
#include <hip/hip_runtime.h>

namespace mnrf_object {

constexpr float EPS32 = 1.1920928955078125e-07f;  // torch.finfo(float32).eps, utils/func.py:5

struct Move {       // how a level's rays go into the object's frame
    int posed; float A[9]; float p[3]; float scale; float t[3];
};

// pose: a HOST array of 12 floats (row-major 3x4 [A | p]) or null
inline Move make_move(const float* pose, float scale, float tx, float ty, float tz) {
    Move m{pose != nullptr, {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, {0.f, 0.f, 0.f}, scale, {tx, ty, tz}};
    if (pose)
        for (int k = 0; k < 3; ++k) {
            for (int j = 0; j < 3; ++j) m.A[k * 3 + j] = pose[k * 4 + j];
            m.p[k] = pose[k * 4 + 3];
        }
    return m;
}

// eval.py:175-217 on one ray r (8 floats) -> q (8 floats): with a pose o = A o + p (two steps: the product, then the sum),
// d = l2_normalize(A d) (utils/func.py:5-7); then o = o * scale, then o = o + t (two roundings); near / far are copied
__device__ inline void move_ray(const Move& M, const float* __restrict__ r, float* __restrict__ q) {
    float o[3] = {r[0], r[1], r[2]};
    float d[3] = {r[3], r[4], r[5]};
    if (M.posed) {
        float ro[3], rd[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ro[k] = M.A[k * 3 + 0] * o[0] + M.A[k * 3 + 1] * o[1] + M.A[k * 3 + 2] * o[2];
            rd[k] = M.A[k * 3 + 0] * d[0] + M.A[k * 3 + 1] * d[1] + M.A[k * 3 + 2] * d[2];
        }
        const float len = sqrtf(fmaxf(rd[0] * rd[0] + rd[1] * rd[1] + rd[2] * rd[2], EPS32));
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            o[k] = ro[k] + M.p[k];
            d[k] = rd[k] / len;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float scaled = o[k] * M.scale;
        q[k] = scaled + M.t[k];
        q[3 + k] = d[k];
    }
    q[6] = r[6];
    q[7] = r[7];
}

struct Merge {      // the level's maps and the constants of the merge
    float scale; float pose_scale0; float near; float* rgb; float* depth; float* mask;
};

// eval.py:261-291 on one ray: row `src` of the object's maps into row `dst` of the level's.  The object's depth back in the
// scene's units (two divisions, in the reference's order), the object where it is opaque (`> 0.8` of the accumulated weight,
// depth > 0: "remove white bg") and not behind the scene's foreground (the scene's depth of this level, valid when beyond the
// global near).  Comparisons with NaN are false.  -> whether the ray took the object
__device__ inline bool merge_ray(const Merge& M, const float* obj_rgb, const float* obj_depth, const float* obj_opacity,
                                 long long src, long long dst) {
    const float d = obj_depth[src] / M.scale / M.pose_scale0;                                  // eval.py:261-265
    const float depth = M.depth[dst];
    const bool obj = d > 0.f && obj_opacity[src] > 0.8f;                                       // eval.py:268-272
    const bool blocked = d > depth && depth > M.near;                                          // eval.py:275-281, 169-171
    const bool use = obj && !blocked;                                                          // eval.py:282-284
    if (use) {                                                                                 // eval.py:285-291
        M.rgb[dst * 3 + 0] = obj_rgb[src * 3 + 0];
        M.rgb[dst * 3 + 1] = obj_rgb[src * 3 + 1];
        M.rgb[dst * 3 + 2] = obj_rgb[src * 3 + 2];
        M.depth[dst] = d;
        if (M.mask) M.mask[dst] = 0.f;
    }
    return use;
}

}  // namespace mnrf_object
