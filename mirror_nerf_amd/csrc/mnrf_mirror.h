// mnrf_mirror.h -- the per-ray device functions the mirror-placing kernels share: place_mirror_kernel (mnrf_apps.hip, one
// axis-aligned mirror, eval.py:364-504) and place_mirrors_kernel (mnrf_mirrors.hip, 1..8 mirrors on any plane).  Each
// expression is written once here, as single fp32 operations in the reference's order (the files are compiled with
// -ffp-contract=off and IEEE division and square root), so both kernels evaluate the same bits for an axis-aligned mirror.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mnrf.h"

namespace mnrf_mirror {

// eval.py:391-398 / 435-442: the plane x = pos (axis MNRF_PLANE_X; (u, w) = (y, z)) or y = pos (MNRF_PLANE_Y; (u, w) = (x, z)),
// (p - o_a) / d_a * d_b + o_b
__device__ inline void axis_point(int axis, float pos, const float* o, const float* d, float* x, float& u, float& w) {
    const bool y = axis == MNRF_PLANE_Y;
    const float oa = y ? o[1] : o[0], da = y ? d[1] : d[0];
    const float ob = y ? o[0] : o[1], db = y ? d[0] : d[1];
    const float t = (pos - oa) / da;
    u = t * db + ob;
    w = t * d[2] + o[2];
    x[0] = y ? u : pos;
    x[1] = y ? pos : u;
    x[2] = w;
}

// A plane through c with unit normal n and in-plane unit axes eu, ew: t = n.(c - o) / n.d, x = t d + o, (u, w) = (eu, ew).(x - c)
__device__ inline void frame_point(const float* c, const float* n, const float* eu, const float* ew, const float* o, const float* d,
                                   float* x, float& u, float& w) {
    const float e0 = c[0] - o[0], e1 = c[1] - o[1], e2 = c[2] - o[2];
    const float num = (n[0] * e0 + n[1] * e1) + n[2] * e2;
    const float den = (n[0] * d[0] + n[1] * d[1]) + n[2] * d[2];
    const float t = num / den;
    x[0] = t * d[0] + o[0];
    x[1] = t * d[1] + o[1];
    x[2] = t * d[2] + o[2];
    const float r0 = x[0] - c[0], r1 = x[1] - c[1], r2 = x[2] - c[2];
    u = (eu[0] * r0 + eu[1] * r1) + eu[2] * r2;
    w = (ew[0] * r0 + ew[1] * r1) + ew[2] * r2;
}

// eval.py:403-414 / 445-456; every comparison with a NaN is false, so a NaN coordinate counts as inside
__device__ inline bool in_rect(float u, float w, const float* rect) {
    return !(u < rect[0] || w < rect[2] || u > rect[1] || w > rect[3]);
}

// the ellipse inscribed in rect; the border (q == 1) and a NaN are inside
__device__ inline bool in_ellipse(float u, float w, const float* rect) {
    const float uc = (rect[0] + rect[1]) * 0.5f, ru = (rect[1] - rect[0]) * 0.5f;
    const float wc = (rect[2] + rect[3]) * 0.5f, rw = (rect[3] - rect[2]) * 0.5f;
    const float a = (u - uc) / ru, b = (w - wc) / rw;
    const float q = a * a + b * b;
    return !(q > 1.f);
}

// eval.py:461-463: torch.norm(o - x)
__device__ inline float distance(const float* o, const float* x) {
    const float e0 = o[0] - x[0], e1 = o[1] - x[1], e2 = o[2] - x[2];
    return sqrtf(e0 * e0 + e1 * e1 + e2 * e2);
}

// eval.py:466-474: sum((x - o) * d); positive when the intersection lies on the ray and not on its backward extension
__device__ inline float side(const float* o, const float* d, const float* x) {
    return (x[0] - o[0]) * d[0] + (x[1] - o[1]) * d[1] + (x[2] - o[2]) * d[2];
}

// eval.py:477-483 with eval.py:169-171: the foreground occludes the mirror (depth of the level before any edit, the global near)
__device__ inline bool blocked(float dist, float depth, float near) { return dist > depth && depth > near; }

}  // namespace mnrf_mirror
