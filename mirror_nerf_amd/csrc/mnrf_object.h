// mnrf_object.h -- the per-ray device functions of app_reflect_newly_placed_objects (eval.py:173-291) that more than one
// kernel evaluates: the move of a ray into the object's frame (mnrf_object_rays, mnrf_object_cull, mnrf_objects_cull), the
// cull decision against object bounds (mnrf_object_cull, mnrf_objects_cull) and the depth-ordered merge of the object's maps
// (mnrf_object_merge, mnrf_object_merge_indexed, mnrf_objects_merge).  One definition each: the kernels that share them give
// the same bits.  Compiled with -ffp-contract=off and IEEE division: the expressions are the reference's, in its order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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

struct Bounds {     // object bounds: a box in the object's frame cut into R cells per axis, one bit per cell (include/mnrf.h)
    double lo[3], cell[3]; int R[3]; const uint32_t* bits; int words;
};

// box_lo, box_hi: HOST arrays of 3 floats; without bits the whole box is one set cell (Rx, Ry, Rz are not read)
inline Bounds make_bounds(const float* box_lo, const float* box_hi, int Rx, int Ry, int Rz, const uint32_t* bits) {
    Bounds b{};
    const int R[3] = {bits ? Rx : 1, bits ? Ry : 1, bits ? Rz : 1};
    for (int a = 0; a < 3; ++a) {
        b.lo[a] = (double)box_lo[a];
        b.cell[a] = ((double)box_hi[a] - (double)box_lo[a]) / R[a];
        b.R[a] = R[a];
    }
    b.bits = bits;
    b.words = (R[0] + 31) / 32;
    return b;
}

constexpr double H = 0.5 + 1.0 / 64.0;        // half-width, in cells, of the neighbourhood looked at around a march sample
constexpr double MARGIN = 1.0 / 4096.0;       // growth of a cell, in cell extents, in the exact test

// Does the segment {o + d z : z in [zn, zf]} meet the closed box [a0, a1] grown by e?  Slabs; a NaN never says no.
__device__ inline bool segment_meets_box(const double* o, const double* d, double zn, double zf, const double* a0,
                                         const double* a1, const double* e) {
    double t0 = zn, t1 = zf;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double b0 = a0[a] - e[a], b1 = a1[a] + e[a];
        if (d[a] == 0.0) {
            if (o[a] < b0 || o[a] > b1) return false;
        } else {
            const double ta = (b0 - o[a]) / d[a], tb = (b1 - o[a]) / d[a];
            t0 = fmax(t0, fmin(ta, tb));
            t1 = fmin(t1, fmax(ta, tb));
        }
    }
    return !(t0 > t1);
}

// The rule of include/mnrf.h on one object-frame ray q.  The segment is clipped to the box (grown by H cells), walked in at
// most max(R) + 3 samples no further apart than one cell on any axis; around each sample the set cells within H cells are
// tested exactly.  A cell the segment meets lies within half a cell of the nearest sample on every axis, so it is looked at.
__device__ inline bool keep_ray(const Bounds& A, const float* q) {
    bool finite = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) finite = finite && (fabsf(q[c]) <= 3.4028234663852886e38f);   // false for inf and NaN
    if (!finite) return true;
    const double o[3] = {q[0], q[1], q[2]}, d[3] = {q[3], q[4], q[5]};
    const double zn = q[6], zf = q[7];
    if (zf < zn) return false;                                         // an empty segment meets nothing
    double e[3], blo[3], bhi[3], grow[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        e[a] = A.cell[a] * MARGIN + fabs(o[a]) * 0x1p-40;
        blo[a] = A.lo[a];
        bhi[a] = A.lo[a] + A.cell[a] * A.R[a];
        grow[a] = A.cell[a] * H;
    }
    if (!A.bits) return segment_meets_box(o, d, zn, zf, blo, bhi, e);  // the whole box is one set cell
    // clip to the grown box
    double t0 = zn, t1 = zf, dt = 1.7976931348623157e308;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double b0 = blo[a] - grow[a], b1 = bhi[a] + grow[a];
        if (d[a] == 0.0) {
            if (o[a] < b0 || o[a] > b1) return false;
        } else {
            const double ta = (b0 - o[a]) / d[a], tb = (b1 - o[a]) / d[a];
            t0 = fmax(t0, fmin(ta, tb));
            t1 = fmin(t1, fmax(ta, tb));
            dt = fmin(dt, A.cell[a] / fabs(d[a]));
        }
    }
    if (t0 > t1) return false;
    // (t1 - t0) / dt <= R + 2 H on the axis that gave dt, so n <= max(R) + 2: the trip count is bounded by Rx + Ry + Rz + 3
    const int cap = A.R[0] + A.R[1] + A.R[2] + 2;
    const double steps = ceil((t1 - t0) / dt);
    const int n = steps < (double)cap ? (int)steps : cap;             // (a zero direction: dt is huge, n = 0, one sample)
    const double step = n > 0 ? (t1 - t0) / n : 0.0;
    for (int s = 0; s <= n; ++s) {
        const double t = t0 + step * s;
        int c0[3], c1[3];
        bool any = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double u = (o[a] + d[a] * t - A.lo[a]) / A.cell[a];
            const double f0 = fmax(floor(u - H), 0.0), f1 = fmin(floor(u + H), (double)(A.R[a] - 1));
            any = any && f0 <= f1;
            c0[a] = (int)f0;
            c1[a] = (int)f1;
        }
        if (!any) continue;
        for (int k = c0[2]; k <= c1[2]; ++k)
            for (int j = c0[1]; j <= c1[1]; ++j) {
                const uint32_t* row = A.bits + ((long long)k * A.R[1] + j) * A.words;
                for (int i = c0[0]; i <= c1[0]; ++i) {
                    if (!((row[i >> 5] >> (i & 31)) & 1u)) continue;
                    const double a0[3] = {A.lo[0] + A.cell[0] * i, A.lo[1] + A.cell[1] * j, A.lo[2] + A.cell[2] * k};
                    const double a1[3] = {A.lo[0] + A.cell[0] * (i + 1), A.lo[1] + A.cell[1] * (j + 1), A.lo[2] + A.cell[2] * (k + 1)};
                    if (segment_meets_box(o, d, zn, zf, a0, a1, e)) return true;
                }
            }
    }
    return false;
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
