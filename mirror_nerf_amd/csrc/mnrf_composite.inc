// mnrf_composite.inc -- alpha compositing of ONE ray by one wavefront (models/rendering.py:181-264, 362-367), shared by
// composite_kernel (mnrf_render.hip: per-sample inputs from HBM) and the ray-fused fine pass of the field kernel
// (mnrf_field_split.inc FUSE: per-sample inputs from LDS, never written to HBM).  ONE body, so that both produce the same
// maps bit for bit: the transmittance T_i = prod_{j<i} (1 - alpha_j + 1e-10) is an exclusive prefix product over the lanes
// (Hillis-Steele over __shfl_up), carried across 64-sample blocks; 13 wave reductions at the end.
// Included inside a namespace that provides wave_sum(float).  `Src`: has_noise/has_rgb/has_mirror/has_pn/has_gn,
// z(s), sigma(s), noise(s), rgb(s,k), mirror(s), pn(s,k), gn(s,k) for sample s of this ray; has_w / w(s): the weights themselves,
// formed before by composite_mirror_value() from the same inputs (the scan is then not repeated).
struct CompMaps {
    float* weights;      // this ray's row of the (n_rays, S) weights, or null
    float* opacity; float* rgb_map; float* depth; float* mirror_mask;
    float* surf_normal; float* surf_normal_grad; float* normal_dif; float* x_surface;
    const float* rays;   // (n_rays, 8): x_surface = o + d * depth
    int white_back;
};

// One 64-sample block of the weights: alpha of sample s (rendering.py:182-192), the exclusive prefix product of the transmittance
// over the lanes (195), carried across blocks in `carry`, w = alpha * T (197-199).  The ONE place where weights are formed: whoever
// calls it with the same inputs gets the same bits.  `zv`: the sample's depth (0 outside the ray).
template <class Src>
__device__ __forceinline__ float composite_weight(const Src& src, int S, int s, bool in, int lane, float& carry, float& zv) {
    float alpha = 0.f;
    zv = 0.f;
    if (in) {
        zv = src.z(s);
        const float delta = s + 1 < S ? src.z(s + 1) - zv : 1e10f;   // rendering.py:182-186
        float sv = src.sigma(s);
        if (src.has_noise()) sv = sv + src.noise(s);
        alpha = 1.f - expf(-delta * fmaxf(sv, 0.f));                 // 190-192
    }
    const float t = in ? (1.f - alpha) + 1e-10f : 1.f;              // 195
    float incl = t;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float up = __shfl_up(incl, o);
        if (lane >= o) incl *= up;
    }
    float excl = __shfl_up(incl, 1);
    if (lane == 0) excl = 1.f;
    const float w = alpha * (carry * excl);                         // 197-199
    carry = carry * __shfl(incl, 63);
    return w;
}

// The composited mirror value of the ray alone, in every lane: the weights of composite_weight() and the mirror sum in the order
// and with the reduction of composite_ray() below, so the value equals the mirror_mask that composite_ray() writes for the same
// inputs bit for bit.  For a kernel that decides from it BEFORE the colours exist (the blended-level variant of the ray-fused
// pass).  `w_keep` (or null): the weights are kept there for the composite_ray() that follows (Src::has_w / w).
template <class Src>
__device__ __forceinline__ float composite_mirror_value(const Src& src, int S, int lane, float* w_keep) {
    float carry = 1.f;
    float a_m = 0.f;
#pragma unroll
    for (int base = 0; base < S; base += 64) {
        const int s = base + lane;
        const bool in = s < S;
        float zv;
        const float w = composite_weight(src, S, s, in, lane, carry, zv);
        if (in) {
            if (w_keep) w_keep[s] = w;
            a_m += w * src.mirror(s);
        }
    }
    return wave_sum(a_m);
}

template <class Src>
__device__ __forceinline__ void composite_ray(const Src& src, int S, int lane, long long ray, const CompMaps& A) {
    float carry = 1.f;
    float a_op = 0.f, a_d = 0.f, a_m = 0.f, a_nd = 0.f;
    float a_c[3] = {0.f, 0.f, 0.f}, a_n[3] = {0.f, 0.f, 0.f}, a_g[3] = {0.f, 0.f, 0.f};
    for (int base = 0; base < S; base += 64) {
        const int s = base + lane;
        const bool in = s < S;
        float zv, w;
        if (src.has_w()) {      // the weights were formed before, by composite_mirror_value()
            zv = in ? src.z(s) : 0.f;
            w = in ? src.w(s) : 0.f;
        } else {
            w = composite_weight(src, S, s, in, lane, carry, zv);
        }
        if (in) {
            if (A.weights) A.weights[s] = w;
            a_op += w;
            a_d += w * zv;
            if (src.has_rgb()) { a_c[0] += w * src.rgb(s, 0); a_c[1] += w * src.rgb(s, 1); a_c[2] += w * src.rgb(s, 2); }
            if (src.has_mirror()) a_m += w * src.mirror(s);
            float pn[3] = {0.f, 0.f, 0.f}, gn[3] = {0.f, 0.f, 0.f};
            if (src.has_pn()) {
#pragma unroll
                for (int k = 0; k < 3; ++k) { pn[k] = src.pn(s, k); a_n[k] += pn[k] * w; }
            }
            if (src.has_gn()) {
#pragma unroll
                for (int k = 0; k < 3; ++k) { gn[k] = src.gn(s, k); a_g[k] += gn[k] * w; }
            }
            if (src.has_pn() && src.has_gn()) {
                const float d0 = gn[0] - pn[0], d1 = gn[1] - pn[1], d2 = gn[2] - pn[2];
                a_nd += w * (d0 * d0 + d1 * d1 + d2 * d2);
            }
        }
    }
    // (a sum whose input the source does not have stays 0 without its reduction: with a source that knows this at compile time,
    // as the rgb / depth variant of the ray-fused pass does, those shuffles are not even emitted)
    a_op = wave_sum(a_op);
    a_d = wave_sum(a_d);
    if (src.has_mirror()) a_m = wave_sum(a_m);
    if (src.has_pn() && src.has_gn()) a_nd = wave_sum(a_nd);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (src.has_rgb()) a_c[k] = wave_sum(a_c[k]);
        if (src.has_pn()) a_n[k] = wave_sum(a_n[k]);
        if (src.has_gn()) a_g[k] = wave_sum(a_g[k]);
    }
    if (lane == 0) {
        if (A.opacity) A.opacity[ray] = a_op;
        if (A.rgb_map) {
#pragma unroll
            for (int k = 0; k < 3; ++k) A.rgb_map[ray * 3 + k] = A.white_back ? a_c[k] + (1.f - a_op) : a_c[k];
        }
        if (A.depth) A.depth[ray] = a_d;
        if (A.mirror_mask) A.mirror_mask[ray] = a_m;
        if (A.surf_normal) { for (int k = 0; k < 3; ++k) A.surf_normal[ray * 3 + k] = a_n[k]; }
        if (A.surf_normal_grad) { for (int k = 0; k < 3; ++k) A.surf_normal_grad[ray * 3 + k] = a_g[k]; }
        if (A.normal_dif) A.normal_dif[ray] = a_nd;
        if (A.x_surface) {
            const float* r = A.rays + ray * 8;
            for (int k = 0; k < 3; ++k) A.x_surface[ray * 3 + k] = r[k] + r[3 + k] * a_d;   // 362-367
        }
    }
}
