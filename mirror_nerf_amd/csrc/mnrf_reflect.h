// mnrf_reflect.h -- the reflected direction of one ray, shared by every kernel that builds secondary rays (reflect_compact_kernel
// and reflect_all_kernel of mnrf_render.hip, reflect_jitter_fan_kernel of mnrf_rough.hip): one set of expressions, one order,
// so the same ray, normal and draw give the same bits whichever launch formed them.
#pragma once

namespace mnrf_reflect {

constexpr float EPS32 = 1.1920928955078125e-07f;  // torch.finfo(float32).eps, utils/func.py:5

// normal: the ray's 3 normal components; noise: its 3 standard-normal draws or null (eval.py:506-511, 625-660: normal + draw * std);
// d: the ray's direction.  r = 2 (w.n) n - w with n = l2n(normal [+ noise * std]), w = l2n(-d) (utils/func.py:5-7,
// train.py:217-228, eval.py:515-523); every operation a single fp32 one (the library is compiled with -ffp-contract=off).
__device__ __forceinline__ void direction(const float* __restrict__ normal, const float* __restrict__ noise, float noise_std,
                                          const float d[3], float r[3]) {
    float nv[3], wvv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        nv[k] = normal[k];
        if (noise) nv[k] = nv[k] + noise[k] * noise_std;
        wvv[k] = -d[k];
    }
    const float ninv = 1.f / sqrtf(fmaxf(nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2], EPS32));
    const float winv = 1.f / sqrtf(fmaxf(wvv[0] * wvv[0] + wvv[1] * wvv[1] + wvv[2] * wvv[2], EPS32));
#pragma unroll
    for (int k = 0; k < 3; ++k) { nv[k] = nv[k] * ninv; wvv[k] = wvv[k] * winv; }
    const float c = wvv[0] * nv[0] + wvv[1] * nv[1] + wvv[2] * nv[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) r[k] = 2.f * c * nv[k] - wvv[k];
}

}  // namespace mnrf_reflect
