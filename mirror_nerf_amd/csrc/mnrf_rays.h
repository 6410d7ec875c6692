// mnrf_rays.h -- the pin-hole ray of one pixel (datasets/ray_utils.py:6-53 + blender.py:159-168), shared by the frame kernel
// (mnrf_render.hip: generate_rays_kernel) and the ray bank (mnrf_bank.hip), so that a gathered ray has the bits of the same
// pixel of mnrf_generate_rays: one sequence of fp32 operations, compiled with -ffp-contract=off in both translation units.
#pragma once
#include <hip/hip_runtime.h>

// pixel (column i, row j) of an H x W frame with camera-to-world m (3x4, row-major) -> o[0..8) = [origin, direction, near, far]
__device__ __forceinline__ void mnrf_pinhole_ray(int i, int j, int H, int W, float focal, const float* m, float near, float far,
                                                 float* __restrict__ o) {
    const float dx = ((float)i - (float)W / 2.f) / focal;   // no +0.5 (ray_utils.py:19-24)
    const float dy = -((float)j - (float)H / 2.f) / focal;
    const float dz = -1.f;
    float d[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) d[r] = dx * m[r * 4] + dy * m[r * 4 + 1] + dz * m[r * 4 + 2];
    const float nrm = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    o[0] = m[3]; o[1] = m[7]; o[2] = m[11];
    o[3] = d[0] / nrm; o[4] = d[1] / nrm; o[5] = d[2] / nrm;
    o[6] = near; o[7] = far;
}
