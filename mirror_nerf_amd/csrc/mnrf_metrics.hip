// mnrf_metrics.hip -- structural similarity (SSIM) of rendered frames against their ground truth, on the device.
//
// One windowed-moments kernel serves both definitions the reference uses: scikit-image's structural_similarity
// (tools/eval_metrics.py:25-27: uniform 7x7 window, sample covariance, border cropped) and kornia's ssim behind
// metrics.ssim (metrics.py:18-23: 3x3 Gaussian window, reflect padding, no covariance correction).  They differ only in
// the separable 1-D taps, the border rule, the covariance factor and C1, C2, which are arguments.
//   ssim_tile_kernel    a workgroup takes a TW x TH tile of the output of one (frame, channel): it stages the pred and gt
//                       tiles with their halo in LDS (read in place through the caller's strides, so (H, W, 3) render
//                       outputs and (B, 3, H, W) tensors need no copy), runs the horizontal pass over the five moments
//                       x, y, x^2, y^2, xy into LDS, then the vertical pass, evaluates
//                         S = ((2 ux uy + C1)(2 sxy + C2)) / ((ux^2 + uy^2 + C1)(sx + sy + C2)),  s.. = cov_norm (E[..] - u.u.)
//                       optionally stores S as float32 and writes ONE float64 partial sum
//   ssim_finish_kernel  per frame: the partials in a fixed order, in float64 -> the mean as float32
// Everything between the float32 loads and the float32 stores is float64: sx + sy cancels against C2 = 9e-4, and
// E[x^2] - E[x]^2 in float32 leaves 1e-3 per pixel and 4e-5 in the mean (which also says what bounds
// the kernel's time as far as it has been measured).  No atomics: two runs are bit-identical, and a frame's result does
// not depend on the frames beside it.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mnrf.h"
#include "mnrf_error.h"

namespace {

constexpr int TPB = 256;
constexpr int TW = 32, TH = 16;                         // output tile; TPB threads take TH / (TPB / TW) rows each
constexpr int RMAX = 5;                                 // largest window radius (win_size 11)
constexpr int IW = TW + 2 * RMAX, IH = TH + 2 * RMAX;   // staged tile with halo
constexpr int ROWS_PER_PASS = TPB / TW;
static_assert(TPB % TW == 0 && TH % ROWS_PER_PASS == 0, "tile shape");

struct SsimArgs {
    const float* pred;
    const float* gt;
    long long ps[4], gs[4];      // element strides: pixel (x), row (y), channel, frame
    int H, W, C;
    int Ho, Wo;                  // output size: H - 2r, W - 2r when the border is cropped, H, W when it is reflected
    int tiles_x, tiles_y;
    int r, reflect;
    double taps[2 * RMAX + 1];
    double cov_norm, c1, c2;
    double* partials;
    float* map;                  // (frames, C, Ho, Wo) or null
};

// input coordinate of tap k of output o along an axis of length n; always inside [0, n)
__device__ __forceinline__ int source_index(int o, int n, int reflect, int r) {
    int i = o;                                   // cropped border: output o is centred on input o + r, its window starts at o
    if (reflect) {
        i = o - r;                               // torch "reflect": -1 -> 1, n -> n - 2
        if (i < 0) i = -i;
        if (i >= n) i = 2 * (n - 1) - i;
    }
    return i < 0 ? 0 : (i >= n ? n - 1 : i);     // rows / columns past a ragged tile feed no output
}

__global__ __launch_bounds__(TPB) void ssim_tile_kernel(SsimArgs A) {
    __shared__ float sp[IH][IW + 1], sg[IH][IW + 1];
    __shared__ double hm[5][IH][TW];
    __shared__ double red[TPB / 64];
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int tx = b % A.tiles_x;  b /= A.tiles_x;
    const int ty = b % A.tiles_y;  b /= A.tiles_y;
    const int c = b % A.C;
    const long long f = b / A.C;
    const int ox0 = tx * TW, oy0 = ty * TH;
    const int r = A.r, iw = TW + 2 * r, ih = TH + 2 * r;

    const float* p = A.pred + f * A.ps[3] + c * A.ps[2];
    const float* g = A.gt + f * A.gs[3] + c * A.gs[2];
    for (int i = tid; i < ih * iw; i += TPB) {
        const int iy = i / iw, ix = i - iy * iw;
        const long long y = source_index(oy0 + iy, A.H, A.reflect, r), x = source_index(ox0 + ix, A.W, A.reflect, r);
        sp[iy][ix] = p[y * A.ps[1] + x * A.ps[0]];
        sg[iy][ix] = g[y * A.gs[1] + x * A.gs[0]];
    }
    __syncthreads();

    // horizontal pass: the five moments of every staged row at the tile's TW output columns
    for (int i = tid; i < ih * TW; i += TPB) {
        const int iy = i / TW, col = i % TW;
        double mx = 0., my = 0., mxx = 0., myy = 0., mxy = 0.;
        for (int k = 0; k <= 2 * r; ++k) {
            const double w = A.taps[k], x = sp[iy][col + k], y = sg[iy][col + k];
            mx += w * x;
            my += w * y;
            mxx += w * (x * x);          // products of two float32 are exact in float64
            myy += w * (y * y);
            mxy += w * (x * y);
        }
        hm[0][iy][col] = mx;
        hm[1][iy][col] = my;
        hm[2][iy][col] = mxx;
        hm[3][iy][col] = myy;
        hm[4][iy][col] = mxy;
    }
    __syncthreads();

    // vertical pass and S
    const int col = tid % TW, ox = ox0 + col;
    double sum = 0.;
    for (int row = tid / TW; row < TH; row += ROWS_PER_PASS) {
        const int oy = oy0 + row;
        if (ox >= A.Wo || oy >= A.Ho) continue;
        double ux = 0., uy = 0., exx = 0., eyy = 0., exy = 0.;
        for (int k = 0; k <= 2 * r; ++k) {
            const double w = A.taps[k];
            ux += w * hm[0][row + k][col];
            uy += w * hm[1][row + k][col];
            exx += w * hm[2][row + k][col];
            eyy += w * hm[3][row + k][col];
            exy += w * hm[4][row + k][col];
        }
        const double vx = A.cov_norm * (exx - ux * ux), vy = A.cov_norm * (eyy - uy * uy), vxy = A.cov_norm * (exy - ux * uy);
        const double num = (2. * (ux * uy) + A.c1) * (2. * vxy + A.c2);
        const double den = (ux * ux + uy * uy + A.c1) * (vx + vy + A.c2);
        const double S = num / den;              // identical images: num and den are the same number, S is exactly 1
        sum += S;
        if (A.map) A.map[((f * A.C + c) * A.Ho + oy) * (long long)A.Wo + ox] = (float)S;
    }

    for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o);
    if ((tid & 63) == 0) red[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        double s = 0.;
        for (int w = 0; w < TPB / 64; ++w) s += red[w];
        A.partials[blockIdx.x] = s;
    }
}

// one workgroup per frame: thread t sums partials t, t + TPB, ... in order, then a fixed tree
__global__ __launch_bounds__(TPB) void ssim_finish_kernel(const double* partials, int per_frame, double count, float* out) {
    __shared__ double red[TPB / 64];
    const double* pf = partials + (long long)blockIdx.x * per_frame;
    double s = 0.;
    for (int i = threadIdx.x; i < per_frame; i += TPB) s += pf[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.;
        for (int w = 0; w < TPB / 64; ++w) t += red[w];
        out[blockIdx.x] = (float)(t / count);
    }
}

int64_t tiles_of(int n, int t) { return ((int64_t)n + t - 1) / t; }

}  // namespace

// the workspace for any radius and border rule: the tiles of the H x W image bound the tiles of its (maybe cropped) output
extern "C" int64_t mnrf_ssim_blocks(int H, int W, int frames, int channels) {
    if (H < 1 || W < 1 || frames < 1 || channels < 1) return 0;
    return tiles_of(W, TW) * tiles_of(H, TH) * (int64_t)frames * channels;
}

extern "C" int mnrf_ssim(const float* pred, const int64_t* pred_strides4, const float* gt, const int64_t* gt_strides4, int H,
                         int W, int channels, int frames, const double* taps, int radius, int reflect, double cov_norm,
                         double c1, double c2, double* partials, float* out, float* map, void* stream) {
    if (!pred || !gt || !pred_strides4 || !gt_strides4 || !taps || !partials || !out)
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_ssim: null pointer");
    if (radius < 0 || radius > RMAX) return mnrf_fail(MNRF_ERR_ARG, "mnrf_ssim: window radius must be 0..5");
    if (H < 2 * radius + 1 || W < 2 * radius + 1) return mnrf_fail(MNRF_ERR_ARG, "mnrf_ssim: image smaller than the window");
    if (frames < 1 || channels < 1) return mnrf_fail(MNRF_ERR_ARG, "mnrf_ssim: bad size");
    SsimArgs A;
    A.pred = pred;
    A.gt = gt;
    for (int i = 0; i < 4; ++i) { A.ps[i] = pred_strides4[i]; A.gs[i] = gt_strides4[i]; }
    A.H = H;
    A.W = W;
    A.C = channels;
    A.Ho = reflect ? H : H - 2 * radius;
    A.Wo = reflect ? W : W - 2 * radius;
    A.tiles_x = (int)tiles_of(A.Wo, TW);
    A.tiles_y = (int)tiles_of(A.Ho, TH);
    A.r = radius;
    A.reflect = reflect != 0;
    for (int k = 0; k < 2 * RMAX + 1; ++k) A.taps[k] = k <= 2 * radius ? taps[k] : 0.;
    A.cov_norm = cov_norm;
    A.c1 = c1;
    A.c2 = c2;
    A.partials = partials;
    A.map = map;
    const int64_t per_frame = (int64_t)A.tiles_x * A.tiles_y * channels;
    if (per_frame * frames > 0x7fffffffLL) return mnrf_fail(MNRF_ERR_ARG, "mnrf_ssim: too many tiles for one launch");
    hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)(per_frame * frames)), dim3(TPB), 0, (hipStream_t)stream, A);
    hipLaunchKernelGGL(ssim_finish_kernel, dim3((unsigned)frames), dim3(TPB), 0, (hipStream_t)stream, (const double*)partials,
                       (int)per_frame, (double)A.Ho * A.Wo * channels, out);
    return mnrf_check_launch("mnrf_ssim");
}
