// mnrf_resample.hip -- the ingest step of the ray bank on the device: decoded frames at their native size are resized to the
// training size where they live, instead of on the host before the upload (datasets/real_arkit.py:236-237, 251-264:
// `img.resize(img_wh, Image.LANCZOS)` and `cv2.resize(mask, img_wh, interpolation=cv2.INTER_NEAREST)` per frame).
//
//   resample_pass_kernel   one separable pass of Pillow's 8-bit resampler (its Resample.c path for 8-bit images), along x or y
//   mask_nearest_kernel    nearest-neighbour pick of a 1- or 2-byte mask and the reference's threshold, to int8
//
// ARITHMETIC of a pass.  Output sample i along the resized axis has a window [lo_i, lo_i + n_i) of the source axis and n_i
// fixed-point weights with 22 fraction bits, both made on the host in double (data.lanczos_taps) and handed in as tables:
//   bounds (out, 2) int32   lo_i, n_i
//   taps (ksize, out) int32 tap k of output i at [k * out + i]: transposed, so that in the pass along x the lanes of a wave,
//                           which hold consecutive i, read consecutive words; in the pass along y, i is uniform in a wave
//   value = clamp(((1 << 21) + sum_k source[lo_i + k] * tap[k]) >> 22, 0, 255)        accumulated in 32-bit integers
// The pass along x runs first over every source row into the caller's `tmp` (frames, src_h, dst_w, C) and rounds to 8 bits
// there -- that rounding is part of the definition -- then the pass along y.  A pass whose sizes agree is not run; when both
// agree there is nothing to do and the call is refused (the caller copies).
// With four channels the image is RGBA: the colours are premultiplied where the first pass loads them,
//   t = c * a + 128;  c' = ((t >> 8) + t) >> 8
// and divided out again where the last pass stores them: a of 0 or 255 leaves c', otherwise min(255, 255 * c' / a) in integer
// division.  The alpha channel itself is resampled as it is.
//
// BOUNDS.  The tables come from outside the library, which cannot inspect device memory: every window is clamped to
// [0, source extent) and to ksize taps before it is used, so a wrong table gives wrong pixels but no read outside the frame
// or the table.  Nothing is assumed about alignment (RGB rows are 3 bytes per pixel): samples are read and written as bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/mnrf.h"
#include "mnrf_error.h"

namespace {

constexpr int TPB = 256;                 // a multiple of 64 lanes along the output x
constexpr int PRECISION_BITS = 32 - 8 - 2;
constexpr unsigned ROWS_MAX = 65535;     // gridDim.y; further rows are reached by striding

struct PassArgs {
    const uint8_t* src;      // (frames, src_h, src_w, C)
    uint8_t* dst;            // (frames, dst_h, dst_w, C)
    const int32_t* taps;     // (ksize, out)
    const int32_t* bounds;   // (out, 2)
    long long frames;
    int src_h, src_w, dst_h, dst_w, ksize;
    int premultiply, unpremultiply;
};

__device__ __forceinline__ uint32_t clip8(uint32_t acc) {
    const int32_t v = (int32_t)acc >> PRECISION_BITS;
    return v < 0 ? 0u : (v > 255 ? 255u : (uint32_t)v);
}

// AXIS 0: along x (dst_h == src_h); AXIS 1: along y (dst_w == src_w).  One thread per output pixel, all of its channels.
template <int C, int AXIS>
__global__ __launch_bounds__(TPB) void resample_pass_kernel(PassArgs A) {
    const int ox = blockIdx.x * TPB + threadIdx.x;
    if (ox >= A.dst_w) return;
    const long long rows = A.frames * A.dst_h;
    const int out = AXIS == 0 ? A.dst_w : A.dst_h, extent = AXIS == 0 ? A.src_w : A.src_h;
    for (long long row = blockIdx.y; row < rows; row += gridDim.y) {
        const long long f = row / A.dst_h;
        const int oy = (int)(row - f * A.dst_h);
        const int i = AXIS == 0 ? ox : oy;
        int lo = A.bounds[2 * i], n = A.bounds[2 * i + 1];
        lo = lo < 0 ? 0 : (lo > extent ? extent : lo);
        n = n < 0 ? 0 : n;
        n = n > A.ksize ? A.ksize : n;
        n = n > extent - lo ? extent - lo : n;
        // the first sample of the window and the step to the next one, in pixels
        const long long first = AXIS == 0 ? (f * A.src_h + oy) * A.src_w + lo : (f * A.src_h + lo) * A.src_w + ox;
        const long long step = AXIS == 0 ? 1 : A.src_w;
        const uint8_t* p = A.src + first * C;
        const int32_t* t = A.taps + i;
        uint32_t acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 1u << (PRECISION_BITS - 1);
        for (int k = 0; k < n; ++k) {
            const uint32_t w = (uint32_t)t[(long long)k * out];
            uint32_t v[C];
#pragma unroll
            for (int c = 0; c < C; ++c) v[c] = p[c];
            if (C == 4 && A.premultiply) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint32_t m = v[c] * v[3] + 128u;
                    v[c] = ((m >> 8) + m) >> 8;
                }
            }
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += v[c] * w;      // wraps like Pillow's int; in range for a normalised table
            p += step * C;
        }
        uint32_t b[C];
#pragma unroll
        for (int c = 0; c < C; ++c) b[c] = clip8(acc[c]);
        if (C == 4 && A.unpremultiply && b[3] != 0u && b[3] != 255u) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t q = (255u * b[c]) / b[3];
                b[c] = q > 255u ? 255u : q;
            }
        }
        uint8_t* o = A.dst + ((f * A.dst_h + oy) * A.dst_w + ox) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) o[c] = (uint8_t)b[c];
    }
}

template <typename T>
__global__ __launch_bounds__(TPB) void mask_nearest_kernel(const T* src, int8_t* dst, long long frames, int src_h, int src_w,
                                                           int dst_h, int dst_w) {
    const int ox = blockIdx.x * TPB + threadIdx.x;
    if (ox >= dst_w) return;
    // data._resize_nearest: floor(x * (src / dst)) in double, clamped to the last sample
    int sx = (int)floor((double)ox * ((double)src_w / (double)dst_w));
    sx = sx > src_w - 1 ? src_w - 1 : sx;
    const long long rows = frames * dst_h;
    for (long long row = blockIdx.y; row < rows; row += gridDim.y) {
        const long long f = row / dst_h;
        const int oy = (int)(row - f * dst_h);
        int sy = (int)floor((double)oy * ((double)src_h / (double)dst_h));
        sy = sy > src_h - 1 ? src_h - 1 : sy;
        const unsigned v = src[(f * src_h + sy) * src_w + sx];
        // 8 bit: /255, then the 0.5 thresholds -> >= 128; 16 bit: unscaled, so anything above 0 is a mirror
        dst[(f * dst_h + oy) * dst_w + ox] = (int8_t)(sizeof(T) == 1 ? (v >= 128u) : (v > 0u));
    }
}

dim3 grid_for(int dst_w, int64_t rows) {
    return dim3((unsigned)((dst_w + TPB - 1) / TPB), (unsigned)(rows > ROWS_MAX ? ROWS_MAX : rows));
}

template <int AXIS>
void launch_pass(int channels, const PassArgs& A, hipStream_t s) {
    const dim3 g = grid_for(A.dst_w, A.frames * A.dst_h);
    if (channels == 3) hipLaunchKernelGGL((resample_pass_kernel<3, AXIS>), g, dim3(TPB), 0, s, A);
    else hipLaunchKernelGGL((resample_pass_kernel<4, AXIS>), g, dim3(TPB), 0, s, A);
}

constexpr int64_t BYTES_MAX = 0x7fffffffffffffffLL / 8;
constexpr int SIDE_MAX = 1 << 30;        // block index * TPB stays inside an int

// frames * a * b * c, or -1 when it leaves BYTES_MAX
int64_t product(int64_t frames, int a, int b, int c) {
    int64_t n = frames;
    for (int64_t v : {(int64_t)a, (int64_t)b, (int64_t)c}) {
        if (n > BYTES_MAX / v) return -1;
        n *= v;
    }
    return n;
}

const char* bad_shape(int64_t frames, int src_h, int src_w, int dst_h, int dst_w) {
    if (frames < 1 || src_h < 1 || src_w < 1 || dst_h < 1 || dst_w < 1) return "sizes must be at least 1";
    if (src_h > SIDE_MAX || src_w > SIDE_MAX || dst_h > SIDE_MAX || dst_w > SIDE_MAX) return "sizes are too large";
    if (product(frames, src_h, src_w > dst_w ? src_w : dst_w, 4) < 0 || product(frames, dst_h, dst_w, 4) < 0)
        return "sizes are too large";
    return nullptr;
}

int fail_shape(const char* who, const char* why) {
    char msg[96];
    snprintf(msg, sizeof msg, "%s: %s", who, why);
    return mnrf_fail(MNRF_ERR_ARG, msg);
}

}  // namespace

extern "C" int64_t mnrf_resample_tmp_bytes(int64_t frames, int src_h, int src_w, int dst_h, int dst_w, int channels) {
    if ((channels != 3 && channels != 4) || bad_shape(frames, src_h, src_w, dst_h, dst_w)) return -1;
    if (src_h == dst_h || src_w == dst_w) return 0;      // at most one pass: nothing in between
    return product(frames, src_h, dst_w, channels);
}

extern "C" int mnrf_resample_u8(const uint8_t* src, int64_t frames, int src_h, int src_w, int channels, uint8_t* dst, int dst_h,
                                int dst_w, const int32_t* taps_x, const int32_t* bounds_x, int ksize_x, const int32_t* taps_y,
                                const int32_t* bounds_y, int ksize_y, uint8_t* tmp, void* stream) {
    if (channels != 3 && channels != 4) return mnrf_fail(MNRF_ERR_ARG, "mnrf_resample_u8: channels must be 3 or 4");
    if (const char* why = bad_shape(frames, src_h, src_w, dst_h, dst_w)) {
        return fail_shape("mnrf_resample_u8", why);
    }
    const bool along_x = src_w != dst_w, along_y = src_h != dst_h;
    if (!along_x && !along_y)
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_resample_u8: both passes skipped (the sizes agree): copy instead");
    if (!src || !dst) return mnrf_fail(MNRF_ERR_ARG, "mnrf_resample_u8: null source or destination");
    if (along_x && (!taps_x || !bounds_x || ksize_x < 1))
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_resample_u8: the pass along x needs its taps, bounds and ksize >= 1");
    if (along_y && (!taps_y || !bounds_y || ksize_y < 1))
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_resample_u8: the pass along y needs its taps, bounds and ksize >= 1");
    if (along_x && along_y && !tmp)
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_resample_u8: two passes need the tmp buffer (mnrf_resample_tmp_bytes)");
    hipStream_t s = (hipStream_t)stream;
    if (along_x) {
        const PassArgs A{src, along_y ? tmp : dst, taps_x, bounds_x, (long long)frames, src_h, src_w, src_h, dst_w, ksize_x,
                         1, along_y ? 0 : 1};
        launch_pass<0>(channels, A, s);
    }
    if (along_y) {
        const PassArgs A{along_x ? tmp : src, dst, taps_y, bounds_y, (long long)frames, src_h, dst_w, dst_h, dst_w, ksize_y,
                         along_x ? 0 : 1, 1};
        launch_pass<1>(channels, A, s);
    }
    return mnrf_check_launch("mnrf_resample_u8");
}

extern "C" int mnrf_mask_nearest(const void* src, int sample_bytes, int64_t frames, int src_h, int src_w, int8_t* dst, int dst_h,
                                 int dst_w, void* stream) {
    if (sample_bytes != 1 && sample_bytes != 2) return mnrf_fail(MNRF_ERR_ARG, "mnrf_mask_nearest: samples have 1 or 2 bytes");
    if (const char* why = bad_shape(frames, src_h, src_w, dst_h, dst_w)) {
        return fail_shape("mnrf_mask_nearest", why);
    }
    if (!src || !dst) return mnrf_fail(MNRF_ERR_ARG, "mnrf_mask_nearest: null source or destination");
    if (sample_bytes == 2 && ((uintptr_t)src & 1)) return mnrf_fail(MNRF_ERR_ARG, "mnrf_mask_nearest: 2-byte samples at an odd address");
    const dim3 g = grid_for(dst_w, frames * dst_h);
    hipStream_t s = (hipStream_t)stream;
    if (sample_bytes == 1)
        hipLaunchKernelGGL(mask_nearest_kernel<uint8_t>, g, dim3(TPB), 0, s, (const uint8_t*)src, dst, (long long)frames, src_h,
                           src_w, dst_h, dst_w);
    else
        hipLaunchKernelGGL(mask_nearest_kernel<uint16_t>, g, dim3(TPB), 0, s, (const uint16_t*)src, dst, (long long)frames, src_h,
                           src_w, dst_h, dst_w);
    return mnrf_check_launch("mnrf_mask_nearest");
}
