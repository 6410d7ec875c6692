// mnrf_bank.hip -- training batches from a device-resident image bank (datasets/blender.py:51-108, 159-168, 191-204).
//
// The reference builds every ray of every training image on the host as float32 (12 floats = 48 B per ray) and lets a shuffling
// DataLoader hand out batches.  Here the frames stay on the device as the bytes they were decoded to -- poses (F, 3, 4) float32,
// images (F, H, W, C) uint8, mirror masks (F, H, W) int8: C + 1 bytes per pixel -- and ONE launch turns B pixel indices into
// rays (B, 8), rgbs (B, 3) and mirror_mask (B):
//   bank_gather_kernel   the pixels named by explicit global indices (or start, start + 1, ...: a whole frame)
//   bank_draw_kernel     the B pixels of one step of a shuffled stream, the indices made in registers
// A global index g addresses slot g / (H*W) and pixel g % (H*W); a slot is a frame, or frames[slot] under a frame list (the
// reference's *_wmask subset).  Per row:
//   rays         mnrf_pinhole_ray (mnrf_rays.h): the bits of the same pixel of mnrf_generate_rays
//   rgbs         float(v) / 255.0f per channel; four channels: rgb * a + (1 - a) as separate fp32 multiply, subtract, add
//                (blender.py:128-133)
//   mirror_mask  the int8 value (-1: no ground-truth mask, 0, 1) as a float
//   valid_mask   last channel > 0 (blender.py:129: the alpha of RGBA, the blue of RGB)
// An index outside [0, N) or a frame number outside [0, n_frames) reads nothing and gives a row of NaN (valid 0).
//
// THE SHUFFLED STREAM (the contract; restated in integers by tests/raybank_ref.py).  N = slots * H * W < 2^32.  Lane l of rank r
// in a world of w at step s takes stream position p = (s * w + r) * B + l (64-bit, unsigned); epoch = p / N, i = p % N and
// g = perm(seed, epoch)(i): the stream is one permutation of [0, N) per epoch, every pixel once per epoch, and a batch may
// straddle two epochs.  perm is a keyed bijection that needs no memory:
//   half  = ceil(max(2, bit_length(N - 1)) / 2), mask = 2^half - 1            (a domain of 2^(2 half) < 4 N values)
//   mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16      (uint32; "lowbias32")
//   key_r = mix32(mix32(mix32(mix32(seed_lo + 0x9e3779b9 * (r + 1)) ^ seed_hi) ^ epoch_lo) ^ epoch_hi),  r = 0 .. 5
//   one pass over x: (L, R) = (x >> half, x & mask); six rounds (L, R) <- (R, L ^ (mix32(R ^ key_r) & mask)); x = L << half | R
//   perm(i): x = i; pass; while x >= N: pass       (cycle walking)
// A pass is a balanced Feistel network, a permutation of the power-of-two domain whatever the round function is; the walk from
// i < N stays on i's cycle and therefore reaches a value below N (i itself at the latest), and distinct i end on distinct
// values.  The domain is under 4 N, so the expected number of passes is below 4.
//
// One thread per ray, 256-thread blocks, plain vector stores; B is ~1024: nothing to tune, what it replaces is seven launches
// and their host work.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/mnrf.h"
#include "mnrf_error.h"
#include "mnrf_rays.h"

namespace {

constexpr int TPB = 256;
constexpr int ROUNDS = 6;

struct Outs {
    float* rays;             // (n, 8) or null
    float* rgbs;             // (n, 3) or null
    float* mask;             // (n) or null
    unsigned char* valid;    // (n) or null
    long long* indices;      // (n) or null
};

__device__ __forceinline__ void bank_row(const MnrfBank& b, long long N, long long g, long long row, const Outs& o) {
    if (o.indices) o.indices[row] = g;
    const long long hw = (long long)b.H * b.W;
    long long f = -1, pix = 0;
    if (g >= 0 && g < N) {
        const long long slot = g / hw;
        pix = g - slot * hw;
        f = b.frames ? (long long)b.frames[slot] : slot;
        if (f >= b.n_frames) f = -1;
    }
    if (f < 0) {
        const float q = __builtin_nanf("");
        if (o.rays) for (int k = 0; k < 8; ++k) o.rays[row * 8 + k] = q;
        if (o.rgbs) for (int k = 0; k < 3; ++k) o.rgbs[row * 3 + k] = q;
        if (o.mask) o.mask[row] = q;
        if (o.valid) o.valid[row] = 0;
        return;
    }
    if (o.rays) {
        float m[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) m[k] = b.poses[f * 12 + k];
        mnrf_pinhole_ray((int)(pix % b.W), (int)(pix / b.W), b.H, b.W, b.focal, m, b.near, b.far, o.rays + row * 8);
    }
    const unsigned char* px = b.images + (f * hw + pix) * b.channels;
    if (o.rgbs) {
        float c[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = (float)px[k] / 255.0f;
        if (b.channels == 4) {
            const float a = (float)px[3] / 255.0f;
            const float rest = 1.f - a;
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = c[k] * a + rest;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) o.rgbs[row * 3 + k] = c[k];
    }
    if (o.mask) o.mask[row] = (float)b.masks[f * hw + pix];
    if (o.valid) o.valid[row] = px[b.channels - 1] > 0;
}

__global__ __launch_bounds__(TPB) void bank_gather_kernel(MnrfBank b, long long N, const long long* __restrict__ indices,
                                                          long long start, long long n, Outs o) {
    const long long row = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    bank_row(b, N, indices ? indices[row] : start + row, row, o);
}

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du;
    x ^= x >> 15; x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ uint32_t bank_perm(uint32_t i, uint32_t N, int half, uint64_t seed, uint64_t epoch) {
    uint32_t key[ROUNDS];
#pragma unroll
    for (int r = 0; r < ROUNDS; ++r)
        key[r] = mix32(mix32(mix32(mix32((uint32_t)seed + 0x9e3779b9u * (uint32_t)(r + 1)) ^ (uint32_t)(seed >> 32)) ^ (uint32_t)epoch) ^
                       (uint32_t)(epoch >> 32));
    const uint32_t mask = (1u << half) - 1u;
    uint32_t x = i;
    do {
        uint32_t L = x >> half, R = x & mask;
#pragma unroll
        for (int r = 0; r < ROUNDS; ++r) {
            const uint32_t t = L ^ (mix32(R ^ key[r]) & mask);
            L = R;
            R = t;
        }
        x = (L << half) | R;
    } while (x >= N);
    return x;
}

__global__ __launch_bounds__(TPB) void bank_draw_kernel(MnrfBank b, uint32_t N, int half, uint64_t seed, uint64_t step,
                                                        const long long* __restrict__ step_dev, uint64_t rank, uint64_t world,
                                                        long long batch, Outs o) {
    const long long lane = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= batch) return;
    const uint64_t s = step + (step_dev ? (uint64_t)*step_dev : 0ull);
    const uint64_t p = (s * world + rank) * (uint64_t)batch + (uint64_t)lane;
    const uint64_t epoch = p / N;
    const uint32_t i = (uint32_t)(p - epoch * N);
    bank_row(b, (long long)N, (long long)bank_perm(i, N, half, seed, epoch), lane, o);
}

// shapes and pointers of a bank; N = slots * H * W through *n_out
int check_bank(const MnrfBank* b, const char* who_shape, const char* who_null, int64_t* n_out) {
    if (!b) return mnrf_fail(MNRF_ERR_ARG, who_null);
    if (b->n_frames < 1 || b->H < 1 || b->W < 1 || (b->channels != 3 && b->channels != 4) || b->slots < 0 ||
        (!b->frames && b->slots != b->n_frames))
        return mnrf_fail(MNRF_ERR_ARG, who_shape);
    if ((double)b->slots * (double)b->H * (double)b->W >= 9.0e18) return mnrf_fail(MNRF_ERR_ARG, who_shape);   // three 31-bit factors
    *n_out = (int64_t)b->slots * b->H * b->W;
    return MNRF_OK;
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + TPB - 1) / TPB); }

}  // namespace

extern "C" int mnrf_bank_gather(const MnrfBank* bank, const int64_t* indices, int64_t start, int64_t n, float* rays, float* rgbs,
                                float* mirror_mask, uint8_t* valid_mask, void* stream) {
    int64_t N = 0;
    const int rc = check_bank(bank, "mnrf_bank_gather: bad bank shape (frames, H, W >= 1, 3 or 4 channels, slots)",
                              "mnrf_bank_gather: null bank", &N);
    if (rc) return rc;
    if (n < 0 || n > 0x7fffffffLL * TPB) return mnrf_fail(MNRF_ERR_ARG, "mnrf_bank_gather: bad row count");
    if (!indices && (start < 0 || start > N || n > N - start))
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_bank_gather: start .. start + n leaves the bank");
    if (n == 0) return MNRF_OK;
    if (!bank->poses || !bank->images || !bank->masks) return mnrf_fail(MNRF_ERR_ARG, "mnrf_bank_gather: null bank array");
    const Outs o{rays, rgbs, mirror_mask, valid_mask, nullptr};
    hipLaunchKernelGGL(bank_gather_kernel, dim3(blocks_of(n)), dim3(TPB), 0, (hipStream_t)stream, *bank, (long long)N,
                       (const long long*)indices, (long long)start, (long long)n, o);
    return mnrf_check_launch("mnrf_bank_gather");
}

extern "C" int mnrf_bank_draw(const MnrfBank* bank, uint64_t seed, int64_t step, const int64_t* step_dev, int rank, int world,
                              int64_t batch, float* rays, float* rgbs, float* mirror_mask, uint8_t* valid_mask,
                              int64_t* indices_out, void* stream) {
    int64_t N = 0;
    const int rc = check_bank(bank, "mnrf_bank_draw: bad bank shape (frames, H, W >= 1, 3 or 4 channels, slots)",
                              "mnrf_bank_draw: null bank", &N);
    if (rc) return rc;
    if (N >= (1LL << 32)) return mnrf_fail(MNRF_ERR_ARG, "mnrf_bank_draw: slots * H * W must be below 2^32 (the permutation's domain)");
    if (N < 1) return mnrf_fail(MNRF_ERR_ARG, "mnrf_bank_draw: the bank has no pixel to draw from");
    if (world < 1 || rank < 0 || rank >= world) return mnrf_fail(MNRF_ERR_ARG, "mnrf_bank_draw: rank must lie in [0, world)");
    if (step < 0) return mnrf_fail(MNRF_ERR_ARG, "mnrf_bank_draw: negative step");
    if (batch < 0 || batch > 0x7fffffffLL) return mnrf_fail(MNRF_ERR_ARG, "mnrf_bank_draw: bad batch size");
    if (batch == 0) return MNRF_OK;
    if (!bank->poses || !bank->images || !bank->masks) return mnrf_fail(MNRF_ERR_ARG, "mnrf_bank_draw: null bank array");
    int bits = 0;
    for (uint64_t v = (uint64_t)N - 1; v; v >>= 1) ++bits;
    if (bits < 2) bits = 2;
    const Outs o{rays, rgbs, mirror_mask, valid_mask, (long long*)indices_out};
    hipLaunchKernelGGL(bank_draw_kernel, dim3(blocks_of(batch)), dim3(TPB), 0, (hipStream_t)stream, *bank, (uint32_t)N,
                       (bits + 1) / 2, seed, (uint64_t)step, (const long long*)step_dev, (uint64_t)rank, (uint64_t)world,
                       (long long)batch, o);
    return mnrf_check_launch("mnrf_bank_draw");
}
