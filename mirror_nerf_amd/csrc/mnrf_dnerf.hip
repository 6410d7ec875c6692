// mnrf_dnerf.hip -- the D-NeRF object field for gfx950: DirectTemporalNeRF (models/d_nerf/run_dnerf_helpers.py:70-253) with
// D = 8, W = 256, skips = [4], multires 10 / 4 and use_viewdirs, as ONE launch per evaluation:
//   positions -> encoding -> deformation net (8 x 256, skip behind the Linear at index 4, 256 -> 3) -> x + dx ->
//   encoding -> canonical trunk (the same shape) -> alpha | feature -> cat[feature, view encoding] -> 128 -> rgb.
//
// Same shape of computation as the fp32 field kernel (mnrf_field.hip, operand layout in mnrf_layout.h): one workgroup = 4
// waves, every wave owns 32 samples for BOTH networks and keeps their activations in registers; every Linear is
// Out^T = W . In^T on v_mfma_f32_16x16x4_f32 (exact fp32 FMA chains); the weight image streams L2 -> LDS in 16-tile chunks
// (mnrf_field_stream.inc) and is shared by the four waves.  What differs from MirrorNeRF is the position of the skip (the SIXTH
// Linear takes cat[encoding, h], MirrorNeRF's fifth does), the 84-wide first layer of the deformation net and its 3-row head
// in the middle of the launch: hence a parts table and a stage sequence of its own.  The GEMM building block below is the
// scheme of mnrf_field_impl.inc (hand-placed ds_read_b128, counted lgkmcnt waits); that file cannot be included for it, it
// would instantiate MirrorNeRF's kernels into this object.
//
// The time encoding (21 channels) is the same for every sample of a launch: every workgroup adds W_time0[:, 63:84] . embed(t)
// to the first layer's bias in its prologue (256 threads x 21 FMAs) instead of spending k-steps per sample on it.
// Compiled with -ffp-contract=off: every fused multiply-add below is an explicit fmaf().
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mnrf.h"
#include "mnrf_layout.h"
#include "mnrf_error.h"

namespace mnrf {

typedef float f32x4 __attribute__((ext_vector_type(4)));
extern __shared__ __attribute__((aligned(16))) char smem[];

namespace dn {

// ------------------------------------------------------------------ the packed image (floats)
//   [deformation stream 1936 tiles][canonical stream 2352 tiles][deformation biases][canonical biases][time columns]
// The canonical stream starts with trunk + alpha, so a sigma-only launch is the prefix of BOTH streams in one piece.
constexpr int N_PARTS = 24;
constexpr int DEF_TILES = 64 + 4 * 256 + 320 + 2 * 256 + 16;              // 1936: L0(enc) L1..L4 L5(enc,h) L6 L7 out
constexpr int CAN_TILES_SIGMA = 64 + 4 * 256 + 320 + 2 * 256 + 16;        // 1936: ... alpha
constexpr int CAN_TILES = CAN_TILES_SIGMA + 256 + 128 + 16 + 16;          // 2352: feature, views (feature | view), rgb
// bias blocks, each padded to its stage's 16 * nb rows; both start with the trunk's 8 x 256 (what trunk() reads at 256 * layer)
constexpr int DB_OUT = 2048;          // 16 (3 used)
constexpr int DB_FLOATS = 2064;
constexpr int CB_ALPHA = 2048;        // 16 (1 used)
constexpr int CB_FEAT = 2064;         // 256
constexpr int CB_VIEWS = 2320;        // 128
constexpr int CB_RGB = 2448;          // 16 (3 used)
constexpr int CB_FLOATS = 2464;
constexpr int N_TIME = 21;            // 1 + 2 * 10 channels of embed(t)
constexpr int64_t OFF_DEF = 0;
constexpr int64_t OFF_CAN = (int64_t)DEF_TILES * TILE_FLOATS;
constexpr int64_t OFF_DBIAS = OFF_CAN + (int64_t)CAN_TILES * TILE_FLOATS;
constexpr int64_t OFF_CBIAS = OFF_DBIAS + DB_FLOATS;
constexpr int64_t OFF_TIME = OFF_CBIAS + CB_FLOATS;                       // [21][256]: column 63 + j of _time.0, row n at [j * 256 + n]
constexpr int64_t IMAGE_FLOATS = OFF_TIME + N_TIME * 256;
static_assert(DEF_TILES % PAD_TILES == 0 && CAN_TILES_SIGMA % PAD_TILES == 0 && CAN_TILES % PAD_TILES == 0, "chunking");
static_assert(DB_FLOATS <= BIAS_FLOATS && CB_FLOATS <= BIAS_FLOATS && DB_FLOATS % 4 == 0 && CB_FLOATS % 4 == 0, "bias blocks share one LDS region");
static_assert(OFF_DBIAS % 4 == 0 && OFF_CBIAS % 4 == 0, "16-byte loads of the bias blocks");

struct Parts {
    Part p[N_PARTS];
};

// state_dict order: _occ.pts_linears.i -> 2i, views_linears.0 -> 16, feature_linear -> 18, alpha_linear -> 20, rgb_linear -> 22,
// _time.i -> 24 + 2i, _time_out -> 40 (biases at the odd index behind)
inline void build_parts(Parts& T) {
    int n = 0, tile = 0;
    auto add = [&](int param, int n_true, int ld, int ntq, int nb, int col_off, int kind) {
        T.p[n++] = Part{param, n_true, ld, ntq, nb, col_off, kind, tile};
        tile += padded_tiles(ntq * nb);
    };
    for (int net = 0; net < 2; ++net) {
        const int p0 = net == 0 ? 24 : 0;                                   // the deformation net comes first in the image
        add(p0, 256, net == 0 ? ENC_XYZ + N_TIME : ENC_XYZ, 4, 16, 0, KIND_ENC);          // L0: the 63 position columns
        for (int i = 1; i < 5; ++i) add(p0 + 2 * i, 256, 256, 16, 16, 0, KIND_H);         // L1..L4
        add(p0 + 10, 256, 319, 4, 16, 0, KIND_ENC);                                       // L5: encoding columns first
        add(p0 + 10, 256, 319, 16, 16, ENC_XYZ, KIND_H);                                  // L5: hidden columns
        for (int i = 6; i < 8; ++i) add(p0 + 2 * i, 256, 256, 16, 16, 0, KIND_H);         // L6, L7
        if (net == 0) add(40, 3, 256, 16, 1, 0, KIND_H);                                  // _time_out
        else add(20, 1, 256, 16, 1, 0, KIND_H);                                           // alpha_linear
    }
    add(18, 256, 256, 16, 16, 0, KIND_H);                                                 // feature_linear
    add(16, 128, 283, 16, 8, 0, KIND_H);                                                  // views_linears.0: feature columns
    add(16, 128, 283, 2, 8, 256, KIND_DIR);                                               // views_linears.0: view columns
    add(22, 3, 128, 8, 1, 0, KIND_H);                                                     // rgb_linear
}

struct PackArgs {
    const float* params[MNRF_DNERF_N_PARAMS];
    float* packed;
};

__global__ void pack_kernel(PackArgs P, Parts T) {
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= IMAGE_FLOATS) return;
    float v = 0.f;
    if (p < OFF_DBIAS) {
        // ---- tiles: float j of lane l of tile (tq, nb) = W[16*nb + (l&15)][col(4*tq + j, l>>4)]   (mnrf_layout.h)
        const int tile = (int)(p / TILE_FLOATS);
        const int within = (int)(p % TILE_FLOATS);
        const int lane = within >> 2, j = within & 3, g = lane >> 4, i = lane & 15;
        int k = 0;
        while (k + 1 < N_PARTS && T.p[k + 1].tile0 <= tile) ++k;
        const Part pt = T.p[k];
        const int lt = tile - pt.tile0;
        const int tq = lt / pt.nb, nb = lt % pt.nb;   // tq >= ntq: chunk padding behind a short part
        const int n = 16 * nb + i;
        const int t = 4 * tq + j;
        int col;
        if (pt.kind == KIND_ENC) col = enc_col(t, g);
        else {
            col = 16 * (t >> 2) + 4 * g + (t & 3);
            if (pt.kind == KIND_DIR && col >= ENC_DIR) col = -1;
        }
        if (tq < pt.ntq && n < pt.n_true && col >= 0) v = P.params[pt.param][(long long)n * pt.ld + pt.col_off + col];
    } else if (p < OFF_CBIAS) {
        const int b = (int)(p - OFF_DBIAS);
        if (b < DB_OUT) v = P.params[24 + 2 * (b / 256) + 1][b % 256];
        else if (b - DB_OUT < 3) v = P.params[41][b - DB_OUT];
    } else if (p < OFF_TIME) {
        const int b = (int)(p - OFF_CBIAS);
        if (b < CB_ALPHA) v = P.params[2 * (b / 256) + 1][b % 256];
        else if (b < CB_FEAT) { if (b - CB_ALPHA < 1) v = P.params[21][0]; }
        else if (b < CB_VIEWS) v = P.params[19][b - CB_FEAT];
        else if (b < CB_RGB) v = P.params[17][b - CB_VIEWS];
        else if (b - CB_RGB < 3) v = P.params[23][b - CB_RGB];
    } else {
        const int q = (int)(p - OFF_TIME);
        const int j = q / 256, n = q % 256;
        v = P.params[24][n * (ENC_XYZ + N_TIME) + ENC_XYZ + j];
    }
    P.packed[p] = v;
}

// ------------------------------------------------------------------ the kernel's tuning: 32 samples per wave, one wave per SIMD
constexpr int S = 2;
constexpr int CHUNK_TILES = 16;
constexpr int CHUNK_BYTES = CHUNK_TILES * TILE_BYTES;
static_assert(PAD_TILES % CHUNK_TILES == 0, "stream padding");
constexpr int WAVES = 4;
constexpr int WG_THREADS = 64 * WAVES;
constexpr int WG_SAMPLES = WAVES * S * 16;
constexpr int RING_SLOTS = 3;
constexpr int PIECES = CHUNK_TILES / WAVES;
constexpr int LDS_RING = RING_SLOTS * CHUNK_BYTES;
constexpr int LDS_BIAS = LDS_RING;                       // the bias block of the network being evaluated
constexpr int LDS_BYTES = LDS_BIAS + BIAS_FLOATS * 4;

#include "mnrf_field_stream.inc"

// ------------------------------------------------------------------ GEMM building block (the scheme of mnrf_field_impl.inc)
// acc[s][nb] += sum over the part's k-steps of  A(tile) x b[s][4*tq + j].  Every part starts on a chunk seam of the stream.
// A operands are read PF tiles ahead of their MFMAs with hand-placed ds_read_b128 and COUNTED lgkmcnt waits (in-order LDS
// return makes `lgkmcnt(n)` = "all but the n youngest reads have landed"); scripts/check_isa.py asserts that no scalar-memory
// load, which returns out of order on the same counter, sits between the first and the last MFMA of the kernel.
constexpr int U = 4;       // tiles per unit: one counted wait per 32 MFMAs
constexpr int PF = 4;      // tiles in flight ahead of the unit being consumed
constexpr int NBUF = PF + U;

__device__ __forceinline__ void lds_read_tile(f32x4& dst, unsigned addr, int off) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(off) : "memory");
}

// the tiles about to be consumed are in/out operands: that data dependence is what keeps their MFMAs below the wait
#define MNRF_WAIT_CASE(n) \
    if (N == n) asm volatile("s_waitcnt lgkmcnt(" #n ")" : "+v"(t0), "+v"(t1), "+v"(t2), "+v"(t3) : : "memory");
template <int N>
__device__ __forceinline__ void wait_lds_reads_but(f32x4& t0, f32x4& t1, f32x4& t2, f32x4& t3) {
    static_assert(N >= 0 && N <= 4, "PF <= 4");
    MNRF_WAIT_CASE(0) MNRF_WAIT_CASE(1) MNRF_WAIT_CASE(2) MNRF_WAIT_CASE(3) MNRF_WAIT_CASE(4)
}
#undef MNRF_WAIT_CASE

template <int NTQ, int NB, int NACC, int NT>
__device__ __forceinline__ void gemm_part(f32x4 (&acc)[S][NACC], const float (&b)[S][NT], Stream& st, int wave, int lane16) {
    constexpr int NTILES = NTQ * NB;   // the stream pads every part to whole chunks
    static_assert(NTILES % U == 0, "tiles come in units");
    static_assert(4 * NTQ <= NT && NB <= NACC, "operand sizes");
    const unsigned ring = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem + (unsigned)lane16;
    f32x4 a[NBUF];
    advance(st, wave);
    unsigned base = ring + st.rd_slot * CHUNK_BYTES;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // compiler-issued LDS and scalar traffic is out of the way
#pragma unroll
    for (int i = 0; i < PF && i < NTILES; ++i) lds_read_tile(a[i], base, i * TILE_BYTES);
    // two short nested loops: a single 256-trip loop is only partially unrolled, which turns the register arrays into scratch
    constexpr int NUNITS = NTILES / U;
    constexpr int INNER = NUNITS < 16 ? NUNITS : 16;
    static_assert(NUNITS % INNER == 0, "unit count");
#pragma unroll
    for (int uo = 0; uo < NUNITS / INNER; ++uo) {
#pragma unroll
    for (int ui = 0; ui < INNER; ++ui) {
        const int t = (uo * INNER + ui) * U;
        __builtin_amdgcn_sched_barrier(0);   // one scheduling region per unit (keeps the A-tile live ranges short)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int r = t + PF + u;
            if (r < NTILES) {
                if (r % CHUNK_TILES == 0) {
                    advance(st, wave);
                    base = ring + st.rd_slot * CHUNK_BYTES;
                }
                lds_read_tile(a[r % NBUF], base, (r % CHUNK_TILES) * TILE_BYTES);
            }
        }
        // reads still allowed in flight: everything younger than the unit's last tile
        const int rem = NTILES - t - U;
        const int younger = rem < PF ? rem : PF;
        f32x4& x0 = a[t % NBUF];
        f32x4& x1 = a[(t + 1) % NBUF];
        f32x4& x2 = a[(t + 2) % NBUF];
        f32x4& x3 = a[(t + 3) % NBUF];
        if (younger == 0) wait_lds_reads_but<0>(x0, x1, x2, x3);
        else if (younger == 1) wait_lds_reads_but<1>(x0, x1, x2, x3);
        else if (younger == 2) wait_lds_reads_but<2>(x0, x1, x2, x3);
        else if (younger == 3) wait_lds_reads_but<3>(x0, x1, x2, x3);
        else wait_lds_reads_but<4>(x0, x1, x2, x3);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int tq = (t + u) / NB, nb = (t + u) % NB;
#pragma unroll
                for (int s = 0; s < S; ++s)
                    acc[s][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[(t + u) % NBUF][j], b[s][4 * tq + j], acc[s][nb], 0, 0, 0);
            }
        }
    }
    }
    // step over the pad chunks behind a short part
    constexpr int USED_CHUNKS = (NTILES + CHUNK_TILES - 1) / CHUNK_TILES;
    constexpr int PART_CHUNKS = padded_tiles(NTILES) / CHUNK_TILES;
#pragma unroll
    for (int c = USED_CHUNKS; c < PART_CHUNKS; ++c) advance(st, wave);
}

// acc[s][nb][r] = bias[16*nb + 4*g + r]   (the bias block lives in LDS behind the ring)
template <int NB, int NACC>
__device__ __forceinline__ void init_bias(f32x4 (&acc)[S][NACC], int bias_off, int g) {
    const f32x4* bl = (const f32x4*)(smem + LDS_BIAS) + (bias_off >> 2);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const f32x4 v = bl[nb * 4 + g];
#pragma unroll
        for (int s = 0; s < S; ++s) acc[s][nb] = v;
    }
}

template <int NB, bool RELU, int NT>
__device__ __forceinline__ void to_bform(float (&h)[S][NT], const f32x4 (&acc)[S][NB]) {
    static_assert(NT == 4 * NB, "accumulator block r of a layer is k-steps 4*nb + r of the next");
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) h[s][4 * nb + r] = RELU ? fmaxf(acc[s][nb][r], 0.f) : acc[s][nb][r];
}

// this lane's 16 of the 64 (padded) channels of the position encoding: pairs P = 8g + pp (mnrf_layout.h enc_col)
__device__ __forceinline__ void encode(float (&enc)[S][16], const float (&x)[S][3], int g) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
#pragma unroll
        for (int pp = 0; pp < 8; ++pp) {
            const int P = 8 * g + pp;
            const int f = P / 3;
            const int a = P - 3 * f;
            const float xa = a == 0 ? x[s][0] : (a == 1 ? x[s][1] : x[s][2]);
            float sn, cs;
            sincosf(ldexpf(xa, f), &sn, &cs);    // x * 2^f is exact (run_dnerf_helpers.py:35, 41); accurate range reduction
            if (P >= 30) {                       // raw coordinates ride in the last two pairs
                sn = P == 30 ? x[s][0] : x[s][2];
                cs = P == 30 ? x[s][1] : 0.f;
            }
            enc[s][2 * pp] = sn;
            enc[s][2 * pp + 1] = cs;
        }
    }
}

// 8 x 256 trunk with the skip behind the Linear at index 4 (run_dnerf_helpers.py:129-133, 233-237): h = relu(L7(...)).
__device__ __forceinline__ void trunk(float (&h)[S][64], const float (&enc)[S][16], Stream& st, int wave, int lane16, int g) {
    f32x4 acc[S][16];
    init_bias<16>(acc, 0, g);
    gemm_part<4, 16>(acc, enc, st, wave, lane16);
    to_bform<16, true>(h, acc);
#pragma unroll 1
    for (int l = 1; l < 5; ++l) {
        init_bias<16>(acc, 256 * l, g);
        gemm_part<16, 16>(acc, h, st, wave, lane16);
        to_bform<16, true>(h, acc);
    }
    init_bias<16>(acc, 256 * 5, g);                      // L5: cat[encoding, h], encoding first
    gemm_part<4, 16>(acc, enc, st, wave, lane16);
    gemm_part<16, 16>(acc, h, st, wave, lane16);
    to_bform<16, true>(h, acc);
#pragma unroll 1
    for (int l = 6; l < 8; ++l) {
        init_bias<16>(acc, 256 * l, g);
        gemm_part<16, 16>(acc, h, st, wave, lane16);
        to_bform<16, true>(h, acc);
    }
}

struct Args {
    const float* packed;
    unsigned flags;
    long long B;
    const float* xyz;
    long long xyz_stride;
    const float* rays;
    const float* z_vals;
    int spr;
    const float* dir_emb;
    long long dir_stride;
    float t;
    float* sigma;
    float* rgb;
    float* dx;
};

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

template <bool SIGMA_ONLY, bool CANONICAL>
__global__ __launch_bounds__(WG_THREADS, 1) void dnerf_kernel(Args A) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4;     // lane group = k-slot / row quad
    const int m = lane & 15;     // sample within the group
    const int lane16 = lane * 16;
    float* const lbias = (float*)(smem + LDS_BIAS);

    // ---- bias block of the first network -> LDS (visible behind open_stream's barrier)
    if (CANONICAL) {
        const f32x4* src = (const f32x4*)(A.packed + OFF_CBIAS);
        for (int i = tid; i < CB_FLOATS / 4; i += WG_THREADS) ((f32x4*)lbias)[i] = src[i];
    } else {
        const f32x4* src = (const f32x4*)(A.packed + OFF_DBIAS);
        for (int i = tid + 64; i < DB_FLOATS / 4; i += WG_THREADS) ((f32x4*)lbias)[i] = src[i];     // floats 256 .. : as stored
        // first layer: bias + W_time0[:, 63:84] . embed(t), one row per thread; embed(t) = [t, sin(2^f t), cos(2^f t) ...]
        float b = A.packed[OFF_DBIAS + tid];
        const float* tw = A.packed + OFF_TIME + tid;
        b = fmaf(tw[0], A.t, b);
#pragma unroll
        for (int f = 0; f < NFREQ_XYZ; ++f) {
            float sn, cs;
            sincosf(ldexpf(A.t, f), &sn, &cs);
            b = fmaf(tw[(1 + 2 * f) * 256], sn, b);
            b = fmaf(tw[(2 + 2 * f) * 256], cs, b);
        }
        lbias[tid] = b;
    }

    Stream st;
    if (CANONICAL) open_stream(st, A.packed + OFF_CAN, SIGMA_ONLY ? CAN_TILES_SIGMA : CAN_TILES, wave, lane);
    else open_stream(st, A.packed + OFF_DEF, DEF_TILES + (SIGMA_ONLY ? CAN_TILES_SIGMA : CAN_TILES), wave, lane);

    // ---- sample positions (run_dnerf.py:523-525: multiply, then add -- no FMA)
    long long idx[S];
    bool valid[S];
    float x[S][3];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        long long i = (long long)blockIdx.x * WG_SAMPLES + wave * (S * 16) + s * 16 + m;
        valid[s] = i < A.B;
        if (!valid[s]) i = A.B - 1;
        idx[s] = i;
        if (A.xyz) {
            const float* p = A.xyz + i * A.xyz_stride;
            x[s][0] = p[0]; x[s][1] = p[1]; x[s][2] = p[2];
        } else {
            const long long ray = i / A.spr;
            const float* r = A.rays + ray * 8;
            const float z = A.z_vals[i];
#pragma unroll
            for (int a = 0; a < 3; ++a) x[s][a] = r[a] + r[3 + a] * z;
        }
    }

    float enc[S][16];
    float h[S][64];
    if (!CANONICAL) {
        // ---- deformation net on the encoding of the unwarped point; its skip reads that encoding too
        encode(enc, x, g);
        trunk(h, enc, st, wave, lane16, g);
        f32x4 acc[S][1];
        init_bias<1>(acc, DB_OUT, g);
        gemm_part<16, 1>(acc, h, st, wave, lane16);
        // rows 0..2 of the head live in lane group 0 (lane = sample), registers 0..2: hand them to the other three groups
#pragma unroll
        for (int s = 0; s < S; ++s) {
            float d[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) d[a] = __shfl(acc[s][0][a], m, 64);
            if (A.dx && g == 0 && valid[s]) {
                float* o = A.dx + idx[s] * 3;
                o[0] = d[0]; o[1] = d[1]; o[2] = d[2];
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) x[s][a] = x[s][a] + d[a];       // run_dnerf_helpers.py:152, one fp32 add
        }
        // ---- the canonical network's biases take the LDS region over
        __syncthreads();
        const f32x4* src = (const f32x4*)(A.packed + OFF_CBIAS);
        for (int i = tid; i < CB_FLOATS / 4; i += WG_THREADS) ((f32x4*)lbias)[i] = src[i];
        __syncthreads();
    } else if (A.dx && g == 0) {
#pragma unroll
        for (int s = 0; s < S; ++s)
            if (valid[s]) {
                float* o = A.dx + idx[s] * 3;
                o[0] = 0.f; o[1] = 0.f; o[2] = 0.f;
            }
    }

    // ---- canonical network on the encoding of x + dx
    encode(enc, x, g);
    trunk(h, enc, st, wave, lane16, g);
    {
        f32x4 acc[S][1];
        init_bias<1>(acc, CB_ALPHA, g);
        gemm_part<16, 1>(acc, h, st, wave, lane16);
        if (A.sigma && g == 0) {
#pragma unroll
            for (int s = 0; s < S; ++s)
                if (valid[s]) A.sigma[idx[s]] = acc[s][0][0];              // raw: raw2outputs applies the ReLU
        }
    }
    if (SIGMA_ONLY) return;

    // ---- colour: feature (256 -> 256, no activation); cat[feature, view encoding] -> 128 relu; 128 -> 3
    float fin[S][64];
    {
        f32x4 acc[S][16];
        init_bias<16>(acc, CB_FEAT, g);
        gemm_part<16, 16>(acc, h, st, wave, lane16);
        to_bform<16, false>(fin, acc);
    }
    float de[S][8];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const float* dp = A.dir_emb + (idx[s] / A.spr) * A.dir_stride;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const int e = 16 * (t >> 2) + 4 * g + (t & 3);
            de[s][t] = e < ENC_DIR ? dp[e] : 0.f;
        }
    }
    float hd[S][32];
    {
        f32x4 acc[S][8];
        init_bias<8>(acc, CB_VIEWS, g);
        gemm_part<16, 8>(acc, fin, st, wave, lane16);
        gemm_part<2, 8>(acc, de, st, wave, lane16);
        to_bform<8, true>(hd, acc);
    }
    f32x4 acc[S][1];
    init_bias<1>(acc, CB_RGB, g);
    gemm_part<8, 1>(acc, hd, st, wave, lane16);
    if (A.rgb && g == 0) {
        const bool raw = A.flags & MNRF_DNERF_RAW_RGB;
#pragma unroll
        for (int s = 0; s < S; ++s)
            if (valid[s]) {
                float* o = A.rgb + idx[s] * 3;
#pragma unroll
                for (int a = 0; a < 3; ++a) o[a] = raw ? acc[s][0][a] : sigmoidf_(acc[s][0][a]);
            }
    }
}

}  // namespace dn
}  // namespace mnrf

// ====================================================================== C ABI
using namespace mnrf;

extern "C" int64_t mnrf_dnerf_packed_floats(void) { return dn::IMAGE_FLOATS; }

extern "C" int mnrf_dnerf_pack_weights(const float* const* params, float* packed, void* stream) {
    if (!params || !packed) return mnrf_fail(MNRF_ERR_ARG, "mnrf_dnerf_pack_weights: null pointer");
    dn::PackArgs P;
    for (int i = 0; i < MNRF_DNERF_N_PARAMS; ++i) {
        if (!params[i]) return mnrf_fail(MNRF_ERR_ARG, "mnrf_dnerf_pack_weights: null parameter pointer");
        P.params[i] = params[i];
    }
    P.packed = packed;
    dn::Parts T;
    dn::build_parts(T);
    const int threads = 256;
    const int blocks = (int)((dn::IMAGE_FLOATS + threads - 1) / threads);
    hipLaunchKernelGGL(dn::pack_kernel, dim3(blocks), dim3(threads), 0, (hipStream_t)stream, P, T);
    return mnrf_check_launch("mnrf_dnerf_pack_weights");
}

extern "C" int mnrf_dnerf_forward(const float* packed, unsigned flags, int64_t B, const float* xyz, int64_t xyz_stride,
                                  const float* rays, const float* z_vals, int spr, const float* dir_emb, int64_t dir_stride,
                                  float t, float* sigma, float* rgb, float* dx, void* stream) {
    if (!packed) return mnrf_fail(MNRF_ERR_ARG, "mnrf_dnerf_forward: packed weights are null");
    if (flags & ~(MNRF_DNERF_SIGMA_ONLY | MNRF_DNERF_RAW_RGB | MNRF_DNERF_CANONICAL))
        return mnrf_fail(MNRF_ERR_ARG, "mnrf_dnerf_forward: unknown flag bits");
    if (B < 0) return mnrf_fail(MNRF_ERR_ARG, "mnrf_dnerf_forward: negative sample count");
    const bool sigma_only = flags & MNRF_DNERF_SIGMA_ONLY;
    const bool canonical = flags & MNRF_DNERF_CANONICAL;
    if (!xyz && (!rays || !z_vals)) return mnrf_fail(MNRF_ERR_ARG, "mnrf_dnerf_forward: need xyz or rays+z_vals");
    if (xyz && xyz_stride < 3) return mnrf_fail(MNRF_ERR_ARG, "mnrf_dnerf_forward: xyz_stride < 3");
    if (spr < 1) return mnrf_fail(MNRF_ERR_ARG, "mnrf_dnerf_forward: samples per ray must be >= 1");
    if (!xyz && B % spr != 0) return mnrf_fail(MNRF_ERR_ARG, "mnrf_dnerf_forward: B not a multiple of spr");
    if (!sigma_only && !dir_emb) return mnrf_fail(MNRF_ERR_ARG, "mnrf_dnerf_forward: dir_emb required unless SIGMA_ONLY");
    if (!sigma_only && dir_stride < ENC_DIR) return mnrf_fail(MNRF_ERR_ARG, "mnrf_dnerf_forward: dir_stride < 27");
    if (!(t == t) || t - t != 0.f) return mnrf_fail(MNRF_ERR_ARG, "mnrf_dnerf_forward: the time must be finite");
    if (B == 0) return MNRF_OK;
    const long long blocks = (B + dn::WG_SAMPLES - 1) / dn::WG_SAMPLES;
    if (blocks > 0x7fffffff) return mnrf_fail(MNRF_ERR_ARG, "mnrf_dnerf_forward: too many samples for one launch");
    dn::Args A{packed, flags, (long long)B, xyz, (long long)xyz_stride, rays, z_vals, spr, dir_emb, (long long)dir_stride, t,
               sigma, rgb, dx};
    const dim3 grid((unsigned)blocks), block(dn::WG_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (sigma_only && canonical) hipLaunchKernelGGL((dn::dnerf_kernel<true, true>), grid, block, dn::LDS_BYTES, s, A);
    else if (sigma_only) hipLaunchKernelGGL((dn::dnerf_kernel<true, false>), grid, block, dn::LDS_BYTES, s, A);
    else if (canonical) hipLaunchKernelGGL((dn::dnerf_kernel<false, true>), grid, block, dn::LDS_BYTES, s, A);
    else hipLaunchKernelGGL((dn::dnerf_kernel<false, false>), grid, block, dn::LDS_BYTES, s, A);
    return mnrf_check_launch("mnrf_dnerf_forward");
}
