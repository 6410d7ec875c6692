// mnrf_field_impl.inc -- body of the fused field kernel, included once per tuning variant from
// mnrf_field.hip inside its own namespace, with these names defined by the includer:
//   S        16-sample groups per wave (2: one wave per SIMD, 1: two workgroups per CU)
//   MIN_WAVES_PER_SIMD  second argument of __launch_bounds__
// See mnrf_field.hip for the description of the computation.
// CHUNK_TILES: LDS staging granule of this tuning (16 or 32 tiles; must divide PAD_TILES)
constexpr int CHUNK_BYTES = CHUNK_TILES * TILE_BYTES;
static_assert(PAD_TILES % CHUNK_TILES == 0, "stream padding");
constexpr int WAVES = 4;
constexpr int WG_THREADS = 64 * WAVES;
constexpr int WG_SAMPLES = WAVES * S * 16;
constexpr int RING_SLOTS = 3;
constexpr int PIECES = CHUNK_TILES / WAVES;   // 1 KiB LDS-DMA pieces each wave issues per chunk
constexpr int LDS_RING = RING_SLOTS * CHUNK_BYTES;  // staging ring
constexpr int LDS_BIAS = LDS_RING;         // bias block
constexpr int LDS_MASK = LDS_BIAS + BIAS_FLOATS * 4;   // relu masks [8 layers][S][256 threads] x 8 B (GRAD only)
constexpr int LDS_BYTES = LDS_MASK;
constexpr int LDS_BYTES_GRAD = LDS_MASK + 8 * S * WG_THREADS * 8;

#include "mnrf_field_stream.inc"

// ------------------------------------------------------------------ GEMM building block
// acc[s][nb] += sum over the part's k-steps of  A(tile) x b[s][4*tq + j].
// Every part starts on a chunk seam of the stream.  A operands are read PF tiles ahead of their
// MFMAs with hand-placed ds_read_b128 and COUNTED lgkmcnt waits: left to itself hipcc sinks the
// reads next to their first use and drains lgkmcnt to 0 (676 full drains per 1700 reads), which
// exposes the LDS latency to the MFMA pipe.  In-order LDS return makes `lgkmcnt(n)` = "all but
// the n youngest reads have landed"; scripts/check_isa.py asserts that no scalar-memory load
// (out-of-order on the same counter) sits between the first and the last MFMA of the kernel.
// Tiles are consumed in units of U = 2: one counted wait per 8*S MFMAs, and with one sample group
// per wave (S == 1) consecutive MFMAs still alternate between two accumulators (the dependent-issue
// latency of v_mfma_f32_16x16x4_f32 is 40 cycles against a 32-cycle issue interval).
constexpr int U = S == 2 ? 4 : 2;   // s2 has the registers for a longer unit
constexpr int PF = 4;      // tiles in flight ahead of the unit being consumed
constexpr int NBUF = PF + U;

// `off` is a compile-time constant once the tile loops are unrolled: it goes into the instruction's
// 16-bit offset field, so a chunk needs one address register and no per-tile VALU add (every
// non-MFMA issue state between two MFMAs costs matrix-pipe time).
__device__ __forceinline__ void lds_read_tile(f32x4& dst, unsigned addr, int off) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(off) : "memory");
}

// Wait until all but the N youngest LDS reads have landed.  The tiles about to be consumed are
// in/out operands of the statement: MFMA builtins are pure register operations that the optimiser
// moves freely across `asm volatile` (a "memory" clobber does not order them), so the only thing
// that keeps a consumer below its wait is this data dependence.
#define MNRF_WAIT_CASE(n)                                                                                   \
    if (N == n) {                                                                                           \
        if (U == 2) asm volatile("s_waitcnt lgkmcnt(" #n ")" : "+v"(t0), "+v"(t1) : : "memory");          \
        else asm volatile("s_waitcnt lgkmcnt(" #n ")" : "+v"(t0), "+v"(t1), "+v"(t2), "+v"(t3) : : "memory"); \
    }
template <int N>
__device__ __forceinline__ void wait_lds_reads_but(f32x4& t0, f32x4& t1, f32x4& t2, f32x4& t3) {
    static_assert(N >= 0 && N <= 4, "PF <= 4");
    MNRF_WAIT_CASE(0) MNRF_WAIT_CASE(1) MNRF_WAIT_CASE(2) MNRF_WAIT_CASE(3) MNRF_WAIT_CASE(4)
}
#undef MNRF_WAIT_CASE

template <int NTQ, int NB, int NACC, int NT>
__device__ __forceinline__ void gemm_part(f32x4 (&acc)[S][NACC], const float (&b)[S][NT], Stream& st,
                                          int& tile0, int wave, int lane16) {
    constexpr int NTILES = NTQ * NB;   // the stream pads every part to whole chunks
    static_assert(NTILES % U == 0, "tiles come in units");
    const unsigned ring = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem + (unsigned)lane16;
    f32x4 a[NBUF];
    advance(st, wave);
    unsigned base = ring + st.rd_slot * CHUNK_BYTES;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // compiler-issued LDS traffic (bias reads, mask stores) is out of the way
#pragma unroll
    for (int i = 0; i < PF && i < NTILES; ++i) lds_read_tile(a[i], base, i * TILE_BYTES);
    // two short nested loops: a single 256-trip loop is only partially unrolled by hipcc, which turns
    // the register arrays into scratch
    constexpr int NUNITS = NTILES / U;
    constexpr int INNER = NUNITS < 16 ? NUNITS : 16;
    static_assert(NUNITS % INNER == 0, "unit count");
#pragma unroll
    for (int uo = 0; uo < NUNITS / INNER; ++uo) {
#pragma unroll
    for (int ui = 0; ui < INNER; ++ui) {
        const int t = (uo * INNER + ui) * U;
        // one scheduling region per unit: without it the scheduler drags MFMAs many tiles away from
        // their wait, stretches the A-tile live ranges and spills (s1 runs at ~250 of 256 registers)
        __builtin_amdgcn_sched_barrier(0);
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
        f32x4& x2 = a[(t + 2) % NBUF];     // third and fourth tile of the unit: named only when U == 4
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
                for (int s = 0; s < S; ++s) {
                    acc[s][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[(t + u) % NBUF][j], b[s][4 * tq + j],
                                                                      acc[s][nb], 0, 0, 0);
                }
            }
        }
    }
    }
    // a tuning whose chunk is smaller than the stream's padding unit steps over the pad chunks
    constexpr int USED_CHUNKS = (NTILES + CHUNK_TILES - 1) / CHUNK_TILES;
    constexpr int PART_CHUNKS = padded_tiles(NTILES) / CHUNK_TILES;
#pragma unroll
    for (int c = USED_CHUNKS; c < PART_CHUNKS; ++c) advance(st, wave);
    tile0 += padded_tiles(NTILES);
}

// acc[s][nb][r] = bias[16*nb + 4*g + r]   (bias block lives in LDS behind the ring)
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

template <int NB, int NACC>
__device__ __forceinline__ void zero_acc(f32x4 (&acc)[S][NACC]) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int s = 0; s < S; ++s) acc[s][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
}

// h = relu(acc); with WANT_MASK the 64-bit relu mask of the layer (bit t <=> the
// pre-activation feeding k-step t is > 0) is parked in LDS for the gradient pass.
template <bool WANT_MASK>
__device__ __forceinline__ void relu_to(float (&h)[S][64], const f32x4 (&acc)[S][16], int layer, int tid,
                                        unsigned long long* gmask) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
        uint64_t m = 0;
#pragma unroll
        for (int nb = 0; nb < 16; ++nb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = acc[s][nb][r];
                if (WANT_MASK) m |= (uint64_t)(v > 0.f) << (4 * nb + r);
                h[s][4 * nb + r] = fmaxf(v, 0.f);
            }
        }
        if (WANT_MASK) {
            ((uint64_t*)(smem + LDS_MASK))[(layer * S + s) * WG_THREADS + tid] = m;
            if (gmask) gmask[(layer * S + s) * WG_THREADS + tid] = m;   // training: kept for the backward kernel
        }
    }
}

__device__ __forceinline__ void apply_mask(float (&gr)[S][64], int layer, int tid) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const uint64_t m = ((const uint64_t*)(smem + LDS_MASK))[(layer * S + s) * WG_THREADS + tid];
#pragma unroll
        for (int t = 0; t < 64; ++t) gr[s][t] = ((m >> t) & 1ull) ? gr[s][t] : 0.f;
    }
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }

// Store a B-form activation (NT k-steps = 4*NT/4 columns per lane) as [sample][4*... logical columns].
template <int NT>
__device__ __forceinline__ void save_bform(float* sec, long long B, int width, const float (&x)[S][NT],
                                           const long long (&idx)[S], const bool (&valid)[S], int g) {
    (void)B;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        if (!valid[s]) continue;
        f32x4* o = (f32x4*)(sec + idx[s] * width);
#pragma unroll
        for (int nb = 0; nb < NT / 4; ++nb)      // (non-temporal like the split path's rows, mnrf_field_split.inc row_store: 11 KB per
            __builtin_nontemporal_store(f32x4{x[s][4 * nb], x[s][4 * nb + 1], x[s][4 * nb + 2], x[s][4 * nb + 3]}, o + nb * 4 + g);      // sample streamed past the weight stream in L2)
    }
}

// ------------------------------------------------------------------ the kernel
template <bool SIGMA_ONLY, bool GRAD>
__global__ __launch_bounds__(WG_THREADS, MIN_WAVES_PER_SIMD) void field_kernel(FieldArgs A) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4;     // lane group = k-slot / row quad
    const int m = lane & 15;     // sample within the group
    const int lane16 = lane * 16;

    // bias block -> LDS (read by init_bias, visible after the first advance() barrier)
    {
        const f32x4* src = (const f32x4*)(A.packed + OFF_BIAS);
        f32x4* dst = (f32x4*)(smem + LDS_BIAS);
        for (int i = tid; i < BIAS_FLOATS / 4; i += WG_THREADS) dst[i] = src[i];
    }

    Stream st;
    open_stream(st, A.packed + OFF_FWD, SIGMA_ONLY ? FWD_TILES_SIGMA : FWD_TILES, wave, lane);

    // ---- sample positions (rendering.py:302: multiply, then add -- no FMA)
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

    // ---- xyz encoding, this lane's 16 of the 64 (padded) channels: pairs P = 8g + pp
    float enc[S][16];
#pragma unroll
    for (int s = 0; s < S; ++s) {
#pragma unroll
        for (int pp = 0; pp < 8; ++pp) {
            const int P = 8 * g + pp;
            const int f = P / 3;
            const int a = P - 3 * f;
            const float xa = a == 0 ? x[s][0] : (a == 1 ? x[s][1] : x[s][2]);
            float sn, cs;
            sincosf(ldexpf(xa, f), &sn, &cs);   // 2^f * x is exact (mirror_nerf.py:17, 36)
            if (P >= 30) {                       // raw coordinates ride in the last two pairs
                sn = P == 30 ? x[s][0] : x[s][2];
                cs = P == 30 ? x[s][1] : 0.f;
            }
            enc[s][2 * pp] = sn;
            enc[s][2 * pp + 1] = cs;
        }
    }

    unsigned long long* gmask = A.save_mask ? A.save_mask + (long long)blockIdx.x * (N_MASKS * S * WG_THREADS) : nullptr;
    if (A.save_x) save_bform(A.save_x + (long long)SEC_ENC * A.B, A.B, 64, enc, idx, valid, g);
    int tile0 = 0;
    float h[S][64];
    {
        // ---- L1: enc(64) -> 256
        f32x4 acc[S][16];
        __syncthreads();   // bias block visible
        init_bias<16>(acc, BIAS_L, g);
        gemm_part<4, 16>(acc, enc, st, tile0, wave, lane16);
        relu_to<GRAD>(h, acc, 0, tid, gmask);
        if (A.save_x) save_bform(A.save_x + (long long)SEC_H * A.B, A.B, 256, h, idx, valid, g);
        // ---- L2..L4
#pragma unroll 1
        for (int l = 0; l < 3; ++l) {
            init_bias<16>(acc, BIAS_L + 256 * (1 + l), g);
            gemm_part<16, 16>(acc, h, st, tile0, wave, lane16);
            relu_to<GRAD>(h, acc, 1 + l, tid, gmask);
            if (A.save_x) save_bform(A.save_x + (long long)(SEC_H + 256 * (1 + l)) * A.B, A.B, 256, h, idx, valid, g);
        }
        // ---- L5: cat[enc, h] -> 256  (encoding first: mirror_nerf.py:192-193)
        init_bias<16>(acc, BIAS_L + 256 * 4, g);
        gemm_part<4, 16>(acc, enc, st, tile0, wave, lane16);
        gemm_part<16, 16>(acc, h, st, tile0, wave, lane16);
        relu_to<GRAD>(h, acc, 4, tid, gmask);
        if (A.save_x) save_bform(A.save_x + (long long)(SEC_H + 256 * 4) * A.B, A.B, 256, h, idx, valid, g);
        // ---- L6..L8
#pragma unroll 1
        for (int l = 0; l < 3; ++l) {
            init_bias<16>(acc, BIAS_L + 256 * (5 + l), g);
            gemm_part<16, 16>(acc, h, st, tile0, wave, lane16);
            relu_to<GRAD>(h, acc, 5 + l, tid, gmask);
            if (A.save_x) save_bform(A.save_x + (long long)(SEC_H + 256 * (5 + l)) * A.B, A.B, 256, h, idx, valid, g);
        }
    }
    // h = geo_feat (mirror_nerf.py:195)
    if (A.geo_feat) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
            if (valid[s]) {
                f32x4* o = (f32x4*)(A.geo_feat + idx[s] * 256);
#pragma unroll
                for (int nb = 0; nb < 16; ++nb)
                    o[nb * 4 + g] = f32x4{h[s][4 * nb], h[s][4 * nb + 1], h[s][4 * nb + 2], h[s][4 * nb + 3]};
            }
        }
    }
    // ---- sigma: 256 -> 1 (row 0 of a padded 16-row block lives in lane group 0, reg 0)
    {
        f32x4 acc[S][1];
        init_bias<1>(acc, BIAS_SIG, g);
        gemm_part<16, 1>(acc, h, st, tile0, wave, lane16);
        if (A.sigma && g == 0) {
#pragma unroll
            for (int s = 0; s < S; ++s)
                if (valid[s]) A.sigma[idx[s]] = acc[s][0][0];
        }
    }

    if (!SIGMA_ONLY) {
        // ---- predicted normal: 256 -> 128 -> 3, no activation in between (mirror_nerf.py:85-88)
        {
            float hn[S][32];
            {
                f32x4 acc[S][8];
                init_bias<8>(acc, BIAS_NRM1, g);
                gemm_part<16, 8>(acc, h, st, tile0, wave, lane16);
#pragma unroll
                for (int s = 0; s < S; ++s)
#pragma unroll
                    for (int nb = 0; nb < 8; ++nb)
#pragma unroll
                        for (int r = 0; r < 4; ++r) hn[s][4 * nb + r] = acc[s][nb][r];
                if (A.save_x) save_bform(A.save_x + (long long)SEC_HN * A.B, A.B, 128, hn, idx, valid, g);
            }
            f32x4 acc[S][1];
            init_bias<1>(acc, BIAS_NRM2, g);
            gemm_part<8, 1>(acc, hn, st, tile0, wave, lane16);
            if (A.pred_normal && g == 0) {
#pragma unroll
                for (int s = 0; s < S; ++s)
                    if (valid[s]) {
                        const float a0 = acc[s][0][0], a1 = acc[s][0][1], a2 = acc[s][0][2];
                        // utils/func.py:5-7: eps clamps the squared norm
                        const float inv = 1.f / sqrtf(fmaxf(a0 * a0 + a1 * a1 + a2 * a2, 1.1920928955078125e-07f));
                        float* o = A.pred_normal + idx[s] * 3;
                        o[0] = a0 * inv; o[1] = a1 * inv; o[2] = a2 * inv;
                        if (A.save_inv)   // negative marks the clamped branch (constant denominator)
                            A.save_inv[idx[s]] = (a0 * a0 + a1 * a1 + a2 * a2) > 1.1920928955078125e-07f ? inv : -inv;
                    }
            }
        }
        // ---- mirror probability: 256 -> 128 LeakyReLU(0.01) -> 1 sigmoid (mirror_nerf.py:94-99)
        {
            float hm[S][32];
            {
                f32x4 acc[S][8];
                init_bias<8>(acc, BIAS_MIR1, g);
                gemm_part<16, 8>(acc, h, st, tile0, wave, lane16);
#pragma unroll
                for (int s = 0; s < S; ++s)
#pragma unroll
                    for (int nb = 0; nb < 8; ++nb)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float v = acc[s][nb][r];
                            hm[s][4 * nb + r] = v > 0.f ? v : 0.01f * v;
                        }
                if (A.save_x) {
                    save_bform(A.save_x + (long long)SEC_HM * A.B, A.B, 128, hm, idx, valid, g);
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        uint64_t m = 0;
#pragma unroll
                        for (int t = 0; t < 32; ++t) m |= (uint64_t)(hm[s][t] > 0.f) << t;
                        gmask[(9 * S + s) * WG_THREADS + tid] = m;
                    }
                }
            }
            f32x4 acc[S][1];
            init_bias<1>(acc, BIAS_MIR2, g);
            gemm_part<8, 1>(acc, hm, st, tile0, wave, lane16);
            if (A.is_mirror && g == 0) {
#pragma unroll
                for (int s = 0; s < S; ++s)
                    if (valid[s]) A.is_mirror[idx[s]] = sigmoidf_(acc[s][0][0]);
            }
        }
        // ---- colour: final(256->256, no act) ; cat[final, dir] -> 128 relu ; 128 -> 3 sigmoid
        {
            float fin[S][64];
            {
                f32x4 acc[S][16];
                init_bias<16>(acc, BIAS_FIN, g);
                gemm_part<16, 16>(acc, h, st, tile0, wave, lane16);
#pragma unroll
                for (int s = 0; s < S; ++s)
#pragma unroll
                    for (int nb = 0; nb < 16; ++nb)
#pragma unroll
                        for (int r = 0; r < 4; ++r) fin[s][4 * nb + r] = acc[s][nb][r];
                if (A.save_x) save_bform(A.save_x + (long long)SEC_FIN * A.B, A.B, 256, fin, idx, valid, g);
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
            if (A.save_x) save_bform(A.save_x + (long long)SEC_DIRE * A.B, A.B, 32, de, idx, valid, g);
            float hd[S][32];
            {
                f32x4 acc[S][8];
                init_bias<8>(acc, BIAS_DIR, g);
                gemm_part<16, 8>(acc, fin, st, tile0, wave, lane16);
                gemm_part<2, 8>(acc, de, st, tile0, wave, lane16);
#pragma unroll
                for (int s = 0; s < S; ++s)
#pragma unroll
                    for (int nb = 0; nb < 8; ++nb)
#pragma unroll
                        for (int r = 0; r < 4; ++r) hd[s][4 * nb + r] = fmaxf(acc[s][nb][r], 0.f);
                if (A.save_x) {
                    save_bform(A.save_x + (long long)SEC_HD * A.B, A.B, 128, hd, idx, valid, g);
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        uint64_t m = 0;
#pragma unroll
                        for (int t = 0; t < 32; ++t) m |= (uint64_t)(hd[s][t] > 0.f) << t;
                        gmask[(8 * S + s) * WG_THREADS + tid] = m;
                    }
                }
            }
            f32x4 acc[S][1];
            init_bias<1>(acc, BIAS_RGB, g);
            gemm_part<8, 1>(acc, hd, st, tile0, wave, lane16);
            if (A.rgb && g == 0) {
#pragma unroll
                for (int s = 0; s < S; ++s)
                    if (valid[s]) {
                        float* o = A.rgb + idx[s] * 3;
                        o[0] = sigmoidf_(acc[s][0][0]);
                        o[1] = sigmoidf_(acc[s][0][1]);
                        o[2] = sigmoidf_(acc[s][0][2]);
                    }
            }
        }
    }

    if (GRAD) {
        // ---- d sigma / d xyz in closed form (SURVEY 8a): g = w_sigma; for i = 8..1:
        //      g = (g * relu_mask_i) W_i, the 63 encoding columns of layer 5 and layer 1 feed g_enc.
        open_stream(st, A.packed + OFF_BWD, BWD_TILES, wave, lane);
        tile0 = 0;
        float gr[S][64];
        {
            const f32x4* ws = (const f32x4*)(smem + LDS_BIAS) + (BIAS_WSIG >> 2);
#pragma unroll
            for (int nb = 0; nb < 16; ++nb) {
                const f32x4 v = ws[nb * 4 + g];
#pragma unroll
                for (int s = 0; s < S; ++s)
#pragma unroll
                    for (int r = 0; r < 4; ++r) gr[s][4 * nb + r] = v[r];
            }
        }
        float genc[S][16];
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
            for (int t = 0; t < 16; ++t) genc[s][t] = 0.f;

        // layers 8, 7, 6
#pragma unroll 1
        for (int l = 0; l < 3; ++l) {
            apply_mask(gr, 7 - l, tid);
            f32x4 acc[S][16];
            zero_acc<16>(acc);
            gemm_part<16, 16>(acc, gr, st, tile0, wave, lane16);
#pragma unroll
            for (int s = 0; s < S; ++s)
#pragma unroll
                for (int nb = 0; nb < 16; ++nb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) gr[s][4 * nb + r] = acc[s][nb][r];
        }
        // layer 5: first its 4 encoding row blocks, then its 16 hidden row blocks
        {
            apply_mask(gr, 4, tid);
            {
                f32x4 acc[S][4];
                zero_acc<4>(acc);
                gemm_part<16, 4>(acc, gr, st, tile0, wave, lane16);
#pragma unroll
                for (int s = 0; s < S; ++s)
#pragma unroll
                    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                        for (int r = 0; r < 4; ++r) genc[s][4 * nb + r] = acc[s][nb][r];
            }
            f32x4 acc[S][16];
            zero_acc<16>(acc);
            gemm_part<16, 16>(acc, gr, st, tile0, wave, lane16);
#pragma unroll
            for (int s = 0; s < S; ++s)
#pragma unroll
                for (int nb = 0; nb < 16; ++nb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) gr[s][4 * nb + r] = acc[s][nb][r];
        }
        // layers 4, 3, 2
#pragma unroll 1
        for (int l = 0; l < 3; ++l) {
            apply_mask(gr, 3 - l, tid);
            f32x4 acc[S][16];
            zero_acc<16>(acc);
            gemm_part<16, 16>(acc, gr, st, tile0, wave, lane16);
#pragma unroll
            for (int s = 0; s < S; ++s)
#pragma unroll
                for (int nb = 0; nb < 16; ++nb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) gr[s][4 * nb + r] = acc[s][nb][r];
        }
        // layer 1: 4 encoding row blocks
        {
            apply_mask(gr, 0, tid);
            f32x4 acc[S][4];
            zero_acc<4>(acc);
            gemm_part<16, 4>(acc, gr, st, tile0, wave, lane16);
#pragma unroll
            for (int s = 0; s < S; ++s)
#pragma unroll
                for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) genc[s][4 * nb + r] += acc[s][nb][r];
        }
        // encoding Jacobian: d/dx_a = g[x_a] + sum_f 2^f (g[sin] cos - g[cos] sin)
#pragma unroll
        for (int s = 0; s < S; ++s) {
            float d0 = 0.f, d1 = 0.f, d2 = 0.f;
#pragma unroll
            for (int pp = 0; pp < 8; ++pp) {
                const int P = 8 * g + pp;
                const int f = P / 3;
                const int a = P - 3 * f;
                const float gs = genc[s][2 * pp], gc = genc[s][2 * pp + 1];
                if (P < 30) {
                    const float xa = a == 0 ? x[s][0] : (a == 1 ? x[s][1] : x[s][2]);
                    float sn, cs;
                    sincosf(ldexpf(xa, f), &sn, &cs);   // recomputed: cheaper than 32 live registers
                    const float c = ldexpf(gs * cs - gc * sn, f);
                    d0 += a == 0 ? c : 0.f;
                    d1 += a == 1 ? c : 0.f;
                    d2 += a == 2 ? c : 0.f;
                } else if (P == 30) {
                    d0 += gs;
                    d1 += gc;
                } else {
                    d2 += gs;
                }
            }
            d0 += __shfl_xor(d0, 16); d1 += __shfl_xor(d1, 16); d2 += __shfl_xor(d2, 16);
            d0 += __shfl_xor(d0, 32); d1 += __shfl_xor(d1, 32); d2 += __shfl_xor(d2, 32);
            if (A.normal && g == 0 && valid[s]) {
                // normal = l2_normalize(-grad)  (mirror_nerf.py:145-146)
                const float n0 = -d0, n1 = -d1, n2 = -d2;
                const float sq = n0 * n0 + n1 * n1 + n2 * n2;
                const float inv = 1.f / sqrtf(fmaxf(sq, 1.1920928955078125e-07f));
                float* o = A.normal + idx[s] * 3;
                o[0] = n0 * inv; o[1] = n1 * inv; o[2] = n2 * inv;
                if (A.save_invj) A.save_invj[idx[s]] = sq > 1.1920928955078125e-07f ? inv : -inv;
            }
        }
    }
}


inline int launch(const FieldArgs& A, bool sigma_only, bool grad, hipStream_t s) {
    const long long blocks64 = (A.B + WG_SAMPLES - 1) / WG_SAMPLES;
    if (blocks64 > 0x7fffffff) return -1;
    const dim3 grid((unsigned)blocks64), block(WG_THREADS);
    if (sigma_only && !grad) hipLaunchKernelGGL((field_kernel<true, false>), grid, block, LDS_BYTES, s, A);
    else if (sigma_only && grad) hipLaunchKernelGGL((field_kernel<true, true>), grid, block, LDS_BYTES_GRAD, s, A);
    else if (!grad) hipLaunchKernelGGL((field_kernel<false, false>), grid, block, LDS_BYTES, s, A);
    else hipLaunchKernelGGL((field_kernel<false, true>), grid, block, LDS_BYTES_GRAD, s, A);
    return 0;
}
