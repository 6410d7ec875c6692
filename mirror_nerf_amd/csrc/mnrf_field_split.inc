// mnrf_field_split.inc -- the field kernel on the f16 matrix pipe at fp32 accuracy ("split" tuning).
//
// gfx950 has no fast fp32 / tf32 matrix path: v_mfma_f32_16x16x4_f32 runs at 1/16 of the f16 rate.
// Here every fp32 operand x is carried as two f16 numbers, hi = f16(x) and lo = f16(x - hi)
// (x - hi is exact in fp32; together 22 significand bits), and every Linear is evaluated as
//     W.x  ~=  W_hi.x_hi + W_lo.x_hi + W_hi.x_lo          (the dropped W_lo.x_lo term is 2^-22 relative)
// with three v_mfma_f32_16x16x32_f16 per 32-column block, accumulated in fp32 in ONE accumulator
// (f16 subnormal inputs are not flushed by the gfx950 MFMA -- scripts/exp_f16split.hip -- so the lo
// parts need no scaling).  3 x 16 cycles replace 8 x 32 cycles of the fp32 MFMA for the same block.
// Same structure as mnrf_field_impl.inc: 4 waves x 2 groups of 16 samples, activations stay in their
// lanes between layers (see mnrf_layout.h: the 8 fp32 B operands 8T..8T+7 of a lane are the 8 halves
// of its f16 B operand T), weights stream L2 -> LDS -> registers as hi/lo tile pairs.
// With save_* pointers the GRAD kernels also keep what the training backward needs (activations in fp32, masks).
// Range: the round-toward-zero conversions SATURATE at 65504, so |x| up to 131 008 is still carried (hi and lo both at
// the f16 maximum) and anything larger is silently clipped -- activations of a NeRF are orders of magnitude below that;
// mirror_nerf.verify_split() compares the two arithmetics on a model's own samples.
// Included from mnrf_field.hip inside a namespace that defines S, MIN_WAVES_PER_SIMD, CHUNK_PAIRS.
constexpr int CHUNK_BYTES = CHUNK_PAIRS * PAIR_BYTES;
constexpr int WAVES = 4;
constexpr int WG_THREADS = 64 * WAVES;
constexpr int WG_SAMPLES = WAVES * S * 16;
// RING_SLOTS comes from the includer (3 or 4)
constexpr int PIECES = CHUNK_BYTES / TILE_BYTES / WAVES;   // 1 KiB LDS-DMA pieces each wave issues per chunk
constexpr int U = 2;               // tile pairs per scheduling unit of the GEMM loop
constexpr int PF = S == 3 ? 2 : 4;  // A-operand pairs read ahead of the unit being consumed (<= 12 LDS reads in flight; with 48
                                   // samples per wave a unit lasts 288 cycles and one unit of read-ahead frees 16 registers)
constexpr int NBUF = PF + U;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 h2v __attribute__((ext_vector_type(2)));
// plane stores riding in a GEMM part (gemm_part_impl STB): this lane's corner of tile 0 of the section, and -- backward
// kernel -- the per-sample-group factor 2^(K - k_s + boost) the halves are multiplied with (mnrf_dwp.h "scale")
// Plane stores go out as BUFFER stores: a wave-uniform resource descriptor over the wave's sample block (SGPRs), a uniform
// section offset (SGPR) and one 32-bit lane offset.  (With per-lane 64-bit pointers hipcc hoisted sixteen address pairs per
// section and spilled them in the backward kernel: 254 scratch operations inside its MFMA streams.)
struct StoreCtx {
    __amdgpu_buffer_rsrc_t rsrc;   // this wave's sample block of the planes buffer
    __amdgpu_buffer_rsrc_t rsrc_lo;  // the same for the lo tiles -- or, with MNRF_PLANES_Y_HALF, a descriptor of ZERO records: the
                                   // store is issued (the counted vmcnt waits of the weight stream count it) and dropped by the
                                   // hardware's range check: no write traffic
    char* base;                    // the same as a pointer.  Nothing reads it, but without it hipcc schedules
                                   // field_split_bwd2_kernel differently
    int lane;                      // 32 m + 8 g: row m of the sample group, features 4 g .. 4 g + 3 of a tile
    int soff;                      // byte offset of the first tile the part stores
    h2v fac[S];                    // backward kernel: 2^(K - k_s + boost) per sample group (mnrf_dwp.h "scale")
};
__device__ __forceinline__ __amdgpu_buffer_rsrc_t plane_rsrc(char* sample_block) {
    return __builtin_amdgcn_make_buffer_rsrc(sample_block, 0, 0x7fffffff, 0x00020000);      // raw buffer, gfx9 dword 3
}
static_assert(CHUNK_PAIRS / U == PIECES, "one LDS-DMA piece per wave per unit");
constexpr int LDS_RING = RING_SLOTS * CHUNK_BYTES;
constexpr int LDS_BIAS = LDS_RING;
constexpr int LDS_MASK = LDS_BIAS + BIAS_FLOATS * 4;     // relu masks [8 layers][S][256 threads] x 8 B (GRAD only)
// S = 3 (48 samples per wave, forward only): the xyz-encoding operands are parked in LDS between L1 and L5 (see the kernel)
constexpr int LDS_PARK = LDS_MASK;
constexpr int HEAD_PARK = 6;      // S = 3: lo operands hl[s][0..5] of the heads' input live in LDS while the heads run
constexpr int LDS_PARK_BYTES = S == 3 ? HEAD_PARK * S * WG_THREADS * 16 : 0;      // >= the 2 x S x 2 operands of the encoding
static_assert(S != 3 || HEAD_PARK * S >= 2 * S * 2, "the encoding operands fit the same region");
constexpr int LDS_TILEQ = LDS_MASK + LDS_PARK_BYTES;      // two ints: the next tile of the dynamic queue, double-buffered
constexpr int LDS_BYTES = LDS_TILEQ + 16;
constexpr int LDS_BYTES_GRAD = LDS_MASK + 8 * S * WG_THREADS * 8;
static_assert(LDS_BYTES_GRAD <= 160 * 1024, "LDS budget");
// ray-fused fine pass (S = 3): the head outputs of the workgroup's 192 samples and their depths, [sigma | r | g | b | pn x 3 | mirror | z][sample]
constexpr int LDS_FUSE = LDS_BYTES;
// (+ a tenth row, the ray's compositing weights, in the blended-level variant)
constexpr int LDS_BYTES_FUSE = LDS_BYTES + 10 * WG_SAMPLES * 4;
static_assert(LDS_BYTES_FUSE <= 160 * 1024, "LDS budget");

#include "mnrf_field_split_common.inc"

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
#include "mnrf_composite.inc"
// per-sample inputs of the workgroup's ray for the fused compositing: head outputs from LDS, depths from HBM
struct CompLdsSrc {
    const float* f;      // LDS: [9][WG_SAMPLES]: sigma | r g b | predicted normal x 3 | mirror | depth
    bool pn_on, mir_on;
    __device__ __forceinline__ bool has_w() const { return false; }
    __device__ __forceinline__ float w(int) const { return 0.f; }
    __device__ __forceinline__ bool has_noise() const { return false; }
    __device__ __forceinline__ bool has_rgb() const { return true; }
    __device__ __forceinline__ bool has_mirror() const { return mir_on; }
    __device__ __forceinline__ bool has_pn() const { return pn_on; }
    __device__ __forceinline__ bool has_gn() const { return false; }
    __device__ __forceinline__ float z(int s) const { return f[8 * WG_SAMPLES + s]; }      // (parked by the prologue: a second global read of the depths would double the kernel's HBM reads)
    __device__ __forceinline__ float sigma(int s) const { return f[s]; }
    __device__ __forceinline__ float noise(int) const { return 0.f; }
    __device__ __forceinline__ float rgb(int s, int k) const { return f[(1 + k) * WG_SAMPLES + s]; }
    __device__ __forceinline__ float mirror(int s) const { return f[7 * WG_SAMPLES + s]; }
    __device__ __forceinline__ float pn(int s, int k) const { return f[(4 + k) * WG_SAMPLES + s]; }
    __device__ __forceinline__ float gn(int, int) const { return 0.f; }
};
// ... of the rgb / depth variant (RGB_DEPTH): no mirror head, no normal map -- known at compile time, so the compositing forms
// the colour, depth and opacity sums alone
// ... of the blended-level variant (BLENDED): the colour rows exist only for a ray whose colour branch ran, and the weights were
// formed (and parked in a tenth row) when the ray's mirror value was
struct CompLdsSrcBlended : CompLdsSrc {
    bool colour;
    __device__ __forceinline__ bool has_rgb() const { return colour; }
    __device__ __forceinline__ bool has_w() const { return true; }
    __device__ __forceinline__ float w(int s) const { return f[9 * WG_SAMPLES + s]; }
};
struct CompLdsSrcRgbDepth : CompLdsSrc {
    __device__ __forceinline__ bool has_mirror() const { return false; }
    __device__ __forceinline__ bool has_pn() const { return false; }
};

__device__ __forceinline__ unsigned long long enc_out_of_range(const float (&x)[S][3]) {
    bool big = false;
#pragma unroll
    for (int s = 0; s < S; ++s) big |= !(fabsf(x[s][0]) < ENC_RANGE_LIMIT && fabsf(x[s][1]) < ENC_RANGE_LIMIT && fabsf(x[s][2]) < ENC_RANGE_LIMIT);
    return __builtin_amdgcn_ballot_w64(big);
}

// N fp32 B operands of a lane -> N/8 f16 B operands (hi and lo)
template <int N>
__device__ __forceinline__ void split_b(const float (&x)[S][N], u32x4 (&hi)[S][N / 8], u32x4 (&lo)[S][N / 8],
                                        unsigned long long& sat, float limit = F16_MAX) {
    float tmax = 0.f;
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int T = 0; T < N / 8; ++T)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                unsigned h, l;
                split2(x[s][8 * T + 2 * e], x[s][8 * T + 2 * e + 1], h, l);
                sat_track<false>(tmax, x[s][8 * T + 2 * e], x[s][8 * T + 2 * e + 1]);
                hi[s][T][e] = h;
                lo[s][T][e] = l;
            }
    sat_flush(sat, tmax, limit);
}

__device__ __forceinline__ f32x4 mfma_f16(const u32x4& a, const u32x4& b, const f32x4& c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(h8, a), __builtin_bit_cast(h8, b), c, 0, 0, 0);
}

// relu as one integer max on the bit pattern (a negative float is a negative int; -0 -> +0): fmaxf() costs a second
// VALU to quiet a possible signalling NaN first
__device__ __forceinline__ float relu_(float x) {
    const int i = __builtin_bit_cast(int, x);
    return __builtin_bit_cast(float, i > 0 ? i : 0);
}

// ---- conversion side job.  The fp32 -> (hi, lo) conversion of a layer's outputs is ~4 VALU per element; done in one
// block after the layer's last MFMA it leaves the matrix pipe idle for 1.4-2.5 k cycles per 256-wide layer.  The trunk
// layers are therefore evaluated in two HALVES of 8 row blocks (the split stream stores them half by half), and the
// MFMA stream of one half carries the conversion of the previously finished half, two TASKS per 12-MFMA unit, interleaved
// with the MFMAs by scheduling-group barriers:
//   * half 2 of layer l converts half 1 of layer l into B operands 0..3 -- each one only after half 2 is done with the
//     OLD operand of the same index (unit 4T'+4 on), since the new operands overwrite the layer's inputs in place;
//   * half 1 of layer l+1 converts half 2 of layer l into B operands 4..7 during its T-steps 0..3, which read 0..3.
// One task = two adjacent accumulator registers -> one 32-bit word of the hi and of the lo operand: 11 vector instructions in the
// long form of split2, 8 in the short one (CONV_SHORT; its two-instruction asm statement is placed by the compiler inside the
// sub-group's fenced region, behind the sub-group's first MFMAs like the rest of the task -- checked in the disassembly).  Tasks are numbered so
// that the operands fill in T order: q = 4*S*Trel + 4*s + 2*(nb&1) + rp, nb = 2*Trel + ((q>>1)&1).
constexpr int NTASKS = 16 * S;
template <int ACT, bool WANT_MASK>
__device__ __forceinline__ void conv_task(int q, const f32x4 (&pacc)[S][8], u32x4 (&oh)[S][8], u32x4 (&ol)[S][8],
                                          int t0, int half, uint64_t (&mk)[S], float& tmax) {
    const int trel = q / (4 * S), s = (q / 4) % S, nb = 2 * trel + ((q >> 1) & 1), rp = q & 1;
    const float a0 = pacc[s][nb][2 * rp], a1 = pacc[s][nb][2 * rp + 1];
    if (WANT_MASK) {
        mk[s] |= (uint64_t)(a0 > 0.f) << (4 * (8 * half + nb) + 2 * rp);
        mk[s] |= (uint64_t)(a1 > 0.f) << (4 * (8 * half + nb) + 2 * rp + 1);
    }
    const float v0 = ACT == 1 ? relu_(a0) : a0, v1 = ACT == 1 ? relu_(a1) : a1;
    unsigned h, l;
    split2(v0, v1, h, l);
    sat_track<ACT == 1>(tmax, v0, v1);
    oh[s][t0 + trel][2 * (nb & 1) + rp] = h;
    ol[s][t0 + trel][2 * (nb & 1) + rp] = l;
}

// JOB: -1 none, else the activation of the half layer being converted; tasks run in units USTART .. USTART + NTASKS/TPU - 1
// NPARK > 0 (48-sample tuning, heads): the lo operands of k-steps 0 .. NPARK-1 are not in `bl` but parked in LDS
// ([T][s][thread] x 16 B at LDS_PARK) and fetched one k-step ahead into a small ring -- all 512 registers are taken there.
// STB >= 0 (training forward with operand planes, round 3): the part also STORES its B operands STB .. STB+3 -- inputs it only
// reads, complete before the part starts -- as plane tiles (mnrf_dwp.h), one global_store_dwordx2 behind the last pair of
// MFMAs of each of its first 32 units: the 64 stores per 256-wide section used to go out in one burst between two GEMMs
// while all four matrix pipes waited for HBM (0.65 of the 1.9 ms of the training forward per step).  `sp`: this lane's corner
// of tile 0 of the section.
// JUMP != 0 (blended-level variant of the ray-fused kernel): behind the piece that unit JUMP_T / U issues -- the last piece of
// its chunk -- the FILL pointer moves by JUMP bytes (if `jump_on`, wave-uniform), so that the chunks filled from there on come
// from another place of the image (mnrf_layout.h FOLD_POS_MIRB).  Everything else of the schedule counts chunks, not addresses.
// SKIP: the part's pairs are stepped over -- reads, pieces and seams as ever, no MFMA (padding pairs of that variant's stream).
template <int NT, int NB, int NACC, int NTA, int JOB, bool WANT_MASK, int USTART, int TPU, int POS, int NPARK = 0, int STB = -1,
          int STN = 4, bool SSCALE = false, int JUMP_T = -1, long long JUMP = 0, bool SKIP = false>
__device__ __forceinline__ void gemm_part_impl(f32x4 (&acc)[S][NACC], const u32x4 (&bh)[S][NTA], const u32x4 (&bl)[S][NTA],
                                               Stream& st, int wave, int lane16, const f32x4 (&pacc)[S][8],
                                               u32x4 (&oh)[S][8], u32x4 (&ol)[S][8], int t0, int half, uint64_t (&mk)[S],
                                               const StoreCtx& sc = StoreCtx{}, bool jump_on = true) {
    static_assert(JUMP == 0 || (JUMP_T >= 0 && JUMP_T % U == 0 && JUMP_T < NT * NB && ((POS + JUMP_T) / U) % PIECES == PIECES - 1 && JUMP % CHUNK_BYTES == 0),
                  "the fill pointer jumps between two chunks");
    static_assert(STB < 0 || (S == 2 && NT * NB / U >= 8 * STN && STB + STN <= NTA), "8 store tasks per operand ride on the part's first units");
    static_assert(NT <= NTA, "B operand count");
    static_assert(JOB < 0 || NTASKS % TPU == 0, "tasks per unit");
    static_assert(JOB < 0 || USTART + NTASKS / TPU <= NT * NB / U, "the job fits the part");
    constexpr int NPAIRS = NT * NB;
    static_assert(NPAIRS % U == 0, "pairs come in units");
    const unsigned ring = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem + (unsigned)lane16;
    u32x4 ah[NBUF], al[NBUF];
    constexpr int START = POS % CHUNK_PAIRS;      // position of the part's first pair inside its chunk
    static_assert(POS % U == 0, "parts start on a unit");
    static_assert(NPAIRS >= PF, "a part is at least as long as the read-ahead");
    // the first PF pairs were requested by the previous part's tail (or by prime_stream); rd_slot is the chunk of the
    // last of them, which is also the chunk of this part's next read unless that read opens a new one
    unsigned base = ring + st.rd_slot * CHUNK_BYTES;
#pragma unroll
    for (int i = 0; i < PF; ++i) {
        ah[i] = st.ch[i];
        al[i] = st.cl[i];
    }
    constexpr int NUNITS = NPAIRS / U;
    constexpr int INNER = NUNITS < 16 ? NUNITS : 16;
    static_assert(NUNITS % INNER == 0, "unit count");
    constexpr int NSLOT = NB == 1 ? 4 : 2;      // a unit spans two k-steps when the part has a single row block
    u32x4 pk[NSLOT][S];
    const u32x4* const park = (const u32x4*)(smem + LDS_PARK + wave * 1024 + lane16);
    const auto park_load = [&](int T) {
#pragma unroll
        for (int s = 0; s < S; ++s) pk[T % NSLOT][s] = park[(T * S + s) * WG_THREADS];
    };
    if (NPARK > 0) {
        park_load(0);
        if (NB == 1 && NT > 1) park_load(1);
    }
#pragma unroll
    for (int uo = 0; uo < NUNITS / INNER; ++uo) {
#pragma unroll
    for (int ui = 0; ui < INNER; ++ui) {
        const int t = (uo * INNER + ui) * U;
        if (NPARK > 0) {      // the parked operands of the k-step(s) the NEXT unit enters
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int pnext = t + U + u;
                if (pnext < NPAIRS && pnext % NB == 0 && pnext / NB < NPARK) park_load(pnext / NB);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // reads issued so far: every pair up to t+PF-1; the unit consumes t and t+1
        const int younger = PF - U;      // the read-ahead never stops: PF - U pairs are younger than the unit's
        u32x4& x0 = ah[t % NBUF];
        u32x4& y0 = al[t % NBUF];
        u32x4& x1 = ah[(t + 1) % NBUF];
        u32x4& y1 = al[(t + 1) % NBUF];
        if (younger == 0) wait_lds_reads_but<0>(x0, y0, x1, y1);
        else if (younger == 1) wait_lds_reads_but<2>(x0, y0, x1, y1);
        else wait_lds_reads_but<4>(x0, y0, x1, y1);
        // Three products per pair; the two pairs of a unit and the S sample groups interleave so that an accumulator
        // is touched every 2*S MFMAs (every S when the part has a single row block).  Issued in one block ahead of the
        // MFMAs, the unit's LDS reads left the matrix pipe idle for ~40 cycles per unit (s_memtime marks: 245 cycles per
        // unit against 12 x 16).
        // Six sub-groups of two MFMAs with ONE non-MFMA issue state behind each of the first five -- the unit's four LDS
        // reads and its LDS-DMA piece -- pinned by scheduling barriers: an extra issue state between two MFMAs costs far
        // more when it comes in a block (two reads + the piece behind four MFMAs measured 0.7 % slower).
#pragma unroll
        for (int sg = 0; sg < 6; ++sg) {
            const int ph = sg / 2, u = sg % 2;
            const int T = (t + u) / NB, nb = (t + u) % NB;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const u32x4& a = ph == 1 ? al[(t + u) % NBUF] : ah[(t + u) % NBUF];
                const u32x4& b = ph == 2 ? (T < NPARK ? pk[T % NSLOT][s] : bl[s][T]) : bh[s][T];
                if (!SKIP) acc[s][nb] = mfma_f16(a, b, acc[s][nb]);
            }
            if (JOB >= 0 && (sg == 0 || sg == 2) && TPU == 2) {
                const int unit = t / U - USTART;
                if (unit >= 0 && unit < NTASKS / TPU) {
                    conv_task<(JOB < 0 ? 0 : JOB), WANT_MASK>(unit * TPU + sg / 2, pacc, oh, ol, t0, half, mk, st.tmax);
#pragma unroll
                    for (int k = 0; k < S; ++k) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);
                    }
                }
            } else if (JOB >= 0 && TPU != 2 && sg < TPU) {
                const int unit = t / U - USTART;
                if (unit >= 0 && unit < NTASKS / TPU) {
                    conv_task<(JOB < 0 ? 0 : JOB), WANT_MASK>(unit * TPU + sg, pacc, oh, ol, t0, half, mk, st.tmax);
                    static_assert(JOB < 0 || TPU == 2 || TPU == 3 || TPU == 4 || TPU == 6, "one task behind each of the first TPU sub-groups");
                }
            }
            if (STB >= 0 && sg == 5 && t / U < 8 * STN) {
                // store task k: operand STB + k / 8, half-operand (k / 4) & 1, sample group (k / 2) & 1, plane k & 1
                const int k = t / U;
                const int T = (STB < 0 ? 0 : STB) + k / 8, h = (k / 4) & 1, sgp = (k / 2) & 1;
                const u32x4& w = (k & 1) ? bl[sgp][T < NTA ? T : 0] : bh[sgp][T < NTA ? T : 0];
                __builtin_amdgcn_sched_barrier(0);
                unsigned w0 = w[2 * h], w1 = w[2 * h + 1];
                if (SSCALE) {
                    w0 = __builtin_bit_cast(unsigned, __builtin_bit_cast(h2v, w0) * sc.fac[sgp]);
                    w1 = __builtin_bit_cast(unsigned, __builtin_bit_cast(h2v, w1) * sc.fac[sgp]);
                }
                __builtin_amdgcn_raw_buffer_store_b64(u32x2{w0, w1}, (k & 1) ? sc.rsrc_lo : sc.rsrc, sc.lane,
                                                      sc.soff + ((2 * (T - (STB < 0 ? 0 : STB)) + h) * PL_FB_BYTES + (k & 1) * PL_TILE_BYTES + sgp * 512), PL_STORE_AUX);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (sg < 5) {
                __builtin_amdgcn_sched_barrier(0);
                if (sg < 4) {
                    const int r = t + PF + sg / 2;
                    if (sg % 2 == 0 && (START + r) % CHUNK_PAIRS == 0) {
                        // VMEM operations return in order, so "at most n outstanding" must count the plane stores this part
                        // has issued behind the chunk's last piece as well: one per unit (at sg 5, behind the unit's piece) in
                        // the Y + 1 units before this one, as far as they belong to this part and carry a store task.  (Stores
                        // of an earlier part are not counted: the wait is then stricter than needed, never laxer.)  Without
                        // this the seam would wait for stores issued three units ago -- a synchronous HBM write per chunk.
                        constexpr int Y = PIECES - PF / U;
                        const int lu = t / U;
                        const int hi_u = lu < 8 * STN ? lu : 8 * STN, lo_u = lu - Y - 1 > 0 ? lu - Y - 1 : 0;
                        const int nst = STB >= 0 && hi_u > lo_u ? hi_u - lo_u : 0;
                        if (nst == 0) seam<Y>(st);
                        else if (nst == 1) seam<Y + 1>(st);
                        else if (nst == 2) seam<Y + 2>(st);
                        else if (nst == 3) seam<Y + 3>(st);
                        else if (nst == 4) seam<Y + 4>(st);
                        else if (nst == 5) seam<Y + 5>(st);
                        else if (nst == 6) seam<Y + 6>(st);
                        else if (nst == 7) seam<Y + 7>(st);
                        else seam<Y + 7>(st);
                        static_assert(PIECES - PF / U + 1 <= 7, "store tasks younger than a chunk");
                        base = ring + st.rd_slot * CHUNK_BYTES;
                    }
                    u32x4& d_ = sg % 2 == 0 ? (r < NPAIRS ? ah[r % NBUF] : st.ch[(r - NPAIRS) % PF])
                                            : (r < NPAIRS ? al[r % NBUF] : st.cl[(r - NPAIRS) % PF]);
                    lds_read_half_tile(d_, base, ((START + r) % CHUNK_PAIRS) * PAIR_BYTES + (sg % 2) * TILE_BYTES);
                } else {
                    const int piece = ((POS + t) / U) % PIECES;
                    if (piece == 0) issue_piece<0>(st);
                    else if (piece == 1) issue_piece<1>(st);
                    else if (piece == 2) issue_piece<2>(st);
                    else if (piece == 3) issue_piece<3>(st);
                    else if (piece == 4) issue_piece<(PIECES == 8 ? 4 : 0)>(st);
                    else if (piece == 5) issue_piece<(PIECES == 8 ? 5 : 0)>(st);
                    else if (piece == 6) issue_piece<(PIECES == 8 ? 6 : 0)>(st);
                    else issue_piece<(PIECES == 8 ? 7 : 0)>(st);
                    if (JUMP != 0 && t == JUMP_T) st.fill_src += jump_on ? (unsigned long long)JUMP : 0ull;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    }
    // The next part's first pairs must have LANDED before the compiler may touch their registers (a loop-carried copy, a
    // spill): it takes an asm output for available at once.  Most of their latency has passed behind the last MFMAs.
    carry_wait(st, std::integral_constant<int, PF>{});
    if (JOB >= 0) sat_flush(st.sat, st.tmax);     // the half layer converted by this part's side job is complete
}

// POS: position of the part in its stream, in pairs (mnrf_layout.h)
template <int NT, int NB, int POS, int NPARK = 0, int STB = -1, int STN = 4, bool SSCALE = false, int JUMP_T = -1, long long JUMP = 0,
          int NACC, int NTA>
__device__ __forceinline__ void gemm_part(f32x4 (&acc)[S][NACC], const u32x4 (&bh)[S][NTA], const u32x4 (&bl)[S][NTA],
                                          Stream& st, int wave, int lane16, const StoreCtx& sc = StoreCtx{}) {
    f32x4 pacc[S][8];
    u32x4 oh[S][8], ol[S][8];
    uint64_t mk[S];
    gemm_part_impl<NT, NB, NACC, NTA, -1, false, 0, S, POS, NPARK, STB, STN, SSCALE, JUMP_T, JUMP>(acc, bh, bl, st, wave, lane16, pacc,
                                                                                                  oh, ol, 0, 0, mk, sc);
}

// four pairs at POS stepped over (gemm_part_impl SKIP)
template <int POS>
__device__ __forceinline__ void skip_pairs4(Stream& st, int wave, int lane16) {
    f32x4 acc[S][1], pacc[S][8];
    u32x4 b[S][4], oh[S][8], ol[S][8];
    uint64_t mk[S];
    gemm_part_impl<4, 1, 1, 4, -1, false, 0, S, POS, 0, -1, 4, false, -1, 0, true>(acc, b, b, st, wave, lane16, pacc, oh, ol, 0, 0, mk);
}

// One half (8 row blocks) of a 256-wide trunk layer from NT k-steps of `bh/bl`, while converting the finished half
// `pacc` (relu) into hh/hl[t0 .. t0+3].
// STB: see gemm_part_impl -- the half that converts INTO operands 4..7 (t0 = 4) may store operands 0..3 of its input, the
// half that converts into 0..3 (t0 = 0, from unit 4 T' + 4 on) operands 4..7
template <int NT, int NTA, bool WANT_MASK, int USTART, int TPU, int POS, int STB = -1, int JUMP_T = -1, long long JUMP = 0>
__device__ __forceinline__ void gemm_half(f32x4 (&acc)[S][8], const u32x4 (&bh)[S][NTA], const u32x4 (&bl)[S][NTA], Stream& st,
                                          int wave, int lane16, const f32x4 (&pacc)[S][8], u32x4 (&hh)[S][8], u32x4 (&hl)[S][8],
                                          int t0, int half, uint64_t (&mk)[S], const StoreCtx& sc = StoreCtx{}, bool jump_on = true) {
    gemm_part_impl<NT, 8, 8, NTA, 1, WANT_MASK, USTART, TPU, POS, 0, STB, 4, false, JUMP_T, JUMP>(acc, bh, bl, st, wave, lane16, pacc, hh,
                                                                                                 hl, t0, half, mk, sc, jump_on);
}

// all tasks of a half layer at once (the last half of the trunk has no MFMA stream behind it to hide in)
template <bool WANT_MASK>
__device__ __forceinline__ void conv_half(const f32x4 (&pacc)[S][8], u32x4 (&hh)[S][8], u32x4 (&hl)[S][8], int t0, int half,
                                          uint64_t (&mk)[S], unsigned long long& sat) {
    float tmax = 0.f;
#pragma unroll
    for (int q = 0; q < NTASKS; ++q) conv_task<1, WANT_MASK>(q, pacc, hh, hl, t0, half, mk, tmax);
    sat_flush(sat, tmax);
}

// bias of row blocks 8*half .. 8*half+7 of a 256-wide layer
__device__ __forceinline__ void init_bias_half(f32x4 (&acc)[S][8], int bias_off, int half, int g) {
    const f32x4* bl = (const f32x4*)(smem + LDS_BIAS) + (bias_off >> 2) + 32 * half;
#pragma unroll
    for (int nb = 0; nb < 8; ++nb) {
        const f32x4 v = bl[nb * 4 + g];
#pragma unroll
        for (int s = 0; s < S; ++s) acc[s][nb] = v;
    }
}

// gmask: the training forward also keeps the masks in HBM for the backward kernel (mnrf_field_bwd.inc, same tile map)
__device__ __forceinline__ void store_mask(const uint64_t (&mk)[S], int layer, int tid, unsigned long long* gmask) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
        ((uint64_t*)(smem + LDS_MASK))[(layer * S + s) * WG_THREADS + tid] = mk[s];
        if (gmask) gmask[(layer * S + s) * WG_THREADS + tid] = mk[s];
    }
}

// per-sample outputs (sigma, rgb, predicted normal, mirror probability): plain stores
__device__ __forceinline__ void out_store(float* p, float v) {
    *p = v;
}

// fp32 rows kept for a later kernel (row route of the weight gradients, second-order pass): non-temporal like the operand planes
// (mnrf_dwp.h PL_STORE_AUX) -- gigabytes per step whose write-back otherwise stalls the L2's memory side
__device__ __forceinline__ void row_store(f32x4* p, const f32x4 v) {
    __builtin_nontemporal_store(v, p);
}

// ---- training forward: activations kept for the backward pass, [section][sample][width] in B-form column order
// (element 16*nb + 4*g + r of a sample = accumulator register r of row block nb in lane group g; mnrf_layout.h SEC_*)
template <int NT>
__device__ __forceinline__ void save_bform(float* sec, int width, const float (&x)[S][NT], const int (&idx)[S],
                                           const bool (&valid)[S], int g) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
        if (!valid[s]) continue;
        f32x4* o = (f32x4*)(sec + (long long)idx[s] * width);
#pragma unroll
        for (int nb = 0; nb < NT / 4; ++nb)
            row_store(o + nb * 4 + g, f32x4{x[s][4 * nb], x[s][4 * nb + 1], x[s][4 * nb + 2], x[s][4 * nb + 3]});
    }
}

// NB row blocks starting at block nb0 of a `width`-wide section; ACT as in acc_to_b; returns the (v > 0) bits of the
// NB*4 values in *bits (bit 4*nb + r)
template <int NB, int ACT>
__device__ __forceinline__ void save_acc(float* sec, int width, int nb0, const f32x4 (&acc)[S][NB], const int (&idx)[S],
                                         const bool (&valid)[S], int g, uint64_t (&bits)[S]) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
        uint64_t m = 0;
        f32x4* o = (f32x4*)(sec + (long long)idx[s] * width);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            f32x4 v;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float a = acc[s][nb][r];
                m |= (uint64_t)(a > 0.f) << (4 * nb + r);
                v[r] = ACT == 1 ? relu_(a) : (ACT == 2 ? (a > 0.f ? a : 0.01f * a) : a);
            }
            if (valid[s]) row_store(o + (nb0 + nb) * 4 + g, v);
        }
        bits[s] = m;
    }
}

// ---- training forward, round 3: the hi/lo B operands of a Linear ARE the X operand of its weight-gradient GEMM.  Operand T of
// sample group s (halves e = 4 h + c: feature 16 (2 T + h) + 4 g + c of the section) goes to tile fb0 + 2 T + h of this wave's
// sample block, row 16 s + m, bytes 8 g .. 8 g + 7 (mnrf_dwp.h): one global_store_dwordx2 per half operand and plane, 512
// contiguous bytes per wave instruction (buffer stores: StoreCtx).
template <int NT, int NTA>
__device__ __forceinline__ void store_planes(const StoreCtx& sc, int fb0, const u32x4 (&hi)[S][NTA], const u32x4 (&lo)[S][NTA]) {
    static_assert(S == 2, "a sample block is one wave of two 16-sample groups");
#pragma unroll
    for (int T = 0; T < NT; ++T)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const int off = (fb0 + 2 * T + h) * PL_FB_BYTES + s * 512;
                __builtin_amdgcn_raw_buffer_store_b64(u32x2{hi[s][T][2 * h], hi[s][T][2 * h + 1]}, sc.rsrc, sc.lane, off, PL_STORE_AUX);
                __builtin_amdgcn_raw_buffer_store_b64(u32x2{lo[s][T][2 * h], lo[s][T][2 * h + 1]}, sc.rsrc_lo, sc.lane, off + PL_TILE_BYTES, PL_STORE_AUX);
            }
}

// (v > 0) bits of NB row blocks (bit 4 nb + r), one word per sample group: the relu / leaky-relu masks the backward reads
template <int NB>
__device__ __forceinline__ void store_sign_mask(const f32x4 (&acc)[S][NB], unsigned long long* dst) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
        uint64_t m = 0;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) m |= (uint64_t)(acc[s][nb][r] > 0.f) << (4 * nb + r);
        dst[s * WG_THREADS] = m;
    }
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

// accumulators -> next layer's B operands.  ACT: 0 none, 1 relu, 2 leaky relu(0.01).
// With WANT_MASK the 64-bit relu mask of the layer is parked in LDS for the gradient pass.
template <int NB, int ACT, bool WANT_MASK>
__device__ __forceinline__ void acc_to_b(u32x4 (&hi)[S][NB / 2], u32x4 (&lo)[S][NB / 2], const f32x4 (&acc)[S][NB],
                                         int layer, int tid, unsigned long long& sat) {
    float tmax = 0.f;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        uint64_t m = 0;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float a = acc[s][nb][r];
                if (WANT_MASK) m |= (uint64_t)(a > 0.f) << (4 * nb + r);
                v[r] = ACT == 1 ? relu_(a) : (ACT == 2 ? (a > 0.f ? a : 0.01f * a) : a);
            }
            unsigned h0, l0, h1, l1;
            split2(v[0], v[1], h0, l0);
            split2(v[2], v[3], h1, l1);
            sat_track<ACT == 1>(tmax, v[0], v[1]);
            sat_track<ACT == 1>(tmax, v[2], v[3]);
            hi[s][nb >> 1][2 * (nb & 1)] = h0;
            hi[s][nb >> 1][2 * (nb & 1) + 1] = h1;
            lo[s][nb >> 1][2 * (nb & 1)] = l0;
            lo[s][nb >> 1][2 * (nb & 1) + 1] = l1;
        }
        if (WANT_MASK) ((uint64_t*)(smem + LDS_MASK))[(layer * S + s) * WG_THREADS + tid] = m;
    }
    sat_flush(sat, tmax);
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + expf(-x)); }



// ------------------------------------------------------------------ the kernel
// PLANES (training forward of the split arithmetic): A.save_planes is set and the 8 x 256 hidden sections are stored from
// inside the MFMA streams (gemm_part_impl STB); the smaller sections (encoding, heads) still go out between the GEMMs
// FUSE (eval, maps only; S = 3: one ray of 192 samples per workgroup): the head outputs stay in LDS and wave 0 composites the
// ray at the end -- no per-sample tensor reaches HBM (36 B per sample written and read back otherwise)
// FOLD (every full forward-only kernel): the folded stream (mnrf_layout.h OFF_FOLD_FWD) -- normal_net as one 3 x 256 map in rows
// 1..3 of the sigma block, xyz_encoding_final folded into dir_encoding's h8 columns: 1112 instead of 1308 pairs per sample.  The
// kernels that keep activations for a backward pass (GRAD) need the unfolded heads; the sigma-only ones stay on the split stream
// (same trunk, same sigma row).
// RGB_DEPTH (FUSE only): the caller reads colour and depth alone (the last reflection level of a frame): the stream stops in front
// of the mirror head, which the folded order puts last (mnrf_layout.h FOLD_POS_MIR1), and the compositing wave forms only the
// rgb / depth / opacity sums.
// BLENDED (FUSE only; FieldArgs::fuse 3 / 4): the pass of a level whose colour the caller will blend with the thresholded mirror
// mask, m * reflected + (1 - m) * colour (recursion.stage_b).  A workgroup is one ray, so whether the ray's colour can reach the
// frame is uniform over it: the mirror head runs BEFORE the colour branch, every wave forms the ray's composited mirror value
// from the sigma and mirror rows in LDS (composite_mirror_value: the operations of composite_ray, so the value is the one the
// mirror map gets), and if it is not below 0.5 (m = 1; a NaN too) the workgroup leaves out dir_encoding / view / rgb -- 76 of the
// 1112 pairs -- and writes 0 to the ray's rgb_map row.  The stream is the folded one up to the sigma | normal block; there the
// fill pointer jumps to a chunk-aligned copy of the mirror head behind the bias block (mnrf_layout.h FOLD_POS_MIRB: 68 pairs and 4
// of padding, which are stepped over) and from its end back to dir_encoding, so the other kernels keep their stream as it is.
// Logical positions: is_mirror_net.0 968, is_mirror_net.2 1032, padding 1036, dir_encoding 1040, view 1104, rgb 1112, end 1116.
// The variant also writes the per-sample predicted normals (FieldArgs::pred_normal) when asked: with them and the weights a
// level can take the fused launch under the full result contract.  fuse == 4: the same kernel, no ray skipped.
template <bool SIGMA_ONLY, bool GRAD, bool PLANES, bool FUSE, bool RGB_DEPTH, bool BLENDED = false>
__device__ __forceinline__ void field_split_body(FieldArgs A) {
    static_assert(!PLANES || (GRAD && !SIGMA_ONLY && S == 2), "operand planes: the training forward (32 samples per wave)");
    static_assert(!FUSE || (S == 3 && !SIGMA_ONLY && !GRAD), "ray-fused compositing: the 192-sample fine pass");
    static_assert(!RGB_DEPTH || FUSE, "rgb / depth only: a variant of the ray-fused pass");
    static_assert(!BLENDED || (FUSE && !RGB_DEPTH && CHUNK_PAIRS == 8), "blended level: a variant of the ray-fused pass; its jumps are whole 8-pair chunks");
    constexpr long long JUMP_TO_MIRB = BLENDED ? (long long)(FOLD_POS_MIRB - FOLD_POS_DIR) * PAIR_BYTES : 0;
    constexpr long long JUMP_FROM_MIRB = BLENDED ? (long long)(FOLD_POS_DIR - (FOLD_POS_MIRB + FOLD_MIRB_PAIRS)) * PAIR_BYTES : 0;
    constexpr int JT = BLENDED ? 54 : -1;      // the unit of a 64-pair part that issues the last piece of the first chunk BEHIND the part
    constexpr bool FOLD = !SIGMA_ONLY && !GRAD;
    conv_round_mode();
    float* const fz = (float*)(smem + LDS_FUSE);      // FUSE: [9][WG_SAMPLES]
    // Dynamic tile queue (S = 3, FieldArgs::tile_queue): the launch has one workgroup per CU; the first tile is the workgroup's
    // own id, every further one comes from the global counter -- requested at the START of the tile before, parked in LDS
    // during the prologue, read after the barrier that ends the tile.
    constexpr bool PERSIST = S == 3;
    if constexpr (PLANES) {      // live row count (FieldArgs::n_live): B becomes what exists; a workgroup past it has nothing to do
        if (A.n_live) {
            long long bl = (long long)*A.n_live * A.spr;
            bl = bl < 0 ? 0 : bl;
            if (bl < A.B) A.B = bl;
        }
        if ((long long)blockIdx.x * WG_SAMPLES >= A.B) return;
    }
    const bool queued = PERSIST && A.tile_queue != nullptr;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int tile = blockIdx.x;
    int round = 0;
    unsigned long long sat_all = 0, enc_all = 0;
    {   // bias block -> LDS (read by init_bias behind the __syncthreads() below)
        const f32x4* src = (const f32x4*)(A.packed + (FOLD ? OFF_FOLD_BIAS : OFF_BIAS));
        f32x4* dst = (f32x4*)(smem + LDS_BIAS);
        for (int i = threadIdx.x; i < BIAS_FLOATS / 4; i += WG_THREADS) dst[i] = src[i];
    }
    for (;;) {      // (one pass unless `queued`; body not indented)
    // In the tile loop every lane-derived value is re-derived per tile from an opaque lane id: hoisted out of the loop as
    // invariants they outlive the whole network and hipcc parks them in scratch (122 scratch operations, 23 of them inside
    // the MFMA streams, in the first build of the loop).
    int lane_;
    if (PERSIST) asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_));
    else lane_ = threadIdx.x & 63;
    const int lane = lane_;
    const int tid = PERSIST ? wave * 64 + lane : (int)threadIdx.x;
    const int g = lane >> 4;     // lane group = k-slot / row quad
    const int m = lane & 15;     // sample within the group
    const int lane16 = lane * 16;
    constexpr int HP = (S == 3 && !SIGMA_ONLY && !GRAD) ? HEAD_PARK : 0;      // lo operands of the heads' input parked in LDS
    // training forward, operand planes: this lane's corner of the wave's sample block (S == 2: 32 samples per wave)
    char* const pl = (PLANES || (GRAD && S == 2 && A.save_planes))
                         ? A.save_planes + ((long long)blockIdx.x * WAVES + wave) * PLX_SB_BYTES : nullptr;      // wave-uniform
    // WEAVE (default since round 5): the 64 stores of every hidden section ride inside
    // the MFMA streams of the GEMMs that read the same operands (gemm_part_impl STB), one behind each unit, instead of going out in
    // one burst between two GEMMs.  Round 3 measured it EQUAL (5.96-5.99 against 5.94-5.97 ms per step on the host-driven step of
    // that time).  Round 5 (experiment builds, one box, alternating): the kernel alone 897-924 against
    // 931-949 us per 1024 x 128 launch (the same without any plane store: 781-796; with every store landing in one L2-resident
    // block: 829-834 woven, 864-872 in bursts -- so half of the stores' cost is issue / data path, which weaving halves, and half is
    // the memory system's write side, which it does not touch); in the training step 4.38-4.40 against 4.44-4.50 ms with this kernel
    // woven, 4.26-4.28 with the activation-gradient kernel woven too.
    constexpr bool WEAVE = PLANES;
    constexpr int ST0 = WEAVE ? 0 : -1, ST4 = WEAVE ? 4 : -1;      // store operands 0..3 / 4..7 inside a GEMM part
    StoreCtx sc;
    sc.rsrc = plane_rsrc(pl);
    sc.rsrc_lo = sc.rsrc;
    sc.base = pl;
    sc.lane = 32 * m + 8 * g;
    sc.soff = 0;
    // tile of operand T0 of hidden section `sec` (h1 = 0 .. h8 = 7) for the store side job of a GEMM part
    const auto at_h = [&](int sec, int T0) -> const StoreCtx& {
        sc.soff = (SEC_H / 16 + 16 * sec + 2 * T0) * PL_FB_BYTES;
        return sc;
    };

    // the weight stream starts first: its first two chunks travel while the positions are fetched and encoded
    Stream st;
    st.sat = 0;
    st.tmax = 0.f;
    open_stream<true>(st, A.packed + (FOLD ? OFF_FOLD_FWD : OFF_SPLIT_FWD), wave, lane);
    int next_tile = 0;
    if (queued && tid == 0) next_tile = (int)gridDim.x + atomicAdd(A.tile_queue, 1);

    // ---- sample positions (rendering.py:302: multiply, then add -- no FMA)
    int idx[S];   // sample index (B < 2^31 is checked at launch): one register each instead of two
    bool valid[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        long long i = (long long)tile * WG_SAMPLES + wave * (S * 16) + s * 16 + m;
        valid[s] = i < A.B;
        if (!valid[s]) i = A.B - 1;
        idx[s] = (int)i;
    }
    // The 48-sample tuning has every register taken: there the sample index (and its `valid` bit) is RECOMPUTED at each use
    // after the prologue -- kept, hipcc parks it in scratch (3 stores + 18 loads per tile and twice the HBM write traffic).
    // (unsigned 32-bit arithmetic: B < 2^31 is checked at launch, so index + 191 < 2^32)
    // (S = 3: through an opaque instruction -- hipcc otherwise merges the recomputations into ONE value again and keeps that
    // in scratch, 3 stores + 9 loads per tile in the full kernel)
    const auto m15 = [&]() -> unsigned {
        unsigned r;      // lane & 15 from the execution mask count: no input register at all
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0\n\tv_and_b32 %0, 15, %0" : "=v"(r));
        return r;
    };
    const auto gq = [&]() -> int {      // lane group for the heads' bias reads (S = 3: recomputed, see m15)
        if (S != 3) return g;
        unsigned r;
        asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0\n\tv_lshrrev_b32 %0, 4, %0" : "=v"(r));
        return (int)r;
    };
    const auto sidx = [&](int s) -> int {
        if (S != 3) return idx[s];
        const unsigned i = tile * (unsigned)WG_SAMPLES + (unsigned)(wave * (S * 16) + s * 16) + m15();
        const unsigned last = (unsigned)A.B - 1u;
        return (int)(i < last ? i : last);
    };
    const auto sval = [&](int s) -> bool {
        if (S != 3) return valid[s];
        return tile * (unsigned)WG_SAMPLES + (unsigned)(wave * (S * 16) + s * 16) + m15() < (unsigned)A.B;
    };
    // (a lambda: the density-gradient epilogue fetches the positions again instead of holding six registers through
    // the whole network)
    // (tile loop: wave-uniform values derived from the arguments -- the reciprocal behind `/ A.spr`, the `A.xyz != null`
    // predicate -- are loop invariants too, and with every scalar register taken hipcc keeps them in VECTOR registers parked
    // in scratch; an opaque copy at the use pins the derivation there)
    const auto opaque_spr = [&]() -> int {
        int v = A.spr;
        if (PERSIST) asm volatile("" : "+s"(v));
        return v;
    };
    const auto fetch_positions = [&](float (&x)[S][3]) {
        const float* xyz = A.xyz;
        if (PERSIST) asm volatile("" : "+s"(xyz));
        const int spr = opaque_spr();
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const long long i = sidx(s);
            if (xyz) {
                const float* p = xyz + i * A.xyz_stride;
                x[s][0] = p[0]; x[s][1] = p[1]; x[s][2] = p[2];
            } else {
                const int ray = sidx(s) / spr;      // 32-bit: B < 2^31
                const float* r = A.rays + (long long)ray * 8;
                const float z = A.z_vals[i];
#pragma unroll
                for (int a = 0; a < 3; ++a) x[s][a] = r[a] + r[3 + a] * z;
            }
        }
    };

    // ---- xyz encoding, this lane's 16 of the 64 (padded) channels: pairs P = 8g + pp (mnrf_layout.h enc_col)
    u32x4 eh[S][2], el[S][2];
    unsigned long long enc_range;
    {
        float x[S][3];
        fetch_positions(x);
        if (queued && tid == 0) ((int*)(smem + LDS_TILEQ))[round & 1] = next_tile;
        if (FUSE && g == 0) {      // the ray's depths for the compositing wave (the lines were just fetched: L1 hits)
#pragma unroll
            for (int s = 0; s < S; ++s) fz[8 * WG_SAMPLES + wave * (S * 16) + s * 16 + m] = A.z_vals[sidx(s)];
        }
        enc_range = enc_out_of_range(x);
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
                fast_sincos(ldexpf(xa, f), sn, cs);   // 2^f * x is exact (mirror_nerf.py:17, 36)
                if (P >= 30) {                       // raw coordinates ride in the last two pairs
                    sn = P == 30 ? x[s][0] : x[s][2];
                    cs = P == 30 ? x[s][1] : 0.f;
                }
                enc[s][2 * pp] = sn;
                enc[s][2 * pp + 1] = cs;
            }
        }
        if (GRAD && A.save_x) save_bform<16>(A.save_x + (long long)SEC_ENC * A.B, 64, enc, idx, valid, g);
        split_b<16>(enc, eh, el, st.sat);
        if constexpr (S == 2) { if (pl) store_planes<2, 2>(sc, SEC_ENC / 16, eh, el); }
        if (S == 3) {
            // 48 samples per wave leave no room to hold these 48 registers through L2..L4: L5 reads them back step by step
            u32x4* park = (u32x4*)(smem + LDS_PARK);
#pragma unroll
            for (int T = 0; T < 2; ++T)
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    park[((T * S + s) * 2 + 0) * WG_THREADS + tid] = eh[s][T];
                    park[((T * S + s) * 2 + 1) * WG_THREADS + tid] = el[s][T];
                }
        }
    }
    unsigned long long* gmask = (GRAD && A.save_mask) ? A.save_mask + (long long)tile * (N_MASKS * S * WG_THREADS) : nullptr;
    const bool keep = !PLANES && GRAD && A.save_x != nullptr;     // training forward, fp32 rows (no MNRF_TRAIN_PLANES: the fp32 arithmetic; tests)
    uint64_t unused_bits[S];

    u32x4 hh[S][8], hl[S][8];
    f32x4 accA[S][8], accB[S][8];   // the two halves (row blocks 0-7, 8-15) of the layer in flight
    {
        uint64_t mk[S];
        const auto zero_mask = [&]() {
#pragma unroll
            for (int s = 0; s < S; ++s) mk[s] = 0;
        };
        __syncthreads();   // bias block visible
        prime_stream(st, lane16);
        // ---- L1: enc(64) -> 256.  Half 2 converts half 1 (nothing reads hh yet: four tasks per unit)
        zero_mask();
        init_bias_half(accA, BIAS_L, 0, gq());
        gemm_part<2, 8, 0>(accA, eh, el, st, wave, lane16);
        if (keep) save_acc<8, 1>(A.save_x + (long long)SEC_H * A.B, 256, 0, accA, idx, valid, g, unused_bits);
        init_bias_half(accB, BIAS_L, 1, gq());
        gemm_half<2, 2, GRAD, 0, 2 * S, 16>(accB, eh, el, st, wave, lane16, accA, hh, hl, 0, 0, mk);
        if (keep) save_acc<8, 1>(A.save_x + (long long)SEC_H * A.B, 256, 8, accB, idx, valid, g, unused_bits);
        // ---- L2..L4
#pragma unroll 1
        for (int l = 0; l < 3; ++l) {
            init_bias_half(accA, BIAS_L + 256 * (1 + l), 0, gq());
            gemm_half<8, 8, GRAD, 0, S, 32, ST0>(accA, hh, hl, st, wave, lane16, accB, hh, hl, 4, 1, mk, at_h(l, 0));   // + half 2 of layer l
            if (GRAD) { store_mask(mk, l, tid, gmask); zero_mask(); }
            if (keep) save_acc<8, 1>(A.save_x + (long long)(SEC_H + 256 * (1 + l)) * A.B, 256, 0, accA, idx, valid, g, unused_bits);
            // hh / hl hold the layer's INPUT h_(l+1) in full exactly here: operands 4..7 were completed by the half above,
            // operands 0..3 are overwritten by the half below
            if constexpr (S == 2 && !WEAVE) { if (pl) store_planes<8, 8>(sc, SEC_H / 16 + 16 * l, hh, hl); }
            init_bias_half(accB, BIAS_L + 256 * (1 + l), 1, gq());
            gemm_half<8, 8, GRAD, 4, S, 96, ST4>(accB, hh, hl, st, wave, lane16, accA, hh, hl, 0, 0, mk, at_h(l, 4));   // + half 1 of this layer
            if (keep) save_acc<8, 1>(A.save_x + (long long)(SEC_H + 256 * (1 + l)) * A.B, 256, 8, accB, idx, valid, g, unused_bits);
        }
        // ---- L5: cat[enc, h] -> 256  (encoding first: mirror_nerf.py:192-193); the jobs ride on the 256-wide parts
        init_bias_half(accA, BIAS_L + 256 * 4, 0, gq());
        if (S == 3) {
#pragma unroll
            for (int T = 0; T < 2; ++T) {
                u32x4 ph[S][1], pl[S][1];
                const u32x4* park = (const u32x4*)(smem + LDS_PARK);
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    ph[s][0] = park[((T * S + s) * 2 + 0) * WG_THREADS + tid];
                    pl[s][0] = park[((T * S + s) * 2 + 1) * WG_THREADS + tid];
                }
                if (T == 0) gemm_part<1, 8, 416>(accA, ph, pl, st, wave, lane16);
                else gemm_part<1, 8, 424>(accA, ph, pl, st, wave, lane16);
            }
        } else {
            gemm_part<2, 8, 416>(accA, eh, el, st, wave, lane16);
        }
        gemm_half<8, 8, GRAD, 0, S, 432, ST0>(accA, hh, hl, st, wave, lane16, accB, hh, hl, 4, 1, mk, at_h(3, 0));
        if (GRAD) { store_mask(mk, 3, tid, gmask); zero_mask(); }
        if (keep) save_acc<8, 1>(A.save_x + (long long)(SEC_H + 256 * 4) * A.B, 256, 0, accA, idx, valid, g, unused_bits);
        if constexpr (S == 2 && !WEAVE) { if (pl) store_planes<8, 8>(sc, SEC_H / 16 + 16 * 3, hh, hl); }      // h4
        init_bias_half(accB, BIAS_L + 256 * 4, 1, gq());
        if (S == 3) {
#pragma unroll
            for (int T = 0; T < 2; ++T) {
                u32x4 ph[S][1], pl[S][1];
                const u32x4* park = (const u32x4*)(smem + LDS_PARK);
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    ph[s][0] = park[((T * S + s) * 2 + 0) * WG_THREADS + tid];
                    pl[s][0] = park[((T * S + s) * 2 + 1) * WG_THREADS + tid];
                }
                if (T == 0) gemm_part<1, 8, 496>(accB, ph, pl, st, wave, lane16);
                else gemm_part<1, 8, 504>(accB, ph, pl, st, wave, lane16);
            }
        } else {
            gemm_part<2, 8, 496>(accB, eh, el, st, wave, lane16);
        }
        gemm_half<8, 8, GRAD, 4, S, 512, ST4>(accB, hh, hl, st, wave, lane16, accA, hh, hl, 0, 0, mk, at_h(3, 4));
        if (keep) save_acc<8, 1>(A.save_x + (long long)(SEC_H + 256 * 4) * A.B, 256, 8, accB, idx, valid, g, unused_bits);
        // ---- L6..L8
#pragma unroll 1
        for (int l = 0; l < 3; ++l) {
            init_bias_half(accA, BIAS_L + 256 * (5 + l), 0, gq());
            gemm_half<8, 8, GRAD, 0, S, 576, ST0>(accA, hh, hl, st, wave, lane16, accB, hh, hl, 4, 1, mk, at_h(4 + l, 0));
            if (GRAD) { store_mask(mk, 4 + l, tid, gmask); zero_mask(); }
            if (keep) save_acc<8, 1>(A.save_x + (long long)(SEC_H + 256 * (5 + l)) * A.B, 256, 0, accA, idx, valid, g, unused_bits);
            if constexpr (S == 2 && !WEAVE) { if (pl) store_planes<8, 8>(sc, SEC_H / 16 + 16 * (4 + l), hh, hl); }      // h5..h7
            init_bias_half(accB, BIAS_L + 256 * (5 + l), 1, gq());
            // (BLENDED: the chunk behind L8 -- sigma | normal -- is the last one of the common stream)
            gemm_half<8, 8, GRAD, 4, S, 640, ST4, JT, JUMP_TO_MIRB>(accB, hh, hl, st, wave, lane16, accA, hh, hl, 0, 0, mk, at_h(4 + l, 4), l == 2);
            if (keep) save_acc<8, 1>(A.save_x + (long long)(SEC_H + 256 * (5 + l)) * A.B, 256, 8, accB, idx, valid, g, unused_bits);
        }
        // half 2 of L8 has nothing to hide behind
        conv_half<GRAD>(accB, hh, hl, 4, 1, mk, st.sat);
        if constexpr (S == 2 && !WEAVE) { if (pl) store_planes<8, 8>(sc, SEC_H / 16 + 16 * 7, hh, hl); }      // h8 = geo_feat (PLANES: inside the normal / mirror heads' GEMMs)
        if (HP > 0) {      // 48-sample tuning: the heads read these lo operands back from LDS one k-step at a time
            u32x4* park = (u32x4*)(smem + LDS_PARK);
#pragma unroll
            for (int T = 0; T < HP; ++T)
#pragma unroll
                for (int s = 0; s < S; ++s) park[(T * S + s) * WG_THREADS + tid] = hl[s][T];
        }
        if (GRAD) store_mask(mk, 7, tid, gmask);
        if (S != 3 && A.geo_feat) {     // (the 48-sample tuning has no registers to keep both halves: its launcher declines geo_feat)
            // h8 = geo_feat (mirror_nerf.py:195), fp32: the accumulators of both halves are still intact
#pragma unroll
            for (int s = 0; s < S; ++s) {
                if (valid[s]) {
                    f32x4* o = (f32x4*)(A.geo_feat + (long long)idx[s] * 256);
#pragma unroll
                    for (int nb = 0; nb < 16; ++nb) {
                        const f32x4 v = nb < 8 ? accA[s][nb & 7] : accB[s][nb & 7];
                        o[nb * 4 + g] = f32x4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
                    }
                }
            }
        }
    }
    // predicted normal = l2_normalize of registers R0 .. R0 + 2 of lane group 0 (mirror_nerf.py:85-88)
    const auto put_normal = [&](const f32x4 (&acc)[S][1], auto r0) {
        constexpr int R0 = decltype(r0)::value;
        if (FUSE) {
            if (gq() == 0) {
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    const float a0 = acc[s][0][R0], a1 = acc[s][0][R0 + 1], a2 = acc[s][0][R0 + 2];
                    const float inv = 1.f / sqrtf(fmaxf(a0 * a0 + a1 * a1 + a2 * a2, 1.1920928955078125e-07f));
                    const int q = wave * (S * 16) + s * 16 + (int)m15();
                    fz[4 * WG_SAMPLES + q] = a0 * inv; fz[5 * WG_SAMPLES + q] = a1 * inv; fz[6 * WG_SAMPLES + q] = a2 * inv;
                    if constexpr (BLENDED) {
                        if (A.pred_normal && sval(s)) {
                            float* o = A.pred_normal + (long long)sidx(s) * 3;
                            out_store(o, a0 * inv); out_store(o + 1, a1 * inv); out_store(o + 2, a2 * inv);
                        }
                    }
                }
            }
        } else if (A.pred_normal && g == 0) {
#pragma unroll
            for (int s = 0; s < S; ++s)
                if (sval(s)) {
                    const float a0 = acc[s][0][R0], a1 = acc[s][0][R0 + 1], a2 = acc[s][0][R0 + 2];
                    // utils/func.py:5-7: eps clamps the squared norm
                    const float inv = 1.f / sqrtf(fmaxf(a0 * a0 + a1 * a1 + a2 * a2, 1.1920928955078125e-07f));
                    float* o = A.pred_normal + (long long)sidx(s) * 3;
                    out_store(o, a0 * inv); out_store(o + 1, a1 * inv); out_store(o + 2, a2 * inv);
                    if (GRAD && A.save_inv)   // negative marks the clamped branch (constant denominator)
                        A.save_inv[idx[s]] = (a0 * a0 + a1 * a1 + a2 * a2) > 1.1920928955078125e-07f ? inv : -inv;
                }
        }
    };
    // ---- sigma: 256 -> 1 (row 0 of a padded 16-row block lives in lane group 0, reg 0); FOLD: the folded normal_net in rows 1..3
    {
        f32x4 acc[S][1];
        init_bias<1>(acc, BIAS_SIG, gq());
        gemm_part<8, 1, 960, HP>(acc, hh, hl, st, wave, lane16);
        if (FUSE) {
            if (gq() == 0) {
#pragma unroll
                for (int s = 0; s < S; ++s) fz[wave * (S * 16) + s * 16 + m15()] = acc[s][0][0];
            }
        } else if (A.sigma && g == 0) {
#pragma unroll
            for (int s = 0; s < S; ++s)
                if (sval(s)) out_store(A.sigma + sidx(s), acc[s][0][0]);
        }
        if constexpr (FOLD && !RGB_DEPTH) put_normal(acc, std::integral_constant<int, 1>{});
    }

    bool colour = true;      // BLENDED: false for a ray whose colour the caller's blend multiplies by zero
    if (!SIGMA_ONLY) {
        // ---- predicted normal: 256 -> 128 -> 3, no activation in between (mirror_nerf.py:85-88); FOLD: done above
        if constexpr (!FOLD) {
            u32x4 nh[S][4], nl[S][4];
            {
                f32x4 acc[S][8];
                init_bias<8>(acc, BIAS_NRM1, gq());
                gemm_part<8, 8, 968, HP, ST0>(acc, hh, hl, st, wave, lane16, at_h(7, 0));
                if (keep) save_acc<8, 0>(A.save_x + (long long)SEC_HN * A.B, 128, 0, acc, idx, valid, g, unused_bits);
                acc_to_b<8, 0, false>(nh, nl, acc, 0, tid, st.sat);
                if constexpr (S == 2) { if (pl) store_planes<4, 4>(sc, SEC_HN / 16, nh, nl); }
            }
            f32x4 acc[S][1];
            init_bias<1>(acc, BIAS_NRM2, gq());
            gemm_part<4, 1, 1032>(acc, nh, nl, st, wave, lane16);
            put_normal(acc, std::integral_constant<int, 0>{});
        }
        // ---- mirror probability: 256 -> 128 LeakyReLU(0.01) -> 1 sigmoid (mirror_nerf.py:94-99).  FOLD: behind the colour
        //      branch, where the folded stream has it; RGB_DEPTH: never evaluated (its stream ends in front of it)
        const auto mirror_head = [&]() {
            u32x4 mh[S][4], ml[S][4];
            {
                f32x4 acc[S][8];
                init_bias<8>(acc, BIAS_MIR1, gq());
                // (BLENDED: the chunk behind this part is the last one of the mirror head's copy; dir_encoding follows)
                gemm_part<8, 8, BLENDED ? 968 : FOLD ? FOLD_POS_MIR1 : 1036, HP, ST4, 4, false, JT, JUMP_FROM_MIRB>(acc, hh, hl, st, wave, lane16, at_h(7, 4));
                if (keep) {
                    uint64_t bits[S];
                    save_acc<8, 2>(A.save_x + (long long)SEC_HM * A.B, 128, 0, acc, idx, valid, g, bits);
#pragma unroll
                    for (int s = 0; s < S; ++s) gmask[(9 * S + s) * WG_THREADS + tid] = bits[s];
                } else if (GRAD && pl) {
                    store_sign_mask<8>(acc, gmask + (9 * S) * WG_THREADS + tid);
                }
                acc_to_b<8, 2, false>(mh, ml, acc, 0, tid, st.sat);
                if constexpr (S == 2) { if (pl) store_planes<4, 4>(sc, SEC_HM / 16, mh, ml); }
            }
            f32x4 acc[S][1];
            init_bias<1>(acc, BIAS_MIR2, gq());
            gemm_part<4, 1, BLENDED ? 1032 : FOLD ? FOLD_POS_MIR2 : 1100>(acc, mh, ml, st, wave, lane16);
            if (FUSE) {
                if (gq() == 0) {
#pragma unroll
                    for (int s = 0; s < S; ++s) fz[7 * WG_SAMPLES + wave * (S * 16) + s * 16 + m15()] = sigmoidf_(acc[s][0][0]);
                }
            } else if (A.is_mirror && g == 0) {
#pragma unroll
                for (int s = 0; s < S; ++s)
                    if (sval(s)) out_store(A.is_mirror + sidx(s), sigmoidf_(acc[s][0][0]));
            }
        };
        if constexpr (!FOLD) mirror_head();
        if constexpr (BLENDED) {
            mirror_head();
            skip_pairs4<1036>(st, wave, lane16);
            // sigma, mirror and depth rows of all four waves (raw barrier: the LDS-DMA pieces on their way stay on their way)
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            int dl;
            asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(dl));
            // (wave 0, which composites the ray at the end, keeps the weights it forms here)
            const float mv = composite_mirror_value(CompLdsSrc{fz, false, true}, WG_SAMPLES, dl, wave == 0 ? fz + 9 * WG_SAMPLES : nullptr);
            colour = __builtin_amdgcn_readfirstlane((int)(mv < 0.5f)) != 0 || A.fuse == 4;
        }
        // ---- colour: final(256->256, no act) ; cat[final, dir] -> 128 relu ; 128 -> 3 sigmoid.  FOLD: dir_encoding reads h8
        //      through the folded map (final's 256 outputs are never formed)
        // view-encoding B operands (32 padded columns: one k-step)
        const auto view_operands = [&](u32x4 (&vh)[S][1], u32x4 (&vl)[S][1]) {
            float de[S][8];
            const int gv = gq();
            const int spr = opaque_spr();
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const float* dp = A.dir_emb + (long long)(sidx(s) / spr) * A.dir_stride;
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    const int e = 16 * (t >> 2) + 4 * gv + (t & 3);
                    de[s][t] = e < ENC_DIR ? dp[e] : 0.f;
                }
            }
            if (keep) save_bform<8>(A.save_x + (long long)SEC_DIRE * A.B, 32, de, idx, valid, g);
            split_b<8>(de, vh, vl, st.sat);
            if constexpr (S == 2) { if (pl) store_planes<1, 1>(sc, SEC_DIRE / 16, vh, vl); }
        };
        if (colour) {
            u32x4 dh[S][4], dl[S][4];
            if constexpr (FOLD) {
                u32x4 vh[S][1], vl[S][1];
                view_operands(vh, vl);
                f32x4 acc[S][8];
                init_bias<8>(acc, BIAS_DIR, gq());
                gemm_part<8, 8, BLENDED ? 1040 : FOLD_POS_DIR, HP>(acc, hh, hl, st, wave, lane16);
                gemm_part<1, 8, BLENDED ? 1104 : FOLD_POS_VIEW>(acc, vh, vl, st, wave, lane16);
                acc_to_b<8, 1, false>(dh, dl, acc, 0, tid, st.sat);
            } else {
                u32x4 fh[S][8], fl[S][8];
                {
                    f32x4 acc[S][16];
                    init_bias<16>(acc, BIAS_FIN, gq());
                    gemm_part<8, 16, 1104, HP>(acc, hh, hl, st, wave, lane16);
                    if (keep) save_acc<16, 0>(A.save_x + (long long)SEC_FIN * A.B, 256, 0, acc, idx, valid, g, unused_bits);
                    acc_to_b<16, 0, false>(fh, fl, acc, 0, tid, st.sat);
                    if constexpr (S == 2) { if (pl) store_planes<8, 8>(sc, SEC_FIN / 16, fh, fl); }
                }
                u32x4 vh[S][1], vl[S][1];
                view_operands(vh, vl);
                f32x4 acc[S][8];
                init_bias<8>(acc, BIAS_DIR, gq());
                gemm_part<8, 8, 1232>(acc, fh, fl, st, wave, lane16);
                gemm_part<1, 8, 1296>(acc, vh, vl, st, wave, lane16);
                if (keep) {
                    uint64_t bits[S];
                    save_acc<8, 1>(A.save_x + (long long)SEC_HD * A.B, 128, 0, acc, idx, valid, g, bits);
#pragma unroll
                    for (int s = 0; s < S; ++s) gmask[(8 * S + s) * WG_THREADS + tid] = bits[s];
                } else if (GRAD && pl) {
                    store_sign_mask<8>(acc, gmask + (8 * S) * WG_THREADS + tid);
                }
                acc_to_b<8, 1, false>(dh, dl, acc, 0, tid, st.sat);
                if constexpr (S == 2) { if (pl) store_planes<4, 4>(sc, SEC_HD / 16, dh, dl); }
            }
            f32x4 acc[S][1];
            init_bias<1>(acc, BIAS_RGB, gq());
            gemm_part<4, 1, BLENDED ? 1112 : FOLD ? FOLD_POS_RGB : 1304>(acc, dh, dl, st, wave, lane16);
            if (FUSE) {
                if (gq() == 0) {
#pragma unroll
                    for (int s = 0; s < S; ++s) {
                        const int q = wave * (S * 16) + s * 16 + (int)m15();
                        fz[1 * WG_SAMPLES + q] = sigmoidf_(acc[s][0][0]);
                        fz[2 * WG_SAMPLES + q] = sigmoidf_(acc[s][0][1]);
                        fz[3 * WG_SAMPLES + q] = sigmoidf_(acc[s][0][2]);
                    }
                }
            } else if (A.rgb && g == 0) {
#pragma unroll
                for (int s = 0; s < S; ++s)
                    if (sval(s)) {
                        float* o = A.rgb + (long long)sidx(s) * 3;
                        out_store(o, sigmoidf_(acc[s][0][0]));
                        out_store(o + 1, sigmoidf_(acc[s][0][1]));
                        out_store(o + 2, sigmoidf_(acc[s][0][2]));
                    }
            }
        }
        if constexpr (FOLD && !RGB_DEPTH && !BLENDED) mirror_head();
    }

    if (GRAD) {
        // ---- d sigma / d xyz in closed form (SURVEY 8a): g = w_sigma; for i = 8..1:
        //      g = (g * relu_mask_i) W_i, the 63 encoding columns of layer 5 and layer 1 feed g_enc.
        open_stream<false>(st, A.packed + OFF_SPLIT_BWD, wave, lane);
        prime_stream(st, lane16);
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

        // layers 8..1; layer 5 first emits its 4 encoding row blocks, layer 1 only has those
#pragma unroll 1
        for (int layer = 7; layer >= 0; --layer) {
            u32x4 gh[S][8], gl[S][8];
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const uint64_t mk = ((const uint64_t*)(smem + LDS_MASK))[(layer * S + s) * WG_THREADS + tid];
#pragma unroll
                for (int t = 0; t < 64; ++t) gr[s][t] = ((mk >> t) & 1ull) ? gr[s][t] : 0.f;
            }
            split_b<64>(gr, gh, gl, st.sat);
            if (layer == 4 || layer == 0) {
                f32x4 acc[S][4];
                zero_acc<4>(acc);
                gemm_part<8, 4, 0>(acc, gh, gl, st, wave, lane16);
#pragma unroll
                for (int s = 0; s < S; ++s)
#pragma unroll
                    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
                        for (int r = 0; r < 4; ++r) genc[s][4 * nb + r] += acc[s][nb][r];
            }
            if (layer != 0) {
                f32x4 acc[S][16];
                zero_acc<16>(acc);
                gemm_part<8, 16, 0>(acc, gh, gl, st, wave, lane16);
#pragma unroll
                for (int s = 0; s < S; ++s)
#pragma unroll
                    for (int nb = 0; nb < 16; ++nb)
#pragma unroll
                        for (int r = 0; r < 4; ++r) gr[s][4 * nb + r] = acc[s][nb][r];
            }
        }
        // encoding Jacobian: d/dx_a = g[x_a] + sum_f 2^f (g[sin] cos - g[cos] sin)
        float x[S][3];
        fetch_positions(x);
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
                    fast_sincos(ldexpf(xa, f), sn, cs);
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
                float* o = A.normal + (long long)idx[s] * 3;
                o[0] = n0 * inv; o[1] = n1 * inv; o[2] = n2 * inv;
                if (A.save_invj) A.save_invj[idx[s]] = sq > 1.1920928955078125e-07f ? inv : -inv;
            }
        }
    }
    sat_all |= st.sat;
    enc_all |= enc_range;
    if (FUSE) {
        // the workgroup's 192 samples are ONE ray (launcher: spr == WG_SAMPLES, positions from rays + z_vals): composite it
        // with the body of composite_kernel -- one wavefront, three 64-sample blocks -- reading the head outputs from LDS
        __syncthreads();
        if (wave == 0) {
            const long long ray = tile;
            int cl;      // (opaque: a plain lane id is hoisted out of the tile loop and parked in scratch)
            asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(cl));
            if constexpr (RGB_DEPTH) {      // (the launcher refuses mirror-mask and normal maps for this variant)
                const CompMaps out{A.f_weights ? A.f_weights + ray * WG_SAMPLES : nullptr, A.f_opacity, A.f_rgb_map, A.f_depth, nullptr,
                                   nullptr, nullptr, nullptr, A.f_x_surface, A.rays, A.white_back};
                composite_ray(CompLdsSrcRgbDepth{fz, false, false}, WG_SAMPLES, cl, ray, out);
            } else if constexpr (BLENDED) {
                // (`colour` is what every wave decided above from the same rows: a row is 0 exactly where the mirror map written
                // here is not below 0.5)
                const CompLdsSrcBlended src{{fz, A.f_surf_normal != nullptr, A.f_mirror_mask != nullptr}, colour};
                const CompMaps out{A.f_weights ? A.f_weights + ray * WG_SAMPLES : nullptr, A.f_opacity, colour ? A.f_rgb_map : nullptr, A.f_depth,
                                   A.f_mirror_mask, A.f_surf_normal, nullptr, nullptr, A.f_x_surface, A.rays, A.white_back};
                composite_ray(src, WG_SAMPLES, cl, ray, out);
                if (!colour && A.f_rgb_map && cl < 3) A.f_rgb_map[ray * 3 + cl] = 0.f;
            } else {
                const CompLdsSrc src{fz, A.f_surf_normal != nullptr, A.f_mirror_mask != nullptr};
                const CompMaps out{A.f_weights ? A.f_weights + ray * WG_SAMPLES : nullptr, A.f_opacity, A.f_rgb_map, A.f_depth, A.f_mirror_mask,
                                   A.f_surf_normal, nullptr, nullptr, A.f_x_surface, A.rays, A.white_back};
                composite_ray(src, WG_SAMPLES, cl, ray, out);
            }
        }
    }
    if (!queued) break;
    close_stream();
    __syncthreads();      // every wave is done with the ring, the parked operands and the head outputs of this tile
    // (a raw barrier that lets the tile's output stores drain into the next tile measured the same: 15.38-15.40 vs 15.38-15.44 ms)
    tile = __builtin_amdgcn_readfirstlane(((volatile int*)(smem + LDS_TILEQ))[round & 1]);
    ++round;
    if (tile >= A.n_tiles) break;
    }
    guard_report(A.packed, sat_all, enc_all, MNRF_GUARD_IN_FORWARD);
    close_stream();
    int last_lane;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(last_lane));
    if (queued && wave == 0 && last_lane == 0) {      // the last workgroup out leaves the queue at zero for the next launch
        if (atomicAdd(A.tile_queue + 1, 1) == (int)gridDim.x - 1) {
            atomicExch(A.tile_queue, 0);
            atomicExch(A.tile_queue + 1, 0);
        }
    }
}

template <bool SIGMA_ONLY, bool GRAD, bool PLANES = false, bool FUSE = false>
__global__ __launch_bounds__(WG_THREADS, MIN_WAVES_PER_SIMD) void field_split_kernel(FieldArgs A) {
    field_split_body<SIGMA_ONLY, GRAD, PLANES, FUSE, false>(A);
}
// the rgb / depth variant of the ray-fused pass: a kernel of its own name, so that the instantiations above keep theirs
template <bool ON = true>
__global__ __launch_bounds__(WG_THREADS, MIN_WAVES_PER_SIMD) void field_split_kernel_rgb_depth(FieldArgs A) {
    field_split_body<false, false, false, ON, ON>(A);
}

// the blended-level variant of the ray-fused pass (field_split_body BLENDED)
template <bool ON = true>
__global__ __launch_bounds__(WG_THREADS, MIN_WAVES_PER_SIMD) void field_split_kernel_blended(FieldArgs A) {
    field_split_body<false, false, false, ON, false, ON>(A);
}

// (a template only so that the discarded branch below never instantiates the ray-fused kernels in the S = 2 tunings)
template <bool UNUSED = false>
inline int launch(const FieldArgs& A, bool sigma_only, bool grad, hipStream_t s) {
    const long long blocks64 = (A.B + WG_SAMPLES - 1) / WG_SAMPLES;
    if (blocks64 > 0x7fffffff || A.B > 0x7fffffffLL) return -1;
    dim3 grid((unsigned)blocks64);
    const dim3 block(WG_THREADS);
    if (S == 3 && A.tile_queue) {      // dynamic tile queue (launch_split48 filled it in): one resident workgroup per CU
        if (A.n_tiles != (int)blocks64 || A.resident < 1 || A.resident > A.n_tiles) return -1;
        grid = dim3((unsigned)A.resident);
    }
    if (sigma_only && !grad) hipLaunchKernelGGL((field_split_kernel<true, false>), grid, block, LDS_BYTES, s, A);
    else if (!sigma_only && !grad && S == 3 && A.fuse == 2) {
        if constexpr (S == 3) hipLaunchKernelGGL((field_split_kernel_rgb_depth<>), grid, block, LDS_BYTES_FUSE, s, A);
    } else if (!sigma_only && !grad && S == 3 && A.fuse >= 3) {
        if constexpr (S == 3) hipLaunchKernelGGL((field_split_kernel_blended<>), grid, block, LDS_BYTES_FUSE, s, A);
    } else if (!sigma_only && !grad && S == 3 && A.fuse)
        hipLaunchKernelGGL((field_split_kernel<false, false, false, S == 3>), grid, block, LDS_BYTES_FUSE, s, A);
    else if (!sigma_only && !grad) hipLaunchKernelGGL((field_split_kernel<false, false>), grid, block, LDS_BYTES, s, A);
#ifndef MNRF_SPLIT_NO_GRAD
    else if (sigma_only && grad) hipLaunchKernelGGL((field_split_kernel<true, true>), grid, block, LDS_BYTES_GRAD, s, A);
    else if (S == 2 && A.save_planes) hipLaunchKernelGGL((field_split_kernel<false, true, S == 2>), grid, block, LDS_BYTES_GRAD, s, A);
    else hipLaunchKernelGGL((field_split_kernel<false, true>), grid, block, LDS_BYTES_GRAD, s, A);
#else
    else return -1;
#endif
    return 0;
}
