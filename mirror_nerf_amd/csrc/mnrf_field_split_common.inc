// mnrf_field_split_common.inc -- pieces shared by the split-f16 field kernels (mnrf_field_split.inc, mnrf_field_split_bwd.inc):
// the LDS-DMA weight stream, fast sincos, fp32 -> (hi, lo) conversion, the range guard, hand-placed LDS reads.  Included inside a namespace that defines CHUNK_BYTES, CHUNK_PAIRS, RING_SLOTS, PIECES,
// WAVES, PF (and `smem`).
// ------------------------------------------------------------------ weight stream
// The f16 pipe consumes a 16 KiB chunk in ~800 cycles (the fp32 kernel: 4096), so the cost of issuing
// the LDS-DMA matters: with four 1 KiB pieces per wave issued back to back at every chunk seam behind
// `s_waitcnt vmcnt(0)`, removing the DMA made the first version of this kernel 19 % faster.  Here the
// schedule is static: every wave issues exactly ONE piece per GEMM unit (12 MFMAs), filling the chunk TWO ahead of the
// one being read, into a
// ring of four slots; seams wait with a COUNTED vmcnt (loads return in order, so "at most n outstanding"
// means everything but the n youngest pieces has landed).
// The stream is continuous: parts follow each other without padding, every GEMM unit issues exactly one piece, and
// open_stream() issues the first two chunks, so the fill position is always exactly two chunks (2*PIECES units) ahead
// of the unit being consumed: unit u (counted over the whole stream) issues piece u % PIECES of chunk u / PIECES + 2,
// whose slot held a chunk whose last reads were issued before the seam before last.  A part that starts at pair
// position POS knows all of this statically; the seam that opens a chunk sits where the READ pointer (PF pairs ahead
// of consumption) crosses into it, when PIECES - PF/U pieces are younger than that chunk's (PIECES - i/U for a seam
// in a part's first PF reads, i = index of the read).
// The stream is read up to two chunks past its end (valid memory: the next stream or the tail pad of the
// packed image); those pieces are never consumed, and vmcnt is drained before the ring is reused or the
// workgroup ends (a stale LDS-DMA write must not land in another workgroup's LDS).
struct Stream {
    unsigned long long fill_src;   // wave-uniform: global address of this wave's pieces of the chunk being filled
    unsigned wave_lds;             // wave-uniform: LDS byte address of this wave's pieces in slot 0
    unsigned lane_off;             // 16 * lane
    int fill_slot;                 // ring slot being filled
    int rd_slot;                   // ring slot of the newest readable chunk
    // A operands of the NEXT part's first PF pairs, read by the tail of the part before it (or by open_stream): the
    // stream is continuous, so a part's last units simply keep reading ahead and the LDS latency of a part start is
    // hidden behind the epilogue / conversion work between two GEMMs
    u32x4 ch[PF], cl[PF];
    // range guard (see "range guard" below): lanes that converted an operand at or beyond the f16 maximum, as a
    // wave-uniform ballot mask -- two SGPRs, no vector register is held across the kernel -- and the running |maximum| of
    // the conversions of the half layer in flight (flushed into the mask when the half layer is complete)
    unsigned long long sat;
    float tmax;
};

template <int I>
__device__ __forceinline__ void issue_piece(Stream& st) {
    const unsigned lds = st.wave_lds + st.fill_slot * CHUNK_BYTES + (I / 4) * 4096;   // the immediate is 13-bit signed
    const unsigned long long src = st.fill_src + (I / 4) * 4096;
    // The instruction's immediate offset is added to BOTH the global and the LDS address, so the four pieces of a 4 KiB
    // group share one M0 (the LDS-DMA destination) and one address register pair.  Issued through the builtin, not inline
    // asm: hipcc then writes M0 once per group and -- what matters -- its hazard recognizer sees a VMEM instruction.  An
    // earlier inline-asm form (s_mov m0; s_nop 0; global_load_lds with an SGPR base) sat 3 wait states behind the
    // v_readlane that restores a spilled SGPR in the gradient-pass kernels, 2 short of what a VALU-written SGPR needs
    // before a VMEM read; padding it with s_nop 3 cost 4 % (an extra issue state between MFMAs is a cliff, not a slope).
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)((const char*)src + st.lane_off),
                                     (__attribute__((address_space(3))) void*)(size_t)lds, 16, (I % 4) * TILE_BYTES, 0);
    if (I == PIECES - 1) {
        st.fill_src += CHUNK_BYTES;
        st.fill_slot = st.fill_slot == RING_SLOTS - 1 ? 0 : st.fill_slot + 1;
    }
}

// pieces FROM .. PIECES-1 of the chunk being filled
template <int FROM>
__device__ __forceinline__ void issue_rest(Stream& st) {
    if (FROM <= 0) issue_piece<0>(st);
    if (FROM <= 1) issue_piece<1>(st);
    if (FROM <= 2) issue_piece<2>(st);
    if (FROM <= 3) issue_piece<3>(st);
    if (PIECES == 8) {
        if (FROM <= 4) issue_piece<(PIECES == 8 ? 4 : 0)>(st);
        if (FROM <= 5) issue_piece<(PIECES == 8 ? 5 : 0)>(st);
        if (FROM <= 6) issue_piece<(PIECES == 8 ? 6 : 0)>(st);
        if (FROM <= 7) issue_piece<(PIECES == 8 ? 7 : 0)>(st);
    }
}
__device__ __forceinline__ void issue_chunk(Stream& st) { issue_rest<0>(st); }
static_assert(PIECES == 4 || PIECES == 8, "issue_rest");

// Make the next chunk readable; YOUNGER = pieces this wave has issued after that chunk's.
template <int YOUNGER>
__device__ __forceinline__ void seam(Stream& st) {
    asm volatile("s_waitcnt vmcnt(%0)" : : "n"(YOUNGER) : "memory");
    // raw s_barrier, not __syncthreads(): LDS reads of the previous chunk may stay in flight across it
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    st.rd_slot = st.rd_slot == RING_SLOTS - 1 ? 0 : st.rd_slot + 1;
}

template <bool FIRST>
__device__ __forceinline__ void open_stream(Stream& st, const float* base, int wave, int lane) {
    if (!FIRST) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // nothing of the previous stream is still on its way into the ring
        __syncthreads();                                    // and all waves are done reading it
    }
    st.fill_src = (unsigned long long)(size_t)base + wave * PIECES * TILE_BYTES;
    st.wave_lds = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem + wave * PIECES * TILE_BYTES;
    st.lane_off = lane * 16;
    st.fill_slot = 0;
    st.rd_slot = RING_SLOTS - 1;
    issue_chunk(st);
    issue_chunk(st);
}

__device__ __forceinline__ void close_stream() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

typedef _Float16 h8 __attribute__((ext_vector_type(8)));

// ------------------------------------------------------------------ sin / cos of the encoding arguments
// sincosf() of the device library carries a large-argument path and costs ~5 k cycles per tile for the 32 calls of the
// encoding (prologue marks).  The arguments here are 2^f * x with f <= 9: FOUR-term Cody-Waite reduction by pi/2 = C1 + C2 + C3 +
// C4 with C1 of 8, C2 and C3 of 9 significant bits (round 5; it was three terms, exact for |k| < 4096 only, i.e. |x| < 10..16):
// k * C1..C3 are exact for |k| < 2^15 (|a| < 51 000, |x| < 64 at f = 9 -- ENC_RANGE_LIMIT below), the fused multiply-adds keep
// the remainder to an ulp, and the degree-7 / degree-8 minimax polynomials of cephes sinf / cosf follow on [-pi/4, pi/4].
// Max error against double over |x| <= 64, f = 0..9: 1.12e-7 (scripts/check_fast_sincos.py; 1.10e-7 over |x| <= 10).
constexpr float ENC_RANGE_LIMIT = 64.f;      // positions at or beyond it raise MNRF_GUARD_ENC_RANGE
__device__ __forceinline__ void fast_sincos(float a, float& sn, float& cs) {
    const float k = __builtin_rintf(a * 0.6366197723675814f);
    float r = fmaf(-k, 1.5703125f, a);
    r = fmaf(-k, 4.8351287841796875e-4f, r);
    r = fmaf(-k, 3.1385570764541626e-7f, r);
    r = fmaf(-k, 6.07710062827671e-11f, r);
    const float r2 = r * r;
    const float s = fmaf(fmaf(fmaf(-1.9515295891e-4f, r2, 8.3321608736e-3f), r2, -1.6666654611e-1f), r2 * r, r);
    const float c = fmaf(fmaf(fmaf(2.443315711809948e-5f, r2, -1.388731625493765e-3f), r2, 4.166664568298827e-2f), r2 * r2,
                         fmaf(-0.5f, r2, 1.0f));
    const int q = (int)k & 3;
    const float ss = (q & 1) ? c : s, cc = (q & 1) ? s : c;
    sn = (q & 2) ? -ss : ss;
    cs = ((q + 1) & 2) ? -cc : cc;
}

// ------------------------------------------------------------------ fp32 -> (hi, lo) f16 pairs
// v_cvt_pkrtz_f16_f32 rounds toward zero, so lo = x - hi has the sign of x: |x - hi - lo| < 2^-20 |x|.
//
// CONV_SHORT (set by the includer; the forward-only tunings h2 and h3): lo in two instructions instead of five, 8 vector
// instructions per value pair instead of 11 (two accumulator reads, two integer max, cvt_pkrtz, mixlo, mixhi, max3).  x - f32(hi)
// is exact in fp32, so fma(-f32(hi), 1, x) is that same number; v_fma_mixlo_f16 / v_fma_mixhi_f16 take a half of hi as an f16
// source (op_sel_hi says "f16", op_sel which half), form the fp32 FMA and write it as one f16 half, rounded by the wave's f16
// rounding mode -- which conv_round_mode() sets to toward-zero at kernel entry: the bits of v_cvt_pkrtz_f16_f32, its saturation
// at 65504 included (tests/test_hip_split_convert.py holds both forms against the definition and the kernels against each other).
// The mode also governs v_cvt_f16_f32, v_cvt_pk_f16_f32, every *_f16 arithmetic instruction and all f64 arithmetic: the kernels
// of these tunings contain none (DESIGN 4.1b; v_cvt_f32_f16 is exact, v_cvt_pkrtz and the MFMAs do not read the mode).
// hipcc does not select the pair by itself (it turns the multiplication by -1 into a subtraction of a converted value), hence
// inline assembly -- a plain, non-volatile statement with register operands, which the compiler schedules like any instruction
// between the sched_barrier(0) fences of gemm_part_impl; it is no VALU to sched_group_barrier(0x002), whose groups hold the
// task's six other instructions -- and with it the wait states the compiler no longer inserts: the ISA asks for 2 between a
// VALU write of a register and an MFMA reading it as A / B, and for 1 between a write of one half of a register (mixhi) and a
// VALU read of it.  The statement ends with mixhi, so both are owed by what follows it.  The words are B operands of a LATER
// GEMM part: an in-stream job ends 12 to 16 units before its part does, L1's ends with the part, and a block conversion
// (conv_half, split_b, acc_to_b) is followed by sat_flush's compare and ballot; then come the next part's bias reads, its
// opening s_waitcnt and a unit's first MFMAs on other operands.  scripts/check_isa.py asserts on every build that no
// instruction within two of a v_fma_mixhi_f16 names its destination.
// The destination is early-clobber: mixlo writes it before mixhi has read hi and x1.
__device__ __forceinline__ void conv_round_mode() {
    // MODE.FP_ROUND[3:2] (f16 / f64 results) = 3, toward zero; [1:0] (fp32) stays.  Per wave, gone with the wave.
    if constexpr (CONV_SHORT) __builtin_amdgcn_s_setreg(1 | (2 << 6) | ((2 - 1) << 11), 3);      // hwreg(HW_REG_MODE, 2, 2)
}
__device__ __forceinline__ void split2(float x0, float x1, unsigned& hi, unsigned& lo) {
    const auto h = __builtin_amdgcn_cvt_pkrtz(x0, x1);
    hi = __builtin_bit_cast(unsigned, h);
    if constexpr (CONV_SHORT) {
        asm("v_fma_mixlo_f16 %0, -%1, 1.0, %2 op_sel_hi:[1,0,0]\n\t"
            "v_fma_mixhi_f16 %0, -%1, 1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
            : "=&v"(lo)
            : "v"(hi), "v"(x0), "v"(x1));
    } else {
        const float r0 = x0 - (float)h[0];
        const float r1 = x1 - (float)h[1];
        const auto l = __builtin_amdgcn_cvt_pkrtz(r0, r1);
        lo = __builtin_bit_cast(unsigned, l);
    }
}

// ------------------------------------------------------------------ range guard
// hi = f16(x) saturates at 65504 under round-toward-zero: from there on the pair no longer carries 22 bits (the residual lo
// has an ulp of 32), and beyond 131 008 the value itself is clipped.  Every conversion folds |x| of its two inputs into a
// running maximum (one v_max3_f32 per pair; the maximum is local to a block conversion, or lives for one half layer when
// the conversion rides in the MFMA stream), which is compared against 65504 once per block and OR-ed, as a wave ballot,
// into the SGPR pair Stream::sat -- the kernels sit at the 512-register limit and a vector register held from the first
// conversion to the last costs them spills (measured: 50-160 scratch operations).  A wave that ends with a non-zero
// mask sets MNRF_GUARD_SATURATED in the guard word at the end of the packed image.  The host reads that word once per
// frame / training step and re-runs the work on the exact fp32 kernels (mirror_nerf.check_guard).  Positions with
// |x| >= 64 (ENC_RANGE_LIMIT: sin / cos arguments of 2^15 and beyond, outside fast_sincos' exact reduction) set MNRF_GUARD_ENC_RANGE.
constexpr float F16_MAX = 65504.f;
template <bool NONNEG>
__device__ __forceinline__ void sat_track(float& tmax, float a, float b) {
    tmax = NONNEG ? __builtin_fmaxf(__builtin_fmaxf(tmax, a), b) : __builtin_fmaxf(__builtin_fmaxf(tmax, fabsf(a)), fabsf(b));
}
__device__ __forceinline__ void sat_flush(unsigned long long& sat, float& tmax, float limit = F16_MAX) {
    sat |= __builtin_amdgcn_ballot_w64(!(tmax < limit));
    tmax = 0.f;
}
// `who`: which pass saturated (MNRF_GUARD_IN_*: diagnostics only -- the host reports it with the warning)
__device__ __forceinline__ void guard_report(const float* packed, unsigned long long sat, unsigned long long enc_range, unsigned who = 0u) {
    if (sat | enc_range) {     // wave-uniform
        if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0)
            atomicOr((unsigned*)(packed + PACKED_FLOATS - 1), (sat ? (MNRF_GUARD_SATURATED | who) : 0u) | (enc_range ? MNRF_GUARD_ENC_RANGE : 0u));
    }
}

// ------------------------------------------------------------------ GEMM building block
// acc[s][nb] += sum_T  A_hi(T,nb) x b_hi[s][T] + A_lo(T,nb) x b_hi[s][T] + A_hi(T,nb) x b_lo[s][T].
// A operands: hand-placed ds_read_b128 (hi at the pair's base, lo 1 KiB behind), PF pairs ahead of
// their MFMAs, consumed in units of U pairs behind one counted lgkmcnt wait (see mnrf_field_impl.inc
// for why the wait carries the tiles as in/out operands).

__device__ __forceinline__ void lds_read_half_tile(u32x4& dst, unsigned addr, int off) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(off) : "memory");
}

#define MNRF_WAIT_CASE(n) \
    if (N == n) asm volatile("s_waitcnt lgkmcnt(" #n ")" : "+v"(t0), "+v"(t1), "+v"(t2), "+v"(t3) : : "memory");
template <int N>
__device__ __forceinline__ void wait_lds_reads_but(u32x4& t0, u32x4& t1, u32x4& t2, u32x4& t3) {
    static_assert(N >= 0 && N <= 4 && N % 2 == 0, "reads come in pairs, PF - U <= 2 pairs are younger");
    MNRF_WAIT_CASE(0) MNRF_WAIT_CASE(2) MNRF_WAIT_CASE(4)
}
#undef MNRF_WAIT_CASE

// The PF carried pairs (Stream::ch / cl) must have LANDED before the compiler may touch their registers (a loop-carried
// copy, a spill): it takes an asm output for available at once, so the wait names them as in/out operands.
__device__ __forceinline__ void carry_wait(Stream& st, std::integral_constant<int, 4>) {
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(st.ch[0]), "+v"(st.cl[0]), "+v"(st.ch[1]), "+v"(st.cl[1]), "+v"(st.ch[2]), "+v"(st.cl[2]), "+v"(st.ch[3]),
                   "+v"(st.cl[3])
                 :
                 : "memory");
}
__device__ __forceinline__ void carry_wait(Stream& st, std::integral_constant<int, 2>) {
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(st.ch[0]), "+v"(st.cl[0]), "+v"(st.ch[1]), "+v"(st.cl[1]) : : "memory");
}

// First reads of a stream (positions 0 .. PF-1), called right before its first GEMM -- not in open_stream(), whose
// LDS-DMA should travel while the caller still has other work -- ; every later part finds its first PF pairs already
// requested by its predecessor.
__device__ __forceinline__ void prime_stream(Stream& st, int lane16) {
    const unsigned ring = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem + (unsigned)lane16;
    seam<PIECES>(st);
    const unsigned base = ring + st.rd_slot * CHUNK_BYTES;
    static_assert(PF <= CHUNK_PAIRS, "the first reads stay inside chunk 0");
#pragma unroll
    for (int i = 0; i < PF; ++i) {
        lds_read_half_tile(st.ch[i], base, i * PAIR_BYTES);
        lds_read_half_tile(st.cl[i], base, i * PAIR_BYTES + TILE_BYTES);
    }
    carry_wait(st, std::integral_constant<int, PF>{});
}

