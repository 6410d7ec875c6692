// mnrf_field_split_bwd.inc -- backward of the field (training) on the f16 matrix pipe, included after
// mnrf_field_split.inc inside a split tuning's namespace (same tile: 4 waves x 32 samples).
//
// Same computation, inputs and outputs as field_bwd_kernel (mnrf_field_bwd.inc): given dL/d{sigma, rgb, pred_normal,
// is_mirror} per sample and the masks / head outputs the training forward saved, back-propagate through the four heads
// and the 8x256 trunk on the transposed weight streams and write the pre-activation gradient dY of every Linear (the A
// operands of the dW GEMMs), dL/dxyz and dL/d(view encoding).  Autograd equivalent: loss.backward() through
// models/mirror_nerf.py:189-212.
//
// Arithmetic: W^T g  ~=  W_hi.g_hi + W_lo.g_hi + W_hi.g_lo as in the forward kernel.  Gradients, unlike activations, have
// no natural scale (a compositing weight of 1e-9 gives seeds of 1e-12, far below f16's 6e-8), but the map from a
// sample's seeds to all of its gradients is LINEAR: every sample's seeds are multiplied by one power of two that
// puts the largest of them at 2^6 (exact), and every stored gradient is multiplied by its inverse (exact).

// x[S][N] -> N/8 B operands
template <int N>
__device__ __forceinline__ void to_b(const float (&x)[S][N], u32x4 (&hi)[S][N / 8], u32x4 (&lo)[S][N / 8], unsigned long long& sat,
                                     float limit = F16_MAX) {
    split_b<N>(x, hi, lo, sat, limit);
}

template <int NB, int NT>
__device__ __forceinline__ void acc_out(float (&dst)[S][NT], const f32x4 (&acc)[S][NB]) {
    static_assert(NT == 4 * NB, "shape");
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[s][4 * nb + r] = acc[s][nb][r];
}

// store a B-form vector multiplied by the sample's inverse scale 2^-k
template <int NT>
__device__ __forceinline__ void save_scaled(float* sec, int width, const float (&x)[S][NT], const int (&k)[S],
                                            const int (&idx)[S], const bool (&valid)[S], int g) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
        if (!valid[s]) continue;
        f32x4* o = (f32x4*)(sec + (long long)idx[s] * width);
#pragma unroll
        for (int nb = 0; nb < NT / 4; ++nb)
            row_store(o + nb * 4 + g, f32x4{ldexpf(x[s][4 * nb], -k[s]), ldexpf(x[s][4 * nb + 1], -k[s]),
                                            ldexpf(x[s][4 * nb + 2], -k[s]), ldexpf(x[s][4 * nb + 3], -k[s])});
    }
}

// ---- round 3: dY as operand planes (mnrf_dwp.h).  The hi/lo halves of sample s carry 2^k_s dY; the weight-gradient GEMM
// contracts over samples and needs one scale per launch: halves are multiplied by 2^(K - k_s) <= 1 (packed f16 multiply,
// exact until the product drops below f16's 2^-24, i.e. below 2^-30 of the largest seed of the launch; a factor below 2^-24
// is zero).  NH = 2: both halves of every operand (32-wide k steps); NH = 1: the 16-row seed blocks use half 0 only.
template <int NT, int NH, int NTA>
__device__ __forceinline__ void store_dy_planes(const StoreCtx& sc, int fb0, const u32x4 (&hi)[S][NTA], const u32x4 (&lo)[S][NTA]) {
    static_assert(S == 2, "a sample block is one wave of two 16-sample groups");
#pragma unroll
    for (int T = 0; T < NT; ++T)
#pragma unroll
        for (int h = 0; h < NH; ++h)
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const int off = (fb0 + NH * T + h) * PL_FB_BYTES + s * 512;
                // (built element by element in an unrolled loop, `a[c] = ...`, hipcc 7.2 kept only element 0 of every operand:
                // caught in the ISA, hence the explicit constructors)
                const auto mul = [&](unsigned w) { return __builtin_bit_cast(unsigned, __builtin_bit_cast(h2v, w) * sc.fac[s]); };
                __builtin_amdgcn_raw_buffer_store_b64(u32x2{mul(hi[s][T][2 * h]), mul(hi[s][T][2 * h + 1])}, sc.rsrc, sc.lane, off, PL_STORE_AUX);
                __builtin_amdgcn_raw_buffer_store_b64(u32x2{mul(lo[s][T][2 * h]), mul(lo[s][T][2 * h + 1])}, sc.rsrc_lo, sc.lane,
                                                      off + PL_TILE_BYTES, PL_STORE_AUX);
            }
}

// PLANES: dY goes out as operand planes (A.dY_planes, A.seedmax) instead of fp32 rows (A.dY)
template <bool PLANES>
__global__ __launch_bounds__(WG_THREADS, 1) void field_split_bwd_kernel(FieldBwdArgs A) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4;
    const int m = lane & 15;
    const int lane16 = lane * 16;
    if constexpr (PLANES) {      // live row count (FieldBwdArgs::n_live)
        if (A.n_live) {
            long long bl = (long long)*A.n_live * A.spr;
            bl = bl < 0 ? 0 : bl;
            if (bl < A.B) A.B = bl;
        }
        if ((long long)blockIdx.x * WG_SAMPLES >= A.B) return;
    }
    const unsigned long long* gm = A.save_mask + (long long)blockIdx.x * (N_MASKS * S * WG_THREADS);

    Stream st;
    st.sat = 0;
    st.tmax = 0.f;
    open_stream<true>(st, A.packed + OFF_SPLIT_HBWD, wave, lane);

    int idx[S];   // sample index (B < 2^31 is checked at launch): one register each instead of two
    bool valid[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        long long i = (long long)blockIdx.x * WG_SAMPLES + wave * (S * 16) + s * 16 + m;
        valid[s] = i < A.B;
        if (!valid[s]) i = A.B - 1;
        idx[s] = (int)i;
    }
    // 0: that head's gradient stops at geo_feat (the --detach_density_* options); index 0 = normal head, 1 = mirror head
    float keep[2][S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        keep[0][s] = (A.cut & MNRF_CUT_NORMAL_HEAD) ? 0.f : 1.f;
        keep[1][s] = (A.cut & MNRF_CUT_MIRROR_HEAD) ? 0.f : 1.f;
        if (A.keep_mirror && A.keep_mirror[A.xyz ? idx[s] : idx[s] / A.spr] == 0.f) keep[1][s] = 0.f;
    }

    // ---- seeds (pre-activation gradients of the four output layers), read by all four lanes of a sample so that the
    //      sample's scale is known without a shuffle
    float s_sig[S], s_rgb[S][3], s_pn[S][3], s_mir[S];
    int k[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const long long i = idx[s];
        s_sig[s] = (A.g_sigma && valid[s]) ? A.g_sigma[i] : 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float y = A.rgb[i * 3 + c];
            s_rgb[s][c] = (A.g_rgb && valid[s]) ? A.g_rgb[i * 3 + c] * y * (1.f - y) : 0.f;
        }
        s_pn[s][0] = s_pn[s][1] = s_pn[s][2] = 0.f;
        if (A.g_pn && valid[s]) {
            const float inv = A.save_inv[i];
            const float g0 = A.g_pn[i * 3], g1 = A.g_pn[i * 3 + 1], g2 = A.g_pn[i * 3 + 2];
            if (inv > 0.f) {   // d(v/|v|) = (g - pn (pn.g)) / |v|
                const float p0 = A.pn[i * 3], p1 = A.pn[i * 3 + 1], p2 = A.pn[i * 3 + 2];
                const float dt = p0 * g0 + p1 * g1 + p2 * g2;
                s_pn[s][0] = (g0 - p0 * dt) * inv; s_pn[s][1] = (g1 - p1 * dt) * inv; s_pn[s][2] = (g2 - p2 * dt) * inv;
            } else {           // eps clamp active: the denominator is the constant sqrt(eps)
                s_pn[s][0] = -g0 * inv; s_pn[s][1] = -g1 * inv; s_pn[s][2] = -g2 * inv;
            }
        }
        {
            const float y = A.is_mirror[i];
            s_mir[s] = (A.g_m && valid[s]) ? A.g_m[i] * y * (1.f - y) : 0.f;
        }
        float mx = fabsf(s_sig[s]);
#pragma unroll
        for (int c = 0; c < 3; ++c) mx = fmaxf(mx, fmaxf(fabsf(s_rgb[s][c]), fabsf(s_pn[s][c])));
        mx = fmaxf(mx, fabsf(s_mir[s]));
        // 2^k * mx in [2^6, 2^7); zero / non-finite seeds keep k = 0
        const int e = (int)((__builtin_bit_cast(unsigned, mx) >> 23) & 0xffu);
        k[s] = (e == 0 || e == 255) ? 0 : A.seed_log2 - (e - 127);
        s_sig[s] = ldexpf(s_sig[s], k[s]);
        s_mir[s] = ldexpf(s_mir[s], k[s]);
#pragma unroll
        for (int c = 0; c < 3; ++c) { s_rgb[s][c] = ldexpf(s_rgb[s][c], k[s]); s_pn[s][c] = ldexpf(s_pn[s][c], k[s]); }
    }

    // operand planes: this lane's corner of the wave's sample block, and every sample's factor 2^(K - k_s)
    // dY plane stores inside the GEMMs that read the same operands (default since round 5, see mnrf_field_split.inc: 4.34-4.36
    // against 4.44-4.50 ms per training step with only this kernel woven; round 3 measured a loss)
    constexpr bool WEAVE = PLANES;
    char* const pl = PLANES ? A.dY_planes + ((long long)blockIdx.x * WAVES + wave) * PLY_SB_BYTES : nullptr;      // wave-uniform
    h2v fac[S];
    {
        const unsigned mxb = PLANES ? *A.seedmax : 0u;
        const int E = (int)((mxb >> 23) & 0xffu);
        const int K = (E == 0 || E == 255) ? 0 : A.seed_log2 - (E - 127);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            int d = K - k[s];
            d = (d > 0 ? 0 : d) + PL_BOOST_LOG2;      // (K <= k_s by construction; zero / non-finite seeds keep k_s = 0)
            const _Float16 f = d < -24 ? (_Float16)0.f : (_Float16)ldexpf(1.f, d);
            fac[s] = h2v{f, f};
        }
    }
    StoreCtx sc;
#pragma unroll
    for (int s = 0; s < S; ++s) sc.fac[s] = fac[s];
    // tile of feature block fb of this lane's sample block: where the store side job of a GEMM part begins
    sc.rsrc = plane_rsrc(pl);
    sc.rsrc_lo = (PLANES && A.y_half) ? __builtin_amdgcn_make_buffer_rsrc(pl, 0, 0, 0x00020000) : sc.rsrc;      // zero records: dropped
    sc.base = pl;
    sc.lane = 32 * m + 8 * g;
    sc.soff = 0;
    const auto at_fb = [&](int fb) -> const StoreCtx& {
        sc.soff = fb * PL_FB_BYTES;
        return sc;
    };
    // a plane overflows where a scaled gradient reaches 65504 / 2^PL_BOOST_LOG2: the range guard fires there already
    const float glimit = PLANES ? F16_MAX / (float)(1 << PL_BOOST_LOG2) : F16_MAX;
    // ---- dL/dh8 starts with the sigma head, w_sigma * dL/dsigma -- but not HERE (round 4): the 128 registers of g8 used to be
    // live through the whole colour branch below, whose own vectors fill the register file, and ~65 of them went to scratch and
    // back (VMEM operations in the middle of the weight stream's counted waits).  w_sigma waits in LDS behind the ring and g8 is
    // formed where the colour branch delivers its share: (w_sigma * dL/dsigma) + share, the same two roundings in the same order.
    float g8[S][64];
    ((float*)(smem + LDS_RING))[tid] = (A.packed + OFF_BIAS + BIAS_WSIG)[tid];      // 256 threads, 256 weights
    // ... and so do this thread's 20 activation-mask words (thread-private slots: no barrier): a global load in the middle of the
    // streams is a VMEM operation that the counted waits of the weight stream queue behind, an LDS read is not
    unsigned long long* const lm = (unsigned long long*)(smem + LDS_RING + 1024) + tid;
    {
        unsigned long long mw[N_MASKS * S];
#pragma unroll
        for (int i = 0; i < N_MASKS * S; ++i) mw[i] = gm[i * WG_THREADS + tid];
#pragma unroll
        for (int i = 0; i < N_MASKS * S; ++i) lm[i * WG_THREADS] = mw[i];
    }
    __syncthreads();
    // a 3-row seed as the B operand of a 16-row contraction padded to one 32-wide step: rows 0..2 live in lane group 0
    auto seed_b = [&](const float (&v)[S][3], float (&b8)[S][8]) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
#pragma unroll
            for (int c = 0; c < 8; ++c) b8[s][c] = 0.f;
            if (g == 0) { b8[s][0] = v[s][0]; b8[s][1] = v[s][1]; b8[s][2] = v[s][2]; }
        }
    };
    auto save_seed = [&](float* sec, const float (&b8)[S][8]) {
        float b4[S][4];
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
            for (int c = 0; c < 4; ++c) b4[s][c] = b8[s][c];
        if (!PLANES && A.dY) save_scaled<4>(sec, 16, b4, k, idx, valid, g);
    };

    if (PLANES) {      // the sigma seed as a 16-row block (row 0): the A operand of sigma's weight gradient
        float b8[S][8];
#pragma unroll
        for (int s = 0; s < S; ++s) {
#pragma unroll
            for (int c = 0; c < 8; ++c) b8[s][c] = 0.f;
            if (g == 0) b8[s][0] = s_sig[s];
        }
        u32x4 bh[S][1], bl[S][1];
        to_b<8>(b8, bh, bl, st.sat, glimit);
        store_dy_planes<1, 1, 1>(sc, PLY_SIG, bh, bl);
    }
    prime_stream(st, lane16);
    // ---- colour branch: rgb (sigmoid) <- hd (relu) <- [final | view] ; final <- h8
    {
        float b8[S][8];
        seed_b(s_rgb, b8);
        save_seed(A.dY + (long long)DY_RGB * A.B, b8);
        u32x4 bh[S][1], bl[S][1];
        to_b<8>(b8, bh, bl, st.sat, glimit);
        if (PLANES) store_dy_planes<1, 1, 1>(sc, DY_RGB / 16, bh, bl);
        float dydir[S][32];
        {
            f32x4 acc[S][8];
            zero_acc<8>(acc);
            gemm_part<1, 8, 0>(acc, bh, bl, st, wave, lane16);
            acc_out(dydir, acc);
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const uint64_t mb = lm[(8 * S + s) * WG_THREADS];
#pragma unroll
                for (int t = 0; t < 32; ++t) dydir[s][t] = ((mb >> t) & 1ull) ? dydir[s][t] : 0.f;
            }
        }
        if (!PLANES && A.dY) save_scaled<32>(A.dY + (long long)DY_DIR * A.B, 128, dydir, k, idx, valid, g);
        u32x4 dh[S][4], dl[S][4];
        to_b<32>(dydir, dh, dl, st.sat, glimit);
        float dyfin[S][64];
        {
            f32x4 acc[S][16];
            zero_acc<16>(acc);
            // (operand planes: the 32 stores of dY_dir ride in this GEMM, which reads the same operands)
            if (PLANES && !WEAVE) store_dy_planes<4, 2, 4>(sc, DY_DIR / 16, dh, dl);
            if (WEAVE) gemm_part<4, 16, 8, 0, 0, 4, true>(acc, dh, dl, st, wave, lane16, at_fb(DY_DIR / 16));
            else gemm_part<4, 16, 8>(acc, dh, dl, st, wave, lane16);
            acc_out(dyfin, acc);
        }
        if (!PLANES && A.dY) save_scaled<64>(A.dY + (long long)DY_FIN * A.B, 256, dyfin, k, idx, valid, g);
        {
            f32x4 acc[S][2];
            zero_acc<2>(acc);
            gemm_part<4, 2, 72>(acc, dh, dl, st, wave, lane16);
            if (A.d_dir) {
                float gd[S][8];
                acc_out(gd, acc);
                save_scaled<8>(A.d_dir, 32, gd, k, idx, valid, g);
            }
        }
        {
            u32x4 fh[S][8], fl[S][8];
            to_b<64>(dyfin, fh, fl, st.sat, glimit);
            f32x4 acc[S][16];
            zero_acc<16>(acc);
            if (PLANES && !WEAVE) store_dy_planes<8, 2, 8>(sc, DY_FIN / 16, fh, fl);
            if (WEAVE) gemm_part<8, 16, 80, 0, 0, 8, true>(acc, fh, fl, st, wave, lane16, at_fb(DY_FIN / 16));
            else gemm_part<8, 16, 80>(acc, fh, fl, st, wave, lane16);
            const f32x4* ws = (const f32x4*)(smem + LDS_RING);
#pragma unroll
            for (int nb = 0; nb < 16; ++nb) {
                const f32x4 v = ws[nb * 4 + g];
#pragma unroll
                for (int s = 0; s < S; ++s)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float sig = v[r] * s_sig[s];
                        g8[s][4 * nb + r] = sig + acc[s][nb][r];
                    }
            }
        }
    }
    // ---- predicted normal: pn = v / |v| <- hn (no activation) <- h8 ; mirror: sigmoid <- hm (LeakyReLU 0.01) <- h8
#pragma unroll
    for (int head = 0; head < 2; ++head) {
        float b8[S][8];
        if (head == 0) {
            seed_b(s_pn, b8);
        } else {
            float v[S][3];
#pragma unroll
            for (int s = 0; s < S; ++s) { v[s][0] = s_mir[s]; v[s][1] = 0.f; v[s][2] = 0.f; }
            seed_b(v, b8);
        }
        save_seed(A.dY + (long long)(head == 0 ? DY_NRM2 : DY_MIR2) * A.B, b8);
        u32x4 bh[S][1], bl[S][1];
        to_b<8>(b8, bh, bl, st.sat, glimit);
        if (PLANES) store_dy_planes<1, 1, 1>(sc, (head == 0 ? DY_NRM2 : DY_MIR2) / 16, bh, bl);
        float dy1[S][32];
        {
            f32x4 acc[S][8];
            zero_acc<8>(acc);
            if (head == 0) gemm_part<1, 8, 208>(acc, bh, bl, st, wave, lane16);
            else gemm_part<1, 8, 280>(acc, bh, bl, st, wave, lane16);
            acc_out(dy1, acc);
            if (head == 1) {
#pragma unroll
                for (int s = 0; s < S; ++s) {
                    const uint64_t mb = lm[(9 * S + s) * WG_THREADS];
#pragma unroll
                    for (int t = 0; t < 32; ++t) dy1[s][t] = ((mb >> t) & 1ull) ? dy1[s][t] : 0.01f * dy1[s][t];
                }
            }
        }
        if (!PLANES && A.dY) save_scaled<32>(A.dY + (long long)(head == 0 ? DY_NRM1 : DY_MIR1) * A.B, 128, dy1, k, idx, valid, g);
        u32x4 h1[S][4], l1[S][4];
        to_b<32>(dy1, h1, l1, st.sat, glimit);
        f32x4 acc[S][16];
        zero_acc<16>(acc);
        if (PLANES && !WEAVE) store_dy_planes<4, 2, 4>(sc, (head == 0 ? DY_NRM1 : DY_MIR1) / 16, h1, l1);
        if (WEAVE) {
            if (head == 0) gemm_part<4, 16, 216, 0, 0, 4, true>(acc, h1, l1, st, wave, lane16, at_fb(DY_NRM1 / 16));
            else gemm_part<4, 16, 288, 0, 0, 4, true>(acc, h1, l1, st, wave, lane16, at_fb(DY_MIR1 / 16));
        } else {
            if (head == 0) gemm_part<4, 16, 216>(acc, h1, l1, st, wave, lane16);
            else gemm_part<4, 16, 288>(acc, h1, l1, st, wave, lane16);
        }
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
            for (int nb = 0; nb < 16; ++nb)
#pragma unroll
                for (int r = 0; r < 4; ++r) g8[s][4 * nb + r] += keep[head][s] * acc[s][nb][r];
    }

    // ---- trunk, layers 8..1 (transposed stream shared with the density-gradient pass)
    open_stream<false>(st, A.packed + OFF_SPLIT_BWD, wave, lane);
    prime_stream(st, lane16);
    float genc[S][16];
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int t = 0; t < 16; ++t) genc[s][t] = 0.f;
#pragma unroll 1
    for (int layer = 7; layer >= 0; --layer) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const uint64_t mk = lm[(layer * S + s) * WG_THREADS];
#pragma unroll
            for (int t = 0; t < 64; ++t) g8[s][t] = ((mk >> t) & 1ull) ? g8[s][t] : 0.f;
        }
        if (!PLANES && A.dY) save_scaled<64>(A.dY + (long long)(DY_L + 256 * layer) * A.B, 256, g8, k, idx, valid, g);
        u32x4 gh[S][8], gl[S][8];
        to_b<64>(g8, gh, gl, st.sat, glimit);
        if (PLANES && (layer == 0 || !WEAVE)) store_dy_planes<8, 2, 8>(sc, DY_L / 16 + 16 * layer, gh, gl);      // (layer 1 has no 256-row GEMM to ride in)
        if (layer == 4 || layer == 0) {     // the 4 encoding row blocks of layers 5 and 1
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
            if (WEAVE) gemm_part<8, 16, 0, 0, 0, 8, true>(acc, gh, gl, st, wave, lane16, at_fb(DY_L / 16 + 16 * layer));
            else gemm_part<8, 16, 0>(acc, gh, gl, st, wave, lane16);
            acc_out(g8, acc);
        }
    }
    // ---- encoding Jacobian -> dL/dxyz (the positions are only needed here: fetched now, not held through the kernel)
    if (A.d_xyz) {
        float x[S][3];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const long long i = idx[s];
            if (A.xyz) {
                const float* p = A.xyz + i * A.xyz_stride;
                x[s][0] = p[0]; x[s][1] = p[1]; x[s][2] = p[2];
            } else {
                const float* r = A.rays + (i / A.spr) * 8;
                const float z = A.z_vals[i];
#pragma unroll
                for (int a = 0; a < 3; ++a) x[s][a] = r[a] + r[3 + a] * z;
            }
        }
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
            if (g == 0 && valid[s]) {
                float* o = A.d_xyz + (long long)idx[s] * 3;
                o[0] = ldexpf(d0, -k[s]); o[1] = ldexpf(d1, -k[s]); o[2] = ldexpf(d2, -k[s]);
            }
        }
    }
    guard_report(A.packed, st.sat, 0ull, MNRF_GUARD_IN_BACKWARD);   // a scaled gradient left the f16 range (the positions were checked by the forward)
    close_stream();
}

inline int launch_bwd(const FieldBwdArgs& A, hipStream_t s) {
    const long long blocks64 = (A.B + WG_SAMPLES - 1) / WG_SAMPLES;
    if (blocks64 > 0x7fffffff || A.B > 0x7fffffffLL) return -1;
    constexpr int LDS_BWD = LDS_RING + 1024 + N_MASKS * S * WG_THREADS * 8;      // ring | w_sigma | activation masks
    static_assert(LDS_BWD <= 160 * 1024, "LDS budget");
    if (A.dY_planes) hipLaunchKernelGGL(field_split_bwd_kernel<true>, dim3((unsigned)blocks64), dim3(WG_THREADS), LDS_BWD, s, A);
    else hipLaunchKernelGGL(field_split_bwd_kernel<false>, dim3((unsigned)blocks64), dim3(WG_THREADS), LDS_BWD, s, A);
    return 0;
}

// ------------------------------------------------------------------ second-order term
// Same computation as field_bwd2_kernel (mnrf_field_bwd.inc): the forward TANGENT pass a'_i = D_i W_i a'_{i-1} from
// a'_0 = E'(x) J^ on the forward stream's trunk (consumed half by half, as the forward kernel does), then the
// density-gradient signals b_8..b_1 on the transposed stream; a' and b go to HBM for the dW GEMMs, dL/dx gets the
// diagonal Hessian of the encoding.  The tangents are linear in J^ = dL/dJ, which has no natural scale: each sample's J^
// is multiplied by the power of two that puts its largest component in [1, 2) and the stored tangents by the inverse.
// The signals b start from w_sigma and need none.  Autograd equivalent: the create_graph=True path of
// utils/func.py:10-25 under loss.backward().
// PLANES (round 4): a' and b leave as the operand planes of mnrf_dwp.h ("second-order pass") -- the hi/lo B operands this
// kernel splits for its own GEMMs anyway -- instead of 16.6 KB of fp32 rows per sample; the weight-gradient GEMM of the
// module's tape contracts them in the same launch as the first-order planes.
template <bool PLANES>
__global__ __launch_bounds__(WG_THREADS, 1) void field_split_bwd2_kernel(FieldBwd2Args A) {
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4;
    const int m = lane & 15;
    const int lane16 = lane * 16;
    if constexpr (PLANES) {      // live row count (FieldBwd2Args::n_live)
        if (A.n_live) {
            long long bl = (long long)*A.n_live * A.spr;
            bl = bl < 0 ? 0 : bl;
            if (bl < A.B) A.B = bl;
        }
        if ((long long)blockIdx.x * WG_SAMPLES >= A.B) return;
    }
    const unsigned long long* gm = A.save_mask + (long long)blockIdx.x * (N_MASKS * S * WG_THREADS);

    // the 16 relu-mask words of this thread wait in LDS (thread-private slots), as in field_split_bwd_kernel, and so does w_sigma
    // (the seed of the signal pass: a global load at the switch of the streams would sit in front of the new stream's waits)
    unsigned long long* const lm = (unsigned long long*)(smem + LDS_RING) + tid;
    {
        unsigned long long mw[8 * S];
#pragma unroll
        for (int i = 0; i < 8 * S; ++i) mw[i] = gm[i * WG_THREADS + tid];
#pragma unroll
        for (int i = 0; i < 8 * S; ++i) lm[i * WG_THREADS] = mw[i];
    }
    ((float*)(smem + LDS_RING + 8 * S * WG_THREADS * 8))[tid] = (A.packed + OFF_BIAS + BIAS_WSIG)[tid];
    __syncthreads();

    Stream st;
    st.sat = 0;
    st.tmax = 0.f;
    open_stream<true>(st, A.packed + OFF_SPLIT_FWD, wave, lane);

    int idx[S];   // sample index (B < 2^31 is checked at launch): one register each instead of two
    bool valid[S];
    float x[S][3], jh[S][3];
    int k[S];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        long long i = (long long)blockIdx.x * WG_SAMPLES + wave * (S * 16) + s * 16 + m;
        valid[s] = i < A.B;
        if (!valid[s]) i = A.B - 1;
        idx[s] = (int)i;
        if (A.xyz) {
            const float* p = A.xyz + i * A.xyz_stride;
            x[s][0] = p[0]; x[s][1] = p[1]; x[s][2] = p[2];
        } else {
            const float* r = A.rays + (i / A.spr) * 8;
            const float z = A.z_vals[i];
#pragma unroll
            for (int a = 0; a < 3; ++a) x[s][a] = r[a] + r[3 + a] * z;
        }
        // n = -J * inv  =>  J^ = -(g - n (n.g)) * inv   (clamped: J^ = -g * inv_c)
        const float inv = A.save_invj[i];
        const float g0 = A.g_normal[i * 3], g1 = A.g_normal[i * 3 + 1], g2 = A.g_normal[i * 3 + 2];
        if (inv > 0.f) {
            const float n0 = A.normal[i * 3], n1 = A.normal[i * 3 + 1], n2 = A.normal[i * 3 + 2];
            const float dt = n0 * g0 + n1 * g1 + n2 * g2;
            jh[s][0] = -(g0 - n0 * dt) * inv; jh[s][1] = -(g1 - n1 * dt) * inv; jh[s][2] = -(g2 - n2 * dt) * inv;
        } else {
            jh[s][0] = g0 * inv; jh[s][1] = g1 * inv; jh[s][2] = g2 * inv;
        }
        if (!valid[s]) { jh[s][0] = 0.f; jh[s][1] = 0.f; jh[s][2] = 0.f; }
        const float mx = fmaxf(fabsf(jh[s][0]), fmaxf(fabsf(jh[s][1]), fabsf(jh[s][2])));
        const int e = (int)((__builtin_bit_cast(unsigned, mx) >> 23) & 0xffu);
        k[s] = (e == 0 || e == 255) ? 0 : -(e - 127);      // 2^k * mx in [1, 2): the encoding tangent stays below 2^11
    }
    // ---- a'_0 = E'(x) J^ in the (sin,cos)-pair order of the encoding (scaled by 2^k)
    float te[S][16];
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const float j0 = ldexpf(jh[s][0], k[s]), j1 = ldexpf(jh[s][1], k[s]), j2 = ldexpf(jh[s][2], k[s]);
#pragma unroll
        for (int pp = 0; pp < 8; ++pp) {
            const int P = 8 * g + pp;
            const int f = P / 3;
            const int a = P - 3 * f;
            const float xa = a == 0 ? x[s][0] : (a == 1 ? x[s][1] : x[s][2]);
            const float ja = a == 0 ? j0 : (a == 1 ? j1 : j2);
            float sn, cs;
            fast_sincos(ldexpf(xa, f), sn, cs);
            float es = ldexpf(cs * ja, f), ec = -ldexpf(sn * ja, f);
            if (P >= 30) {
                es = P == 30 ? j0 : j2;
                ec = P == 30 ? j1 : 0.f;
            }
            te[s][2 * pp] = es;
            te[s][2 * pp + 1] = ec;
        }
    }
    // operand planes: this wave's sample block of the X2 (tangents x the sample's factor 2^(K2 - k_s) <= 1) and Y2 (signals x
    // 2^boost) buffers.  The factor rides on the TANGENTS because they have the headroom: a tangent of 2^11 keeps both f16
    // halves normal through 2^-14, a signal of 1e-2 would lose its low half after 2^-8 (measured against float64: the first
    // layers' gradients 2x closer than with the factor on the signals, scripts/check_so_routes.py)
    StoreCtx scx, scy;
    float blimit = F16_MAX;
    if constexpr (PLANES) {
        char* const plx = A.x2_planes + ((long long)blockIdx.x * WAVES + wave) * PL2X_SB_BYTES;      // wave-uniform
        char* const ply = A.y2_planes + ((long long)blockIdx.x * WAVES + wave) * PL2Y_SB_BYTES;
        const int E = (int)((*A.jmax >> 23) & 0xffu);
        const int K2 = (E == 0 || E == 255) ? 0 : -(E - 127);
#pragma unroll
        for (int s = 0; s < S; ++s) {
            int d = K2 - k[s];
            d = d > 0 ? 0 : d;      // (K2 <= k_s by construction; a zero / non-finite J^ keeps k_s = 0 and has zero tangents)
            const _Float16 f = d < -24 ? (_Float16)0.f : (_Float16)ldexpf(1.f, d);
            scx.fac[s] = h2v{f, f};
            scy.fac[s] = h2v{(_Float16)(1 << PL_BOOST_LOG2), (_Float16)(1 << PL_BOOST_LOG2)};
        }
        scx.rsrc = plane_rsrc(plx); scx.rsrc_lo = scx.rsrc; scx.base = plx; scx.lane = 32 * m + 8 * g; scx.soff = 0;
        scy.rsrc = plane_rsrc(ply); scy.rsrc_lo = scy.rsrc; scy.base = ply; scy.lane = 32 * m + 8 * g; scy.soff = 0;
        blimit = F16_MAX / (float)(1 << PL_BOOST_LOG2);      // a boosted signal must stay inside f16: the range guard fires there
        // 2^boost as a 16-row block (row 0): the A operand of dw_sigma += sum_s a'_8[s]
        float b8[S][8];
#pragma unroll
        for (int s = 0; s < S; ++s) {
#pragma unroll
            for (int c = 0; c < 8; ++c) b8[s][c] = 0.f;
            if (g == 0) b8[s][0] = 1.f;
        }
        u32x4 bh[S][1], bl[S][1];
        to_b<8>(b8, bh, bl, st.sat);
        store_dy_planes<1, 1, 1>(scy, PL2Y_SIG, bh, bl);
    } else {
        save_scaled<16>(A.so + (long long)TA_ENC * A.B, 64, te, k, idx, valid, g);
    }
    prime_stream(st, lane16);
    // ---- tangent forward pass (no bias; ReLU replaced by the saved masks), two halves of 8 row blocks per layer
    u32x4 eh[S][2], el[S][2];
    split_b<16>(te, eh, el, st.sat);
    if constexpr (PLANES) store_dy_planes<2, 2, 2>(scx, TA_ENC / 16, eh, el);
    float t[S][64];
    u32x4 th[S][8], tl[S][8];
    // WEAVE2 (round 5, as in the first-order kernels): the 64 plane stores of a 256-wide section ride in the MFMA stream of the GEMM
    // that reads the same operands instead of going out in one burst; sections without such a GEMM behind them (the last tangent,
    // the signal of layer 1) keep the burst.
    constexpr bool WEAVE2 = PLANES;
    constexpr int SX0 = WEAVE2 ? 0 : -1, SX4 = WEAVE2 ? 4 : -1, SY0 = WEAVE2 ? 0 : -1;
    const auto at_x = [&](int layer, int T0) -> const StoreCtx& {      // operand T0 of tangent section `layer` (a'_(layer+1))
        scx.soff = (TA_H / 16 + 16 * layer + 2 * T0) * PL_FB_BYTES;
        return scx;
    };
    const auto at_y = [&](int fb) -> const StoreCtx& {
        scy.soff = fb * PL_FB_BYTES;
        return scy;
    };
    auto finish_layer = [&](const f32x4 (&a0)[S][8], const f32x4 (&a1)[S][8], int layer) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const uint64_t mk = lm[(layer * S + s) * WG_THREADS];
#pragma unroll
            for (int nb = 0; nb < 16; ++nb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = nb < 8 ? a0[s][nb & 7][r] : a1[s][nb & 7][r];
                    t[s][4 * nb + r] = ((mk >> (4 * nb + r)) & 1ull) ? v : 0.f;
                }
        }
        if constexpr (!PLANES) save_scaled<64>(A.so + (long long)(TA_H + 256 * layer) * A.B, 256, t, k, idx, valid, g);
        split_b<64>(t, th, tl, st.sat);
        if constexpr (PLANES) { if (!WEAVE2 || layer == 7) store_dy_planes<8, 2, 8>(scx, TA_H / 16 + 16 * layer, th, tl); }
    };
    {
        f32x4 a0[S][8], a1[S][8];
        zero_acc<8>(a0);
        gemm_part<2, 8, 0>(a0, eh, el, st, wave, lane16);
        zero_acc<8>(a1);
        gemm_part<2, 8, 16>(a1, eh, el, st, wave, lane16);
        finish_layer(a0, a1, 0);
#pragma unroll 1
        for (int l = 0; l < 3; ++l) {      // (th / tl hold a'_(l+1), section l: stored by the two halves that read it)
            zero_acc<8>(a0);
            gemm_part<8, 8, 32, 0, SX0, 4, true>(a0, th, tl, st, wave, lane16, at_x(l, 0));
            zero_acc<8>(a1);
            gemm_part<8, 8, 96, 0, SX4, 4, true>(a1, th, tl, st, wave, lane16, at_x(l, 4));
            finish_layer(a0, a1, 1 + l);
        }
        zero_acc<8>(a0);
        gemm_part<2, 8, 416>(a0, eh, el, st, wave, lane16);
        gemm_part<8, 8, 432, 0, SX0, 4, true>(a0, th, tl, st, wave, lane16, at_x(3, 0));
        zero_acc<8>(a1);
        gemm_part<2, 8, 496>(a1, eh, el, st, wave, lane16);
        gemm_part<8, 8, 512, 0, SX4, 4, true>(a1, th, tl, st, wave, lane16, at_x(3, 4));
        finish_layer(a0, a1, 4);
#pragma unroll 1
        for (int l = 0; l < 3; ++l) {
            zero_acc<8>(a0);
            gemm_part<8, 8, 576, 0, SX0, 4, true>(a0, th, tl, st, wave, lane16, at_x(4 + l, 0));
            zero_acc<8>(a1);
            gemm_part<8, 8, 640, 0, SX4, 4, true>(a1, th, tl, st, wave, lane16, at_x(4 + l, 4));
            finish_layer(a0, a1, 5 + l);
        }
    }
    // ---- density-gradient signals b_8..b_1 (as in the GRAD pass of the forward kernel)
    open_stream<false>(st, A.packed + OFF_SPLIT_BWD, wave, lane);
    prime_stream(st, lane16);
    float gr[S][64];
    {
        const f32x4* ws = (const f32x4*)(smem + LDS_RING + 8 * S * WG_THREADS * 8);
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
        for (int q = 0; q < 16; ++q) genc[s][q] = 0.f;
#pragma unroll 1
    for (int layer = 7; layer >= 0; --layer) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const uint64_t mk = lm[(layer * S + s) * WG_THREADS];
#pragma unroll
            for (int q = 0; q < 64; ++q) gr[s][q] = ((mk >> q) & 1ull) ? gr[s][q] : 0.f;
        }
        if constexpr (!PLANES) save_bform<64>(A.so + (long long)(BS_L + 256 * layer) * A.B, 256, gr, idx, valid, g);
        u32x4 gh[S][8], gl[S][8];
        split_b<64>(gr, gh, gl, st.sat, blimit);
        if constexpr (PLANES) { if (!WEAVE2 || layer == 0) store_dy_planes<8, 2, 8>(scy, 16 * layer, gh, gl); }
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
            gemm_part<8, 16, 0, 0, SY0, 8, true>(acc, gh, gl, st, wave, lane16, at_y(16 * layer));
            acc_out(gr, acc);
        }
    }
    // ---- dL/dx += diag-Hessian of the encoding (contracted with g_enc) times J^
    if (A.d_xyz) {
#pragma unroll
        for (int s = 0; s < S; ++s) {
            float d0 = 0.f, d1 = 0.f, d2 = 0.f;
#pragma unroll
            for (int pp = 0; pp < 8; ++pp) {
                const int P = 8 * g + pp;
                const int f = P / 3;
                const int a = P - 3 * f;
                if (P < 30) {
                    const float xa = a == 0 ? x[s][0] : (a == 1 ? x[s][1] : x[s][2]);
                    float sn, cs;
                    fast_sincos(ldexpf(xa, f), sn, cs);
                    const float c = -ldexpf(genc[s][2 * pp] * sn + genc[s][2 * pp + 1] * cs, 2 * f);
                    d0 += a == 0 ? c : 0.f;
                    d1 += a == 1 ? c : 0.f;
                    d2 += a == 2 ? c : 0.f;
                }
            }
            d0 += __shfl_xor(d0, 16); d1 += __shfl_xor(d1, 16); d2 += __shfl_xor(d2, 16);
            d0 += __shfl_xor(d0, 32); d1 += __shfl_xor(d1, 32); d2 += __shfl_xor(d2, 32);
            if (g == 0 && valid[s]) {
                float* o = A.d_xyz + (long long)idx[s] * 3;
                o[0] += d0 * jh[s][0]; o[1] += d1 * jh[s][1]; o[2] += d2 * jh[s][2];
            }
        }
    }
    guard_report(A.packed, st.sat, 0ull, MNRF_GUARD_IN_SECOND_ORDER);   // a scaled tangent / signal left the f16 range
    close_stream();
}

inline int launch_bwd2(const FieldBwd2Args& A, hipStream_t s) {
    const long long blocks64 = (A.B + WG_SAMPLES - 1) / WG_SAMPLES;
    if (blocks64 > 0x7fffffff || A.B > 0x7fffffffLL) return -1;
    constexpr int LDS_BWD2 = LDS_RING + 8 * S * WG_THREADS * 8 + 1024;      // ring | relu masks | w_sigma
    if (A.x2_planes) hipLaunchKernelGGL(field_split_bwd2_kernel<true>, dim3((unsigned)blocks64), dim3(WG_THREADS), LDS_BWD2, s, A);
    else hipLaunchKernelGGL(field_split_bwd2_kernel<false>, dim3((unsigned)blocks64), dim3(WG_THREADS), LDS_BWD2, s, A);
    return 0;
}
