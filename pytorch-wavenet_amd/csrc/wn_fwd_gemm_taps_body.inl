// wn_fwd_gemm_taps_body.inl -- the body of wn_fwd_gemm_taps<TAPS> and wn_fwd_gemm_taps_ragged<TAPS> (included inside both kernels by wn_forward.h, like
// wn_fwd_gemm_body.inl).  In scope: ta (WnTapsArgs), RAGGED (constexpr bool), rg (WnRagged; only read where RAGGED: t_min is then the zero prefix in
// front of a stream's time 0).
    static_assert(TAPS == 3 || TAPS == 4, "kernel_size 3 and 4 (2 is wn_fwd_gemm's two-view form)");
    const WnGemmArgs& g = ta.g;
    constexpr int TM = 128, TN = 128, KC = WN_GEMM_KC, AP = TM + 1;
    constexpr int NQ = KC / 8;
    constexpr int BT = 256 / KC;
    __shared__ __attribute__((aligned(16))) float smem_f[2 * KC * AP + 2 * KC * TN + (2 * KC * AP) % 4];
    static_assert(2 * KC * AP + 2 * KC * TN >= 4 * WN_EPI_TILE_FLOATS, "the operand buffers hold the four waves' staging tiles");
    float (*a_t)[KC * AP] = reinterpret_cast<float (*)[KC * AP]>(smem_f);                                        // [2][k][row]
    float (*b_s)[KC * TN] = reinterpret_cast<float (*)[KC * TN]>(smem_f + ((2 * KC * AP + 3) & ~3));               // [2][k][col]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const unsigned mtiles = (unsigned)((g.M + TM - 1) / TM), tm_i = blockIdx.x % mtiles, tn_i = blockIdx.x / mtiles;  // row tiles fastest
    const long long m0 = (long long)tm_i * TM;
    const int n0 = (int)tn_i * TN;
    wn_f16v acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[j][i] = 0.f;

    // loader roles as in wn_fwd_gemm: A chunk = 128 rows x KC floats, two threads per row; B chunk = KC x 128
    const int arow = tid >> 1, ahalf = tid & 1;
    const long long am = m0 + arow;
    const bool arow_ok = am < g.M;
    unsigned rq = 0u, rr = 0u;
    uint2* rmap = nullptr;
    if constexpr (RAGGED) {
        __shared__ uint2 rmap_s[TM];   // (stream, time) of the tile's rows, for the epilogue
        rmap = rmap_s;
        if (arow_ok) wn_ragged_row(rg, (unsigned)am, rq, rr);
        if (!ahalf) rmap[arow] = make_uint2(rq, rr);
    }
    const unsigned aq = RAGGED ? rq : (arow_ok ? (unsigned)am / (unsigned)g.rows_per_batch : 0u), arem = RAGGED ? rr : (arow_ok ? (unsigned)am - aq * (unsigned)g.rows_per_batch : 0u);
    const float* a1p = wn_row_at(g.a1, aq, arem) + ahalf * (KC / 2);   // the row of x(t)
    const long long tap_fl = ta.tap_rows * g.a1.row_stride;              // floats between two neighbouring taps
    const long long t_row = g.a1.t0 + (long long)arem;                    // the row's time inside its batch entry
    unsigned okmask = 0;                                                 // bit j: view j of this row exists
#pragma unroll
    for (int j = 0; j < TAPS; ++j) okmask |= (arow_ok && t_row - (TAPS - 1 - j) * ta.tap_rows >= ta.t_min) ? (1u << j) : 0u;
    const int brow = tid / BT, bcol = (tid % BT) * (KC / 2);
    const float* bp = g.bt + (size_t)brow * g.N + n0 + bcol;
    const bool okb = n0 + bcol < g.N;   // (one predicate for the thread's NQ loads: see wn_fwd_gemm)

    float4 va[NQ], vb[NQ];
    int f_tap = 0, f_off = 0;   // the view and the column inside it of the next chunk to fetch
    auto fetch = [&]() {
        const bool ok = (okmask >> f_tap) & 1u;
        const float* src = a1p - (long long)(TAPS - 1 - f_tap) * tap_fl + f_off;
#pragma unroll
        for (int q = 0; q < NQ; ++q) va[q] = ok ? *reinterpret_cast<const float4*>(src + q * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int q = 0; q < NQ; ++q) vb[q] = okb ? *reinterpret_cast<const float4*>(bp + q * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        bp += (size_t)KC * g.N;
        f_off += KC;
        if (f_off == g.k_split) { f_off = 0; ++f_tap; }
    };
    auto stash = [&](int buf) {  // registers -> LDS (A transposed to [k][row])
        float* at = a_t[buf];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const float4 x = va[q];
            const int k = ahalf * (KC / 2) + q * 4;
            at[(k + 0) * AP + arow] = x.x; at[(k + 1) * AP + arow] = x.y; at[(k + 2) * AP + arow] = x.z; at[(k + 3) * AP + arow] = x.w;
        }
        float* bs = b_s[buf] + brow * TN + bcol;
#pragma unroll
        for (int q = 0; q < NQ; ++q) *reinterpret_cast<float4*>(bs + q * 4) = vb[q];
    };

    const int nchunks = TAPS * (g.k_split / KC);
    fetch();
    stash(0);
    __syncthreads();
    for (int kc = 0; kc < nchunks; ++kc) {
        const int buf = kc & 1;
        if (kc + 1 < nchunks) fetch();  // lands while this chunk is multiplied
        const float* at = a_t[buf] + 32 * wv + (lane & 31);
        const float* bs = b_s[buf] + (lane & 31);
        const int kh = lane >> 5;
#pragma unroll
        for (int ks = 0; ks < KC / 2; ++ks) {
            const float a = at[(2 * ks + kh) * AP];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float b = bs[(2 * ks + kh) * TN + 32 * j];
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[j], 0, 0, 0);
            }
        }
        if (kc + 1 < nchunks) stash(buf ^ 1);
        __syncthreads();
    }

    wn_gemm_epilogue<WN_EPI_GATE, 4, false, RAGGED>(g, acc, m0 + 32 * wv, n0, lane, smem_f + wv * WN_EPI_TILE_FLOATS, nullptr, 0, rmap + 32 * wv);   // (the loop's last barrier: nobody reads the operand buffers any more)
