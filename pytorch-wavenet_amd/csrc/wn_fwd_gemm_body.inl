// wn_fwd_gemm_body.inl -- the body of wn_fwd_gemm<EPI> and wn_fwd_gemm_ragged<EPI> (wn_forward.h includes it inside both kernels: ONE text, and the
// kernel that existed first keeps its code object, which a shared device function did not give it).  In scope: g (WnGemmArgs), RAGGED (constexpr bool),
// rg (WnRagged; only read where RAGGED).
    constexpr int TM = 128, TN = 128, KC = WN_GEMM_KC, AP = TM + 1;  // AP: padded row length of the transposed A chunk
    constexpr int NQ = KC / 8;          // float4 per thread per operand and chunk
    constexpr int BT = 256 / KC;        // threads per B row
    // (ONE block: the epilogue re-uses it as the waves' staging tiles once the K loop is done)
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

    // loader roles: A chunk = 128 rows x 32 floats: thread -> row tid/2, 16 floats (4 float4) ; B chunk = 32 x 128: 4 float4 each
    const int arow = tid >> 1, ahalf = tid & 1;
    const long long am = m0 + arow;
    const bool arow_ok = am < g.M;
    unsigned rq = 0u, rr = 0u;
    uint2* rmap = nullptr;
    if constexpr (RAGGED) {
        __shared__ uint2 rmap_s[TM];   // (stream, time) of the tile's rows: written here, read by the epilogue (the K loop's barriers lie between)
        rmap = rmap_s;
        if (arow_ok) wn_ragged_row(rg, (unsigned)am, rq, rr);
        if (!ahalf) rmap[arow] = make_uint2(rq, rr);
    }
    const unsigned aq = RAGGED ? rq : (arow_ok ? (unsigned)am / (unsigned)g.rows_per_batch : 0u), arem = RAGGED ? rr : (arow_ok ? (unsigned)am - aq * (unsigned)g.rows_per_batch : 0u);
    const bool ok0 = RAGGED ? arow_ok : (arow_ok && (int)arem >= g.a_skip_lo[0] && (int)arem < g.rows_per_batch - g.a_skip_hi[0]);
    const bool ok1 = RAGGED ? arow_ok : (arow_ok && (int)arem >= g.a_skip_lo[1] && (int)arem < g.rows_per_batch - g.a_skip_hi[1]);
    const float* a0p = wn_row_at(g.a0, aq, arem);
    const float* a1p = wn_row_at(g.a1, aq, arem);
    const int brow = tid / BT, bcol = (tid % BT) * (KC / 2);

    float4 va[NQ], vb[NQ];  // staging registers of the chunk in flight
    auto fetch = [&](int kc) {  // global -> registers (issued before the multiply of the current chunk)
        const int k0 = kc * KC;
        const bool first = k0 < g.k_split, ok = first ? ok0 : ok1;
        const float* src = first ? a0p + k0 : a1p + (k0 - g.k_split);
#pragma unroll
        for (int q = 0; q < NQ; ++q) va[q] = ok ? *reinterpret_cast<const float4*>(src + ahalf * (KC / 2) + q * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        const float* bsrc = ((first || !g.bt1) ? g.bt + (size_t)(k0 + brow) * g.N : g.bt1 + (size_t)(k0 - g.k_split + brow) * g.N) + n0 + bcol;
        // (ONE predicate for the thread's NQ loads -- N % 32 == 0 and bcol is a multiple of KC / 2 = 4 NQ floats, so they are in range together: with a
        //  predicate per load each one sat in a block of its own with a full wait behind it.  Round 6, profiles/r06_tn_loads.txt.)
        const bool okb = n0 + bcol < g.N;
#pragma unroll
        for (int q = 0; q < NQ; ++q) vb[q] = okb ? *reinterpret_cast<const float4*>(bsrc + q * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    auto stash = [&](int buf) {  // registers -> LDS (A transposed to [k][row])
        float* at = a_t[buf];
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            float4 x = va[q];
            if (g.relu_a) { x.x = fmaxf(x.x, 0.f); x.y = fmaxf(x.y, 0.f); x.z = fmaxf(x.z, 0.f); x.w = fmaxf(x.w, 0.f); }
            const int k = ahalf * (KC / 2) + q * 4;
            at[(k + 0) * AP + arow] = x.x; at[(k + 1) * AP + arow] = x.y; at[(k + 2) * AP + arow] = x.z; at[(k + 3) * AP + arow] = x.w;
        }
        float* bs = b_s[buf] + brow * TN + bcol;
#pragma unroll
        for (int q = 0; q < NQ; ++q) *reinterpret_cast<float4*>(bs + q * 4) = vb[q];
    };

    const int nchunks = g.K / KC;
    fetch(0);
    stash(0);
    __syncthreads();
    for (int kc = 0; kc < nchunks; ++kc) {
        const int buf = kc & 1;
        if (kc + 1 < nchunks) fetch(kc + 1);  // lands while this chunk is multiplied
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

    wn_gemm_epilogue<EPI, 4, false, RAGGED>(g, acc, m0 + 32 * wv, n0, lane, smem_f + wv * WN_EPI_TILE_FLOATS, nullptr, 0, rmap + 32 * wv);   // (the loop's last barrier: nobody reads the operand buffers any more)
