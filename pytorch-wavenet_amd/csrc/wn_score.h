// wn_score.h -- teacher-forced scoring (wn_score): the head of the forward and the row statistics of its logits in ONE kernel (gfx950, device only).
//
// Reference: WavenetTrainer.validate() (wavenet_training.py:89-112): output = model(x); F.cross_entropy(output, target); torch.max(output, 1);
// torch.eq / torch.sum.  wn_forward's head is two products and leaves ev = relu(relu(skip).W1 + b1) [M][E] and the logits [M][256] in HBM;
// scoring needs neither -- per row it needs logsumexp(logits) - logits[target] and the first index of the maximum.
//
// wn_score_head: a workgroup (4 waves) owns 128 rows and all 256 classes; wave w owns rows 32w..32w+31 in BOTH products.  It walks the end
// channels in chunks of WN_SCORE_EC = 64:
//     h      = relu(relu(skip_tile) . W1[:, chunk] + b1[chunk])     K = S, operands streamed through LDS in K pieces (the loaders of wn_fwd_gemm*);
//                                                                    2 accumulator tiles per wave
//     logits += h . W2[chunk, :]                                     K = 64; h goes from the accumulators to an LDS image (fp32 operands: [k][row]
//                                                                    fp32; bf16 operands: [row][k] bf16, rounded to nearest even as wn_fwd_gemm_bf16
//                                                                    rounds ev while staging it) that only the wave that wrote it reads; W2 streams
//                                                                    through LDS; 8 accumulator tiles per wave (128 registers) live across all chunks
// The epilogue adds b2 and reduces, per row, over the 8 tiles of a lane and the 32 lanes that hold the row: maximum with its FIRST index, sum of
// exp(x - max), the target's logit.  Out go 4 bytes of row_nll and 4 of row_pred per row (both optional) and one {sum nll, hits, rows} fp64 partial
// per workgroup, summed in a fixed order; wn_score_reduce folds the partials in a fixed order too: the sums are bit-reproducible.
// Budget: 160 accumulator registers + staging, 2 workgroups per CU (launch bound 256 registers); LDS 65.8 KB (fp32) / 59.4 KB (bf16) per workgroup.
// The skip tile is re-read once per chunk (E / 64 times; the second and later reads are served by the caches), ev and the logits never leave the CU.
//
// Measured at config 5's evaluation batch (profiles/r07_score.txt): with fp32 operands the fused kernel is level with or ahead of the unfused path, with bf16
// operands -- where the head is bound by its reads, not by the matrix cores -- the re-reads cost more than ev and the logits did: the host picks it for fp32 only.
//
// wn_score_rows: the same statistics from logits in HBM (any class count): bf16 operands, the shapes the fused kernel is not written for, A/B runs.
#ifndef WN_SCORE_H
#define WN_SCORE_H

#include "wn_forward.h"

#define WN_SCORE_EC 64    // end channels per chunk
#define WN_SCORE_TM 128   // rows per workgroup

struct WnScoreArgs {
    const float* skip;            // [M][S] fp32 (the finished skip sum, before its ReLU)
    long long M;
    int S, E;
    const float* w1t;             // fp32 operands: end_conv_1 as B^T [S][E]
    const float* w2t;             //                end_conv_2 as B^T [E][256]
    const unsigned short* w1h;    // bf16 operands: end_conv_1 [E][S]
    const unsigned short* w2h;    //                end_conv_2 [256][E]
    const float* b1;              // [E]
    const float* b2;              // [256]
    const long long* targets;     // [M]
    float* row_nll;               // [M] or NULL
    int* row_pred;                // [M] or NULL
    double* part;                 // [workgroups][3]
};

// Per-row statistics of a wave's 32 x 256 logits strip in the MFMA C layout (tile j: class 32 j + (lane & 31); element i: row (i & 3) + 8 (i >> 2) +
// 4 (lane >> 5)).  tot: {sum nll, hits, rows} of the rows this lane reports (lanes with (lane & 31) == 0 report).
static __device__ __forceinline__ void wn_score_strip(const wn_f16v (&acc)[8], const float* b2, const long long* targets, long long mw, long long M, int lane,
                                                      float* row_nll, int* row_pred, double (&tot)[3]) {
    const int col = lane & 31;
    float bias[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) bias[j] = b2[32 * j + col];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const long long m = mw + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
        const bool row_ok = m < M;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = acc[j][i] + bias[j];
        float mx = v[0];
        int arg = col;
#pragma unroll
        for (int j = 1; j < 8; ++j)
            if (v[j] > mx) { mx = v[j]; arg = 32 * j + col; }   // (ascending classes, strict: the first index of the maximum)
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
            const float om = __shfl_xor(mx, o);
            const int oa = __shfl_xor(arg, o);
            if (om > mx || (om == mx && oa < arg)) { mx = om; arg = oa; }
        }
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) sum += expf(v[j] - mx);
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        const long long t = row_ok ? targets[m] : -1;
        const bool valid = t >= 0 && t < 256;
        const int tj = (int)(t >> 5);
        float xt = 0.f;
        if (valid && (int)(t & 31) == col) {
#pragma unroll
            for (int j = 0; j < 8; ++j) xt = tj == j ? v[j] : xt;
        }
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) xt += __shfl_xor(xt, o);
        if (col == 0 && row_ok) {
            const float nll = (mx + logf(sum)) - xt;
            if (row_nll) row_nll[m] = valid ? nll : __uint_as_float(0x7fc00000u);
            if (row_pred) row_pred[m] = arg;
            if (valid) { tot[0] += (double)nll; tot[1] += (long long)arg == t ? 1. : 0.; tot[2] += 1.; }
        }
    }
}

// The workgroup's partial: the 8 reporting lanes' totals (wave order, lower half first) added in order by thread 0.
static __device__ __forceinline__ void wn_score_partial(const double (&tot)[3], double* lds, double* part) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if ((lane & 31) == 0) {
        double* d = lds + (2 * wv + (lane >> 5)) * 3;
        d[0] = tot[0]; d[1] = tot[1]; d[2] = tot[2];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s0 = 0., s1 = 0., s2 = 0.;
        for (int k = 0; k < 8; ++k) { s0 += lds[3 * k]; s1 += lds[3 * k + 1]; s2 += lds[3 * k + 2]; }
        double* p = part + (size_t)blockIdx.x * 3;
        p[0] = s0; p[1] = s1; p[2] = s2;
    }
}

// ---- fp32 operands (v_mfma_f32_32x32x2_f32)
__global__ __launch_bounds__(256, 2) void wn_score_head(WnScoreArgs g) {
    constexpr int TM = WN_SCORE_TM, EC = WN_SCORE_EC, KC = 16, AP = TM + 1;
    constexpr int ST = 2 * KC * 256;   // staging floats: product 2's two W2 pieces (product 1's A and W1 pieces are smaller)
    static_assert(2 * KC * AP + 2 * KC * EC <= ST, "product 1's operand buffers fit the staging block");
    __shared__ __attribute__((aligned(16))) float smem_f[ST + EC * AP];
    float* a_t = smem_f;                       // [2][KC][AP]   A piece, transposed
    float* b_s = smem_f + 2 * KC * AP;         // [2][KC][EC]   W1 piece
    float* w_s = smem_f;                       // [2][KC][256]  W2 piece (product 2)
    float* h_t = smem_f + ST;                  // [EC][AP]      h chunk, transposed; column block 32 w belongs to wave w
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, kh = lane >> 5;
    const long long m0 = (long long)blockIdx.x * TM;
    wn_f16v lacc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) lacc[j][i] = 0.f;
    // loader roles.  A piece: 128 rows x 16 floats, two threads per row;  W1 piece: 16 x 64, one float4 each;  W2 piece: 16 x 256, four float4 each
    const int arow = tid >> 1, ahalf = tid & 1;
    const bool arow_ok = m0 + arow < g.M;
    const float* ap = g.skip + (arow_ok ? (m0 + arow) * (long long)g.S : 0) + ahalf * 8;
    const int brow = tid >> 4, bcol = (tid & 15) * 4, wcol = (tid & 15) * 16;
    const int n1 = g.S / KC;

    for (int e0 = 0; e0 < g.E; e0 += EC) {
        wn_f16v hacc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) hacc[j][i] = 0.f;
        float4 va0, va1, vb;
        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
        auto fetch1 = [&](int kc) {
            const int k0 = kc * KC;
            va0 = arow_ok ? *reinterpret_cast<const float4*>(ap + k0) : zero4;
            va1 = arow_ok ? *reinterpret_cast<const float4*>(ap + k0 + 4) : zero4;
            vb = *reinterpret_cast<const float4*>(g.w1t + (size_t)(k0 + brow) * g.E + e0 + bcol);
        };
        auto put4 = [&](float* at, int k, const float4 x) {
            at[(k + 0) * AP + arow] = fmaxf(x.x, 0.f); at[(k + 1) * AP + arow] = fmaxf(x.y, 0.f);
            at[(k + 2) * AP + arow] = fmaxf(x.z, 0.f); at[(k + 3) * AP + arow] = fmaxf(x.w, 0.f);
        };
        auto stash1 = [&](int buf) {
            float* at = a_t + buf * KC * AP;
            put4(at, ahalf * 8, va0);
            put4(at, ahalf * 8 + 4, va1);
            *reinterpret_cast<float4*>(b_s + buf * KC * EC + brow * EC + bcol) = vb;
        };
        fetch1(0);
        stash1(0);
        __syncthreads();
        for (int kc = 0; kc < n1; ++kc) {
            const int buf = kc & 1;
            if (kc + 1 < n1) fetch1(kc + 1);
            const float* at = a_t + buf * KC * AP + 32 * wv + l31;
            const float* bs = b_s + buf * KC * EC + l31;
#pragma unroll
            for (int ks = 0; ks < KC / 2; ++ks) {
                const float a = at[(2 * ks + kh) * AP];
#pragma unroll
                for (int j = 0; j < 2; ++j) hacc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bs[(2 * ks + kh) * EC + 32 * j], hacc[j], 0, 0, 0);
            }
            if (kc + 1 < n1) stash1(buf ^ 1);
            __syncthreads();
        }
        // h = relu(acc + b1) -> the wave's own columns of h_t (a wave's LDS operations execute in order: no barrier between this and product 2's reads)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float b = g.b1[e0 + 32 * j + l31];
            float* dst = h_t + (32 * j + l31) * AP + 32 * wv + 4 * kh;
#pragma unroll
            for (int i = 0; i < 16; ++i) dst[(i & 3) + 8 * (i >> 2)] = fmaxf(hacc[j][i] + b, 0.f);
        }
        float4 vw0, vw1, vw2, vw3;   // (named registers: an array captured by the lambdas is left in memory by the compiler)
        auto fetch2 = [&](int kc) {
            const float4* src = reinterpret_cast<const float4*>(g.w2t + (size_t)(e0 + kc * KC + brow) * 256 + wcol);
            vw0 = src[0]; vw1 = src[1]; vw2 = src[2]; vw3 = src[3];
        };
        auto stash2 = [&](int buf) {
            float4* dst = reinterpret_cast<float4*>(w_s + buf * KC * 256 + brow * 256 + wcol);
            dst[0] = vw0; dst[1] = vw1; dst[2] = vw2; dst[3] = vw3;
        };
        fetch2(0);
        stash2(0);   // (product 1's last barrier: nobody reads its operand buffers any more)
        __syncthreads();
        for (int kc = 0; kc < EC / KC; ++kc) {
            const int buf = kc & 1;
            if (kc + 1 < EC / KC) fetch2(kc + 1);
            const float* at = h_t + kc * KC * AP + 32 * wv + l31;
            const float* ws = w_s + buf * KC * 256 + l31;
#pragma unroll
            for (int ks = 0; ks < KC / 2; ++ks) {
                const float a = at[(2 * ks + kh) * AP];
#pragma unroll
                for (int j = 0; j < 8; ++j) lacc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, ws[(2 * ks + kh) * 256 + 32 * j], lacc[j], 0, 0, 0);
            }
            if (kc + 1 < EC / KC) stash2(buf ^ 1);
            __syncthreads();
        }
    }
    double tot[3] = {0., 0., 0.};
    wn_score_strip(lacc, g.b2, g.targets, m0 + 32 * wv, g.M, lane, g.row_nll, g.row_pred, tot);
    wn_score_partial(tot, reinterpret_cast<double*>(smem_f), g.part);   // (after the last barrier of the loops)
}

// ---- bf16 operands (v_mfma_f32_32x32x16_bf16, fp32 accumulation): the rounding points of wn_fwd_gemm_bf16 -- relu(skip) and h are rounded to
// nearest even where they become operands, the weights are the pre-converted banks, biases and accumulators stay fp32.
__global__ __launch_bounds__(256, 2) void wn_score_head_bf16(WnScoreArgs g) {
    constexpr int TM = WN_SCORE_TM, EC = WN_SCORE_EC, KC = 32, LD = KC + 8, HL = EC + 8;
    constexpr int ST = 2 * 256 * LD;   // staging bf16: product 2's two W2 pieces
    static_assert(2 * TM * LD + 2 * EC * LD <= ST, "product 1's operand buffers fit the staging block");
    __shared__ __attribute__((aligned(16))) unsigned short smem_h[ST + TM * HL];
    unsigned short* a_s = smem_h;                  // [2][TM][LD]
    unsigned short* b_s = smem_h + 2 * TM * LD;    // [2][EC][LD]
    unsigned short* w_s = smem_h;                  // [2][256][LD]
    unsigned short* h_s = smem_h + ST;             // [TM][HL]   rows 32 w.. belong to wave w
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l31 = lane & 31, kh = lane >> 5;
    const long long m0 = (long long)blockIdx.x * TM;
    wn_f16v lacc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) lacc[j][i] = 0.f;
    // loader roles.  A piece: 128 rows x 32 floats, two threads per row;  W1 piece: 64 channels x 32 bf16, one uint4 each;  W2 piece: 256 classes x 32 bf16
    const int arow = tid >> 1, ahalf = tid & 1;
    const bool arow_ok = m0 + arow < g.M;
    const float* ap = g.skip + (arow_ok ? (m0 + arow) * (long long)g.S : 0) + ahalf * 16;
    const int bch = tid >> 2, bq = tid & 3;
    const int n1 = g.S / KC;

    for (int e0 = 0; e0 < g.E; e0 += EC) {
        wn_f16v hacc[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) hacc[j][i] = 0.f;
        float4 va0, va1, va2, va3;
        uint4 vb;
        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
        auto fetch1 = [&](int kc) {
            const float4* src = reinterpret_cast<const float4*>(ap + kc * KC);
            va0 = arow_ok ? src[0] : zero4; va1 = arow_ok ? src[1] : zero4; va2 = arow_ok ? src[2] : zero4; va3 = arow_ok ? src[3] : zero4;
            vb = *reinterpret_cast<const uint4*>(g.w1h + (size_t)(e0 + bch) * g.S + kc * KC + bq * 8);
        };
        auto relu8 = [](float4 x, float4 y) {
            x.x = fmaxf(x.x, 0.f); x.y = fmaxf(x.y, 0.f); x.z = fmaxf(x.z, 0.f); x.w = fmaxf(x.w, 0.f);
            y.x = fmaxf(y.x, 0.f); y.y = fmaxf(y.y, 0.f); y.z = fmaxf(y.z, 0.f); y.w = fmaxf(y.w, 0.f);
            return wn_pack_bf16x8(x, y);
        };
        auto stash1 = [&](int buf) {
            uint4* ad = reinterpret_cast<uint4*>(a_s + buf * TM * LD + arow * LD + ahalf * 16);
            ad[0] = relu8(va0, va1);
            ad[1] = relu8(va2, va3);
            *reinterpret_cast<uint4*>(b_s + buf * EC * LD + bch * LD + bq * 8) = vb;
        };
        fetch1(0);
        stash1(0);
        __syncthreads();
        for (int kc = 0; kc < n1; ++kc) {
            const int buf = kc & 1;
            if (kc + 1 < n1) fetch1(kc + 1);
            const unsigned short* ar = a_s + buf * TM * LD + (32 * wv + l31) * LD + 8 * kh;
            const unsigned short* br = b_s + buf * EC * LD + l31 * LD + 8 * kh;
#pragma unroll
            for (int ks = 0; ks < KC / 16; ++ks) {
                const wn_bf16x8 a = *reinterpret_cast<const wn_bf16x8*>(ar + 16 * ks);
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    hacc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, *reinterpret_cast<const wn_bf16x8*>(br + 32 * j * LD + 16 * ks), hacc[j], 0, 0, 0);
            }
            if (kc + 1 < n1) stash1(buf ^ 1);
            __syncthreads();
        }
        // h = relu(acc + b1), rounded to bf16 -> the wave's own rows of h_s (in-order LDS: no barrier before product 2 reads them)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float b = g.b1[e0 + 32 * j + l31];
            unsigned short* dst = h_s + (32 * wv + 4 * kh) * HL + 32 * j + l31;
#pragma unroll
            for (int i = 0; i < 16; ++i) dst[((i & 3) + 8 * (i >> 2)) * HL] = (unsigned short)(wn_pack_bf16(fmaxf(hacc[j][i] + b, 0.f), 0.f) & 0xffffu);
        }
        uint4 vw0, vw1, vw2, vw3;   // (named registers: an array captured by the lambdas is left in memory by the compiler)
        auto fetch2 = [&](int kp) {
            const uint4* src = reinterpret_cast<const uint4*>(g.w2h + (size_t)tid * g.E + e0 + kp * KC);
            vw0 = src[0]; vw1 = src[1]; vw2 = src[2]; vw3 = src[3];
        };
        auto stash2 = [&](int buf) {
            uint4* dst = reinterpret_cast<uint4*>(w_s + buf * 256 * LD + tid * LD);
            dst[0] = vw0; dst[1] = vw1; dst[2] = vw2; dst[3] = vw3;
        };
        fetch2(0);
        stash2(0);   // (product 1's last barrier: nobody reads its operand buffers any more)
        __syncthreads();
        for (int kp = 0; kp < EC / KC; ++kp) {
            const int buf = kp & 1;
            if (kp + 1 < EC / KC) fetch2(kp + 1);
            const unsigned short* ar = h_s + (32 * wv + l31) * HL + kp * KC + 8 * kh;
            const unsigned short* wr = w_s + buf * 256 * LD + l31 * LD + 8 * kh;
#pragma unroll
            for (int ks = 0; ks < KC / 16; ++ks) {
                const wn_bf16x8 a = *reinterpret_cast<const wn_bf16x8*>(ar + 16 * ks);
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    lacc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, *reinterpret_cast<const wn_bf16x8*>(wr + 32 * j * LD + 16 * ks), lacc[j], 0, 0, 0);
            }
            if (kp + 1 < EC / KC) stash2(buf ^ 1);
            __syncthreads();
        }
    }
    double tot[3] = {0., 0., 0.};
    wn_score_strip(lacc, g.b2, g.targets, m0 + 32 * wv, g.M, lane, g.row_nll, g.row_pred, tot);
    wn_score_partial(tot, reinterpret_cast<double*>(smem_h), g.part);   // (after the last barrier of the loops)
}

// ---- The same statistics from logits [M][C] in HBM (any C): one wave per row, 8 rows per wave, 32 rows per workgroup; sibling of wn_xent_rows
// with the first-index argmax added.  part[blockIdx] = {sum nll, hits, rows} of the workgroup's rows, added in row order.
#define WN_SCORE_ROWS_PER_WG 32
__global__ __launch_bounds__(256) void wn_score_rows(const float* logits, int C, const long long* targets, long long M, float* row_nll, int* row_pred, double* part) {
    __shared__ double lds[4 * 3];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double tot[3] = {0., 0., 0.};
    for (int r = 0; r < WN_SCORE_ROWS_PER_WG / 4; ++r) {
        const long long m = (long long)blockIdx.x * WN_SCORE_ROWS_PER_WG + wv * (WN_SCORE_ROWS_PER_WG / 4) + r;
        if (m >= M) break;   // (wave-uniform)
        const float* x = logits + m * C;
        float mx = -INFINITY;
        int arg = 0x7fffffff;
        for (int c = lane; c < C; c += 64) {
            const float v = x[c];
            if (v > mx || arg == 0x7fffffff) { mx = v; arg = c; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float om = __shfl_xor(mx, o);
            const int oa = __shfl_xor(arg, o);
            if (om > mx || (om == mx && oa < arg)) { mx = om; arg = oa; }
        }
        float sum = 0.f;
        for (int c = lane; c < C; c += 64) sum += expf(x[c] - mx);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        const long long t = targets[m];
        const bool valid = t >= 0 && t < C;
        if (lane == 0) {
            const float nll = valid ? (mx + logf(sum)) - x[t] : __uint_as_float(0x7fc00000u);
            if (row_nll) row_nll[m] = nll;
            if (row_pred) row_pred[m] = arg;
            if (valid) { tot[0] += (double)nll; tot[1] += (long long)arg == t ? 1. : 0.; tot[2] += 1.; }
        }
    }
    if (lane == 0) { lds[3 * wv] = tot[0]; lds[3 * wv + 1] = tot[1]; lds[3 * wv + 2] = tot[2]; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s0 = 0., s1 = 0., s2 = 0.;
        for (int k = 0; k < 4; ++k) { s0 += lds[3 * k]; s1 += lds[3 * k + 1]; s2 += lds[3 * k + 2]; }
        double* p = part + (size_t)blockIdx.x * 3;
        p[0] = s0; p[1] = s1; p[2] = s2;
    }
}

// sums[0..2] = the partials added in a fixed order, fp64 (one workgroup: thread-strided sums, then a tree -- as wn_xent_reduce)
__global__ __launch_bounds__(1024) void wn_score_reduce(const double* part, long long n, double* sums) {
    __shared__ double red[3][1024];
    double s0 = 0., s1 = 0., s2 = 0.;
    for (long long i = threadIdx.x; i < n; i += 1024) { s0 += part[3 * i]; s1 += part[3 * i + 1]; s2 += part[3 * i + 2]; }
    red[0][threadIdx.x] = s0; red[1][threadIdx.x] = s1; red[2][threadIdx.x] = s2;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            red[0][threadIdx.x] += red[0][threadIdx.x + o]; red[1][threadIdx.x] += red[1][threadIdx.x + o]; red[2][threadIdx.x] += red[2][threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { sums[0] = red[0][0]; sums[1] = red[1][0]; sums[2] = red[2][0]; }
}

#endif  // WN_SCORE_H
