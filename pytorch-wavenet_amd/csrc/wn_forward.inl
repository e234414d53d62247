// wn_forward.inl -- host side of the batched forward (included by wn_runtime.hip; GPU build only): the launchers of the matrix products of
// wn_forward.h, wn_forward / wn_score (WaveNetModel.forward() for one-hot inputs), wn_prime (batched priming of the generation queues).
#include <assert.h>

// One "NN" product C = A . B^T of wn_forward.h.  bn != NULL: bf16 operands (B given as [N][K] bf16 -- or as two [N][ldb] halves
// bn / bn1 --, A rounded while staged), fp32 accumulation; else fp32 operands.  Products with N % 256 == 0 take the 128 x 256 tile.
// rg != NULL: the same tiles under the ragged row map (wn_forward.h: WnRagged; a.M = the table's total, a.rows_per_batch unused) -- kernels that exist
// for fp32 operands and the GATE / PLAIN epilogues only.
static void wn_launch_nn(hipStream_t st, int epi, const WnGemmArgs& a, const unsigned short* bn = nullptr, const unsigned short* bn1 = nullptr, int ldb = 0,
                         const WnRagged* rg = nullptr) {
    const bool wide = bn && a.N % 256 == 0 && epi != WN_EPI_GATE_BWD;
    const unsigned mt = (unsigned)((a.M + 127) / 128), nt = (unsigned)(wide ? a.N / 256 : (a.N + 127) / 128);
    const dim3 grid(mt * nt);   // 1-D (M / 128 can exceed a grid's y limit): row tiles fastest, then column tiles
    if (rg) {
        assert(!bn && (epi == WN_EPI_GATE || epi == WN_EPI_PLAIN));
        if (epi == WN_EPI_GATE) hipLaunchKernelGGL(wn_fwd_gemm_ragged<WN_EPI_GATE>, grid, dim3(256), 0, st, a, *rg);
        else hipLaunchKernelGGL(wn_fwd_gemm_ragged<WN_EPI_PLAIN>, grid, dim3(256), 0, st, a, *rg);
        return;
    }
    if (bn) {
        WnGemmArgsBf16 b;
        b.g = a; b.bn = bn; b.bn1 = bn1; b.ldb = ldb;
        if (wide) {
            if (epi == WN_EPI_GATE && a.a_bf16) hipLaunchKernelGGL((wn_fwd_gemm_bf16<WN_EPI_GATE, 8, true>), grid, dim3(512), 0, st, b);   // (bf16-stored A: the shadow of x)
            else if (epi == WN_EPI_GATE) hipLaunchKernelGGL((wn_fwd_gemm_bf16<WN_EPI_GATE, 8>), grid, dim3(512), 0, st, b);
            else if (a.a_bf16) hipLaunchKernelGGL((wn_fwd_gemm_bf16<WN_EPI_PLAIN, 8, true>), grid, dim3(512), 0, st, b);   // (bf16-stored A: the grouped skip product)
            else hipLaunchKernelGGL((wn_fwd_gemm_bf16<WN_EPI_PLAIN, 8>), grid, dim3(512), 0, st, b);
        } else {
            if (epi == WN_EPI_GATE) hipLaunchKernelGGL((wn_fwd_gemm_bf16<WN_EPI_GATE, 4>), grid, dim3(256), 0, st, b);   // (never with a bf16-stored A: wn_train_layout_ws)
            else if (epi == WN_EPI_GATE_BWD) hipLaunchKernelGGL((wn_fwd_gemm_bf16<WN_EPI_GATE_BWD, 4>), grid, dim3(256), 0, st, b);
            else if (a.a_bf16) hipLaunchKernelGGL((wn_fwd_gemm_bf16<WN_EPI_PLAIN, 4, true>), grid, dim3(256), 0, st, b);   // (bf16-stored A: the residual and dx products)
            else hipLaunchKernelGGL((wn_fwd_gemm_bf16<WN_EPI_PLAIN, 4>), grid, dim3(256), 0, st, b);
        }
        return;
    }
    if (epi == WN_EPI_GATE) hipLaunchKernelGGL(wn_fwd_gemm<WN_EPI_GATE>, grid, dim3(256), 0, st, a);
    else if (epi == WN_EPI_GATE_BWD) hipLaunchKernelGGL(wn_fwd_gemm<WN_EPI_GATE_BWD>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(wn_fwd_gemm<WN_EPI_PLAIN>, grid, dim3(256), 0, st, a);
}

// The filter/gate product of a layer with kernel_size 3 or 4 (wn_fwd_gemm_taps: fp32 operands, the 128 x 128 tile), under the ragged row map where rg != NULL
static void wn_launch_taps(hipStream_t st, int taps, const WnTapsArgs& a, const WnRagged* rg = nullptr) {
    const dim3 grid((unsigned)((a.g.M + 127) / 128) * (unsigned)((a.g.N + 127) / 128));
    if (rg && taps == 3) hipLaunchKernelGGL(wn_fwd_gemm_taps_ragged<3>, grid, dim3(256), 0, st, a, *rg);
    else if (rg) hipLaunchKernelGGL(wn_fwd_gemm_taps_ragged<4>, grid, dim3(256), 0, st, a, *rg);
    else if (taps == 3) hipLaunchKernelGGL(wn_fwd_gemm_taps<3>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(wn_fwd_gemm_taps<4>, grid, dim3(256), 0, st, a);
}

// The same product on bf16 operands (wn_fwd_gemm_taps_bf16): bn = the layer's block of the bf16 bank, [N][taps * R]; N % 256 == 0 takes the
// 128 x 256 tile (wn_launch_nn's rule)
static void wn_launch_taps_bf16(hipStream_t st, int taps, const WnTapsArgs& a, const unsigned short* bn) {
    const bool wide = a.g.N % 256 == 0;
    const dim3 grid((unsigned)((a.g.M + 127) / 128) * (unsigned)(wide ? a.g.N / 256 : (a.g.N + 127) / 128));
    if (wide) {
        if (taps == 3) hipLaunchKernelGGL((wn_fwd_gemm_taps_bf16<3, 8>), grid, dim3(512), 0, st, a, bn);
        else hipLaunchKernelGGL((wn_fwd_gemm_taps_bf16<4, 8>), grid, dim3(512), 0, st, a, bn);
    } else {
        if (taps == 3) hipLaunchKernelGGL((wn_fwd_gemm_taps_bf16<3, 4>), grid, dim3(256), 0, st, a, bn);
        else hipLaunchKernelGGL((wn_fwd_gemm_taps_bf16<4, 4>), grid, dim3(256), 0, st, a, bn);
    }
}

// The input gradient of that product in the training step (wn_bwd_gemm_taps: one launch, dx written exactly once)
static void wn_launch_taps_bwd(hipStream_t st, int taps, const WnTapsBwdArgs& a) {
    const dim3 grid((unsigned)((a.g.M + 127) / 128) * (unsigned)((a.g.N + 127) / 128));
    if (taps == 3) hipLaunchKernelGGL(wn_bwd_gemm_taps<3>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(wn_bwd_gemm_taps<4>, grid, dim3(256), 0, st, a);
}

// One forward layer in one launch (wn_fwd_layer_bf16): `a` = the filter/gate product's arguments (bf16 operands, c_bf16 = 1; a.c.base may be
// NULL: z is not stored), `r` = the residual product's (its bias, cin, c, c_h are used).  Returns false when the shape is not the fused
// kernel's (the caller launches the two products).  WN_NO_FUSED_LAYER=1 (with WN_TESTING=1) switches it off for A/B runs.
static bool wn_fused_layer_enabled() { return !wn_dev_flag("WN_NO_FUSED_LAYER"); }
static bool wn_launch_layer(hipStream_t st, const WnGemmArgs& a, const unsigned short* bn_fg, const WnGemmArgs& r, const unsigned short* bn_res) {
    if (!bn_fg || !bn_res || !a.a_bf16 || a.N != 256 || r.N != 128 || r.K != 128 || a.K % 32 != 0 || a.k_split % 32 != 0 || !a.c_bf16 || a.relu_a || r.relu_a || r.relu_c ||
        r.mask || r.cin_skip_lo || r.M != a.M || r.rows_per_batch != a.rows_per_batch) return false;   // (x from its bf16 shadow, z kept as bf16, the same rows in both products)
    if (!wn_fused_layer_enabled()) return false;
    WnGemmArgsBf16 b;
    b.g = a; b.bn = bn_fg; b.bn1 = nullptr; b.ldb = 0;
    WnLayerArgs la;
    la.bn = bn_res; la.bias = r.bias; la.cin = r.cin; la.c = r.c; la.c_h = r.c_h; la.N = r.N;
    const dim3 grid(wn_layer_grid(a.M));
    hipLaunchKernelGGL(wn_fwd_layer_bf16, grid, dim3(512), 0, st, b, la);
    return true;
}

// The backward's fused pair (wn_bwd_layer_bf16): `a` = the dx product of layer l (bf16-stored A in two views, weight banks bn / bn1 with row
// length ldb), `b` = the gate-derivative product of layer l - 1, whose A operand is `a`'s output.  Returns false when the shapes are not
// the fused kernel's (the caller launches the two products).
static bool wn_launch_bwd_layer(hipStream_t st, const WnGemmArgs& a, const unsigned short* bn, const unsigned short* bn1, int ldb,
                                const WnGemmArgs& b, const unsigned short* bn_res) {
    if (!bn || !bn_res || !a.a_bf16 || a.N != 128 || a.K % 32 != 0 || a.bias || a.relu_a || a.relu_c || a.mask || a.c_h || a.c_bf16 ||
        b.N != 128 || b.K != 128 || !b.c_bf16 || !b.gate_packed || b.M != a.M || b.rows_per_batch != a.rows_per_batch) return false;
    if (b.a0.base != a.c.base || b.a0.t0 != a.c.t0 || b.a0.batch_stride != a.c.batch_stride || b.a0.row_stride != a.c.row_stride) return false;   // (the same rows)
    if (!wn_fused_layer_enabled()) return false;
    if (wn_dev_flag("WN_NO_FUSED_BWD")) return false;   // (A/B: the forward's fused layer alone)
    WnGemmArgsBf16 x, y;
    x.g = a; x.bn = bn; x.bn1 = bn1; x.ldb = ldb;
    y.g = b; y.bn = bn_res; y.bn1 = nullptr; y.ldb = 0;
    hipLaunchKernelGGL(wn_bwd_layer_bf16, dim3(wn_layer_grid(a.M)), dim3(512), 0, st, x, y);
    return true;
}

// ------------------------------------------------------------------------------------------------ product descriptions
// Every field a helper does not name is zero / NULL (= that feature off); the caller sets the few that are special to its product.
// `rows` rows of `cols` elements per batch entry, dense; t0 = the first row a product reads or writes
static WnRowMap wn_rows(const float* base, long long rows, long long cols, long long t0 = 0) { return WnRowMap{base, rows * cols, cols, t0}; }
// C = [a0 (k < k_split) | a1] . B^T (+ bias): M rows in batch entries of rows_per_batch -- the two-view form of the tap products
static WnGemmArgs wn_nn2(const WnRowMap& a0, const WnRowMap& a1, int k_split, int K, const float* bt, int N, const float* bias, const WnRowMap& c, long long M,
                         long long rows_per_batch) {
    WnGemmArgs g = {};
    g.a0 = a0; g.a1 = a1; g.k_split = k_split; g.K = K; g.bt = bt; g.N = N; g.bias = bias; g.c = c; g.M = M; g.rows_per_batch = (int)rows_per_batch;
    return g;
}
// C = A . B^T (+ bias) (+ cin where cin.base != NULL)
static WnGemmArgs wn_nn(const WnRowMap& a, int K, const float* bt, int N, const float* bias, const WnRowMap& c, long long M, long long rows_per_batch,
                        const WnRowMap& cin = WnRowMap{nullptr, 0, 0, 0}) {
    WnGemmArgs g = wn_nn2(a, a, K, K, bt, N, bias, c, M, rows_per_batch);
    g.cin = cin;
    return g;
}
// The weight-gradient form: C [Ka][ldc] (+)= A^T . B over M rows
static WnGemmTnArgs wn_tn(const WnRowMap& a, int Ka, const WnRowMap& b, int Nb, float* c, int ldc, long long M, long long rows_per_batch) {
    WnGemmTnArgs g = {};
    g.a = a; g.Ka = Ka; g.b = b; g.Nb = Nb; g.c = c; g.ldc = ldc; g.M = M; g.rows_per_batch = (int)rows_per_batch;
    return g;
}

// The pieces wn_forward, wn_prime and wn_train_forward share.  `fw` = the packed fp32 bank (layout o), n = batch entries, x = the layer's input at
// the first of its `rows` output positions.
// z = gate([x(t - d) | x(t)] . Wfg^T + b) of layer l   (kernel_size 2)
static WnGemmArgs wn_layer_fg(const WnPlan& pl, const wn_train_layout& o, const float* fw, int l, const WnRowMap& x, long long d, const WnRowMap& z, long long n,
                              long long rows) {
    WnRowMap x0 = x;
    x0.t0 -= d;
    return wn_nn2(x0, x, pl.R, 2 * pl.R, fw + o.fg + (size_t)l * 2 * pl.R * 2 * pl.D, 2 * pl.D, pl.has_bias ? fw + o.bfg + (size_t)l * 2 * pl.D : nullptr, z, n * rows, rows);
}
// z = gate([x(t - (k-1) d) | ... | x(t)] . Wfg^T + b) of layer l, kernel_size k = 3 or 4: the views are formed in the kernel from the view of x(t);
// t_min = the first row of a batch entry of x that exists (in the units of x.t0)
static WnTapsArgs wn_layer_fg_taps(const WnPlan& pl, const wn_train_layout& o, const float* fw, int l, const WnRowMap& x, long long d, const WnRowMap& z, long long n,
                                   long long rows, long long t_min) {
    WnTapsArgs a;
    a.g = wn_nn2(x, x, pl.R, pl.k * pl.R, fw + o.fg + (size_t)l * pl.k * pl.R * 2 * pl.D, 2 * pl.D, pl.has_bias ? fw + o.bfg + (size_t)l * 2 * pl.D : nullptr, z, n * rows, rows);
    a.tap_rows = d; a.t_min = t_min;
    return a;
}
// dx_l = (dx') + sum_j dfg(t + (k-1-j) d) . W_j^T of a layer with kernel_size k = 3 or 4, on the `rows_out` trailing rows of every batch entry.  dfg holds
// `rows_dfg` dense rows of 2D floats per entry, the trailing ones (wn_taps_bwd_shift, wn_plan.h: output row i is dfg's row i - shift where that exists);
// btT = the transposed tap blocks [2D][R] of the layer, tap_stride floats apart; dx / dxin (base NULL: no addend) are views at the first output row.
static WnTapsBwdArgs wn_layer_dx_taps(const WnPlan& pl, const float* dfg, long long rows_dfg, long long rows_out, long long d, const float* btT, long long tap_stride,
                                      const WnRowMap& dxin, const WnRowMap& dx, long long n) {
    const long long sh = wn_taps_bwd_shift(rows_out, rows_dfg);
    WnTapsBwdArgs a;
    const WnRowMap v = wn_rows(dfg, rows_dfg, 2 * pl.D, -sh);
    a.g = wn_nn2(v, v, 2 * pl.D, pl.k * 2 * pl.D, btT, pl.R, nullptr, dx, n * rows_out, rows_out);
    a.g.cin = dxin; a.g.cin_skip_lo = (int)sh;   // (dx' exists on the rows dfg does)
    a.tap_rows = d; a.t_lo = 0; a.t_hi = rows_dfg; a.bt_tap_stride = tap_stride;
    return a;
}
// x' = z . Wres^T + bres + x(t) of layer l
static WnGemmArgs wn_layer_res(const WnPlan& pl, const wn_train_layout& o, const float* fw, int l, const WnRowMap& z, const WnRowMap& x, const WnRowMap& xout,
                               long long n, long long rows) {
    return wn_nn(z, pl.D, fw + o.res + (size_t)l * pl.D * pl.R, pl.R, pl.has_bias ? fw + o.bres + (size_t)l * pl.R : nullptr, xout, n * rows, rows, x);
}
// skip (+)= ZG . [Wskip of the layers first .. first + cnt - 1]^T   (K = cnt * D; the first group also adds bskip_total, the sum of all layers' skip biases)
static WnGemmArgs wn_skip_group(const WnPlan& pl, const wn_train_layout& o, const float* fw, int first, int cnt, const WnRowMap& zg, const float* bskip_total,
                                float* skip, long long n, long long out_len) {
    const WnRowMap sk = wn_rows(skip, out_len, pl.S);
    return wn_nn(zg, cnt * pl.D, fw + o.skip + (size_t)first * pl.D * pl.S, pl.S, (pl.has_bias && first == 0) ? bskip_total : nullptr, sk, n * out_len, out_len,
                 first > 0 ? sk : WnRowMap{nullptr, 0, 0, 0});
}
// head: relu(skip) -> end_conv_1 (+b, relu) -> end_conv_2 (+b)     wavenet_model.py:167-169
struct WnHeadArgs { WnGemmArgs e, logits; };
static WnHeadArgs wn_head(const WnPlan& pl, const wn_train_layout& o, const float* fw, const float* skip, float* ev, float* logits, long long n, long long out_len) {
    WnHeadArgs hd;
    hd.e = wn_nn(wn_rows(skip, out_len, pl.S), pl.S, fw + o.w1, pl.E, fw + o.b1, wn_rows(ev, out_len, pl.E), n * out_len, out_len);
    hd.e.relu_a = 1; hd.e.relu_c = 1;
    hd.logits = wn_nn(wn_rows(ev, out_len, pl.E), pl.E, fw + o.w2, pl.C, fw + o.b2, wn_rows(logits, out_len, pl.C), n * out_len, out_len);
    return hd;
}

// Time geometry of WaveNetModel.forward() for clips of L samples (wavenet_modules.py:10-39 `dilate`, wavenet_model.py:125-196).
// In absolute time every layer's sequence ends at L (a kernel-size-2 dilated conv drops its input's first d positions; kernel_size k: (k - 1) d,
// served from L >= receptive_field + output_length - 1 on only -- wn_plan.h).  Where the
// length of a layer's input is not a multiple of its dilation the reference left-pads it with ZERO ACTIVATIONS (wavenet_modules.py:24-27),
// so layer l's input lives on [a[l], L) preceded by pad[l] = (-(L - a[l])) mod d zeros, and its output on [a[l+1], L) with
// a[l+1] = a[l] - pad[l] + d.  With L >= receptive_field + output_length - 1 none of the returned positions can see a pad zero (the
// regime of rounds 1-3); shorter clips can: the tap x(t - d) then reads as zero for t - d < a[l] (row windows of the GEMMs' A views).
//   rows[l] = trailing positions of layer l's input that are computed = min(rows[l+1] + d, L - a[l]);   zlo[l] = leading output rows of
//   layer l whose tap is a pad zero.
// Returns WN_E_UNSUPPORTED where the reference itself has no defined result: a layer left with no output position, the skip
// un-dilation quirk at a per-row length of 1, fewer than output_length final positions (its view fails).
static int wn_forward_geometry(const wn_handle* h, long long L, long long out_len, WnFwdGeom& g, const char* who) {
    const std::string why = wn_forward_geometry_host(h->dil.data(), h->plan.NL, L, out_len, g, h->plan.k);   // (wn_plan.h: plain host arithmetic, tested with g++)
    if (!why.empty()) return wn_fail(WN_E_UNSUPPORTED, "%s: %s", who, why.c_str());
    return WN_OK;
}

// WaveNetModel.forward() for one-hot inputs (class indices), see wn_forward.h.  Asynchronous on hip_stream.
// What wn_score asks of the forward instead of logits: the head's two products and the row statistics in one kernel (wn_score.h), or -- shapes that kernel is
// not written for, bf16 operands (see wn_fused_score_enabled), WN_NO_FUSED_SCORE=1 with WN_TESTING=1 -- the two head products into the workspace and wn_score_rows over them.
struct WnScoreOut {
    const int64_t* targets;
    float* row_nll;
    int32_t* row_pred;
    double* sums;
};
// Default: the fused kernel with fp32 operands, the unfused path with bf16 operands -- measured at config 5's evaluation batch (profiles/r07_score.txt) the fused
// bf16 kernel is 0.5-1.7 ms SLOWER than the unfused path (it re-reads the skip tile once per chunk of end channels, and with bf16 operands the head is bound by
// those reads, not by the matrix cores); fp32 is level to 0.6 ms faster.  WN_NO_FUSED_SCORE=1 / =0 (with WN_TESTING=1) pins the unfused / the fused path.
static bool wn_fused_score_enabled(wn_handle* h, bool bf16) {
    const char* off = wn_dev_env("WN_NO_FUSED_SCORE");
    if (off) h->dev_overrides = 1;   // (read per call, not at wn_create: the handle reports it from the first scoring call on)
    if (off && (off[0] == '1' || off[0] == '0')) return off[0] == '0';
    return !bf16;
}

// wn_forward / wn_score run on bf16 operands: kernel_size 2 under mode 1 (fwb_ok), kernel_size 3 and 4 under WN_PRECISION_BF16_TAPS (fwb_taps_ok; inference only)
static bool wn_forward_bf16(const wn_handle* h) { return (h->fw_bf16 && h->w.fwb_ok) || (h->fw_bf16_taps && h->w.fwb_taps_ok); }

static int wn_forward_run(wn_handle* h, const int32_t* indices, int64_t N, int64_t L, int64_t out_len, float* logits, const WnScoreOut* score, void* hip_stream,
                          const char* who) {
    if (!h->have_weights) return wn_fail(WN_E_STATE, "%s: wn_load_weights has not been called", who);
    if (N < 1 || out_len < 1) return wn_fail(WN_E_BADARG, "%s: N and output_length must be >= 1", who);
    const WnPlan& pl = h->plan;
    const WnWeights& wt = h->w;
    const int R = pl.R, D = pl.D, S = pl.S, E = pl.E, C = pl.C, NL = pl.NL;
    if (!wt.fwd_ok) return wn_fail(WN_E_UNSUPPORTED, "%s: needs kernel_size 2, 3 or 4 and channel counts that are multiples of 32", who);
    if ((long long)N * L >= 0x7fffffffll) return wn_fail(WN_E_UNSUPPORTED, "%s: N*L must stay below 2^31 rows", who);
    { int rc = rt_hip(hipSetDevice(h->cfg.device_id), "hipSetDevice"); if (rc) return rc; }
    WnFwdGeom geo;
    { int rc = wn_forward_geometry(h, L, out_len, geo, who); if (rc) return rc; }
    const long long Mrows = (long long)N * out_len;
    const bool score_fused = score && C == 256 && S % 32 == 0 && E % WN_SCORE_EC == 0 && wn_fused_score_enabled(h, wn_forward_bf16(h));
    size_t n_part = 0;
    if (score) {   // one fp64 triple per workgroup of the kernel that scores
        n_part = (size_t)(score_fused ? (Mrows + WN_SCORE_TM - 1) / WN_SCORE_TM : (Mrows + WN_SCORE_ROWS_PER_WG - 1) / WN_SCORE_ROWS_PER_WG);
        if (h->score_parts < n_part) {
            if (h->pending) { int rc = wn_wait(h); if (rc) return rc; }
            (void)hipDeviceSynchronize();
            if (!rt_grow(h->d_score_part, h->score_parts, n_part, 3)) return wn_fail(WN_E_NOMEM, "%s: %lld partial sums", who, (long long)n_part);
        }
    }
    const std::vector<long long>& need = geo.rows;
    const int taps = pl.k;   // 2: the two-view product of wn_fwd_gemm; 3, 4: wn_fwd_gemm_taps, or wn_fwd_gemm_taps_bf16 under WN_PRECISION_BF16_TAPS
    if (taps != 2)
        for (int l = 0; l < NL; ++l)
            if (geo.zlo[l] != 0 || L - need[l + 1] - (long long)(taps - 1) * h->dil[l] < 0) return wn_fail(WN_E_UNSUPPORTED, "%s: kernel_size %d does not serve zero-padded taps", who, taps);
    const size_t x_fl = (size_t)N * L * R, z_fl = (size_t)N * need[1 < NL ? 1 : NL] * D > (size_t)N * need[NL] * D ? (size_t)N * need[1 < NL ? 1 : NL] * D : (size_t)N * need[NL] * D;
    // The skip sum over layers is accumulated G layers at a time: the gate epilogue also drops z (last output_length rows)
    // into column block (l mod G) of ZG [N*out_len][G*D], and one GEMM with K = G*D adds the group to SKIP -- instead of a
    // read-modify-write of the whole SKIP matrix per layer (1.4 GB per layer at config 5).
    const int G = pl.layers < NL ? pl.layers : NL;
    const size_t skip_fl = (size_t)N * out_len * S, e_fl = (size_t)N * out_len * E, zg_fl = (size_t)N * out_len * G * D;
    // bf16 operands at the 128 / 128 shape: a layer is ONE launch (wn_fwd_layer_bf16: z goes from the gate epilogue to the residual product
    // through LDS and is never stored), its matrix operand reads of x take a bf16 shadow written next to x (WnGemmArgs::c_h), z on the skip
    // rows (zg) is stored as bf16.  Same roundings as the two-launch form (every value is rounded to bf16 once, where it becomes an operand).
    const bool fuse = taps == 2 && h->fw_bf16 && h->w.fwb_ok && R == 128 && D == 128 && wn_fused_layer_enabled();
    const size_t xh_fl = fuse ? ((x_fl + 1) / 2 + 63) / 64 * 64 : 0;
    const size_t lg_fl = (score && !score_fused) ? (size_t)Mrows * C : 0;   // (unfused scoring: the logits live in the workspace)
    const size_t total = 2 * x_fl + z_fl + skip_fl + e_fl + zg_fl + 2 * xh_fl + lg_fl;
    if (h->ws_floats < total) {
        if (h->pending) { int rc = wn_wait(h); if (rc) return rc; }
        if (!rt_grow(h->d_ws, h->ws_floats, total)) return wn_fail(WN_E_NOMEM, "%s: workspace of %.1f MB", who, total * 4e-6);
    }
    float* xa = h->d_ws; float* xb = xa + x_fl; float* z = xb + x_fl; float* skip = z + z_fl; float* ev = skip + skip_fl;
    float* zg = ev + e_fl;
    unsigned short* xha = fuse ? reinterpret_cast<unsigned short*>(zg + zg_fl) : nullptr;
    unsigned short* xhb = fuse ? reinterpret_cast<unsigned short*>(zg + zg_fl + xh_fl) : nullptr;
    if (lg_fl) logits = zg + zg_fl + 2 * xh_fl;
    hipStream_t st = (hipStream_t)hip_stream;
    {
        const long long rows = N * L;
        const long long work = rows * (R / 4);
        hipLaunchKernelGGL(wn_fwd_start, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, st, indices, h->w.d_start_t,
                           pl.has_bias ? h->w.d_start_b : nullptr, xa, rows, R, xha);
    }
    const bool bf16 = wn_forward_bf16(h);
    const unsigned short* fwb = wt.d_fwb;
    auto launch = [&](int epi, const WnGemmArgs& a, size_t bank) { wn_launch_nn(st, epi, a, bf16 ? fwb + bank : nullptr); };   // bank: the product's B in the bf16 bank
    const float* fw = wt.d_fw;
    const wn_train_layout& o = wt.fw;
    const WnBf16Layout& ob = wt.fwb;
    float* xin = xa; float* xout = xb;
    unsigned short* xhin = xha; unsigned short* xhout = xhb;
    for (int l = 0; l < NL; ++l) {
        const long long d = h->dil[l], rows = need[l + 1], t0 = L - rows;
        const int gi = l % G;
        // z = gate([x(t-d) | x(t)] . Wfg^T)
        const float* xop = fuse ? reinterpret_cast<const float*>(xhin) : xin;   // (fuse: the bf16 shadow, the row maps count bf16 elements)
        WnGemmArgs a = wn_layer_fg(pl, o, fw, l, wn_rows(xop, L, R, t0), d, wn_rows(z, rows, D), N, rows);
        a.a_skip_lo[0] = (int)geo.zlo[l];   // (short clips: the reference's left zero padding stands in for x(t - d) there)
        a.a_bf16 = fuse ? 1 : 0;
        a.c_bf16 = fuse ? 1 : 0;   // (fuse: z and zg hold bf16)
        a.c2 = wn_rows(fuse ? reinterpret_cast<float*>(reinterpret_cast<unsigned short*>(zg) + (size_t)gi * D) : zg + (size_t)gi * D, out_len, (long long)G * D);
        a.c2_first_row = (int)(rows - out_len);
        WnGemmArgs ar = {};  // x' = z . Wres^T + x(t)   (the last layer's residual output is never consumed, also upstream)
        if (l < NL - 1) {
            ar = wn_layer_res(pl, o, fw, l, wn_rows(z, rows, D), wn_rows(xin, L, R, t0), wn_rows(xout, L, R, t0), N, rows);
            ar.a_bf16 = fuse ? 1 : 0;
            ar.c_h = fuse ? xhout : nullptr;
        }
        bool fused = false;
        if (fuse && l < NL - 1) {
            WnGemmArgs af = a;
            af.c.base = nullptr;   // z itself is not stored: nothing reads it again
            fused = wn_launch_layer(st, af, fwb + ob.fg + (size_t)l * 2 * D * 2 * R, ar, fwb + ob.res + (size_t)l * R * D);
        }
        if (taps != 2) {   // (a's epilogue fields -- c, c2: z and its copy on the skip rows -- carried over)
            WnTapsArgs at = wn_layer_fg_taps(pl, o, fw, l, wn_rows(xin, L, R, t0), d, wn_rows(z, rows, D), N, rows, 0);
            at.g.c2 = a.c2; at.g.c2_first_row = a.c2_first_row;
            if (bf16) wn_launch_taps_bf16(st, taps, at, fwb + ob.fg + (size_t)l * 2 * D * taps * R);
            else wn_launch_taps(st, taps, at);
            if (l < NL - 1) launch(WN_EPI_PLAIN, ar, ob.res + (size_t)l * R * D);
        } else if (!fused) {
            launch(WN_EPI_GATE, a, ob.fg + (size_t)l * 2 * D * 2 * R);
            if (l < NL - 1) launch(WN_EPI_PLAIN, ar, ob.res + (size_t)l * R * D);
        }
        if (gi == G - 1 || l == NL - 1) {  // skip (+)= ZG . [Wskip of the group's layers]^T   (K = layers_in_group * D)
            const int first = l - gi, cnt = gi + 1;
            WnGemmArgs ak = wn_skip_group(pl, o, fw, first, cnt, wn_rows(zg, out_len, (long long)G * D), fw + o.bskip_total, skip, N, out_len);
            ak.a_bf16 = fuse ? 1 : 0;
            launch(WN_EPI_PLAIN, ak, ob.skip + (size_t)(first / G) * S * G * D);
        }
        float* t = xin; xin = xout; xout = t;
        unsigned short* th = xhin; xhin = xhout; xhout = th;
    }
    if (score_fused) {   // head and row statistics in one kernel: neither ev nor the logits reach HBM
        WnScoreArgs sa = {};
        sa.skip = skip; sa.M = Mrows; sa.S = S; sa.E = E;
        sa.w1t = fw + o.w1; sa.w2t = fw + o.w2; sa.b1 = fw + o.b1; sa.b2 = fw + o.b2;
        if (bf16) { sa.w1h = fwb + ob.w1; sa.w2h = fwb + ob.w2; }
        sa.targets = reinterpret_cast<const long long*>(score->targets); sa.row_nll = score->row_nll; sa.row_pred = score->row_pred; sa.part = h->d_score_part;
        if (bf16) hipLaunchKernelGGL(wn_score_head_bf16, dim3((unsigned)n_part), dim3(256), 0, st, sa);
        else hipLaunchKernelGGL(wn_score_head, dim3((unsigned)n_part), dim3(256), 0, st, sa);
    } else {
        const WnHeadArgs hd = wn_head(pl, o, fw, skip, ev, logits, N, out_len);
        launch(WN_EPI_PLAIN, hd.e, ob.w1);
        launch(WN_EPI_PLAIN, hd.logits, ob.w2);
        if (score)
            hipLaunchKernelGGL(wn_score_rows, dim3((unsigned)n_part), dim3(256), 0, st, logits, C, reinterpret_cast<const long long*>(score->targets), Mrows,
                               score->row_nll, score->row_pred, h->d_score_part);
    }
    if (score) hipLaunchKernelGGL(wn_score_reduce, dim3(1), dim3(1024), 0, st, h->d_score_part, (long long)n_part, score->sums);
    return rt_hip(hipGetLastError(), score ? "wn_score launches" : "wn_forward launches");
}

extern "C" int wn_forward(wn_handle* h, const int32_t* indices, int64_t N, int64_t L, int64_t out_len, float* logits, void* hip_stream) {
    g_err[0] = 0;
    if (!h || !indices || !logits) return wn_fail(WN_E_BADARG, "wn_forward: NULL argument");
    if (!h->chains.empty()) return wn_forward(h->chains[0], indices, N, L, out_len, logits, hip_stream);  // every chain holds the weights
    return wn_forward_run(h, indices, N, L, out_len, logits, nullptr, hip_stream, "wn_forward");
}

// Teacher-forced scoring (include/wn_abi.h): wn_forward's stack up to the finished skip rows, then the head and the row statistics (wn_score.h).
extern "C" int wn_score(wn_handle* h, const int32_t* indices, const int64_t* targets, int64_t N, int64_t L, int64_t out_len, float* row_nll, int32_t* row_pred,
                        double* sums, void* hip_stream) {
    g_err[0] = 0;
    if (!h || !indices || !targets || !sums) return wn_fail(WN_E_BADARG, "wn_score: NULL argument");
    if (wn_dev_env("WN_NO_FUSED_SCORE")) h->dev_overrides = 1;   // (the front handle of a job of several chains reports it too)
    if (!h->chains.empty()) return wn_score(h->chains[0], indices, targets, N, L, out_len, row_nll, row_pred, sums, hip_stream);  // every chain holds the weights
    const WnScoreOut so{targets, row_nll, row_pred, sums};
    return wn_forward_run(h, indices, N, L, out_len, nullptr, &so, hip_stream, "wn_score");
}

// Batched (teacher-forced) priming: the n_prime = n_given - 1 priming evaluations of generate_fast (wavenet_model.py:259-269)
// as GEMMs over all given positions at once instead of one chain pass per sample: the layer
// inputs of the whole window are computed with the forward kernels (no skip / head work -- the reference discards those
// outputs) and the newest (k-1)*d+1 columns of every layer are written straight into the queues.  Requires freshly reset queues
// (queue time 0); activations before the stream start are zero at every layer, like DilatedQueue.reset().
//
// Four entry points, one pass.  What a pass does is decided on the host by wn_prime_plan_host (wn_plan.h: WnPrimePlan, plain arithmetic, tested with g++);
// wn_prime_pass carries the plan out.  The forms differ in what they plan and in their checks, which stay with the entry points:
//   wn_prime         one row of samples per stream, all of one length: the rectangle
//   wn_prime_shared  ONE row for all streams: the rectangle of one stream, whose result the ring fill hands to every stream and copy of every handle listed
//   wn_prime_ragged  one row per stream, right-aligned at the queue time n = the longest: the ragged row tables -- or the rectangle where all lengths are n
//   wn_prime_append  wn_prime_ragged's rows (or one shared row) onto queues that hold a history, at any queue time: the plan's append form -- per layer a
//                    history gather in front of the fill and the products, and a fill of all ring slots at the new queue time
static int wn_need_forward_kernels(const wn_handle* h, const char* who) {
    if (!h->w.fwd_ok) return wn_fail(WN_E_UNSUPPORTED, "%s: needs kernel_size 2, 3 or 4 and channel counts that are multiples of 32", who);
    return WN_OK;
}

// The ragged form's row tables, host side: pinned staging that the copy before this one may still be reading (the event says when it is done), one device image
static int wn_prime_stage_tables(wn_handle* h, const WnRaggedPlan& rp, const char* who) {
    const size_t n_tab = rp.start.size();
    if (!h->ragged_ev) { int rc = rt_hip(hipEventCreateWithFlags(&h->ragged_ev, hipEventDisableTiming), "hipEventCreate"); if (rc) { h->ragged_ev = nullptr; return rc; } }
    else { int rc = rt_hip(hipEventSynchronize(h->ragged_ev), "hipEventSynchronize(row tables)"); if (rc) return rc; }
    if (h->ragged_ints < n_tab) {
        { int rc = rt_hip(hipDeviceSynchronize(), "hipDeviceSynchronize"); if (rc) return rc; }   // (kernels of an earlier pass may still read the old image)
        if (h->ragged_host) (void)hipHostFree(h->ragged_host);
        h->ragged_host = nullptr;
        if (hipHostMalloc((void**)&h->ragged_host, n_tab * sizeof(int32_t), hipHostMallocDefault) != hipSuccess) { h->ragged_host = nullptr; h->ragged_ints = 0; return wn_fail(WN_E_NOMEM, "%s: row tables", who); }
        if (!rt_grow(h->d_ragged, h->ragged_ints, n_tab)) return wn_fail(WN_E_NOMEM, "%s: row tables", who);
    }
    memcpy(h->ragged_host, rp.start.data(), n_tab * sizeof(int32_t));
    return WN_OK;
}

// One planned pass.  `h` (a handle with rings, not a front of rounds; checked by the entry point, its device current) runs the products on its weights and in
// its workspace over the rows of `samples` (row_stride apart), and the ring fill writes every layer's newest columns into the rings of the handles of `fill`:
// {h}, or (shared: the plan is one stream's, read with a stream stride of 0) every handle that takes the one row's result -- the members of a front share
// their weights, so member 0 computes for all, and h's own rings are filled only if it is listed.  A row before a stream's start is never computed: both
// halves of the cleared workspace read as zero there at every layer, which is what a reset queue holds.
static int wn_prime_pass(const WnPrimePlan& pp, wn_handle* h, const int32_t* samples, int64_t row_stride, bool shared, wn_handle* const* fill, size_t n_fill,
                         void* hip_stream, const char* who) {
    const WnPlan& pl = h->plan;
    const int R = pl.R, D = pl.D, ns = pp.ns;
    const long long n = pp.n, Lp = pp.Lp, Lt = pp.Lt;   // every stream's activation rows are preceded by Lp rows of zeros (t < 0): the oldest tap's reach
    const bool ragged = !pp.rectangle;
    if (h->ws_floats < pp.total_floats && !rt_grow(h->d_ws, h->ws_floats, pp.total_floats)) return wn_fail(WN_E_NOMEM, "%s: workspace of %.1f MB", who, pp.total_floats * 4e-6);
    if (ragged) { int rc = wn_prime_stage_tables(h, pp.ragged, who); if (rc) return rc; }
    float* xa = h->d_ws; float* xb = xa + pp.x_floats; float* z = xb + pp.x_floats;
    hipStream_t st = (hipStream_t)hip_stream;
    int rc = rt_hip(hipMemsetAsync(xa, 0, 2 * pp.x_floats * 4, st), "hipMemsetAsync(prime workspace)");
    if (rc) return rc;
    if (ragged) {   // the row tables of all layers, uploaded once
        rc = rt_hip(hipMemcpyAsync(h->d_ragged, h->ragged_host, pp.ragged.start.size() * sizeof(int32_t), hipMemcpyHostToDevice, st), "hipMemcpyAsync(row tables)");
        if (rc) return rc;
        rc = rt_hip(hipEventRecord(h->ragged_ev, st), "hipEventRecord(row tables)");
        if (rc) return rc;
    }
    auto table = [&](int t) { return WnRagged{h->d_ragged + (size_t)t * (ns + 1), ns, (int)n}; };
    // x0 = the start_conv column gather over all given positions; rows of stream s start at xa + s*Lt*R + Lp*R
    if (ragged) {   // ONE launch over every stream's own rows
        const long long work = pp.start_rows * (R / 4);
        if (work > 0)
            hipLaunchKernelGGL(wn_fwd_start_ragged, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, st, samples, (long long)row_stride, h->w.d_start_t,
                               pl.has_bias ? h->w.d_start_b : nullptr, xa + Lp * R, Lt * R, table(0), pp.start_rows, R);
    } else {
        for (int s = 0; s < ns; ++s) {
            const long long work = n * (R / 4);
            hipLaunchKernelGGL(wn_fwd_start, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, st, samples + (size_t)s * row_stride,
                               h->w.d_start_t, pl.has_bias ? h->w.d_start_b : nullptr, xa + ((size_t)s * Lt + Lp) * R, n, R);
        }
    }
    const float* fw = h->w.d_fw;
    float* xin = xa; float* xout = xb;
    for (int l = 0; l < pp.NL; ++l) {
        const WnPrimeLayer& y = pp.layer[l];
        if (pp.append) {   // what h's rings hold of layer l's input goes where the other forms read zeros: in front of every stream's rows, ahead of the fill and the products
            const long long work = (long long)ns * y.hist_rows * (R / 4);
            hipLaunchKernelGGL(wn_prime_gather_history, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, st, h->d_rings + h->ring_off[l], R, y.ML, ns, xin + Lp * R,
                               Lt * R, Lp, n, pp.base_time, ragged ? table(0) : WnRagged{nullptr, 0, 0});
        }
        for (size_t i = 0; i < n_fill; ++i) {   // queue of layer l <- newest min(k1*d+1, n) columns of its input: zeros where a stream had not started
            const wn_handle* f = fill[i];       // (append: all k1*d+1 columns, the older ones the gathered history, at the slots of the new queue time)
            const int nf = f->plan.n_streams;
            const long long work = (long long)nf * y.fill_cols * (R / 4);
            if (pp.append)
                hipLaunchKernelGGL(wn_fill_ring_at, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, st, xin + Lp * R, shared ? 0 : Lt * R,
                                   f->d_rings + f->ring_off[l], R, y.ML, nf, f->plan.P, n, y.fill_cols, pp.base_time);
            else
                hipLaunchKernelGGL(wn_fill_ring, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, st, xin + Lp * R, shared ? 0 : Lt * R,
                                   f->d_rings + f->ring_off[l], R, y.ML, nf, f->plan.P, n, y.fill_cols);
        }
        if (l == pp.NL - 1) break;
        if (y.M > 0) {
            // the plan's row maps (x: t - d may be negative: those rows are the zero prefix).  Ragged: every map counts rows from the stream's time 0, the
            // kernels put (stream, time) where (batch entry, row) stand
            const long long d = h->dil[l];
            const WnRowMap zmap = wn_rows(z, y.z_rows, D), x = WnRowMap{xin + Lp * R, Lt * R, R, y.t0}, xo = WnRowMap{xout + Lp * R, Lt * R, R, y.t0};
            const WnRagged tab = ragged ? table(1 + l) : WnRagged{nullptr, 0, 0};
            const WnRagged* rg = ragged ? &tab : nullptr;
            if (pl.k == 2) wn_launch_nn(st, WN_EPI_GATE, wn_layer_fg(pl, h->w.fw, fw, l, x, d, zmap, y.entries, y.rows), nullptr, nullptr, 0, rg);
            else wn_launch_taps(st, pl.k, wn_layer_fg_taps(pl, h->w.fw, fw, l, x, d, zmap, y.entries, y.rows, -Lp), rg);
            wn_launch_nn(st, WN_EPI_PLAIN, wn_layer_res(pl, h->w.fw, fw, l, zmap, x, xo, y.entries, y.rows), nullptr, nullptr, 0, rg);
        }
        float* t = xin; xin = xout; xout = t;
    }
    rc = rt_hip(hipGetLastError(), pp.append ? "wn_prime_append launches" : ragged ? "wn_prime_ragged launches" : "wn_prime launches");
    if (rc) return rc;
    for (size_t i = 0; i < n_fill; ++i) fill[i]->t_base = pp.base_time + n;
    return WN_OK;
}

// The checks and the plan of wn_prime and wn_prime_shared (ns = 1), in their order: nothing to do for n_prime == 0 before the kernels or the queue time matter
static int wn_prime_rectangle(wn_handle* h, const int32_t* first_samples, int64_t n_prime, int64_t row_stride, bool shared, wn_handle* const* fill, size_t n_fill,
                              void* hip_stream, const char* who) {
    if (!h->have_weights) return wn_fail(WN_E_STATE, "%s: wn_load_weights has not been called", who);
    if (n_prime < 0 || row_stride < n_prime) return wn_fail(WN_E_BADARG, "%s: bad n_prime / row_stride", who);
    if (n_prime == 0) return WN_OK;
    { int rc = wn_need_forward_kernels(h, who); if (rc) return rc; }
    if (h->pending) { int rc = wn_wait(h); if (rc) return rc; }
    for (size_t i = 0; i < n_fill; ++i) {
        if (fill[i]->pending) { int rc = wn_wait(fill[i]); if (rc) return rc; }
        if (fill[i]->t_base != 0) return wn_fail(WN_E_STATE, "%s: queues must be freshly reset (queue time is %lld)", who, fill[i]->t_base);
    }
    { int rc = rt_hip(hipSetDevice(h->cfg.device_id), "hipSetDevice"); if (rc) return rc; }
    WnPrimePlan pp;
    const std::string why = wn_prime_plan_host(h->dil.data(), h->plan.NL, h->plan.k, h->plan.R, h->plan.D, nullptr, shared ? 1 : h->plan.n_streams, n_prime, pp);
    if (!why.empty()) return wn_fail(WN_E_UNSUPPORTED, "%s: %s", who, why.c_str());
    return wn_prime_pass(pp, h, first_samples, row_stride, shared, fill, n_fill, hip_stream, who);
}

extern "C" int wn_prime(wn_handle* h, const int32_t* first_samples, int64_t n_prime, int64_t row_stride, void* hip_stream) {
    g_err[0] = 0;
    if (!h || !first_samples) return wn_fail(WN_E_BADARG, "wn_prime: NULL argument");
    if (!h->chains.empty()) {
        if (n_prime < 0 || row_stride < n_prime) return wn_fail(WN_E_BADARG, "wn_prime: bad n_prime / row_stride");
        if (h->pending) { int rc = wn_wait(h); if (rc) return rc; }
        for (size_t i = 0; i < h->chains.size(); ++i) {
            int rc = wn_prime(h->chains[i], first_samples + (size_t)h->chain_first[i] * (size_t)row_stride, n_prime, row_stride, hip_stream);
            if (rc) return rc;
        }
        h->t_base = h->chains[0]->t_base;
        return WN_OK;
    }
    return wn_prime_rectangle(h, first_samples, n_prime, row_stride, false, &h, 1, hip_stream, "wn_prime");
}

// ---- wn_prime_ragged: prompts of unequal length in one batched pass, right-aligned at the queue time n (include/wn_abi.h has the contract).
// What one handle with rings must satisfy before anything is launched -- a front checks EVERY member first, so that an error leaves all of them untouched.
static int wn_prime_ragged_check(wn_handle* h, const char* who) {
    if (!h->have_weights) return wn_fail(WN_E_STATE, "%s: wn_load_weights has not been called", who);
    { int rc = wn_need_forward_kernels(h, who); if (rc) return rc; }
    if (h->pending) { int rc = wn_wait(h); if (rc) return rc; }
    if (h->t_base != 0) return wn_fail(WN_E_STATE, "%s: queues must be freshly reset (queue time is %lld)", who, h->t_base);
    return WN_OK;
}
// One handle's streams (checked: wn_prime_ragged_check; lengths in [0, row_stride], n = the queue time all streams of the job end at, > 0 and >= every length).
// Streams of one length n plan as the rectangle: wn_prime's own launches, bit for bit, no row tables.
static int wn_prime_ragged_member(wn_handle* h, const int32_t* first_samples, const int64_t* n_prime, int64_t row_stride, long long n, void* hip_stream, const char* who) {
    WnPrimePlan pp;
    const std::string why = wn_prime_plan_host(h->dil.data(), h->plan.NL, h->plan.k, h->plan.R, h->plan.D, n_prime, h->plan.n_streams, n, pp);
    if (!why.empty()) return wn_fail(WN_E_UNSUPPORTED, "%s: %s", who, why.c_str());
    { int rc = rt_hip(hipSetDevice(h->cfg.device_id), "hipSetDevice"); if (rc) return rc; }
    return wn_prime_pass(pp, h, first_samples, row_stride, false, &h, 1, hip_stream, who);
}

extern "C" int wn_prime_ragged(wn_handle* h, const int32_t* first_samples, const int64_t* n_prime, int64_t row_stride, void* hip_stream) {
    g_err[0] = 0;
    if (!h || !first_samples || !n_prime) return wn_fail(WN_E_BADARG, "wn_prime_ragged: NULL argument");
    const int ns = h->chains.empty() ? h->plan.n_streams : h->chain_first.back();
    long long n = 0;
    for (int s = 0; s < ns; ++s) {
        if (n_prime[s] < 0 || n_prime[s] > row_stride) return wn_fail(WN_E_BADARG, "wn_prime_ragged: stream %d: length %lld outside [0, row_stride = %lld]", s, (long long)n_prime[s], (long long)row_stride);
        n = n_prime[s] > n ? n_prime[s] : n;
    }
    if (!h->chains.empty()) {
        if (h->pending) { int rc = wn_wait(h); if (rc) return rc; }
        if (h->broken) return wn_fail(WN_E_STATE, "wn_prime_ragged: an earlier job failed half way through its rounds; call wn_reset");
        for (wn_handle* c : h->chains) { int rc = wn_prime_ragged_check(c, "wn_prime_ragged"); if (rc) return rc; }
        if (n == 0) return WN_OK;
        for (size_t i = 0; i < h->chains.size(); ++i) {   // every member ends at the front's n, also one whose own streams are all shorter
            const size_t s0 = (size_t)h->chain_first[i];
            int rc = wn_prime_ragged_member(h->chains[i], first_samples + s0 * (size_t)row_stride, n_prime + s0, row_stride, n, hip_stream, "wn_prime_ragged");
            if (rc) { if (i) h->broken = true; return rc; }   // (members before this one have moved on: as after a job that failed between its rounds)
        }
        h->t_base = h->chains[0]->t_base;
        return WN_OK;
    }
    { int rc = wn_prime_ragged_check(h, "wn_prime_ragged"); if (rc) return rc; }
    if (n == 0) return WN_OK;
    return wn_prime_ragged_member(h, first_samples, n_prime, row_stride, n, hip_stream, "wn_prime_ragged");
}

// wn_prime for a prompt that every stream shares: ONE row of given samples, the stack's products once over it (the workspace of a 1-stream prime), the ring
// fill into every stream and copy -- of every round, where the handle is a front of rounds (the members share member 0's weights: it computes for all).
extern "C" int wn_prime_shared(wn_handle* h, const int32_t* first_samples, int64_t n_prime, void* hip_stream) {
    g_err[0] = 0;
    if (!h || !first_samples) return wn_fail(WN_E_BADARG, "wn_prime_shared: NULL argument");
    if (!h->chains.empty()) {
        if (h->pending) { int rc = wn_wait(h); if (rc) return rc; }
        if (h->broken) return wn_fail(WN_E_STATE, "wn_prime_shared: an earlier job failed half way through its rounds; call wn_reset");
        int rc = wn_prime_rectangle(h->chains[0], first_samples, n_prime, n_prime, true, h->chains.data(), h->chains.size(), hip_stream, "wn_prime_shared");
        if (rc) return rc;
        h->t_base = h->chains[0]->t_base;
        return WN_OK;
    }
    return wn_prime_rectangle(h, first_samples, n_prime, n_prime, true, &h, 1, hip_stream, "wn_prime_shared");
}

// ---- wn_prime_append: the batched pass onto queues that hold a history, at any queue time (include/wn_abi.h has the contract).  The plan's append form
// (wn_plan.h) gathers every layer's ring rows in front of the appended rows and rewrites all ring slots at the new queue time; the products are the ones
// wn_prime_ragged runs over the same lengths.  Everything that can refuse -- arguments, every member's state, every member's plan -- is looked at before
// the first launch, so that an error leaves the queues and the queue time alone.
extern "C" int wn_prime_append(wn_handle* h, const int32_t* samples, const int64_t* n_append, int64_t row_stride, int32_t shared, void* hip_stream) {
    g_err[0] = 0;
    const char* who = "wn_prime_append";
    if (!h || !samples || !n_append) return wn_fail(WN_E_BADARG, "%s: NULL argument", who);
    const bool front = !h->chains.empty();
    const int ns_all = front ? h->chain_first.back() : h->plan.n_streams;
    long long n = 0;
    for (int s = 0; s < (shared ? 1 : ns_all); ++s) {
        if (n_append[s] < 0 || n_append[s] > row_stride) return wn_fail(WN_E_BADARG, "%s: stream %d: length %lld outside [0, row_stride = %lld]", who, s, (long long)n_append[s], (long long)row_stride);
        n = n_append[s] > n ? n_append[s] : n;
    }
    if (h->pending) { int rc = wn_wait(h); if (rc) return rc; }
    if (front && h->broken) return wn_fail(WN_E_STATE, "%s: an earlier job failed half way through its rounds; call wn_reset", who);
    std::vector<wn_handle*> members = front ? h->chains : std::vector<wn_handle*>{h};
    for (wn_handle* c : members) {
        if (!c->have_weights) return wn_fail(WN_E_STATE, "%s: wn_load_weights has not been called", who);
        { int rc = wn_need_forward_kernels(c, who); if (rc) return rc; }
        if (c->pending) { int rc = wn_wait(c); if (rc) return rc; }
        if (c->t_base != members[0]->t_base) return wn_fail(WN_E_STATE, "%s: the rounds stand at different queue times (%lld, %lld); call wn_reset", who, members[0]->t_base, c->t_base);
    }
    if (n == 0) return WN_OK;
    const long long t0 = members[0]->t_base;
    std::vector<WnPrimePlan> plans(shared ? 1 : members.size());
    for (size_t i = 0; i < plans.size(); ++i) {   // shared: ONE stream's rectangle, computed by member 0 for all
        const wn_handle* c = members[i];
        const std::string why = wn_prime_plan_host(c->dil.data(), c->plan.NL, c->plan.k, c->plan.R, c->plan.D, shared ? nullptr : n_append + (front ? h->chain_first[i] : 0),
                                                   shared ? 1 : c->plan.n_streams, n, plans[i], true, t0);
        if (!why.empty()) return wn_fail(WN_E_UNSUPPORTED, "%s: %s", who, why.c_str());
    }
    if (shared) {
        { int rc = rt_hip(hipSetDevice(members[0]->cfg.device_id), "hipSetDevice"); if (rc) return rc; }
        int rc = wn_prime_pass(plans[0], members[0], samples, row_stride, true, members.data(), members.size(), hip_stream, who);
        if (rc) return rc;
    } else {
        for (size_t i = 0; i < members.size(); ++i) {   // every member ends at t0 + the n of ALL streams, also one whose own streams are all shorter
            const size_t s0 = front ? (size_t)h->chain_first[i] : 0;
            int rc = rt_hip(hipSetDevice(members[i]->cfg.device_id), "hipSetDevice");
            rc = rc ? rc : wn_prime_pass(plans[i], members[i], samples + s0 * (size_t)row_stride, row_stride, false, &members[i], 1, hip_stream, who);
            if (rc) { if (i) h->broken = true; return rc; }   // (members before this one have moved on: as after a job that failed between its rounds)
        }
    }
    if (front) h->t_base = h->chains[0]->t_base;
    return WN_OK;
}

// Operand precision of wn_forward's / wn_score's GEMMs: 0 = fp32 (default; matches the reference's fp32 forward to rounding),
// 1 = bf16 operands with fp32 accumulation (the residual stream and all sums stay fp32; kernel_size 2, the training step included),
// WN_PRECISION_BF16_TAPS = the same, and on a kernel_size 3 or 4 handle bf16 operands for wn_forward and wn_score alone (the training
// step of such a handle stays fp32 whatever the mode).  wn_prime always runs fp32.
extern "C" int wn_set_forward_precision(wn_handle* h, int32_t bf16) {
    g_err[0] = 0;
    if (!h) return wn_fail(WN_E_BADARG, "wn_set_forward_precision: NULL handle");
    if (!h->chains.empty()) return wn_set_forward_precision(h->chains[0], bf16);
    if (bf16 && !h->have_weights) return wn_fail(WN_E_STATE, "wn_set_forward_precision: load the weights first");
    if (bf16 == WN_PRECISION_BF16_TAPS && h->plan.k != 2) {
        if (h->plan.k > 4 || h->plan.k < 2) return wn_fail(WN_E_UNSUPPORTED, "wn_set_forward_precision: bf16 operands need kernel_size 2, 3 or 4 (kernel_size %d runs fp32)", h->plan.k);
        if (!h->w.fwb_taps_ok) return wn_fail(WN_E_UNSUPPORTED, "wn_set_forward_precision: bf16 needs R, D, S, E to be multiples of 64");
        h->fw_bf16_taps = 1;
        return WN_OK;
    }
    if (bf16 && h->plan.k != 2) return wn_fail(WN_E_UNSUPPORTED, "wn_set_forward_precision: bf16 operands need kernel_size 2 (kernel_size %d runs fp32)", h->plan.k);
    if (bf16 && !h->w.fwb_ok) return wn_fail(WN_E_UNSUPPORTED, "wn_set_forward_precision: bf16 needs R, D, S, E to be multiples of 64");
    h->fw_bf16 = bf16 ? 1 : 0;
    h->fw_bf16_taps = 0;
    return WN_OK;
}
