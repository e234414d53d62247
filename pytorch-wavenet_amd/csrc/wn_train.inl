// wn_train.inl -- host side of the native training step (included by wn_runtime.hip; GPU build only).
//
// Reference: WavenetTrainer.train (wavenet_training.py:58-107) runs output = model(x); loss = F.cross_entropy(...);
// loss.backward(); optimizer.step().  wn_train_forward / wn_train_backward replace model(x) and the autograd walk through
// WaveNetModel.wavenet (wavenet_model.py:125-171) with fp32 matrix-core GEMMs over all time steps at once:
//
//   forward  (per layer l, rows = the time steps the loss still depends on):
//       [F|G] = [x_l(t-d) | x_l(t)] . Wfg^T + b        T = tanh(F), G = sigmoid(G), z = T*G            (saved: x_l, z, T, G)
//       x_{l+1}(t) = z . Wres^T + bres + x_l(t)          skip += z[last output_length rows] . Wskip^T + bskip
//       logits = relu(relu(skip) . W1^T + b1) . W2^T + b2                                               (saved: skip, e)
//   backward (given dlogits):
//       de = (dlogits . W2) * [e > 0]      dskip = (de . W1) * [skip > 0]       dW2^T = e^T . dlogits   dW1^T = relu(skip)^T . de
//       per layer, last to first, with dx' = dLoss/dx_{l+1}:
//           dz   = dx' . Wres  (+ dskip . Wskip on the skip rows)          dWres^T = z^T . dx'      dWskip^T = z_skiprows^T . dskip
//           dF   = dz * G * (1 - T^2),  dG = dz * T * G * (1 - G)           dWfg^T  = [x_l(t-d) | x_l(t)]^T . [dF|dG]
//           dx_l(t) = dx'(t) + [dF|dG](t) . Wfg(tap 1) + [dF|dG](t+d) . Wfg(tap 0)
//       dstart^T = onehot(indices)^T . dx_0
//   kernel_size k = 3, 4 (fp32 operands; clips of at least receptive_field + output_length - 1 samples, so that every tap of every row exists):
//       [F|G] = [x_l(t-(k-1)d) | ... | x_l(t)] . Wfg^T + b      wn_fwd_gemm_taps<k>, the same gate epilogue (T, G saved, z into Z_b)
//       dWfg^T rows jR.. = x_l(t-(k-1-j)d)^T . [dF|dG]          k single-view launches of wn_bwd_gemm_tn (atomics or deterministic, as every TN product)
//       dx_l(t) = dx'(t) + sum_j [dF|dG](t+(k-1-j)d) . Wfg(tap j)    ONE launch of wn_bwd_gemm_taps<k>, dx_l written exactly once
//   everything else -- residual, grouped skip, head, gate derivative, column sums, start_conv, the two streams and their events -- is the k = 2 code.
//   "NN" products reuse wn_fwd_gemm with re-laid-out banks (rebuilt from `params` by wn_transpose_batched on every forward);
//   "TN" products (weight gradients) use wn_bwd_gemm_tn; bias gradients are column sums.


static int wn_train_layout_ws(const wn_handle* h, long long N, long long L, long long out_len, WnTrainLay& t) {
    const WnPlan& pl = h->plan;
    const int R = pl.R, D = pl.D, S = pl.S, E = pl.E, C = pl.C, NL = pl.NL;
    t.N = N; t.L = L; t.out_len = out_len; t.NL = NL;
    {   // need[l]: trailing positions of layer l's input the loss depends on AND that exist; zlo[l]: rows whose tap is a pad zero (wn_forward_geometry)
        WnFwdGeom geo;
        const int rc = wn_forward_geometry(h, L, out_len, geo, "wn_train_forward");
        if (rc) return rc;
        t.need = geo.rows; t.zlo = geo.zlo;
    }
    if (pl.k != 2)   // (the k-tap products have no row windows for pad zeros: wn_forward's refusal)
        for (int l = 0; l < NL; ++l)
            if (t.zlo[l] != 0 || L - t.need[l + 1] - (long long)(pl.k - 1) * h->dil[l] < 0)
                return wn_fail(WN_E_UNSUPPORTED, "wn_train_forward: kernel_size %d does not serve zero-padded taps", pl.k);
    t.G = pl.layers < NL ? pl.layers : NL;
    { const char* gb = wn_dev_env("WN_TRAIN_SKIP_BLOCK"); if (gb && atoi(gb) > 0) t.G = atoi(gb) < NL ? atoi(gb) : NL; }   // (A/B runs, with WN_TESTING=1: layers per grouped skip product)
    size_t o = 0;
    auto take = [&](size_t n) { size_t r = o; o += (n + 63) & ~(size_t)63; return r; };
    t.x.resize(NL); t.th.resize(NL); t.sg.resize(NL);
    size_t zmax = 0;
    for (int l = 0; l < NL; ++l) {
        const size_t zl = (size_t)N * t.need[l + 1] * D;
        zmax = zl > zmax ? zl : zmax;
        t.x[l] = take((size_t)N * L * R);
        t.th[l] = take(zl); t.sg[l] = take(zl);
    }
    // z of a skip block's layers lives SIDE BY SIDE in one matrix Z_b: row (n, t) = [z_first(n, t) | z_first+1(n, t) | ...] (cnt * D elements; rows
    // aligned at the clips' ends, as many per clip as the block's first layer has).  z_l is a strided VIEW of it (row stride cnt * D, column block
    // l - first, the layer's own trailing rows) -- every consumer takes row maps --, and the last output_length rows of every clip, all columns, ARE the
    // A operand of the block's grouped skip product and of its weight gradient: rounds 2-4 wrote that operand as a second copy of z on the skip rows
    // (`zg`: 4.45 GB per bf16 config-5 step written by the gate epilogues, and as much workspace).  The rows a deeper layer of the block does not have
    // (at most the block's dilations: ~5 %) are never touched.
    t.nblk = (NL + t.G - 1) / t.G;
    t.zb.resize(t.nblk); t.zb_rows.resize(t.nblk);
    for (int b = 0; b < t.nblk; ++b) {
        t.zb_rows[b] = t.need[b * t.G + 1];
        t.zb[b] = take((size_t)N * t.zb_rows[b] * t.cnt(b) * D);
    }
    // The bf16 step keeps a bf16 SHADOW of the residual stream next to the fp32 one.  x_l is a matrix operand four times per step (the
    // two tap views of the filter/gate product and of its weight gradient) and an addend once (the residual); the operand reads convert
    // it to bf16 on their way to LDS anyway.  Written once by the product that produces x_l (WnGemmArgs::c_h), the shadow gives those
    // four reads the same bits at half the bytes: +0.13 GB written, -0.5 GB read per layer at config 5.  The fp32 stream stays what the
    // residual adds run on.
    t.xh.clear();
    if (h->fw_bf16 && h->w.fwb_ok && R % 128 == 0 && (2 * D) % 256 == 0) {   // (the shapes whose filter/gate products take the 256-column tiles: the forms compiled for a bf16-stored x)
        t.xh.resize(NL);
        for (int l = 0; l < NL; ++l) t.xh[l] = take(((size_t)N * L * R + 1) / 2);
    }
    const size_t Mo = (size_t)N * out_len;
    t.skip = take(Mo * S); t.ev = take(Mo * E); t.dzg = take((size_t)t.nblk * Mo * t.G * D); t.bskip_total = take(S);
    t.res_o = take((size_t)NL * R * D); t.skip_o = take((size_t)NL * S * D); t.w1_o = take((size_t)E * S); t.w2_o = take((size_t)C * E);
    t.fgb0 = take((size_t)NL * 2 * D * R); t.fgb1 = take((size_t)NL * 2 * D * R);
    if (pl.k > 2) take((size_t)(pl.k - 2) * NL * 2 * D * R);   // kernel_size 3, 4: the further taps' blocks behind them, tap j at fgb0 + j * (fgb1 - fgb0)
    t.dskip = take(Mo * S); t.de = take(Mo * E); t.dz = take(zmax); t.dfg = take(2 * zmax); t.dfg2 = take(2 * zmax);
    t.dskip_h = (h->fw_bf16 && h->w.fwb_ok) ? take((Mo * S + 1) / 2) : 0;   // (written by the dskip product next to the fp32 matrix: WnGemmArgs::c_h)
    t.dxa = take((size_t)N * L * R); t.dxb = take((size_t)N * L * R);
    t.colsum_tmp = take(S);
    t.idx = take((size_t)N * L);
    // bf16 operand banks (2 bytes each; sizes in floats): the whole parameter blob as it is (backward products) and the
    // transposed forward banks
    t.bw = take((h->w.fw_floats + 1) / 2);
    t.bt_fg = take((size_t)NL * 2 * D * 2 * R / 2); t.bt_res = take((size_t)NL * R * D / 2); t.bt_skip = take((size_t)NL * S * D / 2);
    t.bt_w1 = take((size_t)E * S / 2); t.bt_w2 = take((size_t)C * E / 2);
    t.total = o;
    return WN_OK;
}

// Row maps into Z_b (wn_train_layout_ws).  h16: z is stored as bf16 (the maps count bf16 elements then; the base is a bf16 address behind a float pointer).
static WnRowMap wn_z_map(const WnTrainLay& t, float* ws, int D, int l, bool h16) {       // z_l on its own rows (index 0 = the first of its need[l + 1])
    const int b = l / t.G, gi = l - b * t.G;
    const long long ld = (long long)t.cnt(b) * D, rows_b = t.zb_rows[b];
    float* base = h16 ? reinterpret_cast<float*>(reinterpret_cast<unsigned short*>(ws + t.zb[b]) + (size_t)gi * D) : ws + t.zb[b] + (size_t)gi * D;
    return WnRowMap{base, rows_b * ld, ld, rows_b - t.need[l + 1]};
}
static WnRowMap wn_zg_map(const WnTrainLay& t, float* ws, int D, int b) {                 // the block's z on the last output_length rows of every clip, all columns
    const long long ld = (long long)t.cnt(b) * D, rows_b = t.zb_rows[b];
    return WnRowMap{ws + t.zb[b], rows_b * ld, ld, rows_b - t.out_len};
}

static int wn_train_usable(wn_handle* h, const char* who) {   // a handle whose packed parameter layout is the caller's model
    if (!h->have_weights) return wn_fail(WN_E_STATE, "%s: wn_load_weights has not been called", who);
    if (!h->w.train_ok) return wn_fail(WN_E_UNSUPPORTED, "wn_train: needs kernel_size 2, 3 or 4 and channel counts that are multiples of 32");
    if (h->padded) return wn_fail(WN_E_UNSUPPORTED, "wn_train: this handle runs a zero-padded channel shape (its parameter layout is not the caller's)");
    return WN_OK;
}
static int wn_train_tensors_check(wn_handle* h, const char* who) {
    const int rc = wn_train_usable(h, who);
    return rc ? rc : rt_hip(hipSetDevice(h->cfg.device_id), "hipSetDevice");
}

extern "C" int wn_train_get_layout(wn_handle* h, wn_train_layout* out) {
    g_err[0] = 0;
    if (!h || !out) return wn_fail(WN_E_BADARG, "wn_train_get_layout: NULL argument");
    if (!h->chains.empty()) return wn_train_get_layout(h->chains[0], out);
    { int rc = wn_train_usable(h, "wn_train_get_layout"); if (rc) return rc; }
    *out = h->w.fw;
    return WN_OK;
}

extern "C" int wn_train_set_deterministic(wn_handle* h, int32_t on) {
    g_err[0] = 0;
    if (!h) return wn_fail(WN_E_BADARG, "wn_train_set_deterministic: NULL handle");
    if (!h->chains.empty()) return wn_train_set_deterministic(h->chains[0], on);
    h->deterministic = on != 0;
    return WN_OK;
}

extern "C" int wn_train_export_params(wn_handle* h, float* params, void* hip_stream) {
    g_err[0] = 0;
    if (!h || !params) return wn_fail(WN_E_BADARG, "wn_train_export_params: NULL argument");
    if (!h->chains.empty()) return wn_train_export_params(h->chains[0], params, hip_stream);
    { int rc = wn_train_tensors_check(h, "wn_train_export_params"); if (rc) return rc; }
    return rt_hip(hipMemcpyAsync(params, h->w.d_fw, h->w.fw_floats * 4, hipMemcpyDeviceToDevice, (hipStream_t)hip_stream), "hipMemcpyAsync(params)");
}

// wn_train_pack / wn_train_unpack_grads: see wn_relayout (wn_forward.h) for the piece algebra.  A NULL tensor pointer is skipped (unpack: a gradient the
// caller does not want, e.g. the last layer's residual conv, which never reaches the loss).
static int wn_relayout_run(wn_handle* h, const wn_train_tensors* t, float* flat, bool unpack, hipStream_t st, const char* who) {
    const WnPlan& pl = h->plan;
    const wn_train_layout& o = h->w.fw;
    const int R = pl.R, D = pl.D, S = pl.S, E = pl.E, C = pl.C, NL = pl.NL, k = pl.k;
    if (t->n_layers != NL) return wn_fail(WN_E_BADARG, "%s: n_layers = %d, the model has %d", who, t->n_layers, NL);
    if (!t->filter_w || !t->gate_w || !t->res_w || !t->skip_w) return wn_fail(WN_E_BADARG, "%s: a per-layer pointer array is NULL", who);
    if (pl.has_bias && (!t->filter_b || !t->gate_b || !t->res_b || !t->skip_b)) return wn_fail(WN_E_BADARG, "%s: cfg.bias = 1 but a per-layer bias array is NULL", who);
    std::vector<WnRelayoutBatch> batches;
    WnRelayoutBatch b;
    memset(&b, 0, sizeof(b));
    auto flush = [&]() { if (b.n > 0) { batches.push_back(b); memset(&b, 0, sizeof(b)); } };
    bool missing = false;
    auto piece = [&](void* ref, size_t off, int rows, int cols, int rs, int cs, int ld, int cm_blk, int cm_off) {
        if (!ref) { missing = true; return; }
        if (b.n == WN_RELAYOUT_PIECES) flush();
        WnRelayoutPiece& q = b.p[b.n++];
        q.ref = static_cast<float*>(ref); q.off = (long long)off; q.rows = rows; q.cols = cols; q.rs = rs; q.cs = cs; q.ld = ld; q.cm_blk = cm_blk; q.cm_off = cm_off;
        q.tile0 = b.tiles;
        b.tiles += ((rows + 31) / 32) * ((cols + 31) / 32);
    };
    for (int l = 0; l < NL; ++l) {
        for (int tap = 0; tap < k; ++tap) {   // (D, R, k) -> rows tap * R .. of [kR][2D], columns [F(32) | G(32)] per 32 channels
            const size_t off = o.fg + ((size_t)l * k * R + (size_t)tap * R) * 2 * D;
            piece(t->filter_w[l] ? static_cast<float*>(t->filter_w[l]) + tap : nullptr, off, D, R, k * R, k, 2 * D, 64, 0);
            piece(t->gate_w[l] ? static_cast<float*>(t->gate_w[l]) + tap : nullptr, off, D, R, k * R, k, 2 * D, 64, 32);
        }
        piece(t->res_w[l], o.res + (size_t)l * D * R, R, D, D, 1, R, 32, 0);       // (R, D, 1) -> [D][R]
        piece(t->skip_w[l], o.skip + (size_t)l * D * S, S, D, D, 1, S, 32, 0);     // (S, D, 1) -> [D][S]
        if (pl.has_bias) {
            piece(t->filter_b[l], o.bfg + (size_t)l * 2 * D, D, 1, 1, 0, 0, 64, 0);
            piece(t->gate_b[l], o.bfg + (size_t)l * 2 * D, D, 1, 1, 0, 0, 64, 32);
            piece(t->res_b[l], o.bres + (size_t)l * R, R, 1, 1, 0, 0, 32, 0);
            piece(t->skip_b[l], o.bskip + (size_t)l * S, S, 1, 1, 0, 0, 32, 0);
        }
    }
    piece(t->end1_w, o.w1, E, S, S, 1, E, 32, 0);        // (E, S, 1) -> [S][E]
    piece(t->end1_b, o.b1, E, 1, 1, 0, 0, 32, 0);
    piece(t->end2_w, o.w2, C, E, E, 1, C, 32, 0);        // (C, E, 1) -> [E][C]
    piece(t->end2_b, o.b2, C, 1, 1, 0, 0, 32, 0);
    piece(t->start_w, o.start_t, R, C, C, 1, R, 32, 0);  // (R, C, 1) -> [C][R]
    if (pl.has_bias) piece(t->start_b, o.start_b, R, 1, 1, 0, 0, 32, 0);
    flush();
    if (missing && !unpack) return wn_fail(WN_E_BADARG, "%s: a parameter tensor pointer is NULL", who);
    for (const WnRelayoutBatch& bb : batches) {
        if (unpack) hipLaunchKernelGGL(wn_relayout<true>, dim3((unsigned)bb.tiles), dim3(256), 0, st, bb, flat);
        else hipLaunchKernelGGL(wn_relayout<false>, dim3((unsigned)bb.tiles), dim3(256), 0, st, bb, flat);
    }
    return rt_hip(hipGetLastError(), who);
}

extern "C" int wn_train_pack(wn_handle* h, const wn_train_tensors* tensors, float* params, void* hip_stream) {
    g_err[0] = 0;
    if (!h || !tensors || !params) return wn_fail(WN_E_BADARG, "wn_train_pack: NULL argument");
    if (!h->chains.empty()) return wn_train_pack(h->chains[0], tensors, params, hip_stream);
    { int rc = wn_train_tensors_check(h, "wn_train_pack"); if (rc) return rc; }
    // (sections no tensor maps to -- the bias sections of a model without biases, bskip_total -- read as zero, like the Python pack's torch.zeros)
    int rc = rt_hip(hipMemsetAsync(params, 0, h->w.fw_floats * 4, (hipStream_t)hip_stream), "hipMemsetAsync(params)");
    return rc ? rc : wn_relayout_run(h, tensors, params, false, (hipStream_t)hip_stream, "wn_train_pack");
}

extern "C" int wn_train_unpack_grads(wn_handle* h, const float* grads, const wn_train_tensors* tensors, void* hip_stream) {
    g_err[0] = 0;
    if (!h || !tensors || !grads) return wn_fail(WN_E_BADARG, "wn_train_unpack_grads: NULL argument");
    if (!h->chains.empty()) return wn_train_unpack_grads(h->chains[0], grads, tensors, hip_stream);
    { int rc = wn_train_tensors_check(h, "wn_train_unpack_grads"); if (rc) return rc; }
    return wn_relayout_run(h, tensors, const_cast<float*>(grads), true, (hipStream_t)hip_stream, "wn_train_unpack_grads");
}

static void wn_launch_cvt_t(hipStream_t st, const float* in, long long in_batch_stride, unsigned short* out, int rows, int cols, int batches) {
    hipLaunchKernelGGL(wn_cvt_bf16_transposed, dim3((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32), (unsigned)batches), dim3(256), 0, st,
                       in, in_batch_stride, out, rows, cols);
}

// Deterministic mode (wn_train_set_deterministic / WN_DETERMINISTIC=1): the row splits of a weight-gradient product and the row blocks of a bias
// gradient store their partial results in a workspace -- one per stream the backward uses: the two run side by side -- and a second kernel adds them
// in order.  Bit-equal gradients from run to run for the price of one write and one read of the partial tiles (at most 67 MB per product).
static thread_local WnDetWs* t_tn_det[2] = {nullptr, nullptr};   // [0]: the caller's stream, [1]: the side stream
static thread_local hipStream_t t_tn_side = nullptr;
// The streams of one wn_train_forward / wn_train_backward call: the caller's (`st`) and, after fork(), the handle's side stream (`sd`) next to it, ordered by
// events from the handle's pool.  WN_TRAIN_ONE_STREAM=1 (with WN_TESTING=1) keeps everything on the caller's stream (A/B runs): sd == st, no events waited for.
// While it lives, the call's launches find the handle's partial-tile workspaces (deterministic mode) and the side stream through the thread-locals above.
struct WnTrainStreams {
    wn_handle* h;
    hipStream_t st, sd;
    bool two = false;
    size_t ev_next = 0;   // cursor into h->events
    WnTrainStreams(wn_handle* h_, hipStream_t st_) : h(h_), st(st_), sd(st_) {
        if (h->deterministic) { t_tn_det[0] = &h->det_ws[0]; t_tn_det[1] = &h->det_ws[1]; }
        t_tn_side = nullptr;
    }
    ~WnTrainStreams() { t_tn_det[0] = t_tn_det[1] = nullptr; t_tn_side = nullptr; }
    int fork() {   // from here on sd is the side stream (created on first use)
        two = !wn_dev_flag("WN_TRAIN_ONE_STREAM");
        if (two && !h->side_stream) {
            int rc = rt_hip(hipStreamCreateWithFlags(&h->side_stream, hipStreamNonBlocking), "hipStreamCreateWithFlags");
            if (rc) return rc;
        }
        sd = two ? h->side_stream : st;
        t_tn_side = two ? h->side_stream : nullptr;
        return 0;
    }
    hipEvent_t signal(hipStream_t from) {   // an event recorded on `from` now
        if (ev_next == h->events.size()) {
            hipEvent_t e = nullptr;
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
            h->events.push_back(e);
        }
        hipEvent_t e = h->events[ev_next++];
        (void)hipEventRecord(e, from);
        return e;
    }
    void wait_for(hipStream_t who, hipEvent_t e) const { if (two && e) (void)hipStreamWaitEvent(who, e, 0); }
};
static float* wn_det_part(hipStream_t st, size_t floats) {
    WnDetWs* w = t_tn_det[(t_tn_side && st == t_tn_side) ? 1 : 0];
    if (!w) return nullptr;
    if (w->floats < floats) {
        (void)hipDeviceSynchronize();
        (void)rt_grow(w->buf, w->floats, floats);
    }
    return w->buf;
}

// The weight-gradient kernels read each operand of a row split through a buffer descriptor based at the split's first row, with 32-bit byte offsets
// and a 2 GB window (wn_rsrc): rows beyond it would read as zeros.  True when every split of `rps` rows keeps each operand it reads inside the
// window -- batch-stride jumps included (strides >= 0, batch entries in order).
static bool wn_tn_map_fits(const WnRowMap& map, long long m0, long long m1, int rpb, long long cols, int esize) {
    const long long q0 = m0 / rpb, q1 = (m1 - 1) / rpb;
    auto e = [&](long long q, long long rem) { return q * map.batch_stride + (map.t0 + rem) * map.row_stride; };
    const long long base = e(q0, m0 - q0 * rpb);
    for (long long q = q0; q <= q1; ++q) {   // the last row of each batch entry in range is its farthest
        const long long hi = q == q1 ? m1 - 1 - q1 * rpb : rpb - 1;
        if ((e(q, hi) - base + cols) * esize > 0x7fffffffll) return false;
    }
    return true;
}
static bool wn_tn_splits_fit(const WnGemmTnArgs& a, long long rps) {
    const long long a_cols = a.ka_split > 0 ? a.ka_split : a.Ka;
    for (long long m0 = 0; m0 < a.M; m0 += rps) {
        const long long m1 = m0 + rps < a.M ? m0 + rps : a.M;
        if (!a.a_idx && !wn_tn_map_fits(a.a, m0, m1, a.rows_per_batch, a_cols, a.a_bf16 ? 2 : 4)) return false;
        if (a.ka_split > 0 && !wn_tn_map_fits(a.a1, m0, m1, a.rows_per_batch, a.Ka - a.ka_split, a.a_bf16 ? 2 : 4)) return false;
        if (!wn_tn_map_fits(a.b, m0, m1, a.rows_per_batch, a.Nb, a.b_bf16 ? 2 : 4)) return false;
    }
    return true;
}
// More splits (rows per split a multiple of 32, as the planners make them) until every split fits its window; returns the rows per split.
static long long wn_tn_fit_window(const WnGemmTnArgs& a, long long rps) {
    long long splits = (a.M + rps - 1) / rps;
    while (rps > 32 && !wn_tn_splits_fit(a, rps)) {
        ++splits;
        const long long r = ((a.M + splits - 1) / splits + 31) / 32 * 32;
        if (r < rps) rps = r;
    }
    return rps;
}

static void wn_launch_tn(hipStream_t st, WnGemmTnArgs a, bool bf16 = false) {
    // bf16 products with Nb % 256 == 0 take the 128 x 256 tile (A streamed once per 256 columns of B); rows split by wn_tn_grid (wn_plan.h)
    const bool wide16 = bf16 && !a.a_idx && a.a_bf16 && a.b_bf16 && a.Nb % 256 == 0;   // (both operands stored as bf16: the filter/gate weight gradient on the shadow of x -- two tap views, ka_split > 0 --, the skip weight gradient on the shadow of dskip)
    const bool wide = wide16 || (bf16 && !a.a_idx && !a.a_bf16 && a.Nb % 256 == 0);
    // both operands stored as bf16 and 256-column multiples on both sides: 256 x 256 tiles, one workgroup per CU, three chunks in flight (wn_bwd_wfg_bf16,
    // round 6) -- the filter/gate weight gradient of a 128 / 128 layer on the shadow of x (one tile: both tap views) and the grouped skip weight gradient
    // on the shadow of dskip.  WN_NO_TALL_WFG=1 with WN_TESTING=1: the 128 x 256 tiles of rounds 3-5.
    // (Measured, one stream, stand-alone: the filter/gate gradient 145 -> 134 us per layer; the grouped skip gradient 855 -> 892 us in ten 256 x 256 tiles per
    //  row split -- it stays on the 128 x 256 tiles unless WN_TALL_SKIP=1 asks for it.  Step: 54.6 -> 54.2 ms.  profiles/r06_tn_loads.txt.)
    const bool tall_skip = wn_dev_flag("WN_TALL_SKIP");
    if (wide16 && !a.relu_a && a.Nb % 256 == 0 && ((a.ka_split == 128 && a.Ka == 256) || (a.ka_split == 0 && a.Ka % 256 == 0 && tall_skip))) {
        if (!wn_dev_flag("WN_NO_TALL_WFG")) {
            const int tiles = (a.Ka / 256) * (a.Nb / 256);
            int want_t = 256;   // workgroups in flight: one per CU
            { const char* wv = wn_dev_env("WN_TALL_WANT"); if (wv && atoi(wv) > 0) want_t = atoi(wv); }
            long long splits = want_t / tiles > 1 ? want_t / tiles : 1;
            if (splits >= 8) splits -= splits % 8;
            long long rps = (a.M + splits - 1) / splits;
            rps = wn_tn_fit_window(a, (rps + 31) / 32 * 32);
            splits = (a.M + rps - 1) / rps;
            a.rows_per_split = rps; a.tiles_ka = a.Ka / 256; a.n_splits = (int)splits;
            a.part = wn_det_part(st, (size_t)splits * a.Ka * a.Nb);
            hipLaunchKernelGGL(wn_bwd_wfg_bf16, dim3(8u * (unsigned)tiles * (unsigned)((splits + 7) / 8)), dim3(512), 0, st, a);
            if (a.part)
                hipLaunchKernelGGL(wn_tn_reduce, dim3((unsigned)(((long long)a.Ka * a.Nb / 4 + 255) / 256)), dim3(256), 0, st, a.part, (int)splits, a.Ka, a.Nb, a.c, a.ldc, a.c_trans);
            return;
        }
    }
    // How many workgroups share the rows (each adds its 128 x 128 / 128 x 256 partial tile with fp32 atomics).  The bf16 forms: 512 -- one full round of
    // the resident slots (two 512-thread or three 256-thread workgroups per CU), half the atomic traffic of round 4's 1024 for the 128-column form:
    // 57.6 -> 55.5 ms per config-5 step (384-640: level; 256: 55.6; the 256-column form at 256 / 384 / 768 / 1024: 60.5 / 55.1 / 56.6 / 60.0 against
    // 54.9 at 512; profiles/r05_training_step_byte_cuts.txt).  The fp32 kernel is matrix-pipe bound and wants the rows spread wider: 1024 (512: 179 -> 194 ms).
    int want = (wide || (bf16 && !a.a_idx)) ? 512 : 1024;
    { const char* wv = wn_dev_env(wide ? "WN_TN_WANT_WIDE" : "WN_TN_WANT"); if (wv && atoi(wv) > 0) want = atoi(wv); }   // (A/B runs, with WN_TESTING=1)
    WnTnGrid tg = wn_tn_grid(a.M, a.Ka, a.Nb, wide ? 256 : 128, want);
    { const long long rps = wn_tn_fit_window(a, tg.rows_per_split);
      if (rps != tg.rows_per_split) { tg.rows_per_split = rps; tg.splits = (int)((a.M + rps - 1) / rps); tg.blocks = 8u * (unsigned)(tg.tiles_ka * tg.tiles_nb) * (unsigned)((tg.splits + 7) / 8); } }
    a.rows_per_split = tg.rows_per_split;
    a.tiles_ka = tg.tiles_ka; a.n_splits = tg.splits;
    const dim3 grid(tg.blocks);   // wn_tile_of: the tiles of a row split share an XCD
    a.part = wn_det_part(st, (size_t)tg.splits * a.Ka * a.Nb);   // (NULL outside the deterministic mode: atomics)
    // (b_bf16 / a_bf16: that operand is stored as bf16 -- [dF|dG] in the filter/gate weight gradient, z in the residual and skip ones)
    if (wide16) hipLaunchKernelGGL((wn_bwd_gemm_tn_bf16<8, true, true>), grid, dim3(512), 0, st, a);
    else if (wide && a.b_bf16) hipLaunchKernelGGL((wn_bwd_gemm_tn_bf16<8, false, true>), grid, dim3(512), 0, st, a);
    else if (wide) hipLaunchKernelGGL((wn_bwd_gemm_tn_bf16<8, false, false>), grid, dim3(512), 0, st, a);
    else if (bf16 && !a.a_idx && a.b_bf16) hipLaunchKernelGGL((wn_bwd_gemm_tn_bf16<4, false, true>), grid, dim3(256), 0, st, a);
    else if (bf16 && !a.a_idx && a.a_bf16) hipLaunchKernelGGL((wn_bwd_gemm_tn_bf16<4, true, false>), grid, dim3(256), 0, st, a);
    else if (bf16 && !a.a_idx) hipLaunchKernelGGL((wn_bwd_gemm_tn_bf16<4, false, false>), grid, dim3(256), 0, st, a);  // bf16 matrix operands, fp32 accumulation
    else hipLaunchKernelGGL(wn_bwd_gemm_tn, grid, dim3(256), 0, st, a);
    if (a.part)
        hipLaunchKernelGGL(wn_tn_reduce, dim3((unsigned)(((long long)a.Ka * a.Nb / 4 + 255) / 256)), dim3(256), 0, st, a.part, tg.splits, a.Ka, a.Nb, a.c, a.ldc, a.c_trans);
}

static void wn_launch_colsum(hipStream_t st, const WnRowMap& x, long long M, int rows_per_batch, int N, float* out, bool x16 = false) {
    const unsigned blocks = (unsigned)((M + 511) / 512);
    float* part = (N % 4 == 0) ? wn_det_part(st, (size_t)blocks * N) : nullptr;
    if (x16) hipLaunchKernelGGL(wn_bwd_colsum<true>, dim3(blocks, (unsigned)((N + 63) / 64)), dim3(64), 0, st, x, M, rows_per_batch, N, out, part);
    else hipLaunchKernelGGL(wn_bwd_colsum<false>, dim3(blocks, (unsigned)((N + 63) / 64)), dim3(64), 0, st, x, M, rows_per_batch, N, out, part);
    if (part) hipLaunchKernelGGL(wn_tn_reduce, dim3((unsigned)((N / 4 + 255) / 256)), dim3(256), 0, st, part, (int)blocks, 1, N, out, N, 0);
}

static void wn_launch_transpose(hipStream_t st, const float* in, long long in_batch_stride, float* out, int rows, int cols, int batches) {
    hipLaunchKernelGGL(wn_transpose_batched, dim3((unsigned)((cols + 31) / 32), (unsigned)((rows + 31) / 32), (unsigned)batches), dim3(256), 0, st,
                       in, in_batch_stride, out, rows, cols);
}

// (Round 4 tried the side stream at the LOWEST queue priority -- the chain's workgroups first, the side work in what is left: 63.7 -> 70.5 ms
//  per bf16 config-5 step.  The side work is a third of the step's kernel time; starved, it is left over at the end.
//  profiles/r04_fused_forward_layer.txt.)
extern "C" int wn_train_forward(wn_handle* h, const float* params, const int32_t* indices, int64_t N, int64_t L, int64_t out_len,
                                float* logits, void* hip_stream) {
    g_err[0] = 0;
    if (!h || !params || !indices || !logits) return wn_fail(WN_E_BADARG, "wn_train_forward: NULL argument");
    if (!h->chains.empty()) return wn_train_forward(h->chains[0], params, indices, N, L, out_len, logits, hip_stream);
    if (!h->have_weights) return wn_fail(WN_E_STATE, "wn_train_forward: wn_load_weights has not been called");
    if (N < 1 || out_len < 1) return wn_fail(WN_E_BADARG, "wn_train_forward: N and output_length must be >= 1");
    const WnPlan& pl = h->plan;
    const int R = pl.R, D = pl.D, S = pl.S, E = pl.E, C = pl.C, NL = pl.NL;
    if (!h->w.train_ok) return wn_fail(WN_E_UNSUPPORTED, "wn_train_forward: needs kernel_size 2, 3 or 4 and channel counts that are multiples of 32");
    if (h->padded) return wn_fail(WN_E_UNSUPPORTED, "wn_train_forward: this handle runs a zero-padded channel shape (its parameter layout is not the caller's)");
    if ((long long)N * L >= 0x7fffffffll) return wn_fail(WN_E_UNSUPPORTED, "wn_train_forward: N*L must stay below 2^31 rows");
    { int rc = rt_hip(hipSetDevice(h->cfg.device_id), "hipSetDevice"); if (rc) return rc; }
    WnTrainLay& t = h->train;
    h->train_valid = false;
    hipStream_t st = (hipStream_t)hip_stream;
    WnTrainStreams ts(h, st);
    { int rc = wn_train_layout_ws(h, N, L, out_len, t); if (rc) return rc; }
    if (h->tws_floats < t.total) {
        (void)hipDeviceSynchronize();
        if (!rt_grow(h->d_tws, h->tws_floats, t.total)) return wn_fail(WN_E_NOMEM, "wn_train_forward: workspace of %.1f MB", t.total * 4e-6);
    }
    float* ws = h->d_tws;
    const float* fw = params;
    const wn_train_layout& o = h->w.fw;
    int rc = rt_hip(hipMemcpyAsync(ws + t.idx, indices, (size_t)N * L * 4, hipMemcpyDeviceToDevice, st), "hipMemcpyAsync(indices)");
    if (rc) return rc;
    // operand layouts of the backward products, rebuilt from the (just updated) parameters
    wn_launch_transpose(st, fw + o.res, (long long)D * R, ws + t.res_o, D, R, NL);      // [D][R] -> [R][D]
    for (int b = 0; b < t.nblk; ++b) {  // per block of G layers: [cnt*D][S] -> [S][cnt*D], the operand of the backward's grouped skip product
        const int first = b * t.G;
        wn_launch_transpose(st, fw + o.skip + (size_t)first * D * S, 0, ws + t.skip_o + (size_t)first * S * D, t.cnt(b) * D, S, 1);
    }
    wn_launch_transpose(st, fw + o.w1, 0, ws + t.w1_o, S, E, 1);                         // [S][E] -> [E][S]
    wn_launch_transpose(st, fw + o.w2, 0, ws + t.w2_o, E, C, 1);                         // [E][C] -> [C][E]
    for (int tap = 0; tap < pl.k; ++tap)   // tap j's rows of every layer -> [2D][R], block j of the workspace (fgb0, fgb1, ...)
        wn_launch_transpose(st, fw + o.fg + (size_t)tap * R * 2 * D, (long long)pl.k * R * 2 * D, ws + t.fgb0 + (size_t)tap * (t.fgb1 - t.fgb0), R, 2 * D, NL);
    const int G = t.G;
    const bool bf16 = h->fw_bf16 && h->w.fwb_ok;
    t.bf16 = bf16;
    auto h16 = [&](size_t off) { return reinterpret_cast<unsigned short*>(ws + off); };   // a bf16 bank of the workspace
    unsigned short *bw = h16(t.bw), *bt_fg = h16(t.bt_fg), *bt_res = h16(t.bt_res), *bt_skip = h16(t.bt_skip), *bt_w1 = h16(t.bt_w1), *bt_w2 = h16(t.bt_w2);
    if (bf16) {
        const long long n = (long long)h->w.fw_floats;
        hipLaunchKernelGGL(wn_cvt_bf16, dim3((unsigned)((n / 2 + 256) / 256)), dim3(256), 0, st, fw, bw, n);
        wn_launch_cvt_t(st, fw + o.fg, (long long)2 * R * 2 * D, bt_fg, 2 * R, 2 * D, NL);        // [2R][2D] -> [2D][2R]
        wn_launch_cvt_t(st, fw + o.res, (long long)D * R, bt_res, D, R, NL);                          // [D][R] -> [R][D]
        wn_launch_cvt_t(st, fw + o.skip, (long long)G * D * S, bt_skip, G * D, S, NL / G);            // [G*D][S] -> [S][G*D] per full block
        if (NL % G) {   // the last block is shorter when G does not divide NL (WN_TRAIN_SKIP_BLOCK): [cnt*D][S] -> [S][cnt*D] of its own
            const int first = NL - NL % G;
            wn_launch_cvt_t(st, fw + o.skip + (size_t)first * D * S, 0, bt_skip + (size_t)first * S * D, (NL % G) * D, S, 1);
        }
        wn_launch_cvt_t(st, fw + o.w1, 0, bt_w1, S, E, 1);
        wn_launch_cvt_t(st, fw + o.w2, 0, bt_w2, E, C, 1);
    }
    if (pl.has_bias) {  // the grouped skip GEMM adds the sum of all layers' skip biases once
        rc = rt_hip(hipMemsetAsync(ws + t.bskip_total, 0, (size_t)S * 4, st), "hipMemsetAsync");
        if (rc) return rc;
        wn_launch_colsum(st, WnRowMap{fw + o.bskip, 0, S, 0}, NL, NL, S, ws + t.bskip_total);
    }
    {
        const long long rows = N * L, work = rows * (R / 4);
        hipLaunchKernelGGL(wn_fwd_start, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, st, indices, fw + o.start_t,
                           pl.has_bias ? fw + o.start_b : nullptr, ws + t.x[0], rows, R,
                           (bf16 && !t.xh.empty()) ? reinterpret_cast<unsigned short*>(ws + t.xh[0]) : (unsigned short*)nullptr);
    }
    float* skip = ws + t.skip; float* ev = ws + t.ev;
    // The grouped skip product of a block (zg . [Wskip of its layers]: 1.2 ms at config 5) hangs off the layer chain -- the next block's
    // layers do not need it, only the head does: it runs on the side stream next to them (see wn_train_backward for the two-stream scheme).
    rc = ts.fork();
    if (rc) return rc;
    const hipStream_t sd = ts.sd;
    for (int l = 0; l < NL; ++l) {
        const long long d = h->dil[l], rows = t.need[l + 1], t0 = L - rows;
        const int gi = l % G;
        float* xin = ws + t.x[l];
        const WnRowMap zmap = wn_z_map(t, ws, D, l, bf16);   // z_l: a strided view of the block's Z_b (wn_train_layout_ws)
        const bool shadow = bf16 && !t.xh.empty();   // matrix operand reads of x take its bf16 shadow (wn_train_layout_ws)
        const float* xop = shadow ? ws + t.xh[l] : xin;   // (a bf16 matrix behind a float pointer: the row maps count bf16 elements then)
        // (z: no second copy on the skip rows: the grouped skip product reads those rows of Z_b where they lie)
        WnGemmArgs a = wn_layer_fg(pl, o, fw, l, wn_rows(xop, L, R, t0), d, zmap, N, rows);
        a.a_skip_lo[0] = (int)t.zlo[l];   // (short clips: the reference's left zero padding stands in for x(t - d) on these rows)
        a.a_bf16 = shadow ? 1 : 0;
        a.gate_t = ws + t.th[l]; a.gate_g = ws + t.sg[l];
        a.gate_packed = bf16 ? 1 : 0;  // bf16 step: tanh and sigmoid saved as one {bf16, bf16} dword per element (half the bytes, written once)
        a.c_bf16 = bf16 ? 1 : 0;       //            z (and its copy on the skip rows, zg) stored as bf16
        WnGemmArgs ar = {};   // the residual product x_{l+1} = z . Wres^T + bias + x_l
        if (l < NL - 1) {
            ar = wn_layer_res(pl, o, fw, l, zmap, wn_rows(xin, L, R, t0), wn_rows(ws + t.x[l + 1], L, R, t0), N, rows);
            if (shadow) ar.c_h = reinterpret_cast<unsigned short*>(ws + t.xh[l + 1]);
            ar.a_bf16 = bf16 ? 1 : 0;
        }
        // (bf16 step, the 128/128 shape: both products of the layer in one launch, z handed over in LDS -- wn_fwd_layer_bf16)
        const bool fused = bf16 && l < NL - 1 && wn_launch_layer(st, a, bt_fg + (size_t)l * 2 * D * 2 * R, ar, bt_res + (size_t)l * R * D);
        if (pl.k != 2) {   // kernel_size 3, 4 (fp32 operands): the k views of x are formed in the kernel; the same epilogue, gates saved, z into Z_b
            WnTapsArgs at = wn_layer_fg_taps(pl, o, fw, l, wn_rows(xin, L, R, t0), d, zmap, N, rows, 0);
            at.g.gate_t = a.gate_t; at.g.gate_g = a.gate_g;
            wn_launch_taps(st, pl.k, at);
            if (l < NL - 1) wn_launch_nn(st, WN_EPI_PLAIN, ar);
        } else if (!fused) {
            wn_launch_nn(st, WN_EPI_GATE, a, bf16 ? bt_fg + (size_t)l * 2 * D * 2 * R : nullptr);
            if (l < NL - 1) wn_launch_nn(st, WN_EPI_PLAIN, ar, bf16 ? bt_res + (size_t)l * R * D : nullptr);
        }
        if (gi == G - 1 || l == NL - 1) {
            const int first = l - gi, cnt = gi + 1;
            WnGemmArgs ak = wn_skip_group(pl, o, fw, first, cnt, wn_zg_map(t, ws, D, first / G), ws + t.bskip_total, skip, N, out_len);
            ak.a_bf16 = bf16 ? 1 : 0;
            ts.wait_for(sd, ts.signal(st));   // the block's Z_b is complete (every gate product of the block ran on the caller's stream)
            wn_launch_nn(sd, WN_EPI_PLAIN, ak, bf16 ? bt_skip + (size_t)(first / G) * S * G * D : nullptr);
        }
    }
    ts.wait_for(st, ts.signal(sd));   // skip is complete
    const WnHeadArgs hd = wn_head(pl, o, fw, skip, ev, logits, N, out_len);
    wn_launch_nn(st, WN_EPI_PLAIN, hd.e, bf16 ? bt_w1 : nullptr);
    wn_launch_nn(st, WN_EPI_PLAIN, hd.logits, bf16 ? bt_w2 : nullptr);
    rc = rt_hip(hipGetLastError(), "wn_train_forward launches");
    if (rc) return rc;
    h->train_valid = true;
    return WN_OK;
}

extern "C" int wn_train_backward(wn_handle* h, const float* params, const float* dlogits, float* grads, void* hip_stream) {
    g_err[0] = 0;
    if (!h || !params || !dlogits || !grads) return wn_fail(WN_E_BADARG, "wn_train_backward: NULL argument");
    if (!h->chains.empty()) return wn_train_backward(h->chains[0], params, dlogits, grads, hip_stream);
    if (!h->train_valid) return wn_fail(WN_E_STATE, "wn_train_backward: no wn_train_forward to differentiate");
    { int rc = rt_hip(hipSetDevice(h->cfg.device_id), "hipSetDevice"); if (rc) return rc; }
    const WnPlan& pl = h->plan;
    const int R = pl.R, D = pl.D, S = pl.S, E = pl.E, C = pl.C, NL = pl.NL;
    const WnTrainLay& t = h->train;
    const wn_train_layout& o = h->w.fw;
    hipStream_t st = (hipStream_t)hip_stream;
    WnTrainStreams ts(h, st);
    const long long N = t.N, L = t.L, out_len = t.out_len, Mo = N * out_len;
    float* ws = h->d_tws;
    (void)params;  // the operand layouts of this step's parameters were rebuilt by wn_train_forward
    int rc = rt_hip(hipMemsetAsync(grads, 0, h->w.fw_floats * 4, st), "hipMemsetAsync(grads)");
    if (rc) return rc;
    float* dskip = ws + t.dskip; float* de = ws + t.de;
    // Two streams.  The activation-gradient chain (dz -> [dF|dG] -> dx, layer after layer) is strictly sequential; the weight-gradient
    // products only hang off it (dWres needs dx', dWfg needs [dF|dG], the grouped dWskip needs dskip) and nobody waits for them before
    // the optimizer.  They run on a side stream, ordered by events: every product of the chain then has a second, independent kernel
    // next to it that fills its tail (a 128-row-tile product of 3250 workgroups leaves the last of its four waves of workgroups 17 % full)
    // and uses the memory system while the other one computes.  [dF|dG] is double buffered (layer l writes buffer l & 1): the side
    // stream may still read layer l's while the chain writes layer l-1's; the chain waits for the side stream only where it would
    // overwrite something the side stream has not read yet (dx ping-pong buffer: dWres of layer l before dx of layer l-1; [dF|dG]
    // buffer: dWfg of layer l before the gate derivative of layer l-2).  WN_TRAIN_ONE_STREAM=1 (with WN_TESTING=1) keeps everything on
    // the caller's stream (A/B runs).
    rc = ts.fork();
    if (rc) return rc;
    const hipStream_t sd = ts.sd;
    std::vector<hipEvent_t> res_read(NL, nullptr), fg_read(NL, nullptr);   // side stream: dWres / dWfg of layer l have read their operands
    // bf16 mode: the "NN" products take their weight operand ([N][K] bf16) straight from the bf16 copy of the parameter blob
    const unsigned short* bw = t.bf16 ? reinterpret_cast<const unsigned short*>(ws + t.bw) : nullptr;
    const float* skip = ws + t.skip; const float* ev = ws + t.ev;
    const WnRowMap dlg_map = wn_rows(dlogits, out_len, C), ev_map = wn_rows(ev, out_len, E), de_map = wn_rows(de, out_len, E), skip_map = wn_rows(skip, out_len, S),
                   dskip_map = wn_rows(dskip, out_len, S);
    // ---- head.  Only de and dskip are on the way to the layers; the head's own weight and bias gradients (two products over the rows, three column sums:
    // 0.7 ms at config 5) hang off them like every other weight gradient and run on the side stream, behind the first dzg product the chain waits for
    // (round 4 ran them on the caller's stream in front of dskip).
    auto head_weight_grads = [&](hipStream_t s2) -> int {
        wn_launch_tn(s2, wn_tn(ev_map, E, dlg_map, C, grads + o.w2, C, Mo, out_len), t.bf16);   // dW2^T [E][C] = e^T . dlogits
        wn_launch_colsum(s2, dlg_map, Mo, (int)out_len, C, grads + o.b2);
        WnGemmTnArgs g1 = wn_tn(skip_map, S, de_map, E, grads + o.w1, E, Mo, out_len);   // dW1^T [S][E] = relu(skip)^T . de
        g1.relu_a = 1;
        wn_launch_tn(s2, g1, t.bf16);
        wn_launch_colsum(s2, de_map, Mo, (int)out_len, E, grads + o.b1);
        if (pl.has_bias) {          // every layer's skip bias sees the same gradient
            int rc2 = rt_hip(hipMemsetAsync(ws + t.colsum_tmp, 0, (size_t)S * 4, s2), "hipMemsetAsync");
            if (rc2) return rc2;
            wn_launch_colsum(s2, dskip_map, Mo, (int)out_len, S, ws + t.colsum_tmp);
            for (int l = 0; l < NL; ++l) {
                rc2 = rt_hip(hipMemcpyAsync(grads + o.bskip + (size_t)l * S, ws + t.colsum_tmp, (size_t)S * 4, hipMemcpyDeviceToDevice, s2), "hipMemcpyAsync(dbskip)");
                if (rc2) return rc2;
            }
        }
        return 0;
    };
    {
        WnGemmArgs a = wn_nn(dlg_map, C, ws + t.w2_o, E, nullptr, de_map, Mo, out_len);   // de = (dlogits . W2) * [e > 0]
        a.mask = ev;
        wn_launch_nn(st, WN_EPI_PLAIN, a, bw ? bw + o.w2 : nullptr);
    }
    // bf16 step: dskip is a matrix operand twice per skip block (the dzg product's A, the skip weight gradient's) and an fp32 column sum once (the
    // skip biases): the product also writes the bits those operand reads would round it to (as x has its shadow), they take half the bytes
    unsigned short* dskip_h = t.bf16 ? reinterpret_cast<unsigned short*>(ws + t.dskip_h) : nullptr;
    if (wn_dev_flag("WN_NO_DSKIP_SHADOW")) dskip_h = nullptr;   // (A/B runs, with WN_TESTING=1)
    {
        WnGemmArgs a = wn_nn(de_map, E, ws + t.w1_o, S, nullptr, dskip_map, Mo, out_len);   // dskip = (de . W1) * [skip > 0]
        a.mask = skip; a.c_h = dskip_h;
        wn_launch_nn(st, WN_EPI_PLAIN, a, bw ? bw + o.w1 : nullptr);
    }
    ts.wait_for(sd, ts.signal(st));   // grads cleared, de and dskip complete: the side stream may start
    // The skip path's gradients, one block of G layers at a time (as in the forward):
    //   dzg_b [Mo][cnt*D] = dskip . [Wskip of the block's layers]      dWskip^T of the block [cnt*D][S] = zg^T . dskip
    // so dskip (0.7 GB at config 5) is read twice per block instead of twice per layer; the gate step of a layer adds its column block of
    // dzg_b to dz on the skip rows.  Both products only need dskip: all blocks are enqueued NOW on the side stream, last block first --
    // the chain waits 1.2 ms for the last block's dzg (as it always did) and finds the others ready (one dzg buffer per block).
    std::vector<hipEvent_t> dzg_ready(t.nblk, nullptr);
    // bf16 step: dzg is STORED as bf16 (wn_gemm_epilogue, wn_forward.h) -- element (block b, row, column) of the buffer, as a float pointer the row maps carry
    const bool dzg16 = t.bf16;
    auto dzg_at = [&](int b, size_t col) -> float* {
        const size_t e = (size_t)b * ((size_t)Mo * t.G * D) + col;
        return dzg16 ? reinterpret_cast<float*>(reinterpret_cast<unsigned short*>(ws + t.dzg) + e) : ws + t.dzg + e;
    };
    // dWskip^T of block b.  Nobody waits for it before the optimizer, so it can run on either stream.  Round 6 (profiles/r06_train_timeline.txt): the
    // caller's stream sits idle ~190 us in front of every layer of the chain, waiting for the side stream to have read its double-buffered [dF|dG] / dx
    // buffers (side stream: 30 ms of products per backward, chain: 22 ms) -- but SOME kernel runs 97 % of the time, and moving products to the caller's
    // stream (WN_TRAIN_SKIP_MAIN=1: the five dWskip behind each block of the chain; WN_TRAIN_RES_MAIN=k: every k-th layer's dWres; both with
    // WN_TESTING=1) bought nothing (54.6 -> 54.5-57.4 ms): the step is bound by the bytes its kernels move, not by the queue they wait in.  Default: all on
    // the side stream, as in rounds 4-5.
    const bool skip_main = wn_dev_flag("WN_TRAIN_SKIP_MAIN") && ts.two;   // (measured: no gain -- profiles/r06_train_timeline.txt; default off)
    const char* rsm_env = wn_dev_env("WN_TRAIN_RES_MAIN");
    const int res_main = ts.two && rsm_env ? atoi(rsm_env) : 0;
    auto skip_weight_grads = [&](hipStream_t s2, int b) {
        const int first = b * t.G, cnt = t.cnt(b);
        // (the block's z on the skip rows, where the forward left it)
        WnGemmTnArgs gs = wn_tn(wn_zg_map(t, ws, D, b), cnt * D, dskip_map, S, grads + o.skip + (size_t)first * D * S, S, Mo, out_len);
        if (t.bf16) {   // zg is stored as bf16: it goes in as B (operands swapped, C written transposed -- same [cnt*D][S] gradient)
            WnRowMap zmap = gs.a; gs.a = gs.b; gs.b = zmap; gs.Ka = S; gs.Nb = cnt * D; gs.b_bf16 = 1; gs.c_trans = 1;
            if (dskip_h && (cnt * D) % 256 == 0) { gs.a = wn_rows(reinterpret_cast<const float*>(dskip_h), out_len, S); gs.a_bf16 = 1; }   // (the 256-column tile has the form with both operands stored as bf16)
        }
        wn_launch_tn(s2, gs, t.bf16);
    };
    for (int b = t.nblk - 1; b >= 0; --b) {
        const int first = b * t.G, cnt = t.cnt(b);
        // dzg_b = dskip . [Wskip of the block's layers]; A from dskip's bf16 shadow where there is one (the same bits, half the bytes)
        WnGemmArgs a = wn_nn(dskip_h ? wn_rows(reinterpret_cast<const float*>(dskip_h), out_len, S) : dskip_map, S, ws + t.skip_o + (size_t)first * S * D, cnt * D, nullptr,
                             wn_rows(dzg_at(b, 0), out_len, (long long)cnt * D), Mo, out_len);
        a.a_bf16 = dskip_h ? 1 : 0; a.c_bf16 = dzg16 ? 1 : 0;
        wn_launch_nn(sd, WN_EPI_PLAIN, a, bw ? bw + o.skip + (size_t)first * D * S : nullptr);
        if (ts.two) dzg_ready[b] = ts.signal(sd);
        if (b == t.nblk - 1) { rc = head_weight_grads(sd); if (rc) return rc; }   // (behind the one product the chain is waiting for)
        if (!skip_main) skip_weight_grads(sd, b);
    }
    // ---- layers, last to first
    float* dxn = ws + t.dxa;  // dLoss/dx_{l+1}
    float* dxc = ws + t.dxb;  // dLoss/dx_l
    // The arguments of layer k's gate-derivative product dz = dx' . Wres -> [dF | dG] (+ the layer's share of dzg on the skip rows): the
    // gate derivative is the product's epilogue (WN_EPI_GATE_BWD), dz is never written (round 2: dz to HBM, then a streaming gate kernel).
    auto gate_bwd_args = [&](int k, const float* dx_in) {
        const long long rows_k = t.need[k + 1];
        const int cnt_k = t.cnt(k / t.G);
        // bf16 step: [dF|dG] is STORED as bf16 (it only ever feeds bf16 matrix operands)
        WnGemmArgs g = wn_nn(wn_rows(dx_in, L, R, L - rows_k), R, ws + t.res_o + (size_t)k * R * D, D, nullptr, wn_rows(ws + ((k & 1) ? t.dfg2 : t.dfg), rows_k, 2 * D),
                             N * rows_k, rows_k);
        g.c_bf16 = t.bf16 ? 1 : 0;
        g.c2 = wn_rows(dzg_at(k / t.G, (size_t)(k % t.G) * D), out_len, (long long)cnt_k * D);   // (bf16 step: bf16 elements)
        g.c2_first_row = (int)(rows_k - out_len);
        g.gate_t = ws + t.th[k]; g.gate_g = ws + t.sg[k]; g.gate_packed = t.bf16 ? 1 : 0;
        return g;
    };
    // what the chain has to wait for before it may write layer k's [dF|dG]: the buffer's previous reader (dWfg of layer k + 2, side stream)
    // and -- entering a block from above -- the block's dzg (side stream, enqueued before the loop)
    auto gate_bwd_waits = [&](int k) {
        if (k + 2 < NL) ts.wait_for(st, fg_read[k + 2]);
        if (k % t.G == t.cnt(k / t.G) - 1) ts.wait_for(st, dzg_ready[k / t.G]);
    };
    bool have_dfg = false;   // [dF|dG] of the layer at hand came out of the previous iteration's fused launch (wn_bwd_layer_bf16)
    for (int l = NL - 1; l >= 0; --l) {
        const long long d = h->dil[l], rows = t.need[l + 1], t0 = L - rows, M = N * rows;
        const float* xin = ws + t.x[l];
        const bool has_res = l < NL - 1;
        float* dfg = ws + ((l & 1) ? t.dfg2 : t.dfg);
        const int gi = l % t.G, cnt = t.cnt(l / t.G);
        if (!have_dfg) gate_bwd_waits(l);
        if (has_res) {
            if (!have_dfg) wn_launch_nn(st, WN_EPI_GATE_BWD, gate_bwd_args(l, dxn), bw ? bw + o.res + (size_t)l * D * R : nullptr);
            WnGemmTnArgs g = wn_tn(wn_z_map(t, ws, D, l, t.bf16), D, wn_rows(dxn, L, R, t0), R, grads + o.res + (size_t)l * D * R, R, M, rows);   // dWres^T [D][R] = z^T . dx'
            g.a_bf16 = t.bf16 ? 1 : 0;   // z is stored as bf16 in the bf16 step (here as A: ~1000 row splits, see wn_bwd_gemm_tn_bf16)
            const bool res_here = res_main > 0 && l % res_main == 0;   // (this layer's dWres on the caller's stream: in order behind dx', no event)
            hipStream_t sr = res_here ? st : sd;
            wn_launch_tn(sr, g, t.bf16);   // (dx' is complete: the side stream waited for the dx product of layer l + 1, below)
            if (pl.has_bias) wn_launch_colsum(sr, wn_rows(dxn, L, R, t0), M, (int)rows, R, grads + o.bres + (size_t)l * R);
            if (ts.two && !res_here) res_read[l] = ts.signal(sd);
        } else {   // the last layer has no residual output: dz is its share of dzg alone
            const long long work = M * D / 4;   // (four channels per thread; no residual share: dz = NULL, nothing zero-filled)
            const float* no_dz = nullptr;
            hipLaunchKernelGGL(t.bf16 ? wn_bwd_gate<true> : wn_bwd_gate<false>, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, st, no_dz, ws + t.th[l], ws + t.sg[l], dfg,
                               M, D, dzg_at(l / t.G, (size_t)gi * D), cnt * D, (int)rows, (int)out_len);
        }
        ts.wait_for(sd, ts.signal(st));   // [dF|dG] of this layer is complete
        // dWfg^T [2R][2D]: rows 0..R-1 = x_l(t - d)^T . dfg (tap 0), rows R.. = x_l(t)^T . dfg (tap 1) -- one launch, the taps are two
        // row views of A (ka_split): the workgroups of the two taps run side by side and read the same rows of dfg (worth 5 ms of the round-3 step against a
        // launch per tap: profiles/archive/r03_train_step_gate_epilogue_merged_taps.txt; shapes whose R is no multiple of the tile keep the two launches).
        const bool shadow = t.bf16 && !t.xh.empty();   // (the bf16 shadow of x: both operands of this product are stored as bf16 then)
        const float* xop = shadow ? ws + t.xh[l] : xin;
        const WnRowMap dfg_map = wn_rows(dfg, rows, 2 * D);
        WnGemmTnArgs g = wn_tn(wn_rows(xop, L, R, t0 - d), 2 * R, dfg_map, 2 * D, grads + o.fg + (size_t)l * 2 * R * 2 * D, 2 * D, M, rows);
        g.a1 = wn_rows(xop, L, R, t0); g.ka_split = R;
        g.a_bf16 = shadow ? 1 : 0; g.b_bf16 = t.bf16 ? 1 : 0;
        g.a_skip_lo = (int)t.zlo[l];   // tap 0 on the rows where the forward read a pad zero: no contribution
        if (pl.k != 2) {   // kernel_size 3, 4: one single-view product per tap -- view x_l(t - (k-1-j) d), rows j R .. of the gradient (every tap exists: wn_train_layout_ws)
            for (int tap = 0; tap < pl.k; ++tap) {
                WnGemmTnArgs g1 = wn_tn(wn_rows(xin, L, R, t0 - (long long)(pl.k - 1 - tap) * d), R, dfg_map, 2 * D,
                                        grads + o.fg + ((size_t)l * pl.k + tap) * R * 2 * D, 2 * D, M, rows);
                wn_launch_tn(sd, g1, false);
            }
        } else if (R % 128 == 0) {
            wn_launch_tn(sd, g, t.bf16);
        } else
        for (int tap = 0; tap < 2; ++tap) {
            WnGemmTnArgs g1 = g;
            g1.a = tap ? g.a1 : g.a; g1.ka_split = 0; g1.Ka = R; g1.c = g.c + (size_t)tap * R * 2 * D;
            if (tap) g1.a_skip_lo = 0;
            wn_launch_tn(sd, g1, t.bf16);
        }
        if (pl.has_bias) wn_launch_colsum(sd, dfg_map, M, (int)rows, 2 * D, grads + o.bfg + (size_t)l * 2 * D, t.bf16);
        if (ts.two) fg_read[l] = ts.signal(sd);
        // dx_l on ITS rows [lo, L) (the last need[l] time steps; lo = t0 - sh with sh = d, or less where the clip is so short that layer
        // l's input starts later than t0 - d) in ONE product over two row-shifted views of dfg:
        //     dx_l(t) = dx'(t) [t >= t0]  +  dfg(t) . Wfg(tap 1) [t >= t0]  +  dfg(t + d) . Wfg(tap 0) [t < L - d]
        // K = 4D: columns 0..2D-1 take dfg(t) against tap 1's rows, columns 2D.. take dfg(t + d) against tap 0's.  The views' row
        // windows (a_skip_*) read as zero where a shift runs off dfg, so nothing is cleared first and dx_l is written exactly once
        // (round 2: a memset of dx and two read-modify-write products per layer).  (Positions before lo do not exist: what the forward
        // read there were the reference's pad zeros, which have no gradient.)
        const long long rows_l = t.need[l], sh = rows_l - rows;   // 0 <= sh <= d
        if (l + 1 < NL) ts.wait_for(st, res_read[l + 1]);   // (dx_l goes into the buffer dWres of layer l + 1 read dx_{l+2} from)
        // a0 = dfg(t): row (t - t0) = rem - sh, valid from rem = sh;  a1 = dfg(t + d): row rem + d - sh, valid while rem < rows_l - d
        WnGemmArgs a = wn_nn2(wn_rows(dfg, rows, 2 * D, -sh), wn_rows(dfg, rows, 2 * D, d - sh), 2 * D, 4 * D, ws + t.fgb1 + (size_t)l * 2 * D * R, R, nullptr,
                              wn_rows(dxc, L, R, t0 - sh), N * rows_l, rows_l);
        a.a_skip_lo[0] = (int)sh; a.a_skip_hi[1] = (int)d; a.a_bf16 = t.bf16 ? 1 : 0;
        a.bt1 = ws + t.fgb0 + (size_t)l * 2 * D * R;
        if (has_res) { a.cin = wn_rows(dxn, L, R, t0 - sh); a.cin_skip_lo = (int)sh; }
        if (pl.k != 2) {   // kernel_size 3, 4: the k forward-shifted views of dfg against the k transposed tap blocks, one launch (wn_bwd_gemm_taps)
            wn_launch_taps_bwd(st, pl.k, wn_layer_dx_taps(pl, dfg, rows, rows_l, d, ws + t.fgb0 + (size_t)l * 2 * D * R, (long long)(t.fgb1 - t.fgb0),
                                                          has_res ? wn_rows(dxn, L, R, t0 - sh) : WnRowMap{nullptr, 0, 0, 0}, wn_rows(dxc, L, R, t0 - sh), N));
            have_dfg = false;
        } else {
            const unsigned short* w = bw ? bw + o.fg + (size_t)l * 2 * R * 2 * D : nullptr;  // native [2R][2D]: rows 0..R-1 tap 0, R.. tap 1
            // bf16 step, the 128 / 128 shape: this product and layer l - 1's gate-derivative product (same rows, dx_l as its A operand) are
            // ONE launch -- dx_l is handed over in LDS (wn_bwd_layer_bf16).  Layer l - 1's waits move in front of it.
            have_dfg = false;
            if (t.bf16 && l >= 1 && w) {
                const WnGemmArgs ag = gate_bwd_args(l - 1, dxc);
                if (ag.M == a.M && ag.a0.t0 == a.c.t0 && R == 128 && D == 128 && wn_fused_layer_enabled()) {
                    gate_bwd_waits(l - 1);
                    have_dfg = wn_launch_bwd_layer(st, a, w + (size_t)R * 2 * D, w, 2 * D, ag, bw + o.res + (size_t)(l - 1) * D * R);
                }
            }
            if (!have_dfg) wn_launch_nn(st, WN_EPI_PLAIN, a, w ? w + (size_t)R * 2 * D : nullptr, w, 2 * D);
        }
        ts.wait_for(sd, ts.signal(st));   // dx_l is complete: dWres of layer l - 1 may read it (fused: [dF|dG] of layer l - 1 as well)
        if (skip_main && gi == 0) skip_weight_grads(st, l / t.G);   // (the chain has left block l / G: its skip weight gradient behind it, on this stream)
        float* tmp = dxn; dxn = dxc; dxc = tmp;
    }
    // ---- start_conv: dstart^T [C][R] = onehot(indices)^T . dx_0 over the rows dx_0 exists on (the last need[0] time steps) -- in FRONT of the join: it
    // only needs dx_0, and runs next to what the side stream still has to do (the first layer's weight gradients)
    {
        const long long r0 = t.need[0], f0 = L - r0;
        WnGemmTnArgs g = wn_tn(WnRowMap{nullptr, L, 1, f0}, C, wn_rows(dxn, L, R, f0), R, grads + o.start_t, R, N * r0, r0);
        g.a_idx = reinterpret_cast<const int32_t*>(ws + t.idx);
        wn_launch_tn(st, g, t.bf16);
        if (pl.has_bias) wn_launch_colsum(st, wn_rows(dxn, L, R, f0), N * r0, (int)r0, R, grads + o.start_b);
    }
    ts.wait_for(st, ts.signal(sd));   // join: every weight gradient is complete before the caller's stream goes on
    return rt_hip(hipGetLastError(), "wn_train_backward launches");
}

extern "C" int wn_train_loss(wn_handle* h, const float* logits, const int64_t* targets, int64_t M, float* loss, float* dlogits, void* hip_stream) {
    g_err[0] = 0;
    if (!h || !logits || !targets || !loss) return wn_fail(WN_E_BADARG, "wn_train_loss: NULL argument");
    if (!h->chains.empty()) return wn_train_loss(h->chains[0], logits, targets, M, loss, dlogits, hip_stream);
    if (M < 1) return wn_fail(WN_E_BADARG, "wn_train_loss: M must be >= 1");
    if (h->plan.C != 256) return wn_fail(WN_E_UNSUPPORTED, "wn_train_loss: classes = %d (the fused loss is written for 256)", h->plan.C);
    { int rc = rt_hip(hipSetDevice(h->cfg.device_id), "hipSetDevice"); if (rc) return rc; }
    if (h->xent_rows < (size_t)M) {
        (void)hipDeviceSynchronize();
        if (!rt_grow(h->d_xent, h->xent_rows, (size_t)M)) return wn_fail(WN_E_NOMEM, "wn_train_loss: %lld row losses", (long long)M);
    }
    hipStream_t st = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(wn_xent_rows, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, logits, reinterpret_cast<const long long*>(targets), (long long)M,
                       (float)(1.0 / (double)M), h->d_xent, dlogits);
    hipLaunchKernelGGL(wn_xent_reduce, dim3(1), dim3(1024), 0, st, h->d_xent, (long long)M, 1.0 / (double)M, loss);
    return rt_hip(hipGetLastError(), "wn_train_loss launches");
}
