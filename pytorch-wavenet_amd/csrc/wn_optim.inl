// wn_optim.inl -- host side of the fused Adam step (included by wn_runtime.hip; GPU build only; kernels: wn_optim.h).

extern "C" int wn_adam_step(const wn_adam_args* a) {
    g_err[0] = 0;
    if (!a || a->n_tensors < 0 || (a->n_tensors > 0 && (!a->sizes || !a->params || !a->grads || !a->exp_avg || !a->exp_avg_sq)) || !a->scratch)
        return wn_fail(WN_E_BADARG, "wn_adam_step: NULL argument");
    if (a->step < 1 || !(a->beta1 >= 0. && a->beta1 < 1.) || !(a->beta2 >= 0. && a->beta2 < 1.) || !(a->eps >= 0.))
        return wn_fail(WN_E_BADARG, "wn_adam_step: step must be >= 1, betas in [0, 1), eps >= 0");
    if (a->flags & ~(int64_t)(WN_ADAM_NORM_ONLY | WN_ADAM_NORM_KEEP | WN_ADAM_NORM_GIVEN)) return wn_fail(WN_E_BADARG, "wn_adam_step: unknown flags");
    if ((a->flags & WN_ADAM_NORM_ONLY) && (a->flags & WN_ADAM_NORM_GIVEN)) return wn_fail(WN_E_BADARG, "wn_adam_step: NORM_ONLY and NORM_GIVEN exclude each other");
    // (no handle: the caller's current device is left as it was -- torch's current device is process state the parameters' device must not change)
    struct DeviceGuard {
        int prev = -1;
        ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    } guard;
    { int cur = -1; if (hipGetDevice(&cur) == hipSuccess && cur != a->device_id) guard.prev = cur; else (void)hipGetLastError(); }
    { int rc = rt_hip(hipSetDevice(a->device_id), "hipSetDevice"); if (rc) return rc; }
    hipStream_t st = (hipStream_t)a->hip_stream;
    const bool norm_only = (a->flags & WN_ADAM_NORM_ONLY) != 0;
    const bool clip = a->max_grad_norm > 0. || norm_only;
    double* acc = static_cast<double*>(a->scratch);
    WnAdamScalars k;   // every fp32 scalar is the double torch forms in Python, rounded once (torch/optim/adam.py: _multi_tensor_adam)
    const double bc1 = 1.0 - pow(a->beta1, (double)a->step), bc2 = 1.0 - pow(a->beta2, (double)a->step);
    k.neg_step = (float)(-(a->lr / bc1)); k.sqrt_bc2 = (float)sqrt(bc2);
    k.one_minus_b1 = (float)(1.0 - a->beta1); k.b2 = (float)a->beta2; k.one_minus_b2 = (float)(1.0 - a->beta2); k.eps = (float)a->eps;
    k.weight_decay = (float)a->weight_decay; k.max_norm = (clip && !norm_only) ? (float)a->max_grad_norm : 0.f;
    k.lerp_hi = k.one_minus_b1 >= 0.5f ? 1 : 0;
    // batches of up to WN_OPT_TENSORS tensors (skipping the ones without a gradient: torch's optimisers do)
    std::vector<WnOptBatch> batches;
    WnOptBatch b;
    memset(&b, 0, sizeof(b));
    auto flush = [&]() { if (b.n > 0) { batches.push_back(b); memset(&b, 0, sizeof(b)); } };
    for (int i = 0; i < a->n_tensors; ++i) {
        if (!a->grads[i] || a->sizes[i] <= 0) continue;
        if (!a->params[i] || !a->exp_avg[i] || !a->exp_avg_sq[i]) return wn_fail(WN_E_BADARG, "wn_adam_step: tensor %d has a gradient but no parameter / state pointer", i);
        const long long chunks = (a->sizes[i] + WN_OPT_CHUNK - 1) / WN_OPT_CHUNK;
        if (b.n == WN_OPT_TENSORS || (long long)b.chunk0[b.n] + chunks > 0x3fffffffll) flush();
        b.p[b.n] = static_cast<float*>(a->params[i]); b.g[b.n] = static_cast<float*>(a->grads[i]);
        b.m[b.n] = static_cast<float*>(a->exp_avg[i]); b.v[b.n] = static_cast<float*>(a->exp_avg_sq[i]);
        b.size[b.n] = a->sizes[i];
        b.chunk0[b.n + 1] = b.chunk0[b.n] + (int)chunks;
        b.n++;
    }
    flush();
    // The norm of a clipped step is the norm of ALL gradients that are clipped together (clip_grad_norm_(model.parameters())): a caller with several
    // parameter groups first adds every group's sum of squares into `scratch` (NORM_ONLY; NORM_KEEP from the second group on), then steps each group on
    // the total (NORM_GIVEN).  One group: one call, no flags.
    if (clip && !(a->flags & WN_ADAM_NORM_GIVEN)) {
        if (!(a->flags & WN_ADAM_NORM_KEEP)) {
            int rc = rt_hip(hipMemsetAsync(acc, 0, sizeof(double), st), "hipMemsetAsync(norm)");
            if (rc) return rc;
        }
        for (const WnOptBatch& bb : batches) hipLaunchKernelGGL(wn_opt_sumsq, dim3((unsigned)bb.chunk0[bb.n]), dim3(256), 0, st, bb, acc);
    }
    if (norm_only) return rt_hip(hipGetLastError(), "wn_adam_step launches");
    for (const WnOptBatch& bb : batches)
        hipLaunchKernelGGL(wn_opt_adam, dim3((unsigned)bb.chunk0[bb.n]), dim3(256), 0, st, bb, k, clip ? acc : nullptr, clip ? a->total_norm : nullptr);
    return rt_hip(hipGetLastError(), "wn_adam_step launches");
}
