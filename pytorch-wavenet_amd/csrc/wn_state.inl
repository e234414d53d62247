// wn_state.inl -- a stream's generation state as data (included by wn_runtime.hip; GPU build only): the canonical, time-free form of the dilation
// queues, the two kernels that move it out of and into the rings, and wn_state_floats / wn_state_save / wn_state_load (include/wn_abi.h).
//
// Canonical form: for the layers l = 0 .. NL-1 in order a block of ML_l x R_own fp32, ML_l = (k-1) d_l + 1, R_own = the caller's residual channels.  Row j
// of a block is the layer's input at time t - ML_l + j (t = the handle's queue time): row 0 the oldest, the last row the newest, rows of negative times
// the zeros of wn_reset.  On a handle at time t that row lives in ring slot (t + j) mod ML_l -- the slot rule of the kernels, slot of x[t'] = t' mod ML.
// The form knows nothing of queue time, layer split (the P identical copies), padding, kernel variant or rounds.

// What both kernels need to find a row: the handle's ring table, the canonical ROW offsets (row_off[l] = sum of ML below l, row_off[NL] = all rows; in
// rows, so that one table serves the padded and the caller's channel count) and the dilations.
struct WnStateGeom {
    const int64_t* ring_off;   // [NL] floats: first float of layer l's rings ([P][n_streams][ML][R])
    const int64_t* row_off;    // [NL + 1] canonical rows
    const int32_t* dil;        // [NL]
    int NL, k, R, R_own, n_streams, P;
};

__device__ __forceinline__ int wn_state_layer(const WnStateGeom& g, long long row) {   // the layer whose block holds canonical row `row`
    int lo = 0, hi = g.NL - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (g.row_off[mid] <= row) lo = mid; else hi = mid - 1; }
    return lo;
}

// state <- copy 0 of stream `stream`'s rings, un-rotated by the queue time t; the caller's channels only.  One thread per float4 (VEC: R and R_own
// multiples of 4) or per float of the canonical form, all layers in one launch.
template <bool VEC>
__global__ __launch_bounds__(256) void wn_state_gather(WnStateGeom g, const float* rings, long long t, int stream, float* state) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int W = VEC ? g.R_own / 4 : g.R_own;
    if (i >= g.row_off[g.NL] * W) return;
    const long long row = i / W;
    const int q = (int)(i % W);
    const int l = wn_state_layer(g, row);
    const long long ML = (long long)(g.k - 1) * g.dil[l] + 1, j = row - g.row_off[l];
    const float* src = rings + g.ring_off[l] + ((long long)stream * ML + (t + j) % ML) * g.R;
    float* dst = state + row * g.R_own;
    if (VEC) *reinterpret_cast<float4*>(dst + 4 * q) = *reinterpret_cast<const float4*>(src + 4 * q);
    else dst[q] = src[q];
}

// every copy of the rings of the streams s0 .. s0 + count - 1 <- ONE state, rotated to the queue time t; the channels beyond R_own get zeros.  Every
// slot of those streams is written (a block holds ML rows), nothing else is.  One thread per float4 / float of a ring row, the P copies in a loop.
template <bool VEC>
__global__ __launch_bounds__(256) void wn_state_scatter(WnStateGeom g, float* rings, long long t, int s0, int count, const float* state) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int W = VEC ? g.R / 4 : g.R;
    const long long per_stream = g.row_off[g.NL] * W;
    if (i >= per_stream * count) return;
    const int s = s0 + (int)(i / per_stream);
    const long long rem = i % per_stream, row = rem / W;
    const int q = (int)(rem % W);
    const int l = wn_state_layer(g, row);
    const long long ML = (long long)(g.k - 1) * g.dil[l] + 1, j = row - g.row_off[l], slot = (t + j) % ML;
    const float* src = state + row * g.R_own;
    float* ring = rings + g.ring_off[l];
    if (VEC) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (4 * q < g.R_own) v = *reinterpret_cast<const float4*>(src + 4 * q);
        for (int c = 0; c < g.P; ++c) *reinterpret_cast<float4*>(ring + (((long long)c * g.n_streams + s) * ML + slot) * g.R + 4 * q) = v;
    } else {
        const float v = q < g.R_own ? src[q] : 0.f;
        for (int c = 0; c < g.P; ++c) ring[(((long long)c * g.n_streams + s) * ML + slot) * g.R + q] = v;
    }
}

// float4 accesses need both channel counts to be multiples of 4 and a 16-byte aligned state (the rings are: hipMalloc, offsets in whole rows)
static bool wn_state_vec(const WnStateGeom& g, const void* state) { return g.R % 4 == 0 && g.R_own % 4 == 0 && (reinterpret_cast<uintptr_t>(state) & 15) == 0; }

static void wn_state_launch_gather(hipStream_t st, const WnStateGeom& g, long long rows, const float* rings, long long t, int stream, float* state) {
    const bool vec = wn_state_vec(g, state);
    const long long work = rows * (vec ? g.R_own / 4 : g.R_own);
    const dim3 grid((unsigned)((work + 255) / 256));
    if (vec) hipLaunchKernelGGL(wn_state_gather<true>, grid, dim3(256), 0, st, g, rings, t, stream, state);
    else hipLaunchKernelGGL(wn_state_gather<false>, grid, dim3(256), 0, st, g, rings, t, stream, state);
}
static void wn_state_launch_scatter(hipStream_t st, const WnStateGeom& g, long long rows, float* rings, long long t, int s0, int count, const float* state) {
    const bool vec = wn_state_vec(g, state);
    const long long work = rows * (vec ? g.R / 4 : g.R) * count;
    const dim3 grid((unsigned)((work + 255) / 256));
    if (vec) hipLaunchKernelGGL(wn_state_scatter<true>, grid, dim3(256), 0, st, g, rings, t, s0, count, state);
    else hipLaunchKernelGGL(wn_state_scatter<false>, grid, dim3(256), 0, st, g, rings, t, s0, count, state);
}

static WnStateGeom wn_state_geom(const wn_handle* h) {   // (a handle that owns rings: not the front of rounds)
    const WnPlan& pl = h->plan;
    return WnStateGeom{h->d_ring_off, h->d_state_off, h->d_dil, pl.NL, pl.k, pl.R, h->export_R ? h->export_R : pl.R, pl.n_streams, pl.P};
}
static long long wn_state_rows(const wn_handle* h) {
    long long rows = 0;
    for (int l = 0; l < h->plan.NL; ++l) rows += (long long)(h->plan.k - 1) * h->dil[l] + 1;
    return rows;
}

extern "C" int wn_state_floats(wn_handle* h, int64_t* out) {
    g_err[0] = 0;
    if (!h || !out) return wn_fail(WN_E_BADARG, "wn_state_floats: NULL argument");
    *out = (int64_t)wn_state_rows(h) * (h->export_R ? h->export_R : h->plan.R);
    return WN_OK;
}

extern "C" int wn_state_save(wn_handle* h, int32_t stream, float* state, void* hip_stream) {
    g_err[0] = 0;
    if (!h || !state) return wn_fail(WN_E_BADARG, "wn_state_save: NULL argument");
    if (stream < 0 || stream >= h->plan.n_streams) return wn_fail(WN_E_BADARG, "wn_state_save: stream %d of %d", (int)stream, h->plan.n_streams);
    if (h->pending) { int rc = wn_wait(h); if (rc) return rc; }
    if (!h->chains.empty()) {   // rounds: the member that owns the stream (wn_export_queue's rule)
        size_t i = 0;
        while (stream >= h->chain_first[i + 1]) ++i;
        return wn_state_save(h->chains[i], stream - h->chain_first[i], state, hip_stream);
    }
    { int rc = rt_hip(hipSetDevice(h->cfg.device_id), "hipSetDevice"); if (rc) return rc; }
    wn_state_launch_gather((hipStream_t)hip_stream, wn_state_geom(h), wn_state_rows(h), h->d_rings, h->t_base, stream, state);
    return rt_hip(hipGetLastError(), "wn_state_save launch");
}

extern "C" int wn_state_load(wn_handle* h, int32_t stream_first, int32_t stream_count, const float* state, void* hip_stream) {
    g_err[0] = 0;
    if (!h || !state) return wn_fail(WN_E_BADARG, "wn_state_load: NULL argument");
    if (stream_first < 0 || stream_count < 1 || (long long)stream_first + stream_count > h->plan.n_streams)
        return wn_fail(WN_E_BADARG, "wn_state_load: streams [%d, %d + %d) of %d", (int)stream_first, (int)stream_first, (int)stream_count, h->plan.n_streams);
    if (h->broken) return wn_fail(WN_E_STATE, "wn_state_load: an earlier job failed half way through its rounds; call wn_reset");
    if (h->pending) { int rc = wn_wait(h); if (rc) return rc; }
    if (!h->chains.empty()) {   // rounds: every member takes its part of the range
        const int lo = stream_first, hi = stream_first + stream_count;
        for (size_t i = 0; i < h->chains.size(); ++i) {
            const int a = lo > h->chain_first[i] ? lo : h->chain_first[i], b = hi < h->chain_first[i + 1] ? hi : h->chain_first[i + 1];
            if (a >= b) continue;
            int rc = wn_state_load(h->chains[i], a - h->chain_first[i], b - a, state, hip_stream);
            if (rc) return rc;
        }
        return WN_OK;
    }
    { int rc = rt_hip(hipSetDevice(h->cfg.device_id), "hipSetDevice"); if (rc) return rc; }
    wn_state_launch_scatter((hipStream_t)hip_stream, wn_state_geom(h), wn_state_rows(h), h->d_rings, h->t_base, stream_first, stream_count, state);
    return rt_hip(hipGetLastError(), "wn_state_load launch");
}
