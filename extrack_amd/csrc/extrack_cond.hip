// libextrack_hip.so, translation unit: position refinement along a given state path (xt_cond.h) behind extrack_refine_fixed_states.
#include "xt_host.h"

#include "xt_cond.h"

// One lane per track, 64 threads per block; the kernel is bound by memory and LDS capacity, not by registers.
template <int D, int K, bool WS_GLOBAL>
__global__ void __launch_bounds__(256) xt_cond_kernel(XtCondArgs a)
{
    DevCtx cx;
    xt_cond_body<D, K, WS_GLOBAL>(a, cx);
}

template <int D, int K>
static const void* xt_cond_kernel_w(bool ws_global)
{
    return ws_global ? (const void*)xt_cond_kernel<D, K, true> : (const void*)xt_cond_kernel<D, K, false>;
}

static const void* xt_cond_kernel_ptr(int D, int K, bool ws_global)
{
    if (D == 1 && K == 1) return xt_cond_kernel_w<1, 1>(ws_global);
    if (D == 2 && K == 1) return xt_cond_kernel_w<2, 1>(ws_global);
    if (D == 2 && K == 2) return xt_cond_kernel_w<2, 2>(ws_global);
    if (D == 3 && K == 1) return xt_cond_kernel_w<3, 1>(ws_global);
    if (D == 3 && K == 3) return xt_cond_kernel_w<3, 3>(ws_global);
    return nullptr;
}

void xt_cond_release(extrack_ctx* ctx)
{
    if (ctx->d_cond_buf) (void)hipFree(ctx->d_cond_buf);
    ctx->d_cond_buf = nullptr;
    ctx->cond_cap = 0;
}

// The launch path of extrack_refine_fixed_states and of extrack_refine_fixed_states_gaps (extrack_cond_gaps.hip): the two differ in the
// kernel alone.
int xt_refine_fixed_states_launch(extrack_ctx* ctx, const extrack_model* m, int32_t bucket_id, const int8_t* states, double* mu, double* sigma,
                                  double* logdens, bool gaps)
{
    if (!ctx || !states || !mu || !sigma) return xt_fail(ctx, EXTRACK_E_INVALID, "null argument");
    int rc = xt_validate_model(ctx, m);
    if (rc) return rc;
    if (bucket_id < 0 || bucket_id >= (int)ctx->buckets.size()) return xt_fail(ctx, EXTRACK_E_INVALID, "bucket id out of range");
    // everything below is decided on the host, before any device work
    // (the gap-aware entry point refuses sub-steps as extrack_loglik_gaps does: not built, rather than an invalid model)
    if (m->nb_substeps != 1)
        return xt_fail(ctx, gaps ? EXTRACK_E_UNSUPPORTED : EXTRACK_E_INVALID, "refinement along a state path requires nb_substeps == 1");
    const int S = m->n_states;
    if (S < 2 || S > XT_MAX_STATES) return xt_fail(ctx, EXTRACK_E_INVALID, "n_states must be in [2, 8]");
    XtBucket& b = ctx->buckets[bucket_id];
    if (b.d_dt) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "refinement along a state path is not built for per-track time steps");
    const int D = b.D, L = b.L;
    int K;
    if (m->locerr_mode == 0) {
        K = m->locerr_dims;
        if (K != 1 && K != D) return xt_fail(ctx, EXTRACK_E_INVALID, "locerr_dims must be 1 or the track dimensionality");
    } else {
        if (!b.d_sigma) return xt_fail(ctx, EXTRACK_E_INVALID, "per-peak localisation error mode but the bucket has no sigma");
        K = b.KS;
    }
    const size_t nstates = (size_t)b.N * L;
    for (size_t i = 0; i < nstates; ++i)
        if (states[i] >= S) return xt_fail(ctx, EXTRACK_E_INVALID, "state path holds a state >= n_states");  // negative: that track's outputs are NaN

    // rows of one wave's tracks in LDS while they fit a CU, else in the output arrays themselves (xt_cond.h)
    const size_t cu_lds = 160 * 1024;
    bool ws_global = xt_cond_lds_doubles(S, L, D, K, 64, false) * sizeof(double) > cu_lds;
    if (const char* ev = getenv("EXTRACK_COND_WS")) {
        if (!strcmp(ev, "global")) ws_global = true;  // "lds" is the library's own choice wherever the rows fit
    }
    // one wave per block: the blocks share nothing but the step-variance table, and the smallest block leaves the most blocks per CU
    const int tpb = 64;
    const size_t lds = xt_cond_lds_doubles(S, L, D, K, tpb, ws_global) * sizeof(double);
    const int threads = tpb;
    const void* kp = gaps ? xt_cond_gap_kernel_ptr(D, K, ws_global) : xt_cond_kernel_ptr(D, K, ws_global);
    if (!kp) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "fixed-state refinement kernel variant not built");

    XtCondArgs a;
    memset(&a, 0, sizeof(a));
    {
        // the tables of the likelihood's model blob (frame_len plays no part in the header and the step variances)
        XtConfig cgeo;
        const std::string err = xt_build_config(S, 1, 2, cgeo);
        if (!err.empty()) return xt_fail(ctx, EXTRACK_E_INVALID, err);
        XtModelHost mh;
        xt_model_host(m, mh);
        std::vector<double> blob;
        xt_build_blob(mh, cgeo, blob);
        for (int i = 0; i < 8; ++i) a.hdr[i] = blob[i];
        for (int i = 0; i < S * S; ++i) a.d2[i] = blob[(size_t)XT_BLOB_HDR + 4 * (size_t)S * S + i];
    }

    XT_HIP(ctx, hipSetDevice(ctx->device));
    // at every launch, not only when the occupancy is first asked for: the attribute belongs to the kernel, and a smaller request in between would leave it low
    if (lds > 64 * 1024) XT_HIP(ctx, hipFuncSetAttribute(kp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int occ = 0;
    XT_HIP(ctx, xt_occupancy(ctx, kp, threads, lds, &occ));
    const int64_t nbatch = (b.N + tpb - 1) / tpb;
    // one block per batch of 64 tracks: the blocks are independent and cheap to start, so the hardware balances them; beyond 2^20 blocks
    // (or with EXTRACK_COND_MAX_BLOCKS, for tests) a block walks several batches
    int64_t target = 1 << 20;
    if (const char* ev = getenv("EXTRACK_COND_MAX_BLOCKS")) target = std::min<int64_t>(target, std::max(1, atoi(ev)));
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(nbatch, target));

    // device buffer: [N][L][D] mu, [N][L][K] sigma, [N] logdens, [N][L] states (each part 256-byte aligned)
    auto al = [](size_t n) { return (n + 255) & ~(size_t)255; };
    const size_t mu_bytes = nstates * D * sizeof(double), sg_bytes = nstates * K * sizeof(double), ld_bytes = (size_t)b.N * sizeof(double);
    const size_t need = al(mu_bytes) + al(sg_bytes) + al(ld_bytes) + al(nstates);
    if (need > ctx->cond_cap) {
        XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        xt_cond_release(ctx);
        XT_HIP(ctx, hipMalloc(&ctx->d_cond_buf, need));
        ctx->cond_cap = need;
    }
    char* base = (char*)ctx->d_cond_buf;
    a.mu = (double*)base;
    a.sig_out = (double*)(base + al(mu_bytes));
    a.logdens = logdens ? (double*)(base + al(mu_bytes) + al(sg_bytes)) : nullptr;
    int8_t* d_states = (int8_t*)(base + al(mu_bytes) + al(sg_bytes) + al(ld_bytes));
    a.states = d_states;
    a.tracks = b.d_tracks;
    a.sigma = m->locerr_mode ? b.d_sigma : nullptr;
    a.N = b.N;
    a.L = L;
    a.S = S;
    a.TPB = tpb;
    a.locerr_mode = m->locerr_mode;
    a.ws_global = ws_global ? 1 : 0;
    XT_HIP(ctx, hipMemcpyAsync(d_states, states, nstates, hipMemcpyHostToDevice, ctx->stream));
    XT_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    void* kargs[1] = {(void*)&a};
    hipError_t e = hipLaunchKernel(kp, dim3(grid), dim3(threads), kargs, lds, ctx->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return xt_fail(ctx, EXTRACK_E_HIP, std::string("fixed-state refinement kernel launch: ") + hipGetErrorString(e));
    XT_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    ctx->timed = true;
    XT_HIP(ctx, hipMemcpyAsync(mu, a.mu, mu_bytes, hipMemcpyDeviceToHost, ctx->stream));
    XT_HIP(ctx, hipMemcpyAsync(sigma, a.sig_out, sg_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (logdens) XT_HIP(ctx, hipMemcpyAsync(logdens, a.logdens, ld_bytes, hipMemcpyDeviceToHost, ctx->stream));
    XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    xt_set_launch_info(ctx, grid, threads, lds, tpb, occ);
    return EXTRACK_OK;
}

extern "C" int extrack_refine_fixed_states(extrack_ctx* ctx, const extrack_model* m, int32_t bucket_id, const int8_t* states, double* mu,
                                           double* sigma, double* logdens)
{
    return xt_refine_fixed_states_launch(ctx, m, bucket_id, states, mu, sigma, logdens, false);
}
