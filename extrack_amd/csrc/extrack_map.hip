// libextrack_hip.so, translation unit: most-likely state path per track (xt_map.h) behind extrack_map_states.
#include "xt_host.h"

#include "xt_map.h"

// Waves per SIMD asked of the register allocator (256-thread workgroups; 0 = unbounded).  Unbounded the kernels take 161 - 230 VGPRs = 2 - 3
// workgroups per CU; measured on one MI355X, alternating builds: 4 states 5e5 x 60 frame_len 5: unbounded (186 VGPRs, 2 per
// CU) 90.7 ms, 3 waves (168 VGPRs, 40 B/lane scratch, 3 per CU) 75.8 ms; 2 states 1e6 x 30 frame_len 6: 6.54 / 6.53 ms (3 per CU either way).
// 4 waves would cost the 2-state kernels 124 - 316 B/lane of scratch (compiler report; not measured).
#ifndef XT_MAP_WAVES
#define XT_MAP_WAVES 3
#endif
template <int G_, int D, int K, int MAXT>
__global__ void __launch_bounds__(MAXT, (MAXT == 256 && XT_MAP_WAVES ? XT_MAP_WAVES : 1)) xt_map_kernel(XtKernelArgs a, XtMapArgs ma)
{
    DevCtx cx;
    xt_map_body<G_, D, K>(a, ma, cx);
}

template <int G_, int D, int K>
static const void* xt_map_kernel_t(int threads)
{
    return threads <= 256 ? (const void*)xt_map_kernel<G_, D, K, 256> : (const void*)xt_map_kernel<G_, D, K, 1024>;
}

template <int G_>
static const void* xt_map_kernel_dk(int D, int K, int threads)
{
    if (D == 1 && K == 1) return xt_map_kernel_t<G_, 1, 1>(threads);
    if (D == 2 && K == 1) return xt_map_kernel_t<G_, 2, 1>(threads);
    if (D == 2 && K == 2) return xt_map_kernel_t<G_, 2, 2>(threads);
    if (D == 3 && K == 1) return xt_map_kernel_t<G_, 3, 1>(threads);
    if (D == 3 && K == 3) return xt_map_kernel_t<G_, 3, 3>(threads);
    return nullptr;
}

static const void* xt_map_kernel_ptr(int S, int D, int K, int threads)
{
    if (S == 2) return xt_map_kernel_dk<2>(D, K, threads);
    if (S == 3) return xt_map_kernel_dk<3>(D, K, threads);
    if (S == 4) return xt_map_kernel_dk<4>(D, K, threads);
    return nullptr;
}

void xt_map_release(extrack_ctx* ctx)
{
    if (ctx->d_map_ws) (void)hipFree(ctx->d_map_ws);
    if (ctx->d_map_out) (void)hipFree(ctx->d_map_out);
    ctx->d_map_ws = nullptr;
    ctx->d_map_out = nullptr;
    ctx->map_ws_cap = ctx->map_out_cap = 0;
}

static int xt_map_reserve(extrack_ctx* ctx, void** buf, size_t* cap, size_t bytes)
{
    if (bytes <= *cap) return EXTRACK_OK;
    XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr;
    *cap = 0;
    XT_HIP(ctx, hipMalloc(buf, bytes));
    *cap = bytes;
    return EXTRACK_OK;
}

// Tracks per block and LDS bytes of the decoder for one back-pointer placement: as many tracks as fit 256 threads and a 64 KiB budget
// (several blocks per CU), a single track may take up to the CU's 160 KiB (xt_geometry's rule).
static void xt_map_geometry(const XtConfig& c, int D, int K, int L, int bpw, bool bp_lds, int& tpb, size_t& lds)
{
    const size_t fixed = xt_map_lds_doubles(c.S, c.EP, c.NG, D, K, L, bpw, bp_lds, 0) * sizeof(double);
    const size_t per_track = xt_map_lds_doubles(c.S, c.EP, c.NG, D, K, L, bpw, bp_lds, 1) * sizeof(double) - fixed;
    const size_t budget = 64 * 1024;
    const int by_threads = c.NG >= 256 ? 1 : 256 / c.NG;
    const int by_lds = budget > fixed + per_track ? (int)((budget - fixed) / per_track) : 1;
    tpb = std::max(1, std::min(by_threads, by_lds));
    lds = fixed + per_track * tpb;
}

// The launch path of extrack_map_states and of extrack_map_states_gaps (extrack_map_gaps.hip): the two differ in the kernel alone.
int xt_map_states_launch(extrack_ctx* ctx, const extrack_model* m, int32_t bucket_id, int8_t* states, double* score, bool gaps)
{
    if (!ctx || !states) return xt_fail(ctx, EXTRACK_E_INVALID, "null argument");
    int rc = xt_validate_model(ctx, m);
    if (rc) return rc;
    if (bucket_id < 0 || bucket_id >= (int)ctx->buckets.size()) return xt_fail(ctx, EXTRACK_E_INVALID, "bucket id out of range");
    // (the gap-aware entry point refuses sub-steps as extrack_loglik_gaps does: not built, rather than an invalid model)
    if (m->nb_substeps != 1) return xt_fail(ctx, gaps ? EXTRACK_E_UNSUPPORTED : EXTRACK_E_INVALID, "state paths require nb_substeps == 1");
    const int S = m->n_states, F = m->frame_len;
    if (S < 2 || F < 2) return xt_fail(ctx, EXTRACK_E_INVALID, "n_states and frame_len must be >= 2");
    // everything below is decided on the host, before any device work
    if (S > 4) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "state paths are built for n_states <= 4");
    if ((F - 1) * log((double)S) > log(1024.0) + 1e-9)
        return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "state paths: n_states^(frame_len - 1) groups per track do not fit a workgroup (lower frame_len)");
    XtBucket& b = ctx->buckets[bucket_id];
    if (b.d_dt) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "state paths are not built for per-track time steps");
    const int D = b.D, L = b.L;
    int K;
    if (m->locerr_mode == 0) {
        K = m->locerr_dims;
        if (K != 1 && K != D) return xt_fail(ctx, EXTRACK_E_INVALID, "locerr_dims must be 1 or the track dimensionality");
    } else {
        if (!b.d_sigma) return xt_fail(ctx, EXTRACK_E_INVALID, "per-peak localisation error mode but the bucket has no sigma");
        K = b.KS;
    }
    XtConfig cgeo;
    {
        const std::string err = xt_build_config(S, 1, F, cgeo);
        if (!err.empty()) return xt_fail(ctx, EXTRACK_E_INVALID, err);
    }
    // back-pointer words beside the sequence state when that costs neither tracks per block nor blocks per CU, else in global scratch
    const int bpw = xt_map_bp_words(L, F);
    int tpb_g, tpb_l;
    size_t lds_g, lds_l;
    xt_map_geometry(cgeo, D, K, L, bpw, false, tpb_g, lds_g);
    xt_map_geometry(cgeo, D, K, L, bpw, true, tpb_l, lds_l);
    const size_t cu_lds = 160 * 1024;
    if (lds_g > cu_lds) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "state paths: the sequence state of one track exceeds the LDS of a CU (lower frame_len)");
    bool bp_lds = tpb_l == tpb_g && lds_l <= cu_lds && cu_lds / lds_l == cu_lds / lds_g;
    if (const char* ev = getenv("EXTRACK_MAP_BP")) {
        if (!strcmp(ev, "global")) bp_lds = false;
        if (!strcmp(ev, "lds") && lds_l <= cu_lds) bp_lds = true;
    }
    const int tpb = bp_lds ? tpb_l : tpb_g;
    const size_t lds = bp_lds ? lds_l : lds_g;
    const int threads = (tpb * cgeo.NG + 63) / 64 * 64;
    const void* kp = gaps ? xt_map_gap_kernel_ptr(S, D, K, threads) : xt_map_kernel_ptr(S, D, K, threads);
    if (!kp || threads > 1024) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "state-path kernel variant not built");

    XT_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = xt_prepare_config(ctx, m))) return rc;
    const XtConfig& c = ctx->cfg;
    XtModelHost mh;
    xt_model_host(m, mh);
    std::vector<double> blob;
    xt_build_blob(mh, c, blob);
    if ((rc = xt_upload_blob(ctx, blob))) return rc;

    int occ = 0;
    XT_HIP(ctx, xt_occupancy(ctx, kp, threads, lds, &occ));
    const int64_t nbatch = (b.N + tpb - 1) / tpb;
    // the launcher's rule for the likelihood (extrack_ll.hip: xt_ll_plan): several block generations per CU, a block of a small launch still walks
    // >= 4 batches, never fewer blocks than fill the chip once
    int64_t target = (int64_t)occ * ctx->n_cu * ctx->oversub;
    if (!ctx->oversub_forced) target = std::max<int64_t>((int64_t)occ * ctx->n_cu, std::min<int64_t>(target, nbatch / 4));
    if (const char* ev = getenv("EXTRACK_MAP_MAX_BLOCKS")) target = std::min<int64_t>(target, std::max(1, atoi(ev)));  // tests: force the batch loop
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(nbatch, target));

    // outputs: [N] scores, then [N][L] states
    const size_t score_bytes = ((size_t)b.N * sizeof(double) + 255) & ~(size_t)255;
    const size_t state_bytes = (size_t)b.N * L;
    if ((rc = xt_map_reserve(ctx, &ctx->d_map_out, &ctx->map_out_cap, score_bytes + state_bytes))) return rc;
    XtMapArgs ma;
    memset(&ma, 0, sizeof(ma));
    ma.score = (double*)ctx->d_map_out;
    ma.states = (int8_t*)ctx->d_map_out + score_bytes;
    ma.bp_words = bpw;
    ma.Lmax = L;
    if (!bp_lds) {
        // one region per track slot of the grid actually launched (never per track of the bucket)
        const size_t need = (size_t)grid * tpb * bpw * c.NG * sizeof(uint32_t);
        if ((rc = xt_map_reserve(ctx, &ctx->d_map_ws, &ctx->map_ws_cap, need))) return rc;
        ma.bp_ws = (uint32_t*)ctx->d_map_ws;
    }
    XtKernelArgs a;
    memset(&a, 0, sizeof(a));
    xt_fill_args_from_config(c, a);
    a.tracks = b.d_tracks;
    a.sigma = m->locerr_mode ? b.d_sigma : nullptr;
    a.blob = ctx->d_blob;
    a.base_tab = ctx->d_base_tab;
    a.off_tab = ctx->d_off_tab;
    a.N = b.N;
    a.L = L;
    a.isBL = (L != m->max_len) ? 1 : 0;  // tracking.py:1037-1040
    a.ll_const = -(double)(L - 1) * D * 0.5 * XT_LOG2PI;
    a.TPB = tpb;
    a.min_len = m->min_len;
    a.locerr_mode = m->locerr_mode;
    a.KS = b.KS ? b.KS : 1;
    XT_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    void* kargs[2] = {(void*)&a, (void*)&ma};
    hipError_t e = hipLaunchKernel(kp, dim3(grid), dim3(threads), kargs, lds, ctx->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) return xt_fail(ctx, EXTRACK_E_HIP, std::string("state-path kernel launch: ") + hipGetErrorString(e));
    XT_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    ctx->timed = true;
    XT_HIP(ctx, hipMemcpyAsync(states, ma.states, state_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (score) XT_HIP(ctx, hipMemcpyAsync(score, ma.score, (size_t)b.N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    xt_set_launch_info(ctx, grid, threads, lds, tpb, occ);
    return EXTRACK_OK;
}

extern "C" int extrack_map_states(extrack_ctx* ctx, const extrack_model* m, int32_t bucket_id, int8_t* states, double* score)
{
    return xt_map_states_launch(ctx, m, bucket_id, states, score, false);
}
