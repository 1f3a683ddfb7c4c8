// libextrack_hip.so, translation unit: pairwise state posteriors P(state t = i, state t+1 = j | track) and their per-track sums behind
// extrack_predict_pairs / extrack_predict_pairs_gaps - the PAIRS instantiations of the fixed-window body (xt_kernel.h), with and without
// missed detections, and their launcher in stages.  Path choice and geometry: the host-only xt_pair_pick (xt_pair_geom.h).  DESIGN.md section 29.
#include "xt_host.h"

#include "xt_ll_geom.h"
#include "xt_pair_geom.h"

// Waves per SIMD asked of the register allocator: the value of the posterior kernels (extrack_ll.hip: XT_PREDS_WAVES, measured there); the
// pair kernels keep the same values live across a step (pq[S]) and differ in where they add them.
#ifndef XT_PAIRS_WAVES
#define XT_PAIRS_WAVES 3
#endif
template <int G_, int D, int K, bool GAPS, int MAXT>
__global__ void __launch_bounds__(MAXT, (MAXT == 256 ? XT_PAIRS_WAVES : 1)) xt_pair_kernel(XtKernelArgs a)
{
    DevCtx cx;
    xt_track_body<G_, D, K, true, GAPS, true>(a, cx);
}

template <int G_, int D, int K>
static const void* pair_ptr(bool gaps, bool wide)
{
    if (gaps) return wide ? (const void*)xt_pair_kernel<G_, D, K, true, 1024> : (const void*)xt_pair_kernel<G_, D, K, true, 256>;
    return wide ? (const void*)xt_pair_kernel<G_, D, K, false, 1024> : (const void*)xt_pair_kernel<G_, D, K, false, 256>;
}

template <int G_>
static const void* pair_dk(int D, int K, bool gaps, bool wide)
{
    if (D == 1 && K == 1) return pair_ptr<G_, 1, 1>(gaps, wide);
    if (D == 2 && K == 1) return pair_ptr<G_, 2, 1>(gaps, wide);
    if (D == 2 && K == 2) return pair_ptr<G_, 2, 2>(gaps, wide);
    if (D == 3 && K == 1) return pair_ptr<G_, 3, 1>(gaps, wide);
    if (D == 3 && K == 3) return pair_ptr<G_, 3, 3>(gaps, wide);
    return nullptr;
}

// Built where xt_pair_built (xt_pair_geom.h) holds.
static const void* xt_pair_kernel_ptr(int G, int D, int K, bool gaps, bool wide)
{
    if (G == 2) return pair_dk<2>(D, K, gaps, wide);
    if (G == 3) return pair_dk<3>(D, K, gaps, wide);
    if (G == 4) return pair_dk<4>(D, K, gaps, wide);
    return nullptr;
}

// ONE pair launch: one bucket, what is asked, and what the stages leave for each other.
struct XtPairLaunch {
    bool gaps = false;
    XtBucket* b = nullptr;
    int D = 0, K = 0;
    XtPairPick pk;
    const void* kp = nullptr;
    size_t pair_bytes = 0, count_bytes = 0;  // device outputs: [N][L-1][S][S] (0: not asked), [N][S][S] (0: not asked), then the descriptor
    double *d_pairs = nullptr, *d_counts = nullptr;
    XtBucketDesc* d_desc = nullptr;
    XtBucketDesc desc;
    XtKernelArgs a;
    int grid = 0, occ = 0;
};

// Stage 1, on the host, before anything is enqueued or recorded: everything that is refused.
static int xt_pair_check(extrack_ctx* ctx, const extrack_model* m, int32_t bucket_id, const double* pairs, const double* counts, XtPairLaunch& l)
{
    if (!pairs && !counts) return xt_fail(ctx, EXTRACK_E_INVALID, "pair posteriors: both outputs are null");
    int rc = xt_validate_model(ctx, m);
    if (rc) return rc;
    if (bucket_id < 0 || bucket_id >= (int)ctx->buckets.size()) return xt_fail(ctx, EXTRACK_E_INVALID, "bucket id out of range");
    // (sub-steps: refused as extrack_predict / extrack_predict_gaps refuse them)
    if (m->nb_substeps != 1)
        return l.gaps ? xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "missed detections: built for nb_substeps == 1")
                      : xt_fail(ctx, EXTRACK_E_INVALID, "state predictions require nb_substeps == 1");
    if (m->n_states > 4) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, xt_pair_refusal_text(XT_PAIR_NO_STATES));
    XtConfig c;
    const std::string err = xt_build_config(m->n_states, m->nb_substeps, m->frame_len, c);
    if (!err.empty()) return xt_fail(ctx, EXTRACK_E_INVALID, err);
    l.b = &ctx->buckets[bucket_id];
    if (l.b->d_dt) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "pair posteriors are not built for buckets with per-track time steps");
    l.D = l.b->D;
    if (m->locerr_mode == 0) {
        l.K = m->locerr_dims;
        if (l.K != 1 && l.K != l.D) return xt_fail(ctx, EXTRACK_E_INVALID, "locerr_dims must be 1 or the track dimensionality");
    } else {
        if (!l.b->d_sigma) return xt_fail(ctx, EXTRACK_E_INVALID, "per-peak localisation error mode but the bucket has no sigma");
        l.K = l.b->KS;
    }
    l.pk = xt_pair_pick(c, l.D, l.K);
    if (l.pk.refusal != XT_PAIR_FITS) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, xt_pair_refusal_text(l.pk.refusal));
    l.kp = xt_pair_kernel_ptr(l.pk.sel, l.D, l.K, l.gaps, l.pk.wide);
    if (!l.kp) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, xt_pair_refusal_text(XT_PAIR_NO_VARIANT));
    return EXTRACK_OK;
}

// Stage 2: model tables, partial sums, and the output buffer - reserved by the size of THIS call (counts alone: N * S^2 doubles) and kept, as
// the posterior buffer it shares with extrack_predict is.
static int xt_pair_reserve(extrack_ctx* ctx, const extrack_model* m, bool want_pairs, bool want_counts, XtPairLaunch& l)
{
    XT_HIP(ctx, hipSetDevice(ctx->device));
    int rc = xt_prepare(ctx, m);
    if (rc) return rc;
    if ((rc = xt_reserve_partials(ctx, xt_max_grid(ctx)))) return rc;
    const size_t SS = (size_t)m->n_states * m->n_states;
    l.pair_bytes = want_pairs ? (size_t)l.b->N * (l.b->L - 1) * SS * sizeof(double) : 0;
    l.count_bytes = want_counts ? (size_t)l.b->N * SS * sizeof(double) : 0;
    if ((rc = xt_reserve_preds(ctx, l.pair_bytes + l.count_bytes + sizeof(XtBucketDesc)))) return rc;
    l.d_pairs = want_pairs ? ctx->d_preds : nullptr;
    l.d_counts = want_counts ? (double*)((char*)ctx->d_preds + l.pair_bytes) : nullptr;
    l.d_desc = (XtBucketDesc*)((char*)ctx->d_preds + l.pair_bytes + l.count_bytes);
    return EXTRACK_OK;
}

// Stage 3: the bucket descriptor (it travels beside the outputs: the descriptor table of the likelihood launches and its host shadow are left
// alone) and the kernel arguments.
static void xt_pair_args(extrack_ctx* ctx, const extrack_model* m, XtPairLaunch& l)
{
    XtBucketDesc& d = l.desc;
    d = XtBucketDesc();
    d.tracks = l.b->d_tracks;
    d.sigma = m->locerr_mode ? l.b->d_sigma : nullptr;
    d.ll_out = nullptr;
    d.preds_out = l.d_pairs;
    d.N = l.b->N;
    d.L = l.b->L;
    d.isBL = l.b->L != m->max_len ? 1 : 0;  // tracking.py:1037-1040
    d.ll_const = -(double)(l.b->L - 1) * l.D * 0.5 * XT_LOG2PI;
    d.scores_out = l.d_counts;
    XtKernelArgs& a = l.a;
    memset(&a, 0, sizeof(a));
    xt_fill_args_from_config(ctx->cfg, a);
    if (ctx->blob_inline) {
        a.blob = nullptr;
        memcpy(a.blob_inline, ctx->blob_host.data(), ctx->blob_host.size() * sizeof(double));
    } else {
        a.blob = ctx->d_blob;
    }
    a.base_tab = ctx->d_base_tab;
    a.off_tab = ctx->d_off_tab;
    a.partials = ctx->d_partials;
    a.TPB = l.pk.tpb;
    a.min_len = m->min_len;
    a.locerr_mode = m->locerr_mode;
    a.KS = l.b->KS ? l.b->KS : 1;
    a.desc = l.d_desc;
    a.ndesc = 1;
}

// Stage 4: occupancy and grid, by the launcher's rule for the likelihood (extrack_ll.hip: xt_ll_plan).
static hipError_t xt_pair_plan(extrack_ctx* ctx, XtPairLaunch& l)
{
    hipError_t e = xt_occupancy(ctx, l.kp, l.pk.threads, l.pk.lds, &l.occ);
    if (e != hipSuccess) return e;
    const int64_t nbatch = (l.b->N + l.pk.tpb - 1) / l.pk.tpb;
    int64_t target = (int64_t)l.occ * ctx->n_cu * ctx->oversub;
    if (!ctx->oversub_forced) target = std::max<int64_t>((int64_t)l.occ * ctx->n_cu, std::min<int64_t>(target, nbatch / 4));
    if (const char* ev = getenv("EXTRACK_PAIRS_MAX_BLOCKS")) target = std::min<int64_t>(target, std::max(1, atoi(ev)));  // tests: force the batch loop
    target = std::min<int64_t>(target, (int64_t)xt_max_grid(ctx));
    l.grid = (int)std::max<int64_t>(1, std::min<int64_t>(nbatch, target));
    l.a.blk_end[0] = l.grid;
    return hipSuccess;
}

// Stage 5: descriptor copy, launch between the timing events, results to the host.
static int xt_pair_run(extrack_ctx* ctx, XtPairLaunch& l, double* pairs, double* counts)
{
    XT_HIP(ctx, hipMemcpyAsync(l.d_desc, &l.desc, sizeof(XtBucketDesc), hipMemcpyHostToDevice, ctx->stream));
    XT_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    void* kargs[1] = {(void*)&l.a};
    hipError_t e = hipLaunchKernel(l.kp, dim3(l.grid), dim3(l.pk.threads), kargs, l.pk.lds, ctx->stream);
    if (e == hipSuccess) e = hipGetLastError();
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(ctx->stream);  // the descriptor copy reads l.desc
        return xt_fail(ctx, EXTRACK_E_HIP, std::string("pair kernel launch: ") + hipGetErrorString(e));
    }
    XT_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    ctx->timed = true;
    if (pairs) XT_HIP(ctx, hipMemcpyAsync(pairs, l.d_pairs, l.pair_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (counts) XT_HIP(ctx, hipMemcpyAsync(counts, l.d_counts, l.count_bytes, hipMemcpyDeviceToHost, ctx->stream));
    XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    xt_set_launch_info(ctx, l.grid, l.pk.threads, l.pk.lds, l.pk.tpb, l.occ);
    ctx->last_ll_path = l.gaps ? XT_LL_GAPS : XT_LL_GENERAL;
    return EXTRACK_OK;
}

static int xt_predict_pairs_launch(extrack_ctx* ctx, const extrack_model* m, int32_t bucket_id, double* pairs, double* counts, bool gaps)
{
    if (!ctx) return EXTRACK_E_INVALID;
    XtPairLaunch l;
    l.gaps = gaps;
    int rc = xt_pair_check(ctx, m, bucket_id, pairs, counts, l);
    if (rc) return rc;
    if ((rc = xt_pair_reserve(ctx, m, pairs != nullptr, counts != nullptr, l))) return rc;
    xt_pair_args(ctx, m, l);
    const hipError_t e = xt_pair_plan(ctx, l);
    if (e != hipSuccess) return xt_fail(ctx, EXTRACK_E_HIP, std::string("pair kernel occupancy: ") + hipGetErrorString(e));
    return xt_pair_run(ctx, l, pairs, counts);
}

extern "C" int extrack_predict_pairs(extrack_ctx* ctx, const extrack_model* m, int32_t bucket_id, double* pairs, double* counts)
{
    return xt_predict_pairs_launch(ctx, m, bucket_id, pairs, counts, false);
}

extern "C" int extrack_predict_pairs_gaps(extrack_ctx* ctx, const extrack_model* m, int32_t bucket_id, double* pairs, double* counts)
{
    return xt_predict_pairs_launch(ctx, m, bucket_id, pairs, counts, true);
}
