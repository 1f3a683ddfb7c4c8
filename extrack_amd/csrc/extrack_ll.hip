// libextrack_hip.so: the fixed-window likelihood / posterior / sequence-matrix path - kernel wrappers of xt_kernel.h, xt_fast2.h, xt_entry.h and
// xt_big.h, the launcher (xt_launch_group, in stages), xt_gaps_check and the extrack_loglik* / extrack_predict* / extrack_sequence_* entry
// points.  The path choice and launch geometry come from the host-only xt_ll_pick and, for gapped two-state groups, xt_ll_gap_reg2
// (xt_ll_geom.h); context, buckets and the model upload live in extrack_hip.hip.  DESIGN.md sections 23 and 25.
#include "xt_host.h"

#include "xt_dispatch.h"
#include "xt_ll_geom.h"
#include "xt_seqmat.h"

// Waves per SIMD the register allocator is asked to allow (workgroups of 256 threads).  Likelihood kernels: 4, except 4 members per group
// (4 states: 66 ms unbounded against 74 ms at 3 on the 5e5 x 60 set, frame_len 5).  Posterior kernels (226 VGPRs unbounded = 2 waves):
// 3 waves (168 VGPRs, 27-60 spilled dwords) - measured r03: C5 (4 states, 5e5 x 60, frame_len 5) 318 -> 265 ms, 4 waves 365 ms;
// 2 states 1e6 x 30 frame_len 6 18.3 -> 15.2 ms; 3 states 2e5 x 30 frame_len 6 49.6 -> 44.2 ms.  3-state likelihood at 5 waves: frame_len 6 unchanged,
// frame_len 4 3.06 -> 3.94 ms (kept at 4).  Entry-parallel kernel (94 VGPRs unbounded = 5 waves): C5 (nb_substeps 3) 48.6 ms, 6 waves 46.9, 7 waves 46.2.
#ifndef XT_ENTRY_WAVES
#define XT_ENTRY_WAVES 7
#endif
#ifndef XT_LL_WAVES
#define XT_LL_WAVES 4
#endif
#ifndef XT_G4_WAVES
#define XT_G4_WAVES 1
#endif
#ifndef XT_PREDS_WAVES
#define XT_PREDS_WAVES 3
#endif
template <int G_, int D, int K, bool PREDS, int MAXT>
__global__ void __launch_bounds__(MAXT, (MAXT == 256 && !PREDS ? (G_ != 4 ? XT_LL_WAVES : XT_G4_WAVES) : (MAXT == 256 && PREDS ? XT_PREDS_WAVES : 1))) xt_track_kernel(XtKernelArgs a)
{
    DevCtx cx;
    xt_track_body<G_, D, K, PREDS>(a, cx);
    if (!PREDS) xt_fused_total(a);
}

template <int F, int D, int K>
__global__ void __launch_bounds__(64 * XT_F2_WAVES) xt_ll_s2_kernel(XtKernelArgs a)
{
    DevCtx cx;
    xt_ll_s2_body<F, D, K>(a, cx);
    xt_fused_total(a);
}

template <int GP, int D, int K, int MAXT>
__global__ void __launch_bounds__(MAXT, (MAXT == 256 ? XT_ENTRY_WAVES : 1)) xt_entry_kernel(XtKernelArgs a)
{
    DevCtx cx;
    xt_entry_body<GP, D, K>(a, cx);
    xt_fused_total(a);
}

// Models whose sequence state does not fit a workgroup: one lane per track, state in global memory (xt_big.h)
template <int D, int K, bool PREDS>
__global__ void __launch_bounds__(256) xt_big_kernel(XtKernelArgs a, XtBigArgs ba)
{
    DevCtx cx;
    xt_big_body<D, K, PREDS>(a, ba, cx);
    if (!PREDS) xt_fused_total(a);
}
template <int D, int K>
static const void* xt_big_kernel_ptr(bool preds) { return preds ? (const void*)xt_big_kernel<D, K, true> : (const void*)xt_big_kernel<D, K, false>; }
static const void* xt_big_kernel_dk(int D, int K, bool preds)
{
    if (D == 1 && K == 1) return xt_big_kernel_ptr<1, 1>(preds);
    if (D == 2 && K == 1) return xt_big_kernel_ptr<2, 1>(preds);
    if (D == 2 && K == 2) return xt_big_kernel_ptr<2, 2>(preds);
    if (D == 3 && K == 1) return xt_big_kernel_ptr<3, 1>(preds);
    if (D == 3 && K == 3) return xt_big_kernel_ptr<3, 3>(preds);
    return nullptr;
}

// Fixed-order reduction of the per-block partial sums (deterministic for a given launch geometry).
__global__ void __launch_bounds__(256) xt_reduce_partials(const double* __restrict__ partials, int n, double* __restrict__ out)
{
    __shared__ double sh[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += partials[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = sh[0];
}

// Upper bound of the blocks of one launch (= partial-sum slots to reserve).
size_t xt_max_grid(const extrack_ctx* ctx) { return (size_t)ctx->n_cu * 8 * ctx->oversub + XT_MAX_BUCKETS; }

// ONE kernel launch for a set of buckets that share (dims, sigma dims): what is asked, where its outputs go, and what the stages of
// xt_launch_group leave for each other.
struct XtLlLaunch {
    bool preds = false, per_track = false, gaps = false;  // posteriors (else the likelihood, with or without per-track output); missed detections
    double* d_preds = nullptr;  // posteriors: their device buffer
    double* d_seq = nullptr;    // sequence matrix: the log-weight of every sequence of the last position goes here
    size_t poff = 0, desc_off = 0;  // partial sums go to d_partials[poff .. poff + grid), descriptors to ctx->d_desc[desc_off ...]
    double* total_out = nullptr;    // fused total (one launch group): device word that receives the evaluation's total, or nullptr
    double* total_host = nullptr;   // + the pinned host word (device view) or nullptr
    int D = 0, K = 0;
    XtLlPick pk;
    XtKernelArgs a;
    XtBigArgs bargs;
    std::vector<XtBucketDesc> descs;  // buckets served by this launch (<= XT_MAX_BUCKETS)
    int grid = 0, occ = 0;
};

// dims of the group: D of its buckets, K of the localisation error the kernels see
static int xt_ll_dims(extrack_ctx* ctx, const extrack_model* m, const XtBucket& b0, XtLlLaunch& l)
{
    l.D = b0.D;
    if (m->locerr_mode == 0) {
        l.K = m->locerr_dims;
        if (l.K != 1 && l.K != l.D) return xt_fail(ctx, EXTRACK_E_INVALID, "locerr_dims must be 1 or the track dimensionality");
    } else {
        if (!b0.d_sigma) return xt_fail(ctx, EXTRACK_E_INVALID, "per-peak localisation error mode but the bucket has no sigma");
        l.K = b0.KS;
    }
    return EXTRACK_OK;
}

// XtKernelArgs::well_scaled of a 2-state fast-path launch: range of the localisation variance over the launch -> may the fast path drop its
// guards (xt_build_blob)?
static int xt_ll_scaling(const extrack_ctx* ctx, const extrack_model* m, const std::vector<XtBucket*>& bks, int K)
{
    double lo = INFINITY, hi = -INFINITY;
    if (m->locerr_mode == 0) {
        for (int k = 0; k < m->locerr_dims && k < 3; ++k) {
            lo = std::min(lo, m->locerr[k] * m->locerr[k]);
            hi = std::max(hi, m->locerr[k] * m->locerr[k]);
        }
    } else {
        for (XtBucket* b : bks) {
            double s0 = b->sig_min, s1 = b->sig_max;  // NaN when the bucket was attached by device pointer: not provable
            if (m->locerr_mode == 2) {
                const double a0 = s0 * m->slope + m->offset, a1 = s1 * m->slope + m->offset;
                s0 = std::max(std::min(a0, a1), 1e-6);
                s1 = std::max(std::max(a0, a1), 1e-6);
                if (a0 != a0 || a1 != a1) s0 = s1 = NAN;
            }
            lo = (s0 == s0) ? std::min(lo, s0 * s0) : NAN;
            hi = (s1 == s1) ? std::max(hi, s1 * s1) : NAN;
            if (lo != lo || hi != hi) break;
        }
    }
    return ctx->blob_host.size() > 8 ? xt_launch_scaling(ctx->blob_host, lo, hi, m->locerr_mode == 0 && K == 1) : 0;
}

static void xt_ll_descs(const extrack_model* m, const std::vector<XtBucket*>& bks, XtLlLaunch& l)
{
    for (XtBucket* b : bks) {
        XtBucketDesc d;
        d.tracks = b->d_tracks;
        d.sigma = m->locerr_mode ? b->d_sigma : nullptr;
        d.ll_out = l.per_track ? b->d_ll : nullptr;
        d.preds_out = l.d_preds;
        d.N = b->N;
        d.L = b->L;
        d.isBL = (!l.d_seq && b->L != m->max_len) ? 1 : 0;  // tracking.py:1037-1040
        d.ll_const = -(double)(b->L - 1) * l.D * 0.5 * XT_LOG2PI;
        d.seq_out = l.d_seq;
        l.descs.push_back(d);
    }
}

static void xt_ll_args(extrack_ctx* ctx, const extrack_model* m, const std::vector<XtBucket*>& bks, XtLlLaunch& l)
{
    XtKernelArgs& a = l.a;
    memset(&a, 0, sizeof(a));
    xt_fill_args_from_config(ctx->cfg, a);
    if (l.pk.path == XT_LL_REG2 || l.pk.path == XT_LL_FAST2) a.well_scaled = xt_ll_scaling(ctx, m, bks, l.K);
    if (l.pk.path == XT_LL_GAPS_REG2) a.well_scaled = 2;  // what xt_ll_gap_reg2 upgraded on
    if (ctx->blob_inline) {
        a.blob = nullptr;
        memcpy(a.blob_inline, ctx->blob_host.data(), ctx->blob_host.size() * sizeof(double));
    } else {
        a.blob = ctx->d_blob;
    }
    if (l.total_out) {
        a.done = ctx->d_done;
        a.total_out = l.total_out;
        a.total_host = l.total_host;
    }
    a.base_tab = ctx->d_base_tab;
    a.off_tab = ctx->d_off_tab;
    a.partials = ctx->d_partials + l.poff;
    a.TPB = l.pk.tpb;
    a.min_len = m->min_len;
    a.locerr_mode = m->locerr_mode;
    a.KS = bks[0]->KS ? bks[0]->KS : 1;
}

// Kernel address of the pick: xt_dispatch.h hands the instantiation to this functor (nullptr: not built)
struct XtLlKernelOf {
    bool wide, reg2;
    const void* kp = nullptr;
    template <int G_, int D, int K, bool PREDS>
    bool run()
    {
        kp = wide ? (const void*)xt_track_kernel<G_, D, K, PREDS, 1024> : (const void*)xt_track_kernel<G_, D, K, PREDS, 256>;
        return true;
    }
    template <int GP, int D, int K>
    bool run_entry()
    {
        kp = wide ? (const void*)xt_entry_kernel<GP, D, K, 1024> : (const void*)xt_entry_kernel<GP, D, K, 256>;
        return true;
    }
    template <int F, int D, int K>
    bool run_f2()
    {
        kp = reg2 ? xt_r2_kernel(F, D, K, 0) : (const void*)xt_ll_s2_kernel<F, D, K>;  // register-resident variant (xt_reg2.h) | xt_fast2.h
        return true;
    }
};
static const void* xt_ll_kernel(const XtLlPick& pk, int D, int K, bool preds)
{
    XtLlKernelOf k{pk.wide, pk.path == XT_LL_REG2};
    if (pk.path == XT_LL_BIG) return xt_big_kernel_dk(D, K, preds);
    if (pk.path == XT_LL_GAPS) return xt_gap_kernel_ptr(pk.sel, D, K, preds, pk.wide);
    if (pk.path == XT_LL_GAPS_REG2) return xt_r2_gap_kernel(pk.sel, D);
    if (pk.path == XT_LL_REG2 || pk.path == XT_LL_FAST2) xt_dispatch_f2(pk.sel, D, K, k);
    else if (pk.path == XT_LL_ENTRY) xt_dispatch_entry(pk.sel, D, K, k);
    else xt_dispatch(pk.sel, D, K, preds, k);
    return k.kp;
}

// Occupancy and grid split of kernel kp: sets occ, grid and a.blk_end.
static hipError_t xt_ll_plan(extrack_ctx* ctx, const void* kp, XtLlLaunch& l)
{
    const int tracks_per_block = l.pk.tpb;
    const double max_blocks = (double)l.pk.max_blocks;  // > 0: upper bound of the grid (scratch budget of the launch)
    hipError_t e = xt_occupancy(ctx, kp, l.pk.threads, l.pk.lds, &l.occ);
    if (e != hipSuccess) return e;
    // Split the grid over the buckets in proportion to their work (track batches x positions).  The CUs are
    // oversubscribed: waves of equal work do NOT progress equally (VALU issue is arbitrated by age), so a static
    // one-wave-set-per-CU split ends in an under-occupied tail; with several block generations per CU the hardware
    // dispatcher backfills as blocks retire.
    const int nb = (int)l.descs.size();
    double target = (double)l.occ * ctx->n_cu * ctx->oversub;
    int64_t nbsum = 0;
    for (int i = 0; i < nb; ++i) nbsum += (l.descs[i].N + tracks_per_block - 1) / tracks_per_block;
    // small launches: a block should still walk >= 4 batches (its fixed costs - tables, staging set-up, final reduction - are about
    // one batch's worth), but never fewer blocks than fill the chip once.  125 000 x 30 (the 8-way shard of the headline dataset):
    // 8 generations 0.399 ms, 4 generations 0.389 ms, 1 generation 0.423 ms (r04, same box)
    if (!ctx->oversub_forced) target = std::max((double)l.occ * ctx->n_cu, std::min(target, (double)nbsum / 4.0));
    if (max_blocks > 0.0) target = std::max((double)nb, std::min(target, max_blocks));
    // hard bound: the partial-sum slots of a launch (xt_max_grid) and the scratch budget, if any
    int64_t cap = (int64_t)xt_max_grid(ctx);
    if (max_blocks > 0.0) cap = std::min(cap, (int64_t)max_blocks);
    const int64_t g = xt_split_descs(target, cap, l.descs, tracks_per_block, l.a.blk_end);
    if (g < 0) return hipErrorInvalidConfiguration;
    l.grid = (int)g;
    return hipSuccess;
}

// Descriptor upload (when they changed) and the launch of kp on the grid of xt_ll_plan.
static hipError_t xt_ll_enqueue(extrack_ctx* ctx, const void* kp, XtLlLaunch& l)
{
    const int nb = (int)l.descs.size();
    const size_t desc_off = l.desc_off;
    hipError_t e;
    // the descriptors only change when the buckets (or the per-track / posterior outputs) do: keep a host shadow of the device table
    // and skip the copy when it already holds them (one dispatch less per evaluation in a fit)
    bool same = !ctx->no_fused && ctx->desc_shadow.size() >= desc_off + (size_t)nb &&
                memcmp(ctx->desc_shadow.data() + desc_off, l.descs.data(), nb * sizeof(XtBucketDesc)) == 0;
    if (!same) {
        // no blob slot guards this half of the staging area: wait for whatever still reads it
        if (ctx->blob_inline && (e = hipStreamSynchronize(ctx->stream)) != hipSuccess) return e;
        memcpy(ctx->h_desc + desc_off, l.descs.data(), nb * sizeof(XtBucketDesc));
        e = hipMemcpyAsync(ctx->d_desc + desc_off, ctx->h_desc + desc_off, nb * sizeof(XtBucketDesc), hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return e;
        // the staging half is reusable once this copy is done too: move the slot's guard event behind it
        if (!ctx->blob_inline && (e = hipEventRecord(ctx->ev_blob[(ctx->blob_turn - 1u) & 1u], ctx->stream)) != hipSuccess) return e;
        if (ctx->desc_shadow.size() < desc_off + (size_t)nb) ctx->desc_shadow.resize(desc_off + (size_t)nb);
        memcpy(ctx->desc_shadow.data() + desc_off, l.descs.data(), nb * sizeof(XtBucketDesc));
    }
    l.a.desc = ctx->d_desc + desc_off;
    l.a.ndesc = nb;
    void* kargs[2] = {(void*)&l.a, l.pk.path == XT_LL_BIG ? (void*)&l.bargs : nullptr};  // xt_big_kernel: + its scratch description
    e = hipLaunchKernel(kp, dim3(l.grid), dim3(l.pk.threads), kargs, l.pk.lds, ctx->stream);
    return e == hipSuccess ? hipGetLastError() : e;
}

// The launch of one group, in stages: dims -> xt_ll_pick -> descriptors -> kernel arguments (with the fast path's scaling) -> kernel address ->
// plan (occupancy, grid split) -> the global-state kernel's scratch -> enqueue -> launch info.  *grid_out: partial sums written.
static int xt_launch_group(extrack_ctx* ctx, const extrack_model* m, const std::vector<XtBucket*>& bks, XtLlLaunch& l, int* grid_out)
{
    const XtBucket& b0 = *bks[0];
    int rc = xt_ll_dims(ctx, m, b0, l);
    if (rc) return rc;
    // read at every launch, not in extrack_create: tests/test_hip_parity.py toggles both on a live context
    const char* ev = getenv("EXTRACK_FORCE_BIG");
    const bool force_big = ev && atoi(ev) != 0;
    size_t budget_mb = 32 * 1024;
    if ((ev = getenv("EXTRACK_BIG_WS_MB"))) budget_mb = (size_t)std::max(16, atoi(ev));
    l.pk = xt_ll_pick(ctx->cfg, l.D, l.K, m->locerr_mode ? b0.KS : 0, l.preds, l.d_seq != nullptr, l.gaps, ctx->ll_reg2, force_big, budget_mb,
                      (int)bks.size(), ctx->n_cu);
    if (l.pk.path == XT_LL_GAPS && !l.preds && xt_use_reg2(ctx->cfg.S, ctx->cfg.NS, ctx->cfg.F)) {
        // missed detections, two states: the register-resident kernel where its g-form steps are valid (xt_ll_gap_reg2), else the general gap body
        int Lmax = 0;
        for (const XtBucket* b : bks) Lmax = std::max(Lmax, b->L);
        l.pk = xt_ll_gap_reg2(l.pk, ctx->cfg, l.D, l.K, m->locerr_mode ? b0.KS : 0, l.preds, l.per_track, ctx->ll_reg2, xt_ll_scaling(ctx, m, bks, l.K), Lmax,
                              ctx->blob_host.size() > 8 ? ctx->blob_host[7] : NAN, ctx->gap_reg2_fmask);
    }
    const XtLlPick& pk = l.pk;
    if (pk.path == XT_LL_NONE) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, xt_ll_refusal_text(pk.refusal));
    xt_ll_descs(m, bks, l);
    xt_ll_args(ctx, m, bks, l);
    const void* kp = xt_ll_kernel(pk, l.D, l.K, l.preds);
    if (!kp) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, xt_ll_refusal_text(l.preds ? XT_LL_NO_PREDS_G : XT_LL_NO_VARIANT));
    hipError_t e = xt_ll_plan(ctx, kp, l);
    if (e == hipSuccess && pk.path == XT_LL_BIG) {
        // one ws_stride region per wavefront of the launched grid (xt_big_body indexes ws by blockIdx * NW + wave)
        const size_t need = (size_t)l.grid * (pk.threads / 64) * (size_t)pk.ws_stride + 64;
        if ((rc = xt_grow_device(ctx, (void**)&ctx->d_big_ws, &ctx->big_ws_cap, need * sizeof(double), "global-state scratch"))) return rc;
        l.bargs.ws = ctx->d_big_ws;
        l.bargs.ws_stride = pk.ws_stride;
    }
    if (e == hipSuccess) e = xt_ll_enqueue(ctx, kp, l);
    if (e != hipSuccess) return xt_fail(ctx, EXTRACK_E_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    xt_set_launch_info(ctx, l.grid, pk.threads, pk.lds, pk.tpb, l.occ);
    ctx->last_ll_path = pk.path;
    *grid_out = l.grid;
    return EXTRACK_OK;
}

// Missed detections (extrack_loglik_gaps / extrack_predict_gaps): what the gap-aware kernels (extrack_gaps.hip) do not serve is refused here, on
// the host, before anything is enqueued or recorded: nb_substeps, states, per-track time steps, and what xt_ll_pick(gaps = true) refuses.
// `only`: the one bucket of a posterior call, or nullptr for all buckets.
static int xt_gaps_check(extrack_ctx* ctx, const extrack_model* m, const XtBucket* only)
{
    if (m->nb_substeps != 1) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "missed detections: built for nb_substeps == 1");
    if (m->n_states < 2 || m->n_states > 4) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "missed detections: built for 2, 3 and 4 states");
    XtConfig c;
    std::string err = xt_build_config(m->n_states, m->nb_substeps, m->frame_len, c);
    if (!err.empty()) return xt_fail(ctx, EXTRACK_E_INVALID, err);
    for (const XtBucket& b : ctx->buckets) {
        if (only && &b != only) continue;
        if (b.d_dt) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "missed detections: not built for buckets with per-track time steps");
        const int D = b.D, K = m->locerr_mode == 0 ? m->locerr_dims : b.KS;
        if (K != 1 && K != D) return xt_fail(ctx, EXTRACK_E_INVALID, m->locerr_mode == 0 ? "locerr_dims must be 1 or the track dimensionality"
                                                                                         : "per-peak localisation error mode but the bucket has no sigma");
        const XtLlPick pk = xt_ll_pick(c, D, K, m->locerr_mode ? b.KS : 0, only != nullptr, false, true, ctx->ll_reg2, false, 0, 1, ctx->n_cu);
        if (pk.refusal == XT_LL_NO_GAPS_BIG)
            return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "missed detections: n_states^frame_len sequences per track do not fit a workgroup (no gap-aware global-state kernel)");
        if (pk.path == XT_LL_NONE) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "missed detections: kernel variant not built");
    }
    return EXTRACK_OK;
}

static int xt_loglik_enqueue(extrack_ctx* ctx, const extrack_model* m, double* d_total, bool per_track, bool to_host = false, bool gaps = false)
{
    int rc = xt_validate_model(ctx, m);
    if (rc) return rc;
    if (ctx->buckets.empty()) return xt_fail(ctx, EXTRACK_E_INVALID, "no bucket uploaded");
    if (gaps && (rc = xt_gaps_check(ctx, m, nullptr))) return rc;
    XT_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = xt_prepare(ctx, m))) return rc;
    // launch groups: buckets with the same (dims, sigma dims), longest first, at most XT_MAX_BUCKETS per launch
    const std::vector<std::vector<XtBucket*>> groups = xt_launch_groups(ctx, XT_MAX_BUCKETS);
    if (ctx->buckets.size() > (size_t)XT_DESC_CAP / 2) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "too many buckets");
    if ((rc = xt_reserve_partials(ctx, groups.size() * xt_max_grid(ctx)))) return rc;
    if (per_track)
        for (auto& b : ctx->buckets)
            if (!b.d_ll) XT_HIP(ctx, hipMalloc(&b.d_ll, (size_t)b.N * sizeof(double)));
    size_t poff = 0, doff = ctx->blob_inline ? 0 : xt_desc_base(ctx);
    // one launch group (the usual case): the likelihood kernel itself leaves the total in d_total (and in the pinned host word for
    // the synchronous entry point) - ONE dispatch per evaluation instead of five (blob copy, descriptor copy, kernel, reduction, read-back)
    const bool fused = !ctx->no_fused && groups.size() == 1;
    ctx->fused_host = fused && to_host;
    XT_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    for (auto& g : groups) {
        int grid = 0;
        XtLlLaunch l;
        l.per_track = per_track, l.gaps = gaps, l.poff = poff, l.desc_off = doff;
        if (fused) l.total_out = d_total, l.total_host = to_host ? ctx->h_total_dev : nullptr;
        if ((rc = xt_launch_group(ctx, m, g, l, &grid))) return rc;
        poff += (size_t)grid;
        doff += g.size();
    }
    XT_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    ctx->timed = true;
    if (!fused) {
        hipLaunchKernelGGL(xt_reduce_partials, dim3(1), dim3(256), 0, ctx->stream, ctx->d_partials, (int)poff, d_total);
        XT_HIP(ctx, hipGetLastError());
    }
    return EXTRACK_OK;
}

extern "C" int extrack_loglik_async(extrack_ctx* ctx, const extrack_model* model, double* d_total_ll)
{
    if (!ctx) return EXTRACK_E_INVALID;
    return xt_loglik_enqueue(ctx, model, d_total_ll ? d_total_ll : ctx->d_total, false);
}

static int xt_loglik_sync(extrack_ctx* ctx, const extrack_model* model, double* total_ll, double* per_track, bool gaps)
{
    if (!ctx || !total_ll) return xt_fail(ctx, EXTRACK_E_INVALID, "null argument");
    int rc = xt_loglik_enqueue(ctx, model, ctx->d_total, per_track != nullptr, true, gaps);
    if (rc) return rc;
    if (!ctx->fused_host) XT_HIP(ctx, hipMemcpyAsync(ctx->h_total, ctx->d_total, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (per_track) {
        size_t o = 0;
        for (auto& b : ctx->buckets) {
            XT_HIP(ctx, hipMemcpyAsync(per_track + o, b.d_ll, (size_t)b.N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
            o += (size_t)b.N;
        }
    }
    XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *total_ll = *ctx->h_total;
    return EXTRACK_OK;
}

extern "C" int extrack_loglik(extrack_ctx* ctx, const extrack_model* model, double* total_ll, double* per_track)
{
    return xt_loglik_sync(ctx, model, total_ll, per_track, false);
}

extern "C" int extrack_loglik_gaps(extrack_ctx* ctx, const extrack_model* model, double* total_ll, double* per_track)
{
    return xt_loglik_sync(ctx, model, total_ll, per_track, true);
}

// The opening of the calls that launch ONE bucket (posteriors, sequence matrix): validate, bucket id, the host-decided refusals, device, model
// tables, partial sums of one launch.
static int xt_one_bucket_begin(extrack_ctx* ctx, const extrack_model* m, int32_t bucket_id, bool preds, bool gaps)
{
    int rc = xt_validate_model(ctx, m);
    if (rc) return rc;
    if (bucket_id < 0 || bucket_id >= (int)ctx->buckets.size()) return xt_fail(ctx, EXTRACK_E_INVALID, "bucket id out of range");
    if (gaps && (rc = xt_gaps_check(ctx, m, &ctx->buckets[bucket_id]))) return rc;
    if (preds && m->nb_substeps != 1) return xt_fail(ctx, EXTRACK_E_INVALID, "state predictions require nb_substeps == 1");
    XT_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = xt_prepare(ctx, m))) return rc;
    return xt_reserve_partials(ctx, xt_max_grid(ctx));
}

static int xt_predict_sync(extrack_ctx* ctx, const extrack_model* m, int32_t bucket_id, double* preds, bool gaps)
{
    if (!ctx || !preds) return xt_fail(ctx, EXTRACK_E_INVALID, "null argument");
    int rc = xt_one_bucket_begin(ctx, m, bucket_id, true, gaps);
    if (rc) return rc;
    XtBucket& b = ctx->buckets[bucket_id];
    const size_t nb = (size_t)b.N * b.L * m->n_states * sizeof(double);
    if ((rc = xt_reserve_preds(ctx, nb))) return rc;
    double* d_preds = ctx->d_preds;
    int grid = 0;
    hipError_t e = hipEventRecord(ctx->ev0, ctx->stream);
    std::vector<XtBucket*> one(1, &b);
    XtLlLaunch l;
    l.preds = true, l.gaps = gaps, l.d_preds = d_preds, l.desc_off = xt_desc_base(ctx);
    rc = xt_launch_group(ctx, m, one, l, &grid);
    if (rc == EXTRACK_OK) {
        if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
        ctx->timed = true;
        if (e == hipSuccess) e = hipMemcpyAsync(preds, d_preds, nb, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = xt_fail(ctx, EXTRACK_E_HIP, std::string("predict: ") + hipGetErrorString(e));
    }
    return rc;
}

extern "C" int extrack_last_ll_path(const extrack_ctx* ctx, int32_t* path)
{
    if (!ctx || !path) return EXTRACK_E_INVALID;
    *path = ctx->last_ll_path;
    return EXTRACK_OK;
}

extern "C" int extrack_predict(extrack_ctx* ctx, const extrack_model* m, int32_t bucket_id, double* preds)
{
    return xt_predict_sync(ctx, m, bucket_id, preds, false);
}

extern "C" int extrack_predict_gaps(extrack_ctx* ctx, const extrack_model* m, int32_t bucket_id, double* preds)
{
    return xt_predict_sync(ctx, m, bucket_id, preds, true);
}

// Per-sequence log-probabilities of one bucket in the reference's layout (P_Cs_inter_bound_stats' first return value,
// extrack/tracking.py:300-318): raw kernel output -> host -> column order of the reference (xt_seqmat.h).  For small inputs:
// N * S^(frame_len + nb_substeps) doubles go through host memory.
extern "C" int64_t extrack_sequence_columns(int32_t n_states, int32_t len, int32_t nb_substeps, int32_t frame_len, int32_t isBL)
{
    if (n_states < 2 || len < 2 || nb_substeps < 1 || frame_len <= nb_substeps) return -1;
    return xt_seq_columns(n_states, len, nb_substeps, frame_len, isBL);
}

extern "C" int extrack_sequence_matrix(extrack_ctx* ctx, const extrack_model* m, int32_t bucket_id, double* lp, int64_t n_cols)
{
    if (!ctx || !lp) return xt_fail(ctx, EXTRACK_E_INVALID, "null argument");
    int rc = xt_one_bucket_begin(ctx, m, bucket_id, false, false);
    if (rc) return rc;
    XtBucket& b = ctx->buckets[bucket_id];
    const XtConfig& c = ctx->cfg;
    const int isBL = (b.L != m->max_len) ? 1 : 0;
    if (n_cols != xt_seq_columns(c.S, b.L, c.NS, c.F, isBL)) return xt_fail(ctx, EXTRACK_E_INVALID, "sequence matrix: n_cols must be extrack_sequence_columns(...)");
    const size_t nraw = (size_t)b.N * c.E * c.G;
    if (nraw > ((size_t)1 << 28)) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "sequence matrix: more than 2^28 entries = 2 GiB through host memory (it exists for small inputs; the likelihood needs no matrix: split the tracks)");
    if ((rc = xt_reserve_preds(ctx, nraw * sizeof(double)))) return rc;
    int grid = 0;
    std::vector<XtBucket*> one(1, &b);
    XtLlLaunch l;
    l.d_seq = ctx->d_preds, l.desc_off = xt_desc_base(ctx);
    if ((rc = xt_launch_group(ctx, m, one, l, &grid))) return rc;
    std::vector<double> raw(nraw);
    XT_HIP(ctx, hipMemcpyAsync(raw.data(), ctx->d_preds, nraw * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    XtModelHost mh;
    xt_model_host(m, mh);
    xt_seq_reorder(c, mh, b.N, b.L, isBL, raw.data(), lp);
    return EXTRACK_OK;
}
