// libextrack_hip.so, translation unit 2: log-likelihood + exact gradient (xt_grad.h) behind extrack_loglik_grad.
// Replaces the finite-difference loop that lmfit's BFGS runs around cum_Proba_Cs (extrack/tracking.py:1371).
#include "xt_host.h"

#include "xt_grad.h"
#include "xt_grad_host.h"
#include "xt_reg2.h"
#include "xt_gradr.h"
#include "xt_rev.h"
#include "xt_opg.h"

// Waves per SIMD the register allocator is asked to allow.  Measured on C2 (1e6 x 30, 7 directions, PJ = 4): 2 -> 63 ms,
// 3 -> 53 ms (168 VGPRs, 108 B of scratch per lane), 4 -> 60 ms (128 VGPRs, 272 B of scratch).  Three members per group (C3, 13 directions): 3 waves (232 B of
// scratch) 78.8 ms, 2 waves (248 VGPRs, no scratch) 91.5 ms - the spills are not what bounds this kernel (r03).
#ifndef XT_GRAD_WAVES
#define XT_GRAD_WAVES 3
#endif
template <int G_, int D, int K, int MAXT>
__global__ void __launch_bounds__(MAXT, (MAXT == 256 ? XT_GRAD_WAVES : 1)) xt_grad_kernel(XtKernelArgs a, XtGradArgs ga)
{
    DevCtx cx;
    xt_grad_body<G_, D, K>(a, ga, cx);
}

// Column sums of the per-block partials [nrows][ncol] in a fixed order: one workgroup per column.  Column 0 (sum LL) goes to ll_dst
// (nullptr: dropped - every pass recomputes it, only the first one reports it), column 1 + i to out[dst.idx[i]] (the launch may have
// served the directions in another order than the caller's).
struct XtGradDst {
    int32_t idx[16];
};
__global__ void __launch_bounds__(256) xt_grad_reduce(const double* __restrict__ partials, int nrows, int ncol, double* __restrict__ ll_dst,
                                                      double* __restrict__ out, XtGradDst dst)
{
    __shared__ double sh[256];
    const int col = blockIdx.x;
    double s = 0.0;
    for (int i = threadIdx.x; i < nrows; i += 256) s += partials[(int64_t)i * ncol + col];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (col == 0) {
            if (ll_dst) *ll_dst = sh[0];
        } else {
            out[col - 1 < 16 ? dst.idx[col - 1] : col - 1] = sh[0];
        }
    }
}
// out[i] += add[i]: the launch groups after the first leave {sum LL, gradient} in a scratch row that is added to the evaluation's result
__global__ void __launch_bounds__(64) xt_grad_add_kernel(double* __restrict__ out, const double* __restrict__ add, int n)
{
    for (int i = threadIdx.x; i < n; i += 64) out[i] += add[i];
}
static XtGradDst xt_grad_dst_identity(int base)
{
    XtGradDst d;
    for (int i = 0; i < 16; ++i) d.idx[i] = base + i;
    return d;
}

void xt_grad_reduce_launch(hipStream_t st, const double* partials, int nrows, int ncol, double* ll_dst, double* out)
{
    XtGradDst d;
    for (int i = 0; i < 16; ++i) d.idx[i] = i;
    hipLaunchKernelGGL(xt_grad_reduce, dim3(ncol), dim3(256), 0, st, partials, nrows, ncol, ll_dst, out, d);
}

template <int G_>
static const void* grad_dk(int D, int K, bool wide)
{
#define XT_GK(DD, KK) (wide ? (const void*)xt_grad_kernel<G_, DD, KK, 1024> : (const void*)xt_grad_kernel<G_, DD, KK, 256>)
    if (D == 1 && K == 1) return XT_GK(1, 1);
    if (D == 2 && K == 1) return XT_GK(2, 1);
    if (D == 2 && K == 2) return XT_GK(2, 2);
    if (D == 3 && K == 1) return XT_GK(3, 1);
    if (D == 3 && K == 3) return XT_GK(3, 3);
#undef XT_GK
    return nullptr;
}
// The LDS-resident kernel; G outside 2 .. 4: the generic instantiation.  wide: more than 256 threads.  Built where xt_grad_lds_built(gaps = false) holds.
static const void* xt_grad_kernel_ptr(int G, int D, int K, bool wide)
{
    if (G == 2) return grad_dk<2>(D, K, wide);
    if (G == 3) return grad_dk<3>(D, K, wide);
    if (G == 4) return grad_dk<4>(D, K, wide);
    return grad_dk<0>(D, K, wide);
}

// Missed detections (extrack_loglik_grad_gaps / extrack_loglik_scores_gaps): the refusals of extrack_loglik_gaps, decided here on the host
// before anything is enqueued or recorded - nb_substeps >= 2, more than 4 states, buckets with per-track time steps, and models for which
// xt_grad_pick finds no gap-aware kernel (extrack_grad_gaps.hip).
static int xt_grad_gaps_check(extrack_ctx* ctx, const extrack_model* m, int n_dir)
{
    if (m->nb_substeps != 1) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "missed detections: built for nb_substeps == 1");
    if (m->n_states < 2 || m->n_states > 4) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "missed detections: built for 2, 3 and 4 states");
    XtConfig c;
    std::string err = xt_build_config(m->n_states, m->nb_substeps, m->frame_len, c);
    if (!err.empty()) return xt_fail(ctx, EXTRACK_E_INVALID, err);
    for (const XtBucket& b : ctx->buckets) {
        if (b.d_dt) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "missed detections: not built for buckets with per-track time steps");
        const int D = b.D, K = m->locerr_mode == 0 ? m->locerr_dims : b.KS;
        if (K != 1 && K != D) return xt_fail(ctx, EXTRACK_E_INVALID, m->locerr_mode == 0 ? "locerr_dims must be 1 or the track dimensionality"
                                                                                         : "per-peak localisation error mode but the bucket has no sigma");
        if (xt_grad_pick(c, D, K, m->locerr_mode, n_dir, b.L, 1, ctx->n_cu, true, false, ctx->grad_knobs).path == XT_GRAD_NONE)
            return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "missed detections: the model fits neither gap-aware gradient kernel (more than 1024 groups of sequences or more than 160 KiB of LDS per track)");
    }
    return EXTRACK_OK;
}

static int xt_grad_reserve(extrack_ctx* ctx, double** buf, size_t* cap, size_t n)
{
    if (n <= *cap) return EXTRACK_OK;
    XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr;
    *cap = 0;
    XT_HIP(ctx, hipMalloc(buf, n * sizeof(double)));
    *cap = n;
    return EXTRACK_OK;
}

// One likelihood + gradient evaluation on the context's stream, through the stages below; nothing waits for the device: passes and launch
// groups accumulate in stream order.
//   begin -> per launch group: group_begin -> xt_grad_pick -> xt_grad_rev_launch | xt_grad_run_reg2 | xt_grad_run_passes -> group_done -> OPG, events
struct XtGradEval {
    extrack_ctx* ctx;
    const extrack_model* m;
    int n_dir, TB;
    double* d_out;     // device, 1 + n_dir doubles: {sum LL, d sum LL / d theta_i}
    double* d_scores;  // a scores evaluation (else nullptr): device [sum N][n_dir], every track's dLL_n/dtheta from the forward-mode kernels (reverse mode is
                       // bypassed: its adjoints are accumulated across tracks); rows in bucket-id order, columns in launch order
    XtOpgCols* cols;   // cols->idx[c] = the caller's direction of column c
    bool gaps;         // tracks with missed detections (all-NaN rows): the gap-aware instantiations of the two forward-mode bodies only
    std::vector<double> blob;  // the model blob on the host
    // the launch group in hand
    std::vector<XtBucketDesc> descs;
    int D, K, KS, Lmax = 0, group_index = 0;  // Lmax: the longest track length of the group
    size_t doff, poff = 0;  // its descriptors in ctx->d_desc; the free rows of ctx->d_gpartials start here
    double* g_out;          // d_out for the first group; the later ones write a scratch row that group_done adds to d_out
};

// validate, config, model blob, tangent blocks into the pinned staging buffer, copy
static int xt_grad_begin(XtGradEval& ev, const extrack_model_tangent* tangents)
{
    extrack_ctx* ctx = ev.ctx;
    const extrack_model* m = ev.m;
    const int n_dir = ev.n_dir;
    int rc = xt_validate_model(ctx, m);
    if (rc) return rc;
    if (ctx->buckets.empty()) return xt_fail(ctx, EXTRACK_E_INVALID, "no bucket uploaded");
    if (ev.gaps && (rc = xt_grad_gaps_check(ctx, m, n_dir))) return rc;
    for (int i = 0; i < n_dir; ++i)
        if (!tangents[i].ds2 || !tangents[i].Fs || !tangents[i].TrMat || !tangents[i].p_stay)
            return xt_fail(ctx, EXTRACK_E_INVALID, "null tangent field");
    XT_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = xt_prepare_config(ctx, m))) return rc;
    const XtConfig& c = ctx->cfg;
    XtModelHost mh;
    xt_model_host(m, mh);
    xt_build_blob(mh, c, ev.blob);
    if ((rc = xt_upload_blob(ctx, ev.blob))) return rc;
    const int TB = ev.TB = xt_grad_tb_doubles(c.S, c.G);
    // tangent tables: built in a pinned staging buffer the asynchronous copy reads from; an event guards its reuse by the next call
    const size_t ndbl = (size_t)std::max(n_dir, 1) * TB;
    if (ctx->dblob_busy) {
        XT_HIP(ctx, hipEventSynchronize(ctx->ev_dblob));
        ctx->dblob_busy = false;
    }
    if (ndbl > ctx->h_dblob_cap) {
        if (ctx->h_dblob) (void)hipHostFree(ctx->h_dblob);
        ctx->h_dblob = nullptr;
        ctx->h_dblob_cap = 0;
        XT_HIP(ctx, hipHostMalloc((void**)&ctx->h_dblob, ndbl * sizeof(double)));
        ctx->h_dblob_cap = ndbl;
    }
    if (!ctx->ev_dblob) XT_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_dblob, hipEventDisableTiming));
    for (int i = 0; i < n_dir; ++i) xt_build_tangent_block(mh, tangents[i], c, m->locerr_mode, ctx->h_dblob + (size_t)i * TB);
    if ((rc = xt_grad_reserve(ctx, &ctx->d_dblob, &ctx->dblob_cap, ndbl))) return rc;
    XT_HIP(ctx, hipMemcpyAsync(ctx->d_dblob, ctx->h_dblob, ndbl * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    XT_HIP(ctx, hipEventRecord(ctx->ev_dblob, ctx->stream));
    ctx->dblob_busy = true;
    return EXTRACK_OK;
}

// dims of the group, its bucket descriptors (shared by its passes) -> device
static int xt_grad_group_begin(XtGradEval& ev, const std::vector<XtBucket*>& g)
{
    extrack_ctx* ctx = ev.ctx;
    const extrack_model* m = ev.m;
    ev.g_out = ev.group_index == 0 ? ev.d_out : ctx->d_gtmp;
    ev.poff = 0;  // the previous group's reductions precede this group's kernels in the stream: the partial-sum rows are free again
    const XtBucket& b0 = *g[0];
    ev.D = b0.D;
    ev.KS = b0.KS ? b0.KS : 1;
    ev.Lmax = 0;
    for (const XtBucket* b : g) ev.Lmax = std::max(ev.Lmax, (int)b->L);
    if (m->locerr_mode == 0) {
        ev.K = m->locerr_dims;
        if (ev.K != 1 && ev.K != ev.D) return xt_fail(ctx, EXTRACK_E_INVALID, "locerr_dims must be 1 or the track dimensionality");
    } else {
        if (!b0.d_sigma) return xt_fail(ctx, EXTRACK_E_INVALID, "per-peak localisation error mode but the bucket has no sigma");
        ev.K = b0.KS;
    }
    ev.descs.clear();
    for (XtBucket* b : g) {
        XtBucketDesc d;
        d.tracks = b->d_tracks;
        d.sigma = m->locerr_mode ? b->d_sigma : nullptr;
        d.ll_out = nullptr;
        d.preds_out = nullptr;
        d.N = b->N;
        d.L = b->L;
        d.isBL = (b->L != m->max_len) ? 1 : 0;  // tracking.py:1037-1040
        d.ll_const = -(double)(b->L - 1) * ev.D * 0.5 * XT_LOG2PI;
        if (ev.d_scores) {  // rows of the buckets uploaded before this one come first (the order of extrack_loglik's per_track)
            int64_t row0 = 0;
            for (const XtBucket* o = ctx->buckets.data(); o != b; ++o) row0 += o->N;
            d.scores_out = ev.d_scores + row0 * ev.n_dir;
        }
        ev.descs.push_back(d);
    }
    ctx->desc_shadow.clear();  // this path writes the device table itself: the likelihood launcher's shadow of it no longer holds
    memcpy(ctx->h_desc + ev.doff, ev.descs.data(), ev.descs.size() * sizeof(XtBucketDesc));
    XT_HIP(ctx, hipMemcpyAsync(ctx->d_desc + ev.doff, ctx->h_desc + ev.doff, ev.descs.size() * sizeof(XtBucketDesc), hipMemcpyHostToDevice, ctx->stream));
    XT_HIP(ctx, hipEventRecord(ctx->ev_blob[(ctx->blob_turn - 1u) & 1u], ctx->stream));
    return EXTRACK_OK;
}

// the kernel arguments every family shares
static void xt_grad_common_args(const XtGradEval& ev, int tpb, XtKernelArgs& a)
{
    extrack_ctx* ctx = ev.ctx;
    a.desc = ctx->d_desc + ev.doff;
    a.ndesc = (int32_t)ev.descs.size();
    a.blob = ctx->d_blob;
    a.base_tab = ctx->d_base_tab;
    a.off_tab = ctx->d_off_tab;
    a.TPB = tpb;
    a.min_len = ev.m->min_len;
    a.locerr_mode = ev.m->locerr_mode;
    a.KS = ev.KS;
}

// One pass of a forward-mode family (reg2, gradr, lds): NP directions from dblob (+ NU uniform ones, reg2) through kernel kp, then the
// column sums of its per-block partials -> g_out (column 1 + i -> direction dst.idx[i]; sum LL from the first pass only).
struct XtGradPass {
    const void* kp;
    int threads, tpb;
    size_t lds;
    int oversub;    // block generations per CU
    bool est_occ;   // workgroups per CU from the LDS and thread budget of a CU instead of the device query (lds)
    const double* dblob;
    int p0, NP, NU = 0;
    int tan_lds = 0, PJ = 0;  // lds
    bool r2 = false;          // reg2: one global localisation error, no digit tables; udblob / score_ucol0 follow the NF full directions
    int NF = 0, well_scaled = 0;
    XtGradDst dst;
};
static int xt_grad_pass(XtGradEval& ev, const XtGradPass& p)
{
    extrack_ctx* ctx = ev.ctx;
    if (!p.kp) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "gradient kernel variant not built");
    int occ = 0;
    if (p.est_occ) {  // the LDS-resident kernel: its dynamic-LDS limit follows the pass
        if (p.lds > 64 * 1024) XT_HIP(ctx, hipFuncSetAttribute(p.kp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
        occ = std::max(1, std::min((int)((160 * 1024) / p.lds), 2048 / p.threads));
    } else XT_HIP(ctx, xt_occupancy(ctx, p.kp, p.threads, p.lds, &occ));
    XtKernelArgs a;
    memset(&a, 0, sizeof(a));
    xt_fill_args_from_config(ctx->cfg, a);
    XtGradArgs ga;
    memset(&ga, 0, sizeof(ga));
    // grid: blocks per bucket in proportion to its work, CUs oversubscribed (as the likelihood launcher does); at most as many blocks as
    // the free part of the partial-sum buffer has rows
    const int ncol = p.NP + p.NU + 1;
    const int64_t sg = xt_split_descs((double)occ * ctx->n_cu * p.oversub, (int64_t)((ctx->gpartials_cap - ev.poff) / ncol), ev.descs, p.tpb, a.blk_end);
    if (sg < 0 || ev.poff + (size_t)sg * ncol > ctx->gpartials_cap) return xt_fail(ctx, EXTRACK_E_HIP, "gradient partial-sum buffer too small");
    const int grid = (int)sg;
    xt_grad_common_args(ev, p.tpb, a);
    ga.dblob = p.dblob;
    ga.gpartials = ctx->d_gpartials + ev.poff;
    ga.NP = p.NP, ga.TB = ev.TB, ga.tan_lds = p.tan_lds, ga.PJ = p.PJ;
    ga.score_ld = ev.n_dir, ga.score_col0 = p.p0;
    if (p.r2) {
        a.base_tab = a.off_tab = nullptr;
        a.locerr_mode = 0, a.KS = 1, a.well_scaled = p.well_scaled;
        ga.NU = p.NU, ga.score_ucol0 = p.NF;
        ga.udblob = ctx->d_dblob2 + (size_t)p.NF * ev.TB;
    }
    void* kargs[2] = {(void*)&a, (void*)&ga};
    const hipError_t e = hipLaunchKernel(p.kp, dim3(grid), dim3(p.threads), kargs, p.lds, ctx->stream);
    if (e != hipSuccess) return xt_fail(ctx, EXTRACK_E_HIP, std::string("gradient kernel launch: ") + hipGetErrorString(e));
    hipLaunchKernelGGL(xt_grad_reduce, dim3(ncol), dim3(256), 0, ctx->stream, ctx->d_gpartials + ev.poff, grid, ncol, p.p0 == 0 ? ev.g_out : nullptr,
                       ev.g_out + 1, p.dst);
    XT_HIP(ctx, hipGetLastError());
    ev.poff += (size_t)grid * ncol;
    xt_set_launch_info(ctx, grid, p.threads, p.lds, p.tpb, occ);
    return EXTRACK_OK;
}

// reverse mode (xt_rev.h): one launch whatever the number of directions, one log region per track slot of every block, then the projection
static int xt_grad_rev_launch(XtGradEval& ev, const XtGradPick& pk)
{
    extrack_ctx* ctx = ev.ctx;
    const XtConfig& c = ctx->cfg;
    const int TB = ev.TB, tpb = pk.tpb;
    // pk.path == XT_GRAD_GAPS_REV (a gapped group upgraded by xt_grad_gap_rev): the gap-aware instantiation of its twin, everything else as it is
    const void* kp = pk.path == XT_GRAD_GAPS_REV ? xt_rev_gap_kernel_ptr(c.G, ev.D, ev.K, pk.nbuf) : xt_rev_kernel_ptr(c.G, ev.D, ev.K, pk.nbuf);
    if (!kp) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "gradient kernel variant not built");
    if (pk.lds > 64 * 1024) XT_HIP(ctx, hipFuncSetAttribute(kp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pk.lds));
    int occ = 0, rc;
    XT_HIP(ctx, xt_occupancy(ctx, kp, pk.threads, pk.lds, &occ));
    XtKernelArgs a;
    memset(&a, 0, sizeof(a));
    xt_fill_args_from_config(c, a);
    XtRevArgs ra;
    memset(&ra, 0, sizeof(ra));
    const double target = std::min((double)occ * ctx->n_cu * ctx->grad_knobs.rev_oversub, (double)pk.max_blocks);
    // at most max_blocks log regions: the budget holds for the launched grid, not only for the target
    const int64_t sg = xt_split_descs(target, (int64_t)std::min<size_t>(pk.max_blocks, INT64_MAX), ev.descs, tpb, a.blk_end);
    if (sg < 0) return xt_fail(ctx, EXTRACK_E_INVALID, "reverse-mode gradient: no grid split within the log budget");
    const int grid = (int)sg;
    ra.TB = TB, ra.log_stride = pk.log_stride;
    if ((rc = xt_grad_reserve(ctx, &ctx->d_revlog, &ctx->revlog_cap, (size_t)grid * tpb * (size_t)ra.log_stride))) return rc;
    if ((rc = xt_grad_reserve(ctx, &ctx->d_revadj, &ctx->revadj_cap, (size_t)TB))) return rc;
    if ((rc = xt_grad_reserve(ctx, &ctx->d_gpartials, &ctx->gpartials_cap, ev.poff + (size_t)grid * (TB + 1)))) return rc;
    xt_grad_common_args(ev, tpb, a);
    a.base_tab = a.off_tab = nullptr;
    ra.gpartials = ctx->d_gpartials + ev.poff, ra.log = ctx->d_revlog;
    void* kargs[2] = {(void*)&a, (void*)&ra};
    XT_HIP(ctx, hipLaunchKernel(kp, dim3(grid), dim3(pk.threads), kargs, pk.lds, ctx->stream));
    hipLaunchKernelGGL(xt_grad_reduce, dim3(TB + 1), dim3(256), 0, ctx->stream, ctx->d_gpartials + ev.poff, grid, TB + 1, ev.g_out, ctx->d_revadj,
                       xt_grad_dst_identity(0));
    XT_HIP(ctx, hipGetLastError());
    xt_rev_project(ctx->stream, ctx->d_revadj, ctx->d_dblob, TB, ev.n_dir, ev.g_out + 1);
    XT_HIP(ctx, hipGetLastError());
    ev.poff += (size_t)grid * (TB + 1);
    xt_set_launch_info(ctx, grid, pk.threads, pk.lds, tpb, occ);
    return EXTRACK_OK;
}

// two-state models: register-resident kernels (xt_reg2.h), <= 8 directions per pass, tangents in VGPRs.  pk.path == XT_GRAD_GAPS_REG2 (a gapped
// group upgraded by xt_grad_gap_reg2): the gap-aware instantiations and their block size; split, pass order and score columns are the same
static int xt_grad_run_reg2(XtGradEval& ev, const XtGradPick& pk)
{
    const bool gap = pk.path == XT_GRAD_GAPS_REG2;
    extrack_ctx* ctx = ev.ctx;
    const extrack_model* m = ev.m;
    const int n_dir = ev.n_dir, TB = ev.TB;
    // "uniform" directions (xt_r2_uniform_direction, e.g. pBL) cost no per-step work: they ride along with the first pass
    std::vector<int> full, uni;
    for (int i = 0; i < n_dir; ++i)
        ((int)uni.size() < XT_R2_MAXU && xt_r2_uniform_direction(ctx->h_dblob + (size_t)i * TB) ? uni : full).push_back(i);
    if (full.empty()) {
        full.push_back(uni.back());
        uni.pop_back();
    }
    // device copy of the tangent blocks in launch order: full directions first, then the uniform ones
    const int NF = (int)full.size(), NUn = (int)uni.size();
    int rc = xt_grad_reserve(ctx, &ctx->d_dblob2, &ctx->dblob2_cap, (size_t)n_dir * TB);
    if (rc) return rc;
    for (int i = 0; i < n_dir; ++i) {
        const int src = i < NF ? full[i] : uni[i - NF];
        XT_HIP(ctx, hipMemcpyAsync(ctx->d_dblob2 + (size_t)i * TB, ctx->d_dblob + (size_t)src * TB, (size_t)TB * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    }
    const int npass = (NF + pk.maxnp - 1) / pk.maxnp, per = (NF + npass - 1) / npass;
    if (ev.d_scores)
        for (int i = 0; i < n_dir; ++i) ev.cols->idx[i] = i < NF ? full[i] : uni[i - NF];
    double lo = INFINITY, hi = -INFINITY;
    for (int k = 0; k < m->locerr_dims && k < 3; ++k) {
        lo = std::min(lo, m->locerr[k] * m->locerr[k]);
        hi = std::max(hi, m->locerr[k] * m->locerr[k]);
    }
    XtGradPass p = {};
    p.threads = pk.threads, p.tpb = pk.tpb, p.oversub = ctx->grad_knobs.oversub, p.r2 = true, p.NF = NF;
    p.well_scaled = xt_model_well_scaled(ev.blob, lo, hi) ? 1 : 0;
    // gaps: the lazily normalised variant only under the gap-extended bound (xt_grad_gap_reg2_lazy), else the guarded one
    if (gap) p.well_scaled = xt_grad_gap_reg2_lazy(p.well_scaled != 0, ev.Lmax, ev.blob.size() > 8 ? ev.blob[7] : NAN) ? 1 : 0;
    for (int p0 = 0; p0 < NF && !rc; p0 += per) {
        p.p0 = p0, p.NP = std::min(per, NF - p0), p.NU = p0 == 0 ? NUn : 0;
        p.kp = gap ? xt_r2_grad_gap_kernel(ctx->cfg.F, ev.D, p.NP) : xt_r2_kernel(ctx->cfg.F, ev.D, ev.K, p.NP);
        p.lds = gap ? (size_t)xt_r2_grad_gap_block_bytes(p.NP + p.NU, ev.D, pk.tpw) : (size_t)xt_r2_block_bytes(p.NP + p.NU, ev.D, 0, pk.tpw);
        p.dblob = ctx->d_dblob2 + (size_t)p0 * TB;
        p.dst = xt_grad_dst_identity(0);  // column 1 + i of this launch -> the caller's direction index
        for (int i = 0; i < p.NP; ++i) p.dst.idx[i] = full[p0 + i];
        for (int i = 0; i < p.NU; ++i) p.dst.idx[p.NP + i] = uni[i];
        rc = xt_grad_pass(ev, p);
    }
    return rc;
}

// the forward-mode families with the directions in the caller's order: register + LDS exchange (xt_gradr.h: passes of pk.per directions)
// and LDS-resident (xt_grad.h: passes of pk.npass_dir directions, the geometry is that of the pass)
static int xt_grad_run_passes(XtGradEval& ev, const XtGradPick& pk)
{
    extrack_ctx* ctx = ev.ctx;
    const int G = ctx->cfg.G, D = ev.D, K = ev.K, n_dir = ev.n_dir;
    const bool gradr = pk.path == XT_GRAD_GRADR;
    const int step = gradr ? pk.per : pk.npass_dir;
    XtGradPass p = {};
    p.oversub = 4, p.est_occ = !gradr;
    if (gradr) {
        p.kp = ev.gaps ? xt_gradr_gap_kernel_ptr(G, D, K, pk.NPC) : xt_gradr_kernel_ptr(G, D, K, pk.NPC);
        p.threads = pk.threads, p.tpb = pk.tpb, p.lds = pk.lds;
        if (p.kp && p.lds > 64 * 1024) XT_HIP(ctx, hipFuncSetAttribute(p.kp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));  // once for all passes
    }
    for (int p0 = 0, rc; p0 < n_dir; p0 += step) {
        p.p0 = p0, p.NP = std::min(step, n_dir - p0);
        if (!gradr) {
            const XtGradLdsGeom& gm = pk.gm[p.NP == pk.rem ? 1 : 0];
            p.threads = gm.threads, p.tpb = gm.tpb, p.lds = gm.lds, p.tan_lds = gm.tan_lds ? 1 : 0, p.PJ = gm.PJ;
            p.kp = ev.gaps ? xt_grad_gap_kernel_ptr(G, D, K, gm.threads > 256) : xt_grad_kernel_ptr(G, D, K, gm.threads > 256);
        }
        p.dblob = ctx->d_dblob + (size_t)p0 * ev.TB;
        p.dst = xt_grad_dst_identity(p0);
        if ((rc = xt_grad_pass(ev, p))) return rc;
    }
    return EXTRACK_OK;
}

// more than one launch group (more than XT_MAX_BUCKETS track lengths, or buckets of different layouts): the groups after the first left
// {sum LL, gradient} in a scratch row that is added to d_out in stream order
static void xt_grad_group_done(XtGradEval& ev, size_t nbuckets)
{
    if (ev.group_index > 0) hipLaunchKernelGGL(xt_grad_add_kernel, dim3(1), dim3(64), 0, ev.ctx->stream, ev.d_out, ev.ctx->d_gtmp, ev.n_dir + 1);
    ++ev.group_index;
    ev.doff += nbuckets;
}

// Enqueues the kernels of one likelihood + gradient evaluation on the context's stream; d_out (device, 1 + n_dir doubles) receives
// {sum LL, d sum LL / d theta_i}; scores evaluation: d_scores, cols as in XtGradEval, d_opg (device, [n_dir][n_dir], or nullptr) receives
// sum_n s_n s_n^T.
static int xt_grad_enqueue(extrack_ctx* ctx, const extrack_model* m, int32_t n_dir, const extrack_model_tangent* tangents, double* d_out,
                           double* d_scores = nullptr, XtOpgCols* cols = nullptr, double* d_opg = nullptr, bool gaps = false)
{
    XtGradEval ev = {ctx, m, n_dir, 0, d_out, d_scores, cols, gaps};
    int rc = xt_grad_begin(ev, tangents);
    if (rc) return rc;
    const std::vector<std::vector<XtBucket*>> groups = xt_launch_groups(ctx, XT_MAX_BUCKETS);
    if (ctx->buckets.size() > (size_t)XT_DESC_CAP / 2) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "too many buckets");
    if (d_scores && groups.size() > 1)
        return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "per-track scores: buckets of different layouts or more than 64 track lengths");
    int64_t n_total = 0;
    for (auto& b : ctx->buckets) n_total += b.N;
    if (d_scores)
        for (int i = 0; i < XT_OPG_MAXDIR; ++i) cols->idx[i] = i;
    if (groups.size() > 1 && (rc = xt_grad_reserve(ctx, &ctx->d_gtmp, &ctx->gtmp_cap, (size_t)n_dir + 1))) return rc;
    ev.doff = xt_desc_base(ctx);
    // per-block partial sums of every pass of a group, one after the other (a pass has at most 32 blocks per CU)
    if ((rc = xt_grad_reserve(ctx, &ctx->d_gpartials, &ctx->gpartials_cap, ((size_t)ctx->n_cu * 32 * 4 + XT_MAX_BUCKETS) * ((size_t)n_dir + 16)))) return rc;
    if (!ctx->evg0) XT_HIP(ctx, hipEventCreate(&ctx->evg0));
    if (!ctx->evg1) XT_HIP(ctx, hipEventCreate(&ctx->evg1));
    XT_HIP(ctx, hipEventRecord(ctx->evg0, ctx->stream));
    for (const std::vector<XtBucket*>& g : groups) {
        if ((rc = xt_grad_group_begin(ev, g))) return rc;
        const XtGradPick pk0 = xt_grad_pick(ctx->cfg, ev.D, ev.K, m->locerr_mode, n_dir, g[0]->L, (int)g.size(), ctx->n_cu, gaps, d_scores != nullptr,
                                            ctx->grad_knobs);
        if (pk0.path == XT_GRAD_NONE) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, xt_grad_refusal_text(pk0.refusal));
        // missed detections, two states: the gap-aware register-resident kernels where xt_grad_gap_reg2 says so (else pk0 as it is)
        const XtGradPick pk1 = xt_grad_gap_reg2(pk0, ctx->cfg, ev.D, ev.K, m->locerr_mode, n_dir, ev.Lmax, gaps, ctx->grad_knobs, ctx->gap_reg2_fmask);
        // missed detections, any state count: reverse mode where the gap-free twin of the group would run it (never for a scores evaluation)
        const XtGradPick pk = xt_grad_gap_rev(pk1, ctx->cfg, ev.D, ev.K, m->locerr_mode, n_dir, g[0]->L, (int)g.size(), ctx->n_cu, gaps, d_scores != nullptr,
                                              ctx->grad_knobs);
        rc = pk.path == XT_GRAD_REV || pk.path == XT_GRAD_GAPS_REV ? xt_grad_rev_launch(ev, pk)
                                    : (pk.path == XT_GRAD_REG2 || pk.path == XT_GRAD_GAPS_REG2 ? xt_grad_run_reg2(ev, pk) : xt_grad_run_passes(ev, pk));
        if (rc) return rc;
        ctx->last_grad_path = pk.path;
        xt_grad_group_done(ev, g.size());
    }
    if (d_scores && d_opg) {
        if ((rc = xt_grad_reserve(ctx, &ctx->d_opgpart, &ctx->opgpart_cap, (size_t)xt_opg_tiles(n_total) * xt_opg_pairs(n_dir)))) return rc;
        xt_opg_launch(ctx->stream, d_scores, n_total, n_dir, ctx->d_opgpart, d_opg, *cols);
    }
    XT_HIP(ctx, hipGetLastError());
    XT_HIP(ctx, hipEventRecord(ctx->evg1, ctx->stream));
    ctx->grad_timed = true;
    return EXTRACK_OK;
}

extern "C" int extrack_loglik_grad_async(extrack_ctx* ctx, const extrack_model* m, int32_t n_dir, const extrack_model_tangent* tangents,
                                         double* d_out)
{
    if (!ctx || !d_out || n_dir < 0 || (n_dir > 0 && !tangents)) return xt_fail(ctx, EXTRACK_E_INVALID, "null argument");
    if (n_dir == 0) return extrack_loglik_async(ctx, m, d_out);
    return xt_grad_enqueue(ctx, m, n_dir, tangents, d_out);
}

extern "C" int extrack_loglik_grad_gaps_async(extrack_ctx* ctx, const extrack_model* m, int32_t n_dir, const extrack_model_tangent* tangents,
                                              double* d_out)
{
    if (!ctx || !d_out || n_dir < 0 || (n_dir > 0 && !tangents)) return xt_fail(ctx, EXTRACK_E_INVALID, "null argument");
    if (n_dir == 0) {  // no direction: the gap-aware likelihood kernels (which have no enqueue-only entry point: the sum is copied to d_out)
        double ll = 0.0;
        const int rc = extrack_loglik_gaps(ctx, m, &ll, nullptr);
        if (rc) return rc;
        XT_HIP(ctx, hipMemcpyAsync(d_out, &ll, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return EXTRACK_OK;
    }
    return xt_grad_enqueue(ctx, m, n_dir, tangents, d_out, nullptr, nullptr, nullptr, true);
}

static int xt_loglik_grad_sync(extrack_ctx* ctx, const extrack_model* m, int32_t n_dir, const extrack_model_tangent* tangents, double* total_ll,
                               double* grad, bool gaps)
{
    if (!ctx || !total_ll || n_dir < 0 || (n_dir > 0 && (!tangents || !grad))) return xt_fail(ctx, EXTRACK_E_INVALID, "null argument");
    if (n_dir == 0) return gaps ? extrack_loglik_gaps(ctx, m, total_ll, nullptr) : extrack_loglik(ctx, m, total_ll, nullptr);  // no direction: the likelihood kernels
    int rc = xt_grad_reserve(ctx, &ctx->d_gout, &ctx->gout_cap, (size_t)n_dir + 1);
    if (rc) return rc;
    if ((rc = xt_grad_enqueue(ctx, m, n_dir, tangents, ctx->d_gout, nullptr, nullptr, nullptr, gaps))) return rc;
    std::vector<double> host((size_t)n_dir + 1);
    XT_HIP(ctx, hipMemcpyAsync(host.data(), ctx->d_gout, host.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *total_ll = host[0];
    for (int i = 0; i < n_dir; ++i) grad[i] = host[1 + i];
    return EXTRACK_OK;
}

extern "C" int extrack_loglik_grad(extrack_ctx* ctx, const extrack_model* m, int32_t n_dir, const extrack_model_tangent* tangents,
                                   double* total_ll, double* grad)
{
    return xt_loglik_grad_sync(ctx, m, n_dir, tangents, total_ll, grad, false);
}

extern "C" int extrack_loglik_grad_gaps(extrack_ctx* ctx, const extrack_model* m, int32_t n_dir, const extrack_model_tangent* tangents,
                                        double* total_ll, double* grad)
{
    return xt_loglik_grad_sync(ctx, m, n_dir, tangents, total_ll, grad, true);
}

// Validation + the device score matrix [sum N][n_dir] of a scores evaluation (kept with the context)
static int xt_scores_prepare(extrack_ctx* ctx, int32_t n_dir, const extrack_model_tangent* tangents)
{
    if (!ctx || n_dir < 1 || !tangents) return xt_fail(ctx, EXTRACK_E_INVALID, "per-track scores need at least one direction");
    if (n_dir > XT_OPG_MAXDIR) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "per-track scores: more than 32 directions");
    int64_t n_total = 0;
    for (auto& b : ctx->buckets) n_total += b.N;
    if (n_total < 1) return xt_fail(ctx, EXTRACK_E_INVALID, "no track uploaded");
    return xt_grad_reserve(ctx, &ctx->d_scores, &ctx->scores_cap, (size_t)n_total * n_dir);
}

static int xt_loglik_scores_enqueue(extrack_ctx* ctx, const extrack_model* m, int32_t n_dir, const extrack_model_tangent* tangents, double* d_out,
                                    bool gaps)
{
    if (!ctx || !d_out) return xt_fail(ctx, EXTRACK_E_INVALID, "null argument");
    int rc = xt_scores_prepare(ctx, n_dir, tangents);
    if (rc) return rc;
    XtOpgCols cols;
    return xt_grad_enqueue(ctx, m, n_dir, tangents, d_out, ctx->d_scores, &cols, d_out + 1 + n_dir, gaps);
}

extern "C" int extrack_loglik_scores_async(extrack_ctx* ctx, const extrack_model* m, int32_t n_dir, const extrack_model_tangent* tangents,
                                           double* d_out)
{
    return xt_loglik_scores_enqueue(ctx, m, n_dir, tangents, d_out, false);
}

extern "C" int extrack_loglik_scores_gaps_async(extrack_ctx* ctx, const extrack_model* m, int32_t n_dir, const extrack_model_tangent* tangents,
                                                double* d_out)
{
    return xt_loglik_scores_enqueue(ctx, m, n_dir, tangents, d_out, true);
}

static int xt_loglik_scores_sync(extrack_ctx* ctx, const extrack_model* m, int32_t n_dir, const extrack_model_tangent* tangents, double* total_ll,
                                 double* grad, double* opg, double* scores, bool gaps)
{
    if (!ctx || !total_ll) return xt_fail(ctx, EXTRACK_E_INVALID, "null argument");
    int rc = xt_scores_prepare(ctx, n_dir, tangents);
    if (rc) return rc;
    const size_t nd = (size_t)n_dir;
    if ((rc = xt_grad_reserve(ctx, &ctx->d_gout, &ctx->gout_cap, 1 + nd + nd * nd))) return rc;
    XtOpgCols cols;
    if ((rc = xt_grad_enqueue(ctx, m, n_dir, tangents, ctx->d_gout, ctx->d_scores, &cols, opg ? ctx->d_gout + 1 + nd : nullptr, gaps))) return rc;
    std::vector<double> host(1 + nd + nd * nd);
    XT_HIP(ctx, hipMemcpyAsync(host.data(), ctx->d_gout, (opg ? host.size() : 1 + nd) * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (scores) {
        size_t n_total = 0;
        for (auto& b : ctx->buckets) n_total += (size_t)b.N;
        bool launch_order = true;
        for (int i = 0; i < n_dir; ++i) launch_order = launch_order && cols.idx[i] == i;
        std::vector<double> tmp(launch_order ? 0 : n_total * nd);
        XT_HIP(ctx, hipMemcpyAsync(launch_order ? scores : tmp.data(), ctx->d_scores, n_total * nd * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (!launch_order)  // columns from launch order to the caller's order
            for (size_t r = 0; r < n_total; ++r)
                for (int i = 0; i < n_dir; ++i) scores[r * nd + cols.idx[i]] = tmp[r * nd + i];
    } else {
        XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    *total_ll = host[0];
    if (grad)
        for (int i = 0; i < n_dir; ++i) grad[i] = host[1 + i];
    if (opg)
        for (size_t i = 0; i < nd * nd; ++i) opg[i] = host[1 + nd + i];
    return EXTRACK_OK;
}

extern "C" int extrack_loglik_scores(extrack_ctx* ctx, const extrack_model* m, int32_t n_dir, const extrack_model_tangent* tangents,
                                     double* total_ll, double* grad, double* opg, double* scores)
{
    return xt_loglik_scores_sync(ctx, m, n_dir, tangents, total_ll, grad, opg, scores, false);
}

extern "C" int extrack_loglik_scores_gaps(extrack_ctx* ctx, const extrack_model* m, int32_t n_dir, const extrack_model_tangent* tangents,
                                          double* total_ll, double* grad, double* opg, double* scores)
{
    return xt_loglik_scores_sync(ctx, m, n_dir, tangents, total_ll, grad, opg, scores, true);
}

extern "C" int extrack_last_grad_path(const extrack_ctx* ctx, int32_t* path)
{
    if (!ctx || !path) return EXTRACK_E_INVALID;
    *path = ctx->last_grad_path;
    return EXTRACK_OK;
}

extern "C" int extrack_last_grad_ms(extrack_ctx* ctx, float* ms)
{
    if (!ctx || !ms) return EXTRACK_E_INVALID;
    if (ctx->grad_timed) {
        XT_HIP(ctx, hipEventSynchronize(ctx->evg1));
        XT_HIP(ctx, hipEventElapsedTime(&ctx->grad_ms, ctx->evg0, ctx->evg1));
        ctx->grad_timed = false;
    }
    *ms = ctx->grad_ms;
    return EXTRACK_OK;
}
