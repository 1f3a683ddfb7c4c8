// libextrack_hip.so, translation unit: the threshold-fusion variant (xt_th.h) - plan kernel + apply kernel per launch group - behind
// extrack_loglik_th / extrack_loglik_th_async / extrack_sequence_matrix_th, its posteriors (extrack_predict_th: the plan kernel's prediction
// mode) and the plan stage of the frozen-plan gradient (xt_th_plan_groups, extrack_thgrad.hip).  The launch geometry is computed by the
// host-only functions of xt_th_geom.h.
#include "xt_host.h"

#include "xt_dispatch.h"

// Fit mode walks a chunk with up to 1024 threads; prediction / recording mode is bounded by 256 threads with PW waves per SIMD (xt_th_pred_waves).
template <int D, int K, bool PREDS, int WS = -1, int PW = 4>
__global__ void __launch_bounds__(PREDS ? 256 : 1024, PREDS ? PW : 1) xt_th_plan_kernel(XtThArgs a)
{
    DevCtx cx;
    xt_th_plan_body<D, K, PREDS, WS>(a, cx);
}

// The wave-uniform two-buffer variant runs workgroups of up to 16 wavefronts, two per CU when the LDS allows: 24 wavefronts per CU need 6 per
// SIMD, i.e. at most 80 VGPRs - the allocator takes 77.  Round 4 lost that twice (2 states x 30, 1e6 tracks, evaluation 2.65 -> 3.8 ms): a
// branch with a log() compiled into every variant (now the SEQ instantiation) and two more non-inline constants in the exponential (reverted).
// Asking for 6 waves per SIMD through the launch bound instead (79 VGPRs, no spill) changes the schedule: 2.92 ms - no bound here.
template <int D, int K, bool UNI, bool SINGLE, bool DT, bool SEQ = false>
__global__ void __launch_bounds__(1024) xt_th_apply_kernel(XtThArgs a)
{
    DevCtx cx;
    xt_th_apply_body<D, K, UNI, SINGLE, DT, SEQ>(a, cx);
}

// Kernel selection and launch.  Plan kernel: pilot-track state in LDS / in the global workspace are two instantiations, so that the state
// pointers have a known address space.  Apply kernel, by XtThApplyGeom::mode: 0 general (fewer than 64 tracks per tile), 1 wave-uniform with
// two state buffers, 2 wave-uniform with one, 3 general with one state buffer (more than 64 live sequences), 4 general + the per-sequence
// matrix of the last position; each with / without per-track time steps (a.blob_stride != 0).
typedef void (*XtThKernel)(XtThArgs);
enum XtThKind { XT_TH_PLAN, XT_TH_APPLY, XT_TH_PREDICT };

template <int D, int K, bool UNI, bool SINGLE, bool SEQ = false>
static XtThKernel xt_th_apply_dt(bool dt)
{
    return dt ? xt_th_apply_kernel<D, K, UNI, SINGLE, true, SEQ> : xt_th_apply_kernel<D, K, UNI, SINGLE, false, SEQ>;
}

struct XtThPick {
    XtThKind kind;
    const XtThArgs& a;
    int mode;
    XtThKernel kern = nullptr;
    template <int D, int K>
    bool run_dk()
    {
        const bool dt = a.blob_stride != 0;
        if (kind == XT_TH_PLAN) kern = a.ws_lds ? xt_th_plan_kernel<D, K, false, 1> : xt_th_plan_kernel<D, K, false, 0>;
        else if (kind == XT_TH_PREDICT) kern = xt_th_pred_waves(a.S) == 3 ? xt_th_plan_kernel<D, K, true, -1, 3> : xt_th_plan_kernel<D, K, true, -1, 4>;
        else if (mode == 4) kern = xt_th_apply_dt<D, K, false, false, true>(dt);
        else if (mode == 3) kern = xt_th_apply_dt<D, K, false, true>(dt);
        else if (mode == 2) kern = xt_th_apply_dt<D, K, true, true>(dt);
        else if (mode == 1) kern = xt_th_apply_dt<D, K, true, false>(dt);
        else kern = xt_th_apply_dt<D, K, false, false>(dt);
        return true;
    }
};

static hipError_t xt_th_launch(XtThKind kind, const XtThArgs& a, int D, int K, int grid, int threads, size_t lds, int mode, hipStream_t stream)
{
    XtThPick p = {kind, a, mode};
    if (!xt_dispatch_dk(D, K, p)) return hipErrorInvalidDeviceFunction;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)p.kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(p.kern, dim3(grid), dim3(threads), lds, stream, a);
    return hipGetLastError();
}

hipError_t xt_th_launch_predict(extrack_ctx* ctx, const XtThArgs& a, int D, int K, int grid, int threads, size_t lds)
{
    return xt_th_launch(XT_TH_PREDICT, a, D, K, grid, threads, lds, 0, ctx->stream);
}

// Grows the partial-sum array to n entries, keeping what earlier launches of this evaluation wrote.
static int xt_grow_partials(extrack_ctx* ctx, size_t n)
{
    if (n <= ctx->partials_cap) return EXTRACK_OK;
    const size_t cap = std::max(n, ctx->partials_cap * 2);
    double* nw = nullptr;
    XT_HIP(ctx, hipMalloc(&nw, cap * sizeof(double)));
    if (ctx->d_partials) {
        XT_HIP(ctx, hipMemcpyAsync(nw, ctx->d_partials, ctx->partials_cap * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        (void)hipFree(ctx->d_partials);
    }
    ctx->d_partials = nw;
    ctx->partials_cap = cap;
    return EXTRACK_OK;
}

static int xt_th_reserve_plan(extrack_ctx* ctx, XtBucket& b, int chunk, int capE)
{
    const int64_t nchunks = (b.N + chunk - 1) / chunk;
    if (b.th_members && b.th_capE == capE && b.th_chunk == chunk && b.th_nchunks == nchunks) return EXTRACK_OK;
    XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (b.th_members) (void)hipFree(b.th_members);
    if (b.th_mpack) (void)hipFree(b.th_mpack);
    if (b.th_gnew) (void)hipFree(b.th_gnew);
    if (b.th_gstart) (void)hipFree(b.th_gstart);
    if (b.th_hdr) (void)hipFree(b.th_hdr);
    if (b.th_status) (void)hipFree(b.th_status);
    b.th_members = b.th_gstart = nullptr;
    b.th_mpack = nullptr;
    b.th_gnew = nullptr;
    b.th_hdr = b.th_status = nullptr;
    XT_HIP(ctx, hipMalloc(&b.th_members, (size_t)nchunks * b.L * capE * sizeof(uint16_t)));
    XT_HIP(ctx, hipMalloc(&b.th_mpack, (size_t)nchunks * b.L * capE * sizeof(uint32_t)));
    XT_HIP(ctx, hipMalloc(&b.th_gnew, (size_t)nchunks * b.L * capE));
    XT_HIP(ctx, hipMalloc(&b.th_gstart, (size_t)nchunks * b.L * (capE + 1) * sizeof(uint16_t)));
    XT_HIP(ctx, hipMalloc(&b.th_hdr, (size_t)nchunks * b.L * 2 * sizeof(int32_t)));
    XT_HIP(ctx, hipMalloc(&b.th_status, (size_t)nchunks * 4 * sizeof(int32_t)));
    b.th_capE = capE;
    b.th_chunk = chunk;
    b.th_nchunks = nchunks;
    b.th_maxG = -1;
    return EXTRACK_OK;
}


// Per-track time steps (XtBucket::d_dt): the field-of-view table - hence the stay / end-of-track tables - belongs to the chunk
// (tracking.py:507-511: median over the chunk's tracks of the first column of ds).  model->p_stay then holds one table of G entries
// per chunk; `tables[c]` is the table index of the c-th chunk of this launch.  Builds and uploads one blob per chunk.
static int xt_th_chunk_blobs(extrack_ctx* ctx, const extrack_model* m, const std::vector<int64_t>& tables, int G, int64_t* stride_out)
{
    XtModelHost mh;
    xt_model_host(m, mh);
    std::vector<double> all, one;
    int64_t stride = 0;
    for (size_t c = 0; c < tables.size(); ++c) {
        mh.p_stay = m->p_stay + (size_t)tables[c] * G;
        int G2 = 0;
        xt_th_build_blob(mh, one, G2);
        if (c == 0) {
            stride = (int64_t)one.size();
            all.assign((size_t)stride * tables.size(), 0.0);
        }
        memcpy(all.data() + c * (size_t)stride, one.data(), one.size() * sizeof(double));
    }
    int rc = xt_grow_device(ctx, (void**)&ctx->d_th_blobs, &ctx->th_blobs_cap, all.size() * sizeof(double), "chunk blobs");
    if (rc) return rc;
    {
        hipError_t e = hipMemcpy(ctx->d_th_blobs, all.data(), all.size() * sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            char msg[256];
            snprintf(msg, sizeof(msg), "chunk blobs upload (%zu tables, stride %lld, capacity %zu bytes, dst %p): %s", tables.size(), (long long)stride,
                     ctx->th_blobs_cap, (void*)ctx->d_th_blobs, hipGetErrorString(e));
            return xt_fail(ctx, EXTRACK_E_HIP, msg);
        }
    }
    *stride_out = stride;
    return EXTRACK_OK;
}

int xt_th_locerr_dims(extrack_ctx* ctx, const extrack_model* m, XtBucket* const* bks, int nbk, int* K)
{
    if (m->locerr_mode == 0) {
        *K = m->locerr_dims;
    } else {
        for (int i = 0; i < nbk; ++i)
            if (!bks[i]->d_sigma) return xt_fail(ctx, EXTRACK_E_INVALID, "per-peak localisation error mode but the bucket has no sigma");
        *K = bks[0]->KS;
    }
    const int D = bks[0]->D;
    if (!(*K == 1 || (*K == D && D > 1))) return xt_fail(ctx, EXTRACK_E_INVALID, "locerr_dims must be 1 or the track dimensionality");
    return EXTRACK_OK;
}

// What every threshold-fusion entry point does after its own argument checks: threshold and frame_len checks (substeps: the likelihood's
// bound nb_substeps, else the posteriors' 1), device, the model's table blob -> ctx->d_blob, G = n_states^nb_substeps.
static int xt_th_begin(extrack_ctx* ctx, const extrack_model* m, double threshold, bool substeps, int* G)
{
    if (!(threshold >= 0.0)) return xt_fail(ctx, EXTRACK_E_INVALID, "threshold must be >= 0");
    if (m->frame_len <= (substeps ? m->nb_substeps : 1) || m->frame_len > 15)
        return xt_fail(ctx, EXTRACK_E_INVALID, substeps ? "frame_len must be in (nb_substeps, 15]" : "frame_len must be in (1, 15]");
    XT_HIP(ctx, hipSetDevice(ctx->device));
    XtModelHost mh;
    xt_model_host(m, mh);
    std::vector<double> blob;
    std::string err = xt_th_build_blob(mh, blob, *G);
    if (!err.empty()) return xt_fail(ctx, EXTRACK_E_INVALID, err);
    return xt_upload_blob(ctx, blob);
}

// Launch groups: the buckets that share (dims, sigma dims).  Longest tracks first inside a group: a chunk's plan is a serial walk over its
// positions, so the long chunks are the critical path of the plan kernel and must not be the last ones to start.
static std::vector<std::vector<XtBucket*>> xt_th_groups(extrack_ctx* ctx) { return xt_launch_groups(ctx, SIZE_MAX); }

// Device-side copy of a small host array (bucket descriptors, chunk prefix): grows on demand.
static int xt_th_upload_small(extrack_ctx* ctx, void** d_buf, size_t* cap, const void* src, size_t bytes)
{
    int rc = xt_grow_device(ctx, d_buf, cap, bytes, "launch-group table", bytes * 2);
    if (rc) return rc;
    XT_HIP(ctx, hipMemcpyAsync(*d_buf, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    return EXTRACK_OK;
}

static int xt_th_split_streams(extrack_ctx* ctx)
{
    if (ctx->th_streams[0]) return EXTRACK_OK;
    for (int i = 0; i < extrack_ctx::TH_SLOTS; ++i) XT_HIP(ctx, hipStreamCreateWithFlags(&ctx->th_streams[i], hipStreamNonBlocking));
    for (int i = 0; i < extrack_ctx::TH_SLOTS + 1; ++i) XT_HIP(ctx, hipEventCreateWithFlags(&ctx->th_ev[i], hipEventDisableTiming));
    return EXTRACK_OK;
}

// One launch group of a threshold-fusion evaluation: all buckets that share (dims, sigma dims) are served by ONE plan launch
// and ONE apply launch through a device table of bucket descriptors (a real dataset has one bucket per track length; the plan
// kernel of a single small bucket could not fill the GPU and its latency would add up bucket after bucket).  The group goes through the
// stages below on ctx->stream with one set of per-launch buffers (extrack_ctx::ThSlot):
//   planning:  init -> plan_launch -> plan_finish (-> plan_launch -> plan_finish ... while the capacity grows) -> apply
//   frozen:    init -> frozen_sizes -> fill_descs -> apply
struct XtThGroup {
    extrack_ctx* ctx;
    const extrack_model* m;
    const std::vector<XtBucket*>* bks;
    extrack_ctx::ThSlot* sl;
    const std::vector<int64_t>* chunk_base;  // per-track time steps: index of every bucket's first p_stay table, else nullptr
    bool per_track;
    XtThArgs a;
    int D, K, Lmax;
    std::vector<int32_t> chunk_end;
    XtThPlanGeom pg;            // of the plan launch in flight
    bool force_global = false;  // the learned LDS capacities overflowed: plan with the global workspace
    int maxG = 0, sumE = 0;     // of the plan made (or frozen): largest group count of a step / sum of expanded sequences, over the chunks
    int rc = EXTRACK_OK;        // of a failed plan_finish
};
enum XtThPlanState { XT_TH_PLAN_DONE, XT_TH_PLAN_RETRY_GLOBAL, XT_TH_PLAN_RETRY_GROWN, XT_TH_PLAN_FAILED };

// Common kernel arguments, the chunk prefix, the per-chunk blobs of per-track time steps and the status buffers of the group.
static int xt_th_group_init(XtThGroup& g, extrack_ctx* ctx, const extrack_model* m, const std::vector<XtBucket*>& bks, int slot, double threshold,
                            int32_t max_nb_states, int32_t chunk, int G, bool per_track, const std::vector<int64_t>* chunk_base)
{
    g.ctx = ctx, g.m = m, g.bks = &bks, g.sl = &ctx->th_slot[slot], g.chunk_base = chunk_base, g.per_track = per_track;
    const XtBucket& b0 = *bks[0];
    g.D = b0.D;
    const int nbk = (int)bks.size();
    int rc = xt_th_locerr_dims(ctx, m, bks.data(), nbk, &g.K);
    if (rc) return rc;
    XtThArgs& a = g.a;
    memset(&a, 0, sizeof(a));
    a.blob = ctx->d_blob;
    a.S = m->n_states;
    a.NS = m->nb_substeps;
    a.G = G;
    a.F = m->frame_len;
    a.min_len = m->min_len;
    a.locerr_mode = m->locerr_mode;
    a.KS = b0.KS ? b0.KS : 1;
    a.chunk = chunk;
    a.max_nb = max_nb_states;
    a.threshold = threshold;
    a.pcap = std::min(chunk, XT_TH_PILOT);
    a.pair_lanes_max_p = ctx->th_pair_lanes;
    a.plan_bs = ctx->th_plan_bs;
    a.nbuckets = nbk;
    g.chunk_end.resize(nbk);
    int64_t total = 0;
    g.Lmax = 0;
    for (int i = 0; i < nbk; ++i) {
        total += (bks[i]->N + chunk - 1) / chunk;
        if (total > (int64_t)1 << 30) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "too many chunks");
        g.chunk_end[i] = (int32_t)total;
        g.Lmax = std::max(g.Lmax, bks[i]->L);
    }
    a.nchunks = (int32_t)total;
    a.Lmax = g.Lmax;
    a.L = g.Lmax;
    if (chunk_base) {  // per-track time steps: one blob per chunk, in this launch's chunk order
        std::vector<int64_t> tables;
        for (int i = 0; i < nbk; ++i) {
            const int64_t base = (*chunk_base)[bks[i] - &ctx->buckets[0]];
            for (int64_t c = 0; c < (bks[i]->N + chunk - 1) / chunk; ++c) tables.push_back(base + c);
        }
        int64_t stride = 0;
        if ((rc = xt_th_chunk_blobs(ctx, m, tables, G, &stride))) return rc;
        a.blob = ctx->d_th_blobs;
        a.blob_stride = stride;
    }
    // status of every chunk of the group: one device array, one pinned host copy
    const size_t sbytes = (size_t)total * 4 * sizeof(int32_t);
    return xt_grow_device(ctx, (void**)&g.sl->d_status, &g.sl->status_cap, sbytes, "plan status", sbytes * 2, (void**)&g.sl->h_status);
}

// The group's bucket descriptors and chunk prefix -> device (a.buckets, a.chunk_end).
static int xt_th_fill_descs(XtThGroup& g)
{
    extrack_ctx* ctx = g.ctx;
    const extrack_model* m = g.m;
    const int nbk = (int)g.bks->size();
    std::vector<XtThBucket> desc(nbk);
    for (int i = 0; i < nbk; ++i) {
        XtBucket& b = *(*g.bks)[i];
        XtThBucket& k = desc[i];
        k.tracks = b.d_tracks;
        k.sigma = m->locerr_mode ? b.d_sigma : nullptr;
        k.dt = g.chunk_base ? b.d_dt : nullptr;
        k.ll_out = g.per_track ? b.d_ll : nullptr;
        k.preds_out = nullptr;
        k.N = b.N;
        k.L = b.L;
        k.isBL = (b.L != m->max_len) ? 1 : 0;  // tracking.py:1037-1040
        k.ll_const = -(double)(b.L - 1) * g.D * 0.5 * XT_LOG2PI;
        k.members = b.th_members;
        k.mpack = b.th_mpack;
        k.gstart = b.th_gstart;
        k.gnew = b.th_gnew;
        k.hdr = b.th_hdr;
        k.status = g.sl->d_status + (size_t)(i ? g.chunk_end[i - 1] : 0) * 4;
        k.seq_out = b.d_seqth;
        k.seq_stride = b.seqth_stride;
    }
    int rc;
    if ((rc = xt_th_upload_small(ctx, (void**)&g.sl->d_desc, &g.sl->desc_cap, desc.data(), desc.size() * sizeof(XtThBucket)))) return rc;
    if ((rc = xt_th_upload_small(ctx, (void**)&g.sl->d_cend, &g.sl->cend_cap, g.chunk_end.data(), g.chunk_end.size() * sizeof(int32_t)))) return rc;
    g.a.buckets = g.sl->d_desc;
    g.a.chunk_end = g.sl->d_cend;
    return EXTRACK_OK;
}

// Frozen plan: no plan kernel, no read-back - the buckets still hold the plan of the last planning evaluation and the counts that size the apply launch.
static int xt_th_frozen_sizes(XtThGroup& g)
{
    const std::vector<XtBucket*>& bks = *g.bks;
    bool ok = !g.chunk_base;
    for (size_t i = 0; ok && i < bks.size(); ++i)
        ok = bks[i]->th_members && bks[i]->th_maxG >= 0 && bks[i]->th_capE == bks[0]->th_capE && bks[i]->th_chunk == g.a.chunk;
    if (!ok) return xt_fail(g.ctx, EXTRACK_E_INVALID, "frozen plan: no plan of a previous evaluation with this chunk size for these buckets (evaluate once unfrozen first; per-track time steps are not served)");
    g.a.capE = bks[0]->th_capE;
    g.maxG = g.sumE = 0;
    for (XtBucket* b : bks) {
        g.maxG = std::max(g.maxG, b->th_maxG);
        g.sumE = std::max(g.sumE, b->th_sumE);
    }
    return EXTRACK_OK;
}

// Sizes and launches the plan kernel at the context's current capacity and enqueues the copy of its status words.
static int xt_th_plan_launch(XtThGroup& g)
{
    extrack_ctx* ctx = g.ctx;
    XtThArgs& a = g.a;
    int rc, capE = ctx->th_capE;
    while (capE < a.S * a.G) capE *= 2;
    ctx->th_capE = capE;
    a.capE = capE;
    for (XtBucket* b : *g.bks)
        if ((rc = xt_th_reserve_plan(ctx, *b, a.chunk, capE))) return rc;
    if ((rc = xt_th_fill_descs(g))) return rc;
    const XtThPlanGeom& pg = g.pg = xt_th_plan_geom(a.S, a.G, capE, g.D, g.K, a.F, a.NS, a.pcap, a.nchunks, ctx->n_cu, ctx->th_learnP, ctx->th_learnE,
                                                    g.force_global, ctx->th_knobs);
    a.wsP = pg.wsP, a.wsE = pg.wsE, a.ws_lds = pg.ws_lds, a.plan_glb = pg.plan_glb, a.stP = pg.stP, a.stE = pg.stE, a.ws_stride = pg.ws_stride;
    if ((rc = xt_grow_device(ctx, (void**)&g.sl->d_ws, &g.sl->ws_cap, pg.ws_bytes, "plan workspace"))) return rc;
    a.ws = g.sl->d_ws;
    if (!pg.fits) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "plan tables do not fit the 160 KiB LDS of a CU");
    const hipError_t e = xt_th_launch(XT_TH_PLAN, a, g.D, g.K, pg.grid, pg.plan_threads, pg.lds, 0, ctx->stream);
    if (e != hipSuccess) return xt_fail(ctx, EXTRACK_E_HIP, std::string("plan kernel launch: ") + hipGetErrorString(e));
    XT_HIP(ctx, hipMemcpyAsync(g.sl->h_status, g.sl->d_status, (size_t)a.nchunks * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    return EXTRACK_OK;
}

// Waits for the plan in flight and reads its status: the per-bucket counts a later frozen evaluation sizes its launches with, and either the
// learned capacities (done) or what the next plan_launch needs (the global workspace, or a larger capacity).
static XtThPlanState xt_th_plan_finish(XtThGroup& g)
{
    extrack_ctx* ctx = g.ctx;
    const int32_t* st = g.sl->h_status;
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        g.rc = xt_fail(ctx, EXTRACK_E_HIP, std::string("hipStreamSynchronize(ctx->stream): ") + hipGetErrorString(e));
        return XT_TH_PLAN_FAILED;
    }
    int over = 0, maxE = 0;
    g.maxG = g.sumE = 0;
    for (int c = 0; c < g.a.nchunks; ++c) {
        over |= st[(size_t)c * 4];
        maxE = std::max(maxE, st[(size_t)c * 4 + 1]);
        g.maxG = std::max(g.maxG, st[(size_t)c * 4 + 2]);
        g.sumE = std::max(g.sumE, st[(size_t)c * 4 + 3]);
    }
    for (size_t i = 0; i < g.bks->size(); ++i) {
        XtBucket& b = *(*g.bks)[i];
        b.th_maxG = over ? -1 : 0;
        b.th_sumE = 0;
        for (int c = (i ? g.chunk_end[i - 1] : 0); !over && c < g.chunk_end[i]; ++c) {
            b.th_maxG = std::max(b.th_maxG, st[(size_t)c * 4 + 2]);
            b.th_sumE = std::max(b.th_sumE, st[(size_t)c * 4 + 3]);
        }
    }
    if (!over) {
        // several launch groups of one evaluation in flight (th_split_active): the capacities learned are the largest over its segments
        const int lp = g.maxG + g.maxG / 4 + 2, le = maxE + maxE / 4 + 2;
        ctx->th_learnP = ctx->th_split_active ? std::max(ctx->th_learnP_split, lp) : lp;
        ctx->th_learnE = ctx->th_split_active ? std::max(ctx->th_learnE_split, le) : le;
        ctx->th_learnP_split = ctx->th_learnP;
        ctx->th_learnE_split = ctx->th_learnE;
        return XT_TH_PLAN_DONE;
    }
    if (g.pg.ws_lds) {  // the learned LDS capacities were too small for these parameters: redo with the global workspace
        g.force_global = true;
        return XT_TH_PLAN_RETRY_GLOBAL;
    }
    int ncap = g.a.capE;
    while (ncap < std::max(maxE, g.maxG)) ncap *= 2;
    if (ncap == g.a.capE) ncap *= 2;
    if (ncap > XT_TH_MAXCAP_FIT) {
        g.rc = xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "more than 32768 live state sequences per step (threshold fusion expands every sequence by n_states^nb_substeps before it merges): raise threshold, lower max_nb_states or nb_substeps - or use the fixed-window kernel (fusion='window' / extrack_loglik), which serves this model");
        return XT_TH_PLAN_FAILED;
    }
    ctx->th_capE = ncap;
    return XT_TH_PLAN_RETRY_GROWN;
}

// plan_finish, planning again for as long as the capacity has to grow.
static int xt_th_plan_settle(XtThGroup& g)
{
    for (;;) {
        const XtThPlanState st = xt_th_plan_finish(g);
        if (st == XT_TH_PLAN_DONE) return EXTRACK_OK;
        if (st == XT_TH_PLAN_FAILED) return g.rc;
        int rc = xt_th_plan_launch(g);
        if (rc) return rc;
    }
}

// The apply launch of a planned group: partial sums to d_partials[poff .. poff + grid), poff advanced.
static int xt_th_apply(XtThGroup& g, size_t& poff)
{
    extrack_ctx* ctx = g.ctx;
    XtThArgs& a = g.a;
    bool want_seq = false;  // extrack_sequence_matrix_th
    for (XtBucket* b : *g.bks) want_seq = want_seq || b->d_seqth != nullptr;
    const XtThApplyGeom ag = xt_th_apply_geom(a.S, a.G, g.D, g.K, a.locerr_mode ? a.KS : 0, g.Lmax, a.chunk, a.nchunks, a.nbuckets, g.maxG, g.sumE,
                                              want_seq, ctx->n_cu, ctx->th_knobs);
    a.capG = g.maxG;
    a.plan_cap = ag.plan_cap;
    if (!ag.fits) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "live state sequences do not fit the 160 KiB LDS of a CU");
    a.TT = ag.TT;
    a.logTT = ag.logTT;
    a.bpc = ag.bpc;
    int rc = xt_grow_partials(ctx, poff + (size_t)ag.grid);
    if (rc) return rc;
    a.partials = ctx->d_partials + poff;
    const hipError_t e = xt_th_launch(XT_TH_APPLY, a, g.D, g.K, ag.grid, ag.threads, ag.lds, ag.mode, ctx->stream);
    if (e != hipSuccess) return xt_fail(ctx, EXTRACK_E_HIP, std::string("apply kernel launch: ") + hipGetErrorString(e));
    poff += (size_t)ag.grid;
    if (getenv("EXTRACK_TH_DEBUG"))
        fprintf(stderr, "[th] chunks %d  plan: lds_mode %d wsP %d wsE %d stP %d | maxG %d sumE %d plan_cap %d | apply: uni %d single %d TT %d threads %d lds %zu bpc %d grid %d\n",
                a.nchunks, a.ws_lds, a.wsP, a.wsE, a.stP, g.maxG, g.sumE, a.plan_cap, (int)(ag.TT == 64), ag.single_buf, ag.TT, ag.threads, ag.lds, a.bpc, ag.grid);
    xt_set_launch_info(ctx, ag.grid, ag.threads, ag.lds, ag.TT, ag.blocks_per_cu);
    return EXTRACK_OK;
}

// One launch group on ctx->stream with buffer set 0.  after_plan: the plan is all the caller wants (frozen-plan gradient, extrack_thgrad.hip).
static int xt_th_run_group(extrack_ctx* ctx, const extrack_model* m, const std::vector<XtBucket*>& bks, double threshold, int32_t max_nb_states,
                           int32_t chunk, int G, bool per_track, size_t& poff, const std::vector<int64_t>* chunk_base,
                           const XtThAfterPlan* after_plan = nullptr)
{
    XtThGroup g;
    int rc = xt_th_group_init(g, ctx, m, bks, 0, threshold, max_nb_states, chunk, G, per_track, chunk_base);
    if (rc) return rc;
    if (ctx->th_frozen) {
        if ((rc = xt_th_frozen_sizes(g)) || (rc = xt_th_fill_descs(g))) return rc;
    } else if ((rc = xt_th_plan_launch(g)) || (rc = xt_th_plan_settle(g))) {
        return rc;
    }
    if (after_plan) return (*after_plan)(g.a, g.D, g.K, g.maxG, g.Lmax);
    return xt_th_apply(g, poff);
}

// Large multi-bucket group in steady state (capacities learned, buffers allocated), cut into segments by track length: the long buckets' plan -
// whose critical path is the serial walk over the longest chunk, during which most of the chip idles - is in flight on one stream while
// the shorter segments are planned and applied on others.  Segment j runs on side stream j with buffer set j.  All plans are launched
// first (every launch reads the context's capacities before any plan is read back); then, LAST segment first, each plan is read back
// and applied - the shortest plan is the first to finish, and the partial sums are handed out in that order.
static int xt_th_run_split(extrack_ctx* ctx, const extrack_model* m, const std::vector<std::vector<XtBucket*>>& seg, int64_t gchunks, double threshold,
                           int32_t max_nb_states, int32_t chunk, int G, bool per_track, size_t& poff)
{
    int rc = xt_th_split_streams(ctx);
    if (rc) return rc;
    const int nseg = (int)seg.size();
    // partial sums of all apply launches: reserved up front (a reallocation while another stream's kernel writes would be fatal)
    if ((rc = xt_grow_partials(ctx, poff + (size_t)gchunks + (size_t)nseg * ((size_t)ctx->n_cu * 8 * ctx->th_knobs.oversub * 2 + 64)))) return rc;
    hipStream_t main_stream = ctx->stream;
    XT_HIP(ctx, hipEventRecord(ctx->th_ev[extrack_ctx::TH_SLOTS], main_stream));
    for (int j = 0; j < nseg; ++j) XT_HIP(ctx, hipStreamWaitEvent(ctx->th_streams[j], ctx->th_ev[extrack_ctx::TH_SLOTS], 0));
    ctx->th_split_active = true;
    ctx->th_learnP_split = ctx->th_learnE_split = 0;
    std::vector<XtThGroup> g(nseg);
    for (int j = 0; j < nseg && !rc; ++j) {
        ctx->stream = ctx->th_streams[j];
        if (!(rc = xt_th_group_init(g[j], ctx, m, seg[j], j, threshold, max_nb_states, chunk, G, per_track, nullptr))) rc = xt_th_plan_launch(g[j]);
    }
    for (int j = nseg - 1; j >= 0 && !rc; --j) {
        ctx->stream = ctx->th_streams[j];
        if (!(rc = xt_th_plan_settle(g[j]))) rc = xt_th_apply(g[j], poff);
    }
    ctx->stream = main_stream;
    ctx->th_split_active = false;
    // join (also after a failure: nothing may be left running on the side streams)
    for (int j = 0; j < nseg; ++j) {
        (void)hipEventRecord(ctx->th_ev[j], ctx->th_streams[j]);
        (void)hipStreamWaitEvent(main_stream, ctx->th_ev[j], 0);
    }
    if (rc)
        for (int j = 0; j < nseg; ++j) (void)hipStreamSynchronize(ctx->th_streams[j]);
    return rc;
}

// Enqueues one threshold-fusion evaluation; the scalar ends up in d_total (device).  The plan kernel's status words are read back
// between the plan and the apply launch (the apply geometry depends on the live-sequence counts), everything after that is
// stream-ordered.
static int xt_loglik_th_enqueue(extrack_ctx* ctx, const extrack_model* m, double threshold, int32_t max_nb_states, int32_t chunk,
                                double* d_total, bool per_track)
{
    int rc = xt_validate_model(ctx, m);
    if (rc) return rc;
    if (ctx->buckets.empty()) return xt_fail(ctx, EXTRACK_E_INVALID, "no bucket uploaded");
    if (chunk < 1) return xt_fail(ctx, EXTRACK_E_INVALID, "chunk must be >= 1");
    int G = 0;
    if ((rc = xt_th_begin(ctx, m, threshold, true, &G))) return rc;
    if (m->n_states * G > XT_TH_MAXCAP) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "n_states^(nb_substeps+1) exceeds the plan capacity");
    // per-track time steps: every bucket carries a dt array and the model one p_stay table per chunk (buckets in id order)
    bool dt_mode = false;
    std::vector<int64_t> chunk_base(ctx->buckets.size(), 0);
    {
        size_t ndt = 0;
        int64_t acc = 0;
        for (size_t i = 0; i < ctx->buckets.size(); ++i) {
            ndt += ctx->buckets[i].d_dt ? 1 : 0;
            chunk_base[i] = acc;
            acc += (ctx->buckets[i].N + chunk - 1) / chunk;
        }
        dt_mode = ndt > 0;
        if (dt_mode && ndt != ctx->buckets.size()) return xt_fail(ctx, EXTRACK_E_INVALID, "per-track time steps were set for some buckets only");
        if (dt_mode && (int64_t)m->n_p_stay != acc)
            return xt_fail(ctx, EXTRACK_E_INVALID, "per-track time steps: model->n_p_stay must be the number of chunks (one p_stay table per chunk)");
        if (!dt_mode && m->n_p_stay > 1) return xt_fail(ctx, EXTRACK_E_INVALID, "several p_stay tables but no per-track time steps");
    }
    if (per_track)
        for (auto& b : ctx->buckets)
            if (!b.d_ll) XT_HIP(ctx, hipMalloc(&b.d_ll, (size_t)b.N * sizeof(double)));
    const std::vector<std::vector<XtBucket*>> groups = xt_th_groups(ctx);
    size_t poff = 0;
    XT_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    for (const std::vector<XtBucket*>& grp : groups) {
        int64_t gchunks = 0;
        for (XtBucket* b : grp) gchunks += (b->N + chunk - 1) / chunk;
        // segments by track length (the group is sorted longest first)
        std::vector<std::vector<XtBucket*>> seg;
        {
            size_t k0 = 0;
            for (int t = 0; t < 2 && ctx->th_split_pct[t] > 0; ++t) {
                size_t k1 = k0;
                while (k1 < grp.size() && grp[k1]->L * 100 > grp[0]->L * ctx->th_split_pct[t]) ++k1;
                if (k1 > k0) seg.emplace_back(grp.begin() + k0, grp.begin() + k1);
                k0 = k1;
            }
            if (k0 < grp.size()) seg.emplace_back(grp.begin() + k0, grp.end());
        }
        const bool split = !ctx->th_frozen && !ctx->th_no_split && !dt_mode && grp.size() >= 4 && seg.size() >= 2 && gchunks >= ctx->n_cu && ctx->th_learnE > 0;
        rc = split ? xt_th_run_split(ctx, m, seg, gchunks, threshold, max_nb_states, chunk, G, per_track, poff)
                   : xt_th_run_group(ctx, m, grp, threshold, max_nb_states, chunk, G, per_track, poff, dt_mode ? &chunk_base : nullptr);
        if (rc) return rc;
    }
    XT_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    ctx->timed = true;
    hipLaunchKernelGGL(xt_reduce_partials, dim3(1), dim3(256), 0, ctx->stream, ctx->d_partials, (int)poff, d_total);
    XT_HIP(ctx, hipGetLastError());
    return EXTRACK_OK;
}

// The plan stage alone, for every launch group (buckets sharing dims / sigma dims) of the uploaded dataset: validates like
// xt_loglik_th_enqueue, uploads the threshold-fusion blob (ctx->d_blob), runs the plan kernel (capacity growth included) and hands the
// group's arguments to `cb` (extrack_thgrad.hip launches the frozen-plan gradient kernel there).  One stream, no concurrent groups.
int xt_th_plan_groups(extrack_ctx* ctx, const extrack_model* m, double threshold, int32_t max_nb_states, int32_t chunk, const XtThAfterPlan& cb)
{
    int rc = xt_validate_model(ctx, m);
    if (rc) return rc;
    if (ctx->buckets.empty()) return xt_fail(ctx, EXTRACK_E_INVALID, "no bucket uploaded");
    if (chunk < 1) return xt_fail(ctx, EXTRACK_E_INVALID, "chunk must be >= 1");
    for (auto& b : ctx->buckets)
        if (b.d_dt) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "per-track time steps are not served by the frozen-plan gradient");
    if (m->n_p_stay > 1) return xt_fail(ctx, EXTRACK_E_INVALID, "several p_stay tables but no per-track time steps");
    int G = 0;
    if ((rc = xt_th_begin(ctx, m, threshold, true, &G))) return rc;
    if (m->n_states * G > XT_TH_MAXCAP) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "n_states^(nb_substeps+1) exceeds the plan capacity");
    size_t poff = 0;
    for (const std::vector<XtBucket*>& grp : xt_th_groups(ctx))
        if ((rc = xt_th_run_group(ctx, m, grp, threshold, max_nb_states, chunk, G, false, poff, nullptr, &cb))) return rc;
    return EXTRACK_OK;
}

extern "C" int extrack_th_freeze_plan(extrack_ctx* ctx, int32_t on)
{
    if (!ctx) return EXTRACK_E_INVALID;
    ctx->th_frozen = on != 0;
    return EXTRACK_OK;
}

// Per-sequence log-probabilities of the threshold-fusion kernel for ONE bucket taken as one chunk (what P_Cs_inter_bound_stats_th returns first,
// extrack/tracking.py:650, before the caller's log-sum): lp host [n][n_cols] with n_cols = (sequences alive after the last merge) x
// n_states^nb_substeps, column (g, r) = g * n_states^nb_substeps + r in the reference's order; WITHOUT the leaving / bleaching term of isBL
// tracks (a further expansion by n_states^nb_substeps that the caller adds: its factors depend on the model only).  First call with lp ==
// nullptr to get *n_cols_out.  For small inputs: n * n_cols doubles cross the host.
extern "C" int extrack_sequence_matrix_th(extrack_ctx* ctx, const extrack_model* m, int32_t bucket_id, double threshold, int32_t max_nb_states,
                                          double* lp, int64_t n_cols_cap, int64_t* n_cols_out)
{
    if (!ctx || !n_cols_out) return xt_fail(ctx, EXTRACK_E_INVALID, "null argument");
    if (bucket_id < 0 || bucket_id >= (int)ctx->buckets.size()) return xt_fail(ctx, EXTRACK_E_INVALID, "bucket id out of range");
    int rc = xt_validate_model(ctx, m);
    if (rc) return rc;
    XtBucket& b = ctx->buckets[bucket_id];
    if (b.d_dt) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "sequence matrix: per-track time steps are not served");
    int G = 0;
    if ((rc = xt_th_begin(ctx, m, threshold, true, &G))) return rc;
    const int32_t chunk = (int32_t)std::min<int64_t>(b.N, (int64_t)1 << 30);  // the whole bucket is one chunk: its first 30 tracks decide the merges
    std::vector<XtBucket*> one(1, &b);
    // on every way out: the caller's frozen state is back and the bucket's per-sequence output is off
    struct Restore {
        extrack_ctx* ctx;
        XtBucket& b;
        bool was_frozen;
        ~Restore() { ctx->th_frozen = was_frozen, b.d_seqth = nullptr, b.seqth_stride = 0; }
    } restore = {ctx, b, ctx->th_frozen};
    ctx->th_frozen = false;
    size_t poff = 0;
    if ((rc = xt_grow_partials(ctx, 64))) return rc;
    b.d_seqth = nullptr;
    if ((rc = xt_th_run_group(ctx, m, one, threshold, max_nb_states, chunk, G, false, poff, nullptr))) return rc;  // plans (and evaluates once)
    XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // sequences alive after the last merge step (L - 2); two-position tracks have no merge: the S initial ones
    int32_t hd[2] = {0, m->n_states};
    if (b.L >= 3) XT_HIP(ctx, hipMemcpy(hd, b.th_hdr + (size_t)(b.L - 2) * 2, sizeof(hd), hipMemcpyDeviceToHost));
    const int64_t ncols = (int64_t)hd[1] * G;
    *n_cols_out = ncols;
    if (!lp) return EXTRACK_OK;
    if (n_cols_cap < ncols) return xt_fail(ctx, EXTRACK_E_INVALID, "sequence matrix: output capacity too small");
    const size_t nbytes = (size_t)b.N * (size_t)ncols * sizeof(double);
    if ((rc = xt_reserve_preds(ctx, nbytes))) return rc;
    b.d_seqth = ctx->d_preds;
    b.seqth_stride = (int)ncols;
    ctx->th_frozen = true;  // the plan just made, followed once more with the per-sequence output switched on
    poff = 0;
    if ((rc = xt_th_run_group(ctx, m, one, threshold, max_nb_states, chunk, G, false, poff, nullptr))) return rc;
    XT_HIP(ctx, hipMemcpyAsync(lp, ctx->d_preds, nbytes, hipMemcpyDeviceToHost, ctx->stream));
    XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return EXTRACK_OK;
}

extern "C" int extrack_loglik_th_async(extrack_ctx* ctx, const extrack_model* m, double threshold, int32_t max_nb_states, int32_t chunk,
                                       double* d_total_ll)
{
    if (!ctx) return EXTRACK_E_INVALID;
    return xt_loglik_th_enqueue(ctx, m, threshold, max_nb_states, chunk, d_total_ll ? d_total_ll : ctx->d_total, false);
}

extern "C" int extrack_loglik_th(extrack_ctx* ctx, const extrack_model* m, double threshold, int32_t max_nb_states, int32_t chunk,
                                 double* total_ll, double* per_track)
{
    if (!ctx || !total_ll) return xt_fail(ctx, EXTRACK_E_INVALID, "null argument");
    int rc = xt_loglik_th_enqueue(ctx, m, threshold, max_nb_states, chunk, ctx->d_total, per_track != nullptr);
    if (rc) return rc;
    XT_HIP(ctx, hipMemcpyAsync(ctx->h_total, ctx->d_total, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
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

// The launches of one extrack_predict_th call (a.status: one status block per chunk):
// Pass 0 (probe): the first chunks with the state in the global workspace -> live-sequence counts of this model.
// Pass 1: everything with the state in LDS, capacities = 1.5 x the probe's maxima (when that fits ~40 KiB per workgroup).
// Pass 2 (only after an overflow of pass 1, or when LDS does not fit): everything with the global workspace.
static int xt_th_predict_passes(extrack_ctx* ctx, XtThArgs& a, int D, int K, int nb_max)
{
    const int S = a.S, G = a.G, F = a.F, L = a.L;
    extrack_ctx::ThSlot& sl = ctx->th_slot[0];
    hipError_t e = hipSuccess;
    int rc = EXTRACK_OK;
    const int probe_chunks = 512;
    int pass = a.nchunks <= probe_chunks ? 2 : 0, learnP = 0, learnE = 0;
    const int32_t all_chunks = a.nchunks;
    for (;;) {
        int capE = ctx->th_capE;
        while (capE < S * G) capE *= 2;
        ctx->th_capE = capE;
        a.capE = a.wsP = a.wsE = capE;
        a.ws_lds = 0;
        a.nchunks = pass == 0 ? std::min(all_chunks, probe_chunks) : all_chunks;
        a.cmat_words = 0;
        size_t lds = (size_t)xt_th_plan_lds_doubles(S, G, capE, D, K) * sizeof(double);
        if (pass == 1) {
            const int wp = std::min(capE, std::max(S * G, learnP)) | 1, we = std::min(capE, std::max(S * G, learnE)) | 1;  // odd strides: see the fit-mode launcher
            // bit matrix: only what the probed sequence counts need (a workgroup is one wavefront here: LDS decides how many
            // tracks a CU works on at a time)
            const int cst = (S & (S - 1)) == 0 ? S : 1;
            a.cmat_words = std::min(XT_TH_CMAT_WORDS, std::max(64, we * ((we / cst + 32) >> 5)));
            lds = (size_t)xt_th_plan_lds_doubles(S, G, capE, D, K, a.cmat_words) * sizeof(double);
            const size_t need = lds + (size_t)xt_th_ws_doubles(wp, we, D, K, F, 1, S, a.pcap, true) * sizeof(double);
            if (need <= 40 * 1024) {
                a.ws_lds = 1;
                a.wsP = wp;
                a.wsE = we;
                lds = need;
            } else {
                pass = 2;
                a.cmat_words = 0;
                lds = (size_t)xt_th_plan_lds_doubles(S, G, capE, D, K) * sizeof(double);
            }
        }
        const int threads = nb_max <= 2 ? 64 : 256;
        const int grid = (int)std::min<int64_t>(a.nchunks, (int64_t)ctx->n_cu * (threads == 64 ? 4 : 1) * xt_th_pred_waves(S));
        a.ws_stride = xt_th_hist_doubles(a.wsE, a.pcap, true, L) + (a.ws_lds ? 0 : xt_th_ws_doubles(a.wsP, a.wsE, D, K, F, 1, S, a.pcap, true));
        if ((rc = xt_grow_device(ctx, (void**)&sl.d_ws, &sl.ws_cap, (size_t)a.ws_stride * grid * sizeof(double), "predict_th workspace"))) break;
        a.ws = sl.d_ws;
        if (lds > 160 * 1024) {
            rc = xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "plan tables do not fit the 160 KiB LDS of a CU");
            break;
        }
        e = xt_th_launch_predict(ctx, a, D, K, grid, threads, lds);
        if (e == hipSuccess) {
            ctx->th_status_host.resize((size_t)a.nchunks * 4);
            e = hipMemcpyAsync(ctx->th_status_host.data(), a.status, (size_t)a.nchunks * 4 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            rc = xt_fail(ctx, EXTRACK_E_HIP, std::string("predict_th: ") + hipGetErrorString(e));
            break;
        }
        int over = 0, maxE = 0, maxG = 0;
        for (int c = 0; c < a.nchunks; ++c) {
            over |= ctx->th_status_host[(size_t)c * 4];
            maxE = std::max(maxE, ctx->th_status_host[(size_t)c * 4 + 1]);
            maxG = std::max(maxG, ctx->th_status_host[(size_t)c * 4 + 2]);
        }
        if (over && a.ws_lds) {  // the probe's capacities were too small for some track: global workspace for all
            pass = 2;
            continue;
        }
        if (over) {
            int ncap = capE;
            while (ncap < std::max(maxE, maxG)) ncap *= 2;
            if (ncap == capE) ncap *= 2;
            if (ncap > XT_TH_MAXCAP) {
                rc = xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "more than 8192 live state sequences per step (threshold fusion expands every sequence by n_states^nb_substeps before it merges): raise threshold, lower max_nb_states or nb_substeps - or use the fixed-window kernel (fusion='window' / extrack_loglik), which serves this model");
                break;
            }
            ctx->th_capE = ncap;
            continue;
        }
        if (pass == 0) {
            learnP = maxG + maxG / 2 + 2;
            learnE = maxE + maxE / 2 + 2;
            pass = 1;
            continue;
        }
        break;
    }
    a.nchunks = all_chunks;
    return rc;
}

extern "C" int extrack_predict_th(extrack_ctx* ctx, const extrack_model* m, int32_t bucket_id, double threshold, int32_t max_nb_states,
                                  int32_t nb_max, double* preds)
{
    if (!ctx || !preds) return xt_fail(ctx, EXTRACK_E_INVALID, "null argument");
    int rc = xt_validate_model(ctx, m);
    if (rc) return rc;
    if (bucket_id < 0 || bucket_id >= (int)ctx->buckets.size()) return xt_fail(ctx, EXTRACK_E_INVALID, "bucket id out of range");
    if (m->nb_substeps != 1) return xt_fail(ctx, EXTRACK_E_INVALID, "state predictions require nb_substeps == 1");
    if (nb_max < 1) return xt_fail(ctx, EXTRACK_E_INVALID, "nb_max must be >= 1");
    int G = 0;
    if ((rc = xt_th_begin(ctx, m, threshold, false, &G))) return rc;
    XtBucket& b = ctx->buckets[bucket_id];
    const int S = m->n_states, F = m->frame_len, D = b.D;
    int K;
    XtBucket* const bp = &b;
    if ((rc = xt_th_locerr_dims(ctx, m, &bp, 1, &K))) return rc;
    const size_t nbytes = (size_t)b.N * b.L * S * sizeof(double);
    if ((rc = xt_reserve_preds(ctx, nbytes))) return rc;
    double* d_preds = ctx->d_preds;
    XtThArgs a;
    memset(&a, 0, sizeof(a));
    a.tracks = b.d_tracks;
    a.sigma = m->locerr_mode ? b.d_sigma : nullptr;
    a.blob = ctx->d_blob;
    if (b.d_dt) {  // per-track time steps: one p_stay table (one blob) per chunk of nb_max tracks; model->p_stay covers ALL buckets
        const int64_t nch = (b.N + nb_max - 1) / nb_max;
        int64_t base = 0, total = 0;
        for (size_t i = 0; i < ctx->buckets.size(); ++i) {
            if ((int)i == bucket_id) base = total;
            total += (ctx->buckets[i].N + nb_max - 1) / nb_max;
        }
        if ((int64_t)m->n_p_stay != total)
            return xt_fail(ctx, EXTRACK_E_INVALID, "per-track time steps: model->n_p_stay must be the number of chunks (one p_stay table per chunk of nb_max tracks, buckets in id order)");
        std::vector<int64_t> tables((size_t)nch);
        for (int64_t c = 0; c < nch; ++c) tables[(size_t)c] = base + c;
        int64_t stride = 0;
        if ((rc = xt_th_chunk_blobs(ctx, m, tables, G, &stride))) return rc;
        a.blob = ctx->d_th_blobs;
        a.blob_stride = stride;
        a.dt = b.d_dt;
    } else if (m->n_p_stay > 1) {
        return xt_fail(ctx, EXTRACK_E_INVALID, "several p_stay tables but no per-track time steps");
    }
    a.preds_out = d_preds;
    a.N = b.N;
    a.L = b.L;
    a.S = S;
    a.NS = 1;
    a.G = G;
    a.F = F;
    a.isBL = (b.L != m->max_len) ? 1 : 0;
    a.min_len = m->min_len;
    a.locerr_mode = m->locerr_mode;
    a.KS = b.KS ? b.KS : 1;
    a.chunk = nb_max;
    a.nchunks = (int32_t)((b.N + nb_max - 1) / nb_max);
    a.max_nb = max_nb_states;
    a.threshold = threshold;
    a.pcap = std::min(nb_max, XT_TH_PILOT);  // slots of per-track state: the pilots, then the other tracks of the chunk 30 at a time
    a.pair_lanes_max_p = ctx->th_pair_lanes;
    int32_t* d_status = nullptr;
    hipError_t e = hipMalloc(&d_status, (size_t)a.nchunks * 4 * sizeof(int32_t));
    if (e != hipSuccess) return xt_fail(ctx, EXTRACK_E_HIP, std::string("predict_th: ") + hipGetErrorString(e));
    a.status = d_status;
    (void)hipEventRecord(ctx->ev0, ctx->stream);
    rc = xt_th_predict_passes(ctx, a, D, K, nb_max);
    if (rc == EXTRACK_OK) {
        (void)hipEventRecord(ctx->ev1, ctx->stream);
        ctx->timed = true;
        e = hipMemcpyAsync(preds, d_preds, nbytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = xt_fail(ctx, EXTRACK_E_HIP, std::string("predict_th: ") + hipGetErrorString(e));
    }
    (void)hipFree(d_status);
    return rc;
}

extern "C" int extrack_th_plan_step(extrack_ctx* ctx, int32_t bucket_id, int64_t chunk_index, int32_t t, int32_t* n_expanded,
                                    int32_t* n_groups, uint16_t* members, uint16_t* gstart, int32_t cap)
{
    if (!ctx || !n_expanded || !n_groups) return xt_fail(ctx, EXTRACK_E_INVALID, "null argument");
    if (bucket_id < 0 || bucket_id >= (int)ctx->buckets.size()) return xt_fail(ctx, EXTRACK_E_INVALID, "bucket id out of range");
    XtBucket& b = ctx->buckets[bucket_id];
    if (!b.th_members) return xt_fail(ctx, EXTRACK_E_INVALID, "no threshold-fusion evaluation has run on this bucket");
    if (chunk_index < 0 || chunk_index >= b.th_nchunks || t < 1 || t > b.L - 1) return xt_fail(ctx, EXTRACK_E_INVALID, "chunk or step out of range");
    XT_HIP(ctx, hipSetDevice(ctx->device));
    XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    int32_t h[2];
    XT_HIP(ctx, hipMemcpy(h, b.th_hdr + ((size_t)chunk_index * b.L + t) * 2, sizeof(h), hipMemcpyDeviceToHost));
    *n_expanded = h[0];
    *n_groups = h[1];
    if (members && gstart && h[1] > 0) {
        if (cap < h[0] || cap < h[1] + 1) return xt_fail(ctx, EXTRACK_E_INVALID, "output capacity too small");
        XT_HIP(ctx, hipMemcpy(members, b.th_members + ((size_t)chunk_index * b.L + t) * b.th_capE, (size_t)h[0] * sizeof(uint16_t), hipMemcpyDeviceToHost));
        XT_HIP(ctx, hipMemcpy(gstart, b.th_gstart + ((size_t)chunk_index * b.L + t) * (b.th_capE + 1), (size_t)(h[1] + 1) * sizeof(uint16_t),
                              hipMemcpyDeviceToHost));
    }
    return EXTRACK_OK;
}
