// libextrack_hip.so - HIP kernels (gfx950) + C ABI for ExTrack's track-likelihood hot path.
// See include/extrack_hip.h for the contract and xt_kernel.h for the algorithm/data layout.
// This unit: context and buckets, model validation and upload, the grow-only device buffers.  The fixed-window likelihood / posterior path
// lives in extrack_ll.hip, the threshold-fusion path in extrack_th.hip, position refinement in extrack_refine.hip, the gradient in extrack_grad.hip.
#include "xt_host.h"

static std::string g_create_err;

int xt_fail(extrack_ctx* ctx, int code, const std::string& msg)
{
    if (ctx) ctx->err = msg;
    return code;
}

extern "C" int extrack_abi_version(void) { return EXTRACK_ABI_VERSION; }

extern "C" const char* extrack_last_error(const extrack_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

extern "C" int extrack_create(int device_id, extrack_ctx** out)
{
    if (!out) return EXTRACK_E_INVALID;
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_create_err = std::string("no HIP device: ") + hipGetErrorString(e);
        return EXTRACK_E_NODEVICE;
    }
    if (device_id < 0 || device_id >= ndev) {
        g_create_err = "device id out of range";
        return EXTRACK_E_INVALID;
    }
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess) {
        g_create_err = std::string("hipGetDeviceProperties: ") + hipGetErrorString(e);
        return EXTRACK_E_HIP;
    }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        g_create_err = std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
        return EXTRACK_E_NODEVICE;
    }
    extrack_ctx* c = new extrack_ctx();
    c->device = device_id;
    c->n_cu = prop.multiProcessorCount;
    if (const char* ev = getenv("EXTRACK_OVERSUB")) {
        int v = atoi(ev);
        if (v >= 1 && v <= 64) {
            c->oversub = v;
            c->oversub_forced = true;
        }
    }
    if (const char* ev = getenv("EXTRACK_LL_PATH")) c->ll_reg2 = strcmp(ev, "reg2") == 0 ? 1 : (strcmp(ev, "lds") == 0 ? 0 : c->ll_reg2);
    if (const char* ev = getenv("EXTRACK_GAP_REG2_F")) {  // "all" or a list of frame lengths out of 4..7
        int mask = 0;
        if (strcmp(ev, "all") == 0) mask = 0xf0;
        for (const char* p = ev; *p; ++p)
            if (*p >= '4' && *p <= '7') mask |= 1 << (*p - '0');
        c->gap_reg2_fmask = mask;
    }
    XtGradKnobs& gk = c->grad_knobs;
    gk.oversub = c->oversub;
    if (const char* ev = getenv("EXTRACK_GRAD_PATH")) {
        gk.grad_reg2 = strcmp(ev, "lds") == 0 ? 0 : (strcmp(ev, "gradr") == 0 ? 2 : 1);
        gk.grad_rev = strcmp(ev, "rev") == 0 ? 2 : (strcmp(ev, "auto") == 0 ? 1 : 0);
    }
    if (const char* ev = getenv("EXTRACK_REV_OVERSUB")) gk.rev_oversub = std::max(1, atoi(ev));
    if (const char* ev = getenv("EXTRACK_REV_LOG_MB")) gk.rev_log_mb = (size_t)std::max(1, atoi(ev));
    if (const char* ev = getenv("EXTRACK_GRADR_NPC")) gk.gradr_npc = atoi(ev) == 4 ? 4 : (atoi(ev) == 3 ? 3 : 0);
    if (const char* ev = getenv("EXTRACK_GRAD_PJ")) {
        const int v = atoi(ev);
        if (v == 1 || v == 2 || v == 4 || v == 8) gk.lds_pj = v;
    }
    if (const char* ev = getenv("EXTRACK_R2_MAXNP")) {
        const int v = atoi(ev);
        if (v >= 1 && v <= 8) gk.r2_maxnp = v;
    }
    if (const char* ev = getenv("EXTRACK_TH_TT")) {
        int v = atoi(ev);
        if (v >= 1 && v <= 256 && (v & (v - 1)) == 0) c->th_knobs.force_tt = v;
    }
    if (const char* ev = getenv("EXTRACK_TH_THREADS")) {
        int v = atoi(ev);
        if (v >= 64 && v <= 1024 && v % 64 == 0) c->th_knobs.force_threads = v;
    }
    if (const char* ev = getenv("EXTRACK_TH_PLAN_THREADS")) {
        int v = atoi(ev);
        if (v >= 64 && v <= 1024 && v % 64 == 0) {
            c->th_knobs.plan_threads = v;
            c->th_knobs.plan_threads_forced = 1;
        }
    }
    if (const char* ev = getenv("EXTRACK_TH_PLAN_BS")) c->th_plan_bs = atoi(ev);
    if (const char* ev = getenv("EXTRACK_TH_NO_SPLIT")) c->th_no_split = atoi(ev) != 0;
    if (const char* ev = getenv("EXTRACK_TH_SPLIT_PCT")) {
        int hi = 0, lo = 0;
        const int n = sscanf(ev, "%d,%d", &hi, &lo);
        if (n >= 1 && hi > 0 && hi < 100) {
            c->th_split_pct[0] = hi;
            c->th_split_pct[1] = (n == 2 && lo > 0 && lo < hi) ? lo : 0;
        }
    }
    if (const char* ev = getenv("EXTRACK_TH_STAGE_LDS")) c->th_knobs.stage_in_lds_mode = atoi(ev) != 0;
    if (const char* ev = getenv("EXTRACK_TH_NO_GEN_SINGLE")) c->th_knobs.no_gen_single = atoi(ev) != 0;
    if (const char* ev = getenv("EXTRACK_TH_PAIR_LANES")) c->th_pair_lanes = atoi(ev);
    if (const char* ev = getenv("EXTRACK_TH_SINGLE")) c->th_knobs.force_single = atoi(ev) != 0;
    if (getenv("EXTRACK_TH_NO_DIRECT")) c->th_knobs.no_direct = 1;
    if (const char* ev = getenv("EXTRACK_TH_OVERSUB")) {
        int v = atoi(ev);
        if (v >= 1 && v <= 64) c->th_knobs.oversub = v;
    }
#define XT_CREATE(call)                                                             \
    if ((e = (call)) != hipSuccess) {                                               \
        g_create_err = std::string(#call) + ": " + hipGetErrorString(e);            \
        delete c;                                                                   \
        return EXTRACK_E_HIP;                                                       \
    }
    XT_CREATE(hipSetDevice(device_id));
    XT_CREATE(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    XT_CREATE(hipEventCreate(&c->ev0));
    XT_CREATE(hipEventCreate(&c->ev1));
    XT_CREATE(hipEventCreateWithFlags(&c->ev_blob[0], hipEventDisableTiming));
    XT_CREATE(hipEventCreateWithFlags(&c->ev_blob[1], hipEventDisableTiming));
    XT_CREATE(hipMalloc(&c->d_total, sizeof(double)));
    XT_CREATE(hipHostMalloc(&c->h_total, sizeof(double), hipHostMallocMapped));
    XT_CREATE(hipHostGetDevicePointer((void**)&c->h_total_dev, c->h_total, 0));
    XT_CREATE(hipMalloc(&c->d_done, sizeof(unsigned int)));
    XT_CREATE(hipMemset(c->d_done, 0, sizeof(unsigned int)));
    if (const char* ev = getenv("EXTRACK_NO_FUSED")) c->no_fused = atoi(ev) != 0;
    XT_CREATE(hipMalloc(&c->d_desc, XT_DESC_CAP * sizeof(XtBucketDesc)));
    XT_CREATE(hipHostMalloc(&c->h_desc, XT_DESC_CAP * sizeof(XtBucketDesc), hipHostMallocDefault));
#undef XT_CREATE
    *out = c;
    return EXTRACK_OK;
}

static void xt_free_bucket(XtBucket& b)
{
    if (b.owned) {
        if (b.d_tracks) (void)hipFree((void*)b.d_tracks);
        if (b.d_sigma) (void)hipFree((void*)b.d_sigma);
    }
    if (b.d_ll) (void)hipFree(b.d_ll);
    if (b.d_dt) (void)hipFree(b.d_dt);
    if (b.th_members) (void)hipFree(b.th_members);
    if (b.th_mpack) (void)hipFree(b.th_mpack);
    if (b.th_gnew) (void)hipFree(b.th_gnew);
    if (b.th_gstart) (void)hipFree(b.th_gstart);
    if (b.th_hdr) (void)hipFree(b.th_hdr);
    if (b.th_status) (void)hipFree(b.th_status);
    b = XtBucket();
}

extern "C" int extrack_clear_buckets(extrack_ctx* ctx)
{
    if (!ctx) return EXTRACK_E_INVALID;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (auto& b : ctx->buckets) xt_free_bucket(b);
    ctx->buckets.clear();
    xt_map_release(ctx);  // sized by the buckets that just went (extrack_destroy comes through here too)
    xt_cond_release(ctx);
    return EXTRACK_OK;
}

extern "C" void extrack_destroy(extrack_ctx* ctx)
{
    if (!ctx) return;
    extrack_clear_buckets(ctx);
    if (ctx->d_base_tab) (void)hipFree(ctx->d_base_tab);
    if (ctx->d_off_tab) (void)hipFree(ctx->d_off_tab);
    for (extrack_ctx::ThSlot& sl : ctx->th_slot) {
        if (sl.d_ws) (void)hipFree(sl.d_ws);
        if (sl.h_status) (void)hipHostFree(sl.h_status);
        if (sl.d_status) (void)hipFree(sl.d_status);
        if (sl.d_desc) (void)hipFree(sl.d_desc);
        if (sl.d_cend) (void)hipFree(sl.d_cend);
    }
    for (int i = 0; i < extrack_ctx::TH_SLOTS; ++i)
        if (ctx->th_streams[i]) (void)hipStreamDestroy(ctx->th_streams[i]);
    for (int i = 0; i < extrack_ctx::TH_SLOTS + 1; ++i)
        if (ctx->th_ev[i]) (void)hipEventDestroy(ctx->th_ev[i]);
    for (int i = 0; i < 2; ++i) {
        if (ctx->d_blob_s[i]) (void)hipFree(ctx->d_blob_s[i]);
        if (ctx->h_blob_s[i]) (void)hipHostFree(ctx->h_blob_s[i]);
        if (ctx->ev_blob[i]) (void)hipEventDestroy(ctx->ev_blob[i]);
    }
    if (ctx->d_preds) (void)hipFree(ctx->d_preds);
    if (ctx->d_dblob) (void)hipFree(ctx->d_dblob);
    if (ctx->h_dblob) (void)hipHostFree(ctx->h_dblob);
    if (ctx->d_dblob2) (void)hipFree(ctx->d_dblob2);
    if (ctx->ev_dblob) (void)hipEventDestroy(ctx->ev_dblob);
    if (ctx->d_gout) (void)hipFree(ctx->d_gout);
    if (ctx->d_gtmp) (void)hipFree(ctx->d_gtmp);
    if (ctx->d_scores) (void)hipFree(ctx->d_scores);
    if (ctx->d_opgpart) (void)hipFree(ctx->d_opgpart);
    if (ctx->d_revlog) (void)hipFree(ctx->d_revlog);
    if (ctx->d_revadj) (void)hipFree(ctx->d_revadj);
    for (int i = 0; i < extrack_ctx::RF_SLOTS; ++i)
        if (ctx->rf_buf[i]) (void)hipFree(ctx->rf_buf[i]);
    if (ctx->evg0) (void)hipEventDestroy(ctx->evg0);
    if (ctx->evg1) (void)hipEventDestroy(ctx->evg1);
    if (ctx->d_th_blobs) (void)hipFree(ctx->d_th_blobs);
    if (ctx->d_gpartials) (void)hipFree(ctx->d_gpartials);
    if (ctx->d_partials) (void)hipFree(ctx->d_partials);
    if (ctx->d_total) (void)hipFree(ctx->d_total);
    if (ctx->d_big_ws) (void)hipFree(ctx->d_big_ws);
    if (ctx->d_done) (void)hipFree(ctx->d_done);
    if (ctx->h_total) (void)hipHostFree(ctx->h_total);
    if (ctx->d_desc) (void)hipFree(ctx->d_desc);
    if (ctx->h_desc) (void)hipHostFree(ctx->h_desc);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

extern "C" int extrack_set_stream(extrack_ctx* ctx, void* hip_stream)
{
    if (!ctx) return EXTRACK_E_INVALID;
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return EXTRACK_OK;
}

extern "C" int extrack_bucket_count(const extrack_ctx* ctx) { return ctx ? (int)ctx->buckets.size() : EXTRACK_E_INVALID; }

static int xt_check_bucket_shape(extrack_ctx* ctx, int64_t n, int32_t len, int32_t dims, const void* sigma, int32_t sigma_dims)
{
    if (n <= 0) return xt_fail(ctx, EXTRACK_E_INVALID, "bucket must hold at least one track");
    if (len < 2) return xt_fail(ctx, EXTRACK_E_INVALID, "minimal track length = 2");  // tracking.py:149-150
    if (dims < 1 || dims > XT_MAX_DIMS) return xt_fail(ctx, EXTRACK_E_INVALID, "dims must be 1, 2 or 3");
    if (sigma && sigma_dims != 1 && sigma_dims != dims)
        return xt_fail(ctx, EXTRACK_E_INVALID, "sigma_dims must be 1 or dims");  // tracking.py:138-143
    return EXTRACK_OK;
}

extern "C" int extrack_upload_bucket(extrack_ctx* ctx, const double* tracks, int64_t n, int32_t len, int32_t dims,
                                     const double* sigma, int32_t sigma_dims, int32_t* bucket_id_out)
{
    if (!ctx || !tracks) return xt_fail(ctx, EXTRACK_E_INVALID, "null argument");
    int rc = xt_check_bucket_shape(ctx, n, len, dims, sigma, sigma_dims);
    if (rc) return rc;
    XT_HIP(ctx, hipSetDevice(ctx->device));
    XtBucket b;
    b.owned = true;
    b.N = n;
    b.L = len;
    b.D = dims;
    b.KS = sigma ? sigma_dims : 0;
    if (sigma) {  // range of the per-peak errors: lets the 2-state fast path prove its scaling bounds (NaN entries poison their track anyway)
        double lo = INFINITY, hi = -INFINITY;
        const size_t ns = (size_t)n * len * sigma_dims;
        for (size_t i = 0; i < ns; ++i) {
            const double v = sigma[i];
            if (v == v) {
                lo = v < lo ? v : lo;
                hi = v > hi ? v : hi;
            }
        }
        b.sig_min = lo;
        b.sig_max = hi;
    }
    const size_t tb = (size_t)n * len * dims * sizeof(double);
    double* dt = nullptr;
    XT_HIP(ctx, hipMalloc(&dt, tb));
    b.d_tracks = dt;
    hipError_t e = hipMemcpyAsync(dt, tracks, tb, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && sigma) {
        const size_t sb = (size_t)n * len * sigma_dims * sizeof(double);
        double* dsg = nullptr;
        e = hipMalloc(&dsg, sb);
        b.d_sigma = dsg;
        if (e == hipSuccess) e = hipMemcpyAsync(dsg, sigma, sb, hipMemcpyHostToDevice, ctx->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // the caller may free its host buffers on return
    if (e != hipSuccess) {
        xt_free_bucket(b);
        return xt_fail(ctx, EXTRACK_E_HIP, std::string("bucket upload: ") + hipGetErrorString(e));
    }
    ctx->buckets.push_back(b);
    if (bucket_id_out) *bucket_id_out = (int32_t)ctx->buckets.size() - 1;
    return EXTRACK_OK;
}

extern "C" int extrack_attach_bucket(extrack_ctx* ctx, const double* d_tracks, int64_t n, int32_t len, int32_t dims,
                                     const double* d_sigma, int32_t sigma_dims, int32_t* bucket_id_out)
{
    if (!ctx || !d_tracks) return xt_fail(ctx, EXTRACK_E_INVALID, "null argument");
    int rc = xt_check_bucket_shape(ctx, n, len, dims, d_sigma, sigma_dims);
    if (rc) return rc;
    XtBucket b;
    b.owned = false;
    b.d_tracks = d_tracks;
    b.d_sigma = d_sigma;
    b.N = n;
    b.L = len;
    b.D = dims;
    b.KS = d_sigma ? sigma_dims : 0;
    ctx->buckets.push_back(b);
    if (bucket_id_out) *bucket_id_out = (int32_t)ctx->buckets.size() - 1;
    return EXTRACK_OK;
}

extern "C" int extrack_set_bucket_dt(extrack_ctx* ctx, int32_t bucket_id, const double* dt)
{
    if (!ctx) return EXTRACK_E_INVALID;
    if (bucket_id < 0 || bucket_id >= (int)ctx->buckets.size()) return xt_fail(ctx, EXTRACK_E_INVALID, "bucket id out of range");
    XT_HIP(ctx, hipSetDevice(ctx->device));
    XtBucket& b = ctx->buckets[bucket_id];
    XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (b.d_dt) (void)hipFree(b.d_dt);
    b.d_dt = nullptr;
    if (!dt) return EXTRACK_OK;
    const size_t nb = (size_t)b.N * b.L * sizeof(double);
    XT_HIP(ctx, hipMalloc(&b.d_dt, nb));
    XT_HIP(ctx, hipMemcpy(b.d_dt, dt, nb, hipMemcpyHostToDevice));
    return EXTRACK_OK;
}

int xt_validate_model(extrack_ctx* ctx, const extrack_model* m)
{
    if (!m || !m->ds || !m->Fs || !m->TrMat || !m->p_stay) return xt_fail(ctx, EXTRACK_E_INVALID, "null model field");
    if (m->locerr_mode < 0 || m->locerr_mode > 2) return xt_fail(ctx, EXTRACK_E_INVALID, "locerr_mode must be 0, 1 or 2");
    if (m->locerr_mode == 0 && (m->locerr_dims < 1 || m->locerr_dims > 3))
        return xt_fail(ctx, EXTRACK_E_INVALID, "locerr_dims must be 1..3");
    if (m->min_len < 1 || m->max_len < 2) return xt_fail(ctx, EXTRACK_E_INVALID, "min_len must be >= 1 and max_len >= 2");
    return EXTRACK_OK;
}

void xt_model_host(const extrack_model* m, XtModelHost& mh)
{
    mh.S = m->n_states;
    mh.NS = m->nb_substeps;
    mh.locerr_dims = m->locerr_mode == 0 ? m->locerr_dims : 1;
    for (int k = 0; k < 3; ++k) mh.locerr[k] = m->locerr[k];
    mh.slope = m->slope;
    mh.offset = m->offset;
    mh.pBL = m->pBL;
    mh.ds = m->ds;
    mh.Fs = m->Fs;
    mh.TrMat = m->TrMat;
    mh.p_stay = m->p_stay;
}

// Ships a model blob through one of the two pinned staging slots to its device slot (stream-ordered) and makes that slot
// the current one (ctx->d_blob).  The host only waits for the copy issued two evaluations ago.
int xt_upload_blob(extrack_ctx* ctx, const std::vector<double>& blob)
{
    if (blob.size() > ctx->blob_cap) {
        XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (int i = 0; i < 2; ++i) {
            if (ctx->d_blob_s[i]) (void)hipFree(ctx->d_blob_s[i]);
            if (ctx->h_blob_s[i]) (void)hipHostFree(ctx->h_blob_s[i]);
            ctx->d_blob_s[i] = ctx->h_blob_s[i] = nullptr;
            ctx->blob_busy[i] = false;
        }
        ctx->blob_cap = 0;
        for (int i = 0; i < 2; ++i) {
            XT_HIP(ctx, hipMalloc(&ctx->d_blob_s[i], blob.size() * sizeof(double)));
            XT_HIP(ctx, hipHostMalloc(&ctx->h_blob_s[i], blob.size() * sizeof(double), hipHostMallocDefault));
        }
        ctx->blob_cap = blob.size();
    }
    const int slot = (int)(ctx->blob_turn++ & 1u);
    if (ctx->blob_busy[slot]) XT_HIP(ctx, hipEventSynchronize(ctx->ev_blob[slot]));  // the slot's previous copy has left the host buffer
    memcpy(ctx->h_blob_s[slot], blob.data(), blob.size() * sizeof(double));
    XT_HIP(ctx, hipMemcpyAsync(ctx->d_blob_s[slot], ctx->h_blob_s[slot], blob.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    XT_HIP(ctx, hipEventRecord(ctx->ev_blob[slot], ctx->stream));
    ctx->blob_busy[slot] = true;
    ctx->d_blob = ctx->d_blob_s[slot];
    return EXTRACK_OK;
}

// The bucket-descriptor staging area is used in two halves that alternate with the blob slots (same guard events).
size_t xt_desc_base(const extrack_ctx* ctx) { return (size_t)((ctx->blob_turn - 1u) & 1u) * (XT_DESC_CAP / 2); }

int xt_grow_device(extrack_ctx* ctx, void** buf, size_t* cap, size_t bytes, const char* what, size_t alloc, void** pinned)
{
    if (bytes <= *cap) return EXTRACK_OK;
    XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (*buf) (void)hipFree(*buf);
    if (pinned && *pinned) (void)hipHostFree(*pinned);
    *buf = nullptr;
    if (pinned) *pinned = nullptr;
    *cap = 0;
    if (!alloc) alloc = bytes;
    hipError_t e = hipMalloc(buf, alloc);
    if (e == hipSuccess && pinned) e = hipHostMalloc(pinned, alloc, hipHostMallocDefault);
    if (e != hipSuccess) return xt_fail(ctx, EXTRACK_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
    *cap = alloc;
    return EXTRACK_OK;
}

int xt_reserve_preds(extrack_ctx* ctx, size_t bytes) { return xt_grow_device(ctx, (void**)&ctx->d_preds, &ctx->preds_cap, bytes, "posterior buffer"); }

// (Re)builds the digit-slot tables when (S, ns, F) changes.
int xt_prepare_config(extrack_ctx* ctx, const extrack_model* m)
{
    if (ctx->cfg.S != m->n_states || ctx->cfg.NS != m->nb_substeps || ctx->cfg.F != m->frame_len || !ctx->d_base_tab) {
        XtConfig c;
        std::string err = xt_build_config(m->n_states, m->nb_substeps, m->frame_len, c);
        if (!err.empty()) return xt_fail(ctx, EXTRACK_E_INVALID, err);
        XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->d_base_tab) (void)hipFree(ctx->d_base_tab);
        if (ctx->d_off_tab) (void)hipFree(ctx->d_off_tab);
        ctx->d_base_tab = ctx->d_off_tab = nullptr;
        XT_HIP(ctx, hipMalloc(&ctx->d_base_tab, c.base_tab.size() * sizeof(int32_t)));
        XT_HIP(ctx, hipMalloc(&ctx->d_off_tab, c.off_tab.size() * sizeof(int32_t)));
        XT_HIP(ctx, hipMemcpy(ctx->d_base_tab, c.base_tab.data(), c.base_tab.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        XT_HIP(ctx, hipMemcpy(ctx->d_off_tab, c.off_tab.data(), c.off_tab.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        ctx->cfg = c;
    }
    return EXTRACK_OK;
}

// Digit-slot tables + model blob of one evaluation.
int xt_prepare(extrack_ctx* ctx, const extrack_model* m)
{
    int rc = xt_prepare_config(ctx, m);
    if (rc) return rc;
    XtModelHost mh;
    xt_model_host(m, mh);
    xt_build_blob(mh, ctx->cfg, ctx->blob_host);  // kept on the host: the launcher reads the scaling slots of the header
    // a small blob rides in the kernel arguments (XtKernelArgs::blob_inline): no staging copy, one dispatch less per evaluation
    ctx->blob_inline = !ctx->no_fused && ctx->blob_host.size() <= (size_t)XT_INLINE_BLOB;
    if (ctx->blob_inline) return EXTRACK_OK;
    return xt_upload_blob(ctx, ctx->blob_host);
}

int xt_reserve_partials(extrack_ctx* ctx, size_t n)
{
    size_t cap = ctx->partials_cap * sizeof(double);  // partials_cap counts doubles (extrack_th.hip grows the same buffer)
    const int rc = xt_grow_device(ctx, (void**)&ctx->d_partials, &cap, n * sizeof(double), "partial sums");
    ctx->partials_cap = cap / sizeof(double);
    return rc;
}

extern "C" int extrack_last_kernel_ms(extrack_ctx* ctx, float* ms)
{
    if (!ctx || !ms) return EXTRACK_E_INVALID;
    if (!ctx->timed) return xt_fail(ctx, EXTRACK_E_INVALID, "no timed launch yet");
    XT_HIP(ctx, hipEventSynchronize(ctx->ev1));
    XT_HIP(ctx, hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
    return EXTRACK_OK;
}

extern "C" int extrack_last_launch_info(const extrack_ctx* ctx, int32_t info[6])
{
    if (!ctx || !info) return EXTRACK_E_INVALID;
    for (int i = 0; i < 6; ++i) info[i] = ctx->launch_info[i];
    return EXTRACK_OK;
}

extern "C" int extrack_p_stay_table(const double* ds, int32_t S, int32_t ns, const double* cell_dims, int32_t n_cell, double* out)
{
    if (!ds || !out || S < 1 || ns < 1 || (n_cell > 0 && !cell_dims)) return EXTRACK_E_INVALID;
    int G = 1;
    for (int i = 0; i < ns; ++i) G *= S;
    for (int r = 0; r < G; ++r) {
        double sub = 0.0;
        int rr = r;
        for (int c = 0; c < ns; ++c) {
            sub += ds[rr % S] * ds[rr % S];
            rr /= S;
        }
        const double sd = sqrt(sub / ns) + 1e-200;
        double p = 1.0;
        for (int j = 0; j < n_cell; ++j) {
            const double cl = cell_dims[j];
            const double x0 = cl / 2000.0, x1 = cl - cl / 2000.0;
            double acc = 0.0;
            for (int i = 0; i < 1000; ++i) {
                const double x = x0 + (x1 - x0) * (double)i / 999.0;
                // Phi(z) = erfc(-z / sqrt(2)) / 2
                acc += 0.5 * erfc(-((cl - x) / sd) * M_SQRT1_2) - 0.5 * erfc((x / sd) * M_SQRT1_2);
            }
            p *= acc / 1000.0;
        }
        out[r] = p;
    }
    return EXTRACK_OK;
}
