// libextrack_hip.so - HIP kernels (gfx950) + C ABI for ExTrack's track-likelihood hot path.
// See include/extrack_hip.h for the contract and xt_kernel.h for the algorithm/data layout.
// This unit: context and buckets, model upload, the fixed-window likelihood / posterior launcher.  The threshold-fusion path lives in
// extrack_th.hip, position refinement in extrack_refine.hip.
#include "xt_host.h"

#include "xt_dispatch.h"
#include "xt_seqmat.h"
#include "xt_entry.h"
#include "xt_fast2.h"
#include "xt_reg2.h"
#include "xt_big.h"

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
static int xt_prepare(extrack_ctx* ctx, const extrack_model* m)
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

struct DevLauncher {
    extrack_ctx* ctx;
    XtKernelArgs a;
    int threads;
    size_t lds;
    int tracks_per_block = 1;
    // buckets served by this launch (<= XT_MAX_BUCKETS), their descriptors are written at ctx->h_desc[desc_off ...]
    std::vector<XtBucketDesc> descs;
    size_t desc_off = 0;
    int grid = 0, occ = 0;
    hipError_t herr = hipSuccess;
    void* extra_arg = nullptr;  // second kernel argument (xt_big_kernel: its scratch description) or nullptr
    double max_blocks = 0.0;    // > 0: upper bound of the grid (scratch budget of the launch)

    template <int G_, int D, int K, bool PREDS>
    bool run()
    {
        if (threads <= 256) return launch(xt_track_kernel<G_, D, K, PREDS, 256>);
        return launch(xt_track_kernel<G_, D, K, PREDS, 1024>);
    }

    template <int GP, int D, int K>
    bool run_entry()
    {
        if (threads <= 256) return launch(xt_entry_kernel<GP, D, K, 256>);
        return launch(xt_entry_kernel<GP, D, K, 1024>);
    }

    template <int F, int D, int K>
    bool run_f2()
    {
        if (ctx->ll_reg2) {  // register-resident variant (xt_reg2.h)
            const void* kp = xt_r2_kernel(F, D, K, 0);
            return kp ? launch_ptr(kp) : false;
        }
        return launch(xt_ll_s2_kernel<F, D, K>);
    }

    template <class KernT>
    bool launch(KernT kern)
    {
        return launch_ptr((const void*)kern);
    }

    bool launch_ptr(const void* kp)
    {
        if (plan(kp)) enqueue(kp);
        return true;
    }

    // Occupancy and grid split of kernel kp: sets occ, grid and a.blk_end (false + herr on failure).
    bool plan(const void* kp)
    {
        if ((herr = xt_occupancy(ctx, kp, threads, lds, &occ)) != hipSuccess) return false;
        // Split the grid over the buckets in proportion to their work (track batches x positions).  The CUs are
        // oversubscribed: waves of equal work do NOT progress equally (VALU issue is arbitrated by age), so a static
        // one-wave-set-per-CU split ends in an under-occupied tail; with several block generations per CU the hardware
        // dispatcher backfills as blocks retire.
        const int nb = (int)descs.size();
        double target = (double)occ * ctx->n_cu * ctx->oversub;
        int64_t nbsum = 0;
        for (int i = 0; i < nb; ++i) nbsum += (descs[i].N + tracks_per_block - 1) / tracks_per_block;
        // small launches: a block should still walk >= 4 batches (its fixed costs - tables, staging set-up, final reduction - are about
        // one batch's worth), but never fewer blocks than fill the chip once.  125 000 x 30 (the 8-way shard of the headline dataset):
        // 8 generations 0.399 ms, 4 generations 0.389 ms, 1 generation 0.423 ms (r04, same box)
        if (!ctx->oversub_forced) target = std::max((double)occ * ctx->n_cu, std::min(target, (double)nbsum / 4.0));
        if (max_blocks > 0.0) target = std::max((double)nb, std::min(target, max_blocks));
        // hard bound: the partial-sum slots of a launch (xt_max_grid) and the scratch budget, if any
        int64_t cap = (int64_t)xt_max_grid(ctx);
        if (max_blocks > 0.0) cap = std::min(cap, (int64_t)max_blocks);
        const int64_t g = xt_split_descs(target, cap, descs, tracks_per_block, a.blk_end);
        if (g < 0) {
            herr = hipErrorInvalidConfiguration;
            return false;
        }
        grid = (int)g;
        return true;
    }

    // Descriptor upload (when they changed) and the launch of kp on the grid of plan().
    void enqueue(const void* kp)
    {
        const int nb = (int)descs.size();
        // the descriptors only change when the buckets (or the per-track / posterior outputs) do: keep a host shadow of the device table
        // and skip the copy when it already holds them (one dispatch less per evaluation in a fit)
        bool same = !ctx->no_fused && ctx->desc_shadow.size() >= desc_off + (size_t)nb &&
                    memcmp(ctx->desc_shadow.data() + desc_off, descs.data(), nb * sizeof(XtBucketDesc)) == 0;
        if (!same) {
            if (ctx->blob_inline) {  // no blob slot guards this half of the staging area: wait for whatever still reads it
                herr = hipStreamSynchronize(ctx->stream);
                if (herr != hipSuccess) return;
            }
            memcpy(ctx->h_desc + desc_off, descs.data(), nb * sizeof(XtBucketDesc));
            herr = hipMemcpyAsync(ctx->d_desc + desc_off, ctx->h_desc + desc_off, nb * sizeof(XtBucketDesc), hipMemcpyHostToDevice, ctx->stream);
            if (herr != hipSuccess) return;
            if (!ctx->blob_inline) {
                // the staging half is reusable once this copy is done too: move the slot's guard event behind it
                herr = hipEventRecord(ctx->ev_blob[(ctx->blob_turn - 1u) & 1u], ctx->stream);
                if (herr != hipSuccess) return;
            }
            if (ctx->desc_shadow.size() < desc_off + (size_t)nb) ctx->desc_shadow.resize(desc_off + (size_t)nb);
            memcpy(ctx->desc_shadow.data() + desc_off, descs.data(), nb * sizeof(XtBucketDesc));
        }
        a.desc = ctx->d_desc + desc_off;
        a.ndesc = nb;
        void* kargs[2] = {(void*)&a, extra_arg};
        herr = hipLaunchKernel(kp, dim3(grid), dim3(threads), kargs, lds, ctx->stream);
        if (herr == hipSuccess) herr = hipGetLastError();
    }
};

int xt_reserve_partials(extrack_ctx* ctx, size_t n)
{
    if (n <= ctx->partials_cap) return EXTRACK_OK;
    XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->d_partials) (void)hipFree(ctx->d_partials);
    ctx->d_partials = nullptr;
    ctx->partials_cap = 0;
    XT_HIP(ctx, hipMalloc(&ctx->d_partials, n * sizeof(double)));
    ctx->partials_cap = n;
    return EXTRACK_OK;
}

// Launches ONE kernel for a set of buckets that share (dims, sigma dims): partial sums go to d_partials[poff .. poff+grid).
struct XtFuseTotal {
    double* d_total;      // device word that receives the evaluation's total
    double* h_total_dev;  // + the pinned host word (device view) or nullptr
};

static int xt_launch_group(extrack_ctx* ctx, const extrack_model* m, const std::vector<XtBucket*>& bks, bool preds, bool per_track,
                           double* d_preds, size_t poff, size_t desc_off, int* grid_out, double* d_seq = nullptr,
                           const XtFuseTotal* fuse = nullptr, bool gaps = false)
{
    const XtConfig& c = ctx->cfg;
    const XtBucket& b0 = *bks[0];
    const int D = b0.D;
    int K;
    if (m->locerr_mode == 0) {
        K = m->locerr_dims;
        if (K != 1 && K != D) return xt_fail(ctx, EXTRACK_E_INVALID, "locerr_dims must be 1 or the track dimensionality");
    } else {
        if (!b0.d_sigma) return xt_fail(ctx, EXTRACK_E_INVALID, "per-peak localisation error mode but the bucket has no sigma");
        K = b0.KS;
    }
    DevLauncher l;
    l.ctx = ctx;
    memset(&l.a, 0, sizeof(l.a));
    xt_fill_args_from_config(c, l.a);
    int tpb, threads;
    // d_seq (extrack_sequence_matrix): the general kernel writes the log-weight of every sequence of the last position, without the leaving term
    // gaps (extrack_loglik_gaps / extrack_predict_gaps): the general body's gap-aware instantiations only (extrack_gaps.hip), two states included
    const bool fast2 = !d_seq && !gaps && xt_use_fast2(c.S, c.NS, c.F, preds);
    const bool entry = !d_seq && !gaps && !fast2 && xt_use_entry(c.NS, c.G, c.NG, preds);
    if (entry) {
        xt_entry_geometry(c.S, c.G, c.E, c.NG, D, K, tpb, threads, l.lds);
    } else if (fast2) {
        const int tpw = 64 >> (c.F - 1);
        tpb = tpw * XT_F2_WAVES;
        threads = 64 * XT_F2_WAVES;
        l.lds = ctx->ll_reg2 ? (size_t)xt_r2_block_bytes(0, D, m->locerr_mode ? b0.KS : 0, tpw)
                             : (size_t)xt_f2_block_bytes(D, K, m->locerr_mode ? b0.KS : 0, tpw);
    } else {
        xt_geometry(c, D, K, tpb, threads);
        l.lds = xt_lds_bytes(c, D, K, tpb);
    }
    // the sequence state of a track does not fit a workgroup (more than 1024 groups, more than the CU's LDS, posteriors beyond the built group
    // sizes): one lane per track with the state in global memory (xt_big.h)
    bool big = l.lds > 160 * 1024 || (!fast2 && !entry && (threads > 1024 || (preds && c.G > 6)));
    if (const char* ev = getenv("EXTRACK_FORCE_BIG")) big = big || (atoi(ev) != 0 && !d_seq && !gaps);
    XtBigArgs bargs;
    if (big && gaps) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "missed detections: the global-state kernel for big models has no gap-aware variant");
    if (big) {
        if (d_seq) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "sequence matrix: n_states^frame_len sequences per track do not fit a workgroup");
        if (preds && c.F > 15) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "posteriors: frame_len > 15");
        const int NW = 4;
        threads = 64 * NW;
        tpb = threads;
        l.lds = (size_t)(((xt_tab_doubles(c.S, c.G) + 1) & ~1) + threads) * sizeof(double);
        bargs.ws_stride = xt_big_ws_doubles(c.E, D, K);
        size_t budget_mb = 32 * 1024;
        if (const char* ev = getenv("EXTRACK_BIG_WS_MB")) budget_mb = (size_t)std::max(16, atoi(ev));
        const size_t per_block = (size_t)bargs.ws_stride * sizeof(double) * NW;
        const size_t maxb = std::max<size_t>(1, (budget_mb << 20) / per_block);
        if (maxb < bks.size()) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "n_states^frame_len sequences per track: the state of one workgroup per bucket exceeds the scratch budget (EXTRACK_BIG_WS_MB)");
        // the grid never exceeds max_blocks (xt_split_blocks); the scratch is reserved for the grid actually launched, below
        l.max_blocks = (double)std::min<size_t>(maxb, (size_t)ctx->n_cu * 8);
        l.extra_arg = (void*)&bargs;
    }
    l.threads = threads;
    l.tracks_per_block = tpb;
    if (fast2) {
        // range of the localisation variance over the launch -> may the fast path drop its guards (xt_build_blob)?
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
        l.a.well_scaled = ctx->blob_host.size() > 8 ? xt_launch_scaling(ctx->blob_host, lo, hi, m->locerr_mode == 0 && K == 1) : 0;
    }
    l.desc_off = desc_off;
    for (XtBucket* b : bks) {
        XtBucketDesc d;
        d.tracks = b->d_tracks;
        d.sigma = m->locerr_mode ? b->d_sigma : nullptr;
        d.ll_out = per_track ? b->d_ll : nullptr;
        d.preds_out = d_preds;
        d.N = b->N;
        d.L = b->L;
        d.isBL = (!d_seq && b->L != m->max_len) ? 1 : 0;  // tracking.py:1037-1040
        d.ll_const = -(double)(b->L - 1) * D * 0.5 * XT_LOG2PI;
        d.seq_out = d_seq;
        l.descs.push_back(d);
    }
    if (ctx->blob_inline) {
        l.a.blob = nullptr;
        memcpy(l.a.blob_inline, ctx->blob_host.data(), ctx->blob_host.size() * sizeof(double));
    } else {
        l.a.blob = ctx->d_blob;
    }
    if (fuse) {
        l.a.done = ctx->d_done;
        l.a.total_out = fuse->d_total;
        l.a.total_host = fuse->h_total_dev;
    }
    l.a.base_tab = ctx->d_base_tab;
    l.a.off_tab = ctx->d_off_tab;
    l.a.partials = ctx->d_partials + poff;
    l.a.TPB = tpb;
    l.a.min_len = m->min_len;
    l.a.locerr_mode = m->locerr_mode;
    l.a.KS = b0.KS ? b0.KS : 1;
    bool ok;
    if (big) {
        const void* kp = xt_big_kernel_dk(D, K, preds);
        ok = kp != nullptr;
        if (ok && l.plan(kp)) {
            // one ws_stride region per wavefront of the launched grid (xt_big_body indexes ws by blockIdx * NW + wave)
            const size_t need = (size_t)l.grid * (threads / 64) * (size_t)bargs.ws_stride + 64;
            if (need > ctx->big_ws_cap) {
                XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
                if (ctx->d_big_ws) (void)hipFree(ctx->d_big_ws);
                ctx->d_big_ws = nullptr;
                ctx->big_ws_cap = 0;
                XT_HIP(ctx, hipMalloc(&ctx->d_big_ws, need * sizeof(double)));
                ctx->big_ws_cap = need;
            }
            bargs.ws = ctx->d_big_ws;
            l.enqueue(kp);
        }
    } else if (gaps) {
        const void* kp = xt_gap_kernel_ptr(c.NS == 1 ? c.G : 0, D, K, preds, threads > 256);
        ok = kp != nullptr;
        if (ok) l.launch_ptr(kp);
    } else {
        ok = fast2 ? xt_dispatch_f2(c.F, D, K, l) : (entry ? xt_dispatch_entry(xt_entry_gp(c.G), D, K, l) : xt_dispatch(c.G, D, K, preds, l));
    }
    if (!ok)
        return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, preds ? "posteriors are built for n_states <= 6" : "kernel variant not built");
    if (l.herr != hipSuccess) return xt_fail(ctx, EXTRACK_E_HIP, std::string("kernel launch: ") + hipGetErrorString(l.herr));
    xt_set_launch_info(ctx, l.grid, threads, l.lds, tpb, l.occ);
    *grid_out = l.grid;
    return EXTRACK_OK;
}

// Upper bound of the blocks of one launch (= partial-sum slots to reserve).
size_t xt_max_grid(const extrack_ctx* ctx) { return (size_t)ctx->n_cu * 8 * ctx->oversub + XT_MAX_BUCKETS; }

// Missed detections (extrack_loglik_gaps / extrack_predict_gaps): what the gap-aware kernels (extrack_gaps.hip) do not serve is refused here, on
// the host, before anything is enqueued or recorded.  `only`: the one bucket of a posterior call, or nullptr for all buckets.
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
        int tpb, threads;
        xt_geometry(c, D, K, tpb, threads);
        if (threads > 1024 || xt_lds_bytes(c, D, K, tpb) > 160 * 1024)
            return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "missed detections: n_states^frame_len sequences per track do not fit a workgroup (no gap-aware global-state kernel)");
        if (!xt_gap_kernel_ptr(c.G, D, K, only != nullptr, threads > 256)) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "missed detections: kernel variant not built");
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
    XtFuseTotal fz = {d_total, to_host ? ctx->h_total_dev : nullptr};
    ctx->fused_host = fused && to_host;
    XT_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    for (auto& g : groups) {
        int grid = 0;
        if ((rc = xt_launch_group(ctx, m, g, false, per_track, nullptr, poff, doff, &grid, nullptr, fused ? &fz : nullptr, gaps))) return rc;
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

static int xt_predict_sync(extrack_ctx* ctx, const extrack_model* m, int32_t bucket_id, double* preds, bool gaps)
{
    if (!ctx || !preds) return xt_fail(ctx, EXTRACK_E_INVALID, "null argument");
    int rc = xt_validate_model(ctx, m);
    if (rc) return rc;
    if (bucket_id < 0 || bucket_id >= (int)ctx->buckets.size()) return xt_fail(ctx, EXTRACK_E_INVALID, "bucket id out of range");
    if (gaps && (rc = xt_gaps_check(ctx, m, &ctx->buckets[bucket_id]))) return rc;
    if (m->nb_substeps != 1) return xt_fail(ctx, EXTRACK_E_INVALID, "state predictions require nb_substeps == 1");
    XT_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = xt_prepare(ctx, m))) return rc;
    if ((rc = xt_reserve_partials(ctx, xt_max_grid(ctx)))) return rc;
    XtBucket& b = ctx->buckets[bucket_id];
    const size_t nb = (size_t)b.N * b.L * m->n_states * sizeof(double);
    if ((rc = xt_reserve_preds(ctx, nb))) return rc;
    double* d_preds = ctx->d_preds;
    int grid = 0;
    hipError_t e = hipEventRecord(ctx->ev0, ctx->stream);
    std::vector<XtBucket*> one(1, &b);
    rc = xt_launch_group(ctx, m, one, true, false, d_preds, 0, xt_desc_base(ctx), &grid, nullptr, nullptr, gaps);
    if (rc == EXTRACK_OK) {
        if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
        ctx->timed = true;
        if (e == hipSuccess) e = hipMemcpyAsync(preds, d_preds, nb, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = xt_fail(ctx, EXTRACK_E_HIP, std::string("predict: ") + hipGetErrorString(e));
    }
    return rc;
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
    int rc = xt_validate_model(ctx, m);
    if (rc) return rc;
    if (bucket_id < 0 || bucket_id >= (int)ctx->buckets.size()) return xt_fail(ctx, EXTRACK_E_INVALID, "bucket id out of range");
    XT_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = xt_prepare(ctx, m))) return rc;
    if ((rc = xt_reserve_partials(ctx, xt_max_grid(ctx)))) return rc;
    XtBucket& b = ctx->buckets[bucket_id];
    const XtConfig& c = ctx->cfg;
    const int isBL = (b.L != m->max_len) ? 1 : 0;
    if (n_cols != xt_seq_columns(c.S, b.L, c.NS, c.F, isBL)) return xt_fail(ctx, EXTRACK_E_INVALID, "sequence matrix: n_cols must be extrack_sequence_columns(...)");
    const size_t nraw = (size_t)b.N * c.E * c.G;
    if (nraw > ((size_t)1 << 28)) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "sequence matrix: more than 2^28 entries = 2 GiB through host memory (it exists for small inputs; the likelihood needs no matrix: split the tracks)");
    if ((rc = xt_reserve_preds(ctx, nraw * sizeof(double)))) return rc;
    int grid = 0;
    std::vector<XtBucket*> one(1, &b);
    if ((rc = xt_launch_group(ctx, m, one, false, false, nullptr, 0, xt_desc_base(ctx), &grid, ctx->d_preds))) return rc;
    std::vector<double> raw(nraw);
    XT_HIP(ctx, hipMemcpyAsync(raw.data(), ctx->d_preds, nraw * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    XtModelHost mh;
    xt_model_host(m, mh);
    xt_seq_reorder(c, mh, b.N, b.L, isBL, raw.data(), lp);
    return EXTRACK_OK;
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
