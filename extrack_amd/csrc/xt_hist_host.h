// Host side of the histogram kernel: the model tables (plain C++, layout in xt_hist.h) and, for the HIP translation units, the one launch
// path behind extrack_segment_len_hist and extrack_segment_len_hist_gaps.
#pragma once
#include <math.h>

#include <vector>

#include "xt_hist.h"
#include "xt_tables.h"

static inline void xt_hist_build_blob(const XtModelHost& m, std::vector<double>& blob)
{
    const int S = m.S;
    blob.assign((size_t)xt_hist_blob_doubles(S), 0.0);
    for (int k = 0; k < 3; ++k) {
        const double s = m.locerr[k < m.locerr_dims ? k : 0];
        blob[k] = s * s;
    }
    blob[3] = m.slope;
    blob[4] = m.offset;
    const double qq0 = m.pBL + (1.0 - m.p_stay[0]) - m.pBL * (1.0 - m.p_stay[0]);
    for (int s = 0; s < S; ++s) {
        blob[8 + s] = log(m.Fs[s]);
        blob[16 + s] = log(m.p_stay[s] * (1.0 - m.pBL));                             // histograms.py:129
        const double qq = m.pBL + (1.0 - m.p_stay[s]) - m.pBL * (1.0 - m.p_stay[s]);  // histograms.py:229
        blob[24 + s] = log(qq + (S - 1) * qq0);  // the extra end-of-track state summed out: p_stay[0] whenever it differs (argmax quirk)
        for (int t = 0; t < S; ++t) {
            blob[32 + s * S + t] = log(m.TrMat[s * S + t]);
            blob[32 + S * S + s * S + t] = (m.ds[s] * m.ds[s] + m.ds[t] * m.ds[t]) / 2.0;
        }
    }
}

#if defined(__HIPCC__)
#include "xt_host.h"

// Waves per SIMD asked of the register allocator by the 256-thread histogram kernels, plain and gap-aware (measured: extrack_hist.hip).
#ifndef XT_HIST_WAVES
#define XT_HIST_WAVES 5
#endif

hipError_t xt_hist_reduce_launch(hipStream_t stream, const double* partials, int nblocks, int nbins, double* out);  // extrack_hist.hip

// One bucket's histogram: argument checks, geometry, LDS / workspace choice, launch, reduction over the blocks, copy to the host.
// kernel_of(D, K, threads): the kernel of the calling translation unit (plain or gap-aware) for 256 / 512 threads, nullptr = not built.
static inline int xt_hist_run(extrack_ctx* ctx, const extrack_model* m, int32_t bucket_id, int32_t max_nb_states, double* hist,
                              const void* (*kernel_of)(int D, int K, int threads))
{
    if (!ctx || !hist) return xt_fail(ctx, EXTRACK_E_INVALID, "null argument");
    int rc = xt_validate_model(ctx, m);
    if (rc) return rc;
    if (bucket_id < 0 || bucket_id >= (int)ctx->buckets.size()) return xt_fail(ctx, EXTRACK_E_INVALID, "bucket id out of range");
    if (m->nb_substeps != 1) return xt_fail(ctx, EXTRACK_E_INVALID, "state-duration histograms are defined for nb_substeps == 1");
    if (max_nb_states < 1) return xt_fail(ctx, EXTRACK_E_INVALID, "max_nb_states must be >= 1");
    const int S = m->n_states;
    if (S < 2 || S > XT_MAX_STATES) return xt_fail(ctx, EXTRACK_E_INVALID, "n_states must be in [2, 8]");
    XT_HIP(ctx, hipSetDevice(ctx->device));
    XtBucket& b = ctx->buckets[bucket_id];
    const int D = b.D, L = b.L;
    int K;
    XtBucket* const bp = &b;
    if ((rc = xt_th_locerr_dims(ctx, m, &bp, 1, &K))) return rc;
    XtHistArgs a;
    memset(&a, 0, sizeof(a));
    a.bits = S <= 2 ? 1 : (S <= 4 ? 2 : 3);
    a.HW = (L * a.bits + 63) / 64;
    if (a.HW > XT_HIST_MAXW) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "track too long for the state-history words (len * bits per state <= 4096)");
    a.K = max_nb_states;
    a.PC = std::max(max_nb_states, S * S);
    if ((int64_t)a.PC * S > 16384) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "max_nb_states * n_states > 16384 is not built");
    a.NC = 1;
    while (a.NC < a.PC * S) a.NC <<= 1;
    XtModelHost mh;
    xt_model_host(m, mh);
    std::vector<double> blob;
    xt_hist_build_blob(mh, blob);
    if ((rc = xt_upload_blob(ctx, blob))) return rc;
    a.tracks = b.d_tracks;
    a.sigma = m->locerr_mode ? b.d_sigma : nullptr;
    a.blob = ctx->d_blob;
    a.N = b.N;
    a.L = L;
    a.S = S;
    a.KS = b.KS ? b.KS : 1;
    a.locerr_mode = m->locerr_mode;
    a.isBL = (L != m->max_len) ? 1 : 0;
    a.min_l = m->min_len;
    const int KSl = m->locerr_mode ? a.KS : 0;
    // workgroup size 256; 512 threads (2 candidates per thread at max_nb_states 500) were measured SLOWER: 104 vs 79 ms per 1e5 x 30 - twice the
    // stages cross wavefronts (LDS + barrier) and a CU holds the same two tracks (EXTRACK_HIST_THREADS=512 keeps the variant reachable)
    int threads = 256;
    if (const char* ev = getenv("EXTRACK_HIST_THREADS")) threads = atoi(ev) == 512 ? 512 : 256;
    size_t lds = xt_hist_lds_doubles(S, L, D, K, KSl, a.PC, a.NC, a.HW, threads, true) * sizeof(double);
    // parent arrays (the surviving sequences of the previous position) in LDS, or in a per-workgroup region of global memory when that
    // lets more workgroups share a CU: at max_nb_states 500 the LDS copy leaves room for 2 (78 KB each), the global one for 5 - measured
    // r03, 1e5 x 30: 78.3 -> 68.1 ms (then 61.4 ms with the register bound below); at 120 the LDS copy already allows 8 and is the faster one (24.5 vs 26.3 ms)
    const size_t lds_g = xt_hist_lds_doubles(S, L, D, K, KSl, a.PC, a.NC, a.HW, threads, false) * sizeof(double);
    auto per_cu_of = [](size_t bytes) { return (int)std::min<size_t>(8, (160 * 1024) / std::max<size_t>(bytes, 1)); };
    a.par_lds = (lds <= 150 * 1024 && std::min(XT_HIST_WAVES, per_cu_of(lds_g)) <= std::min(XT_HIST_WAVES, per_cu_of(lds))) ? 1 : 0;  // XT_HIST_WAVES workgroups per CU is what the registers allow
    if (const char* ev = getenv("EXTRACK_HIST_PAR_LDS")) a.par_lds = (lds <= 150 * 1024 && atoi(ev) != 0) ? 1 : 0;
    if (!a.par_lds) lds = lds_g;
    if (lds > 160 * 1024) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "candidate arrays do not fit the 160 KiB LDS of a CU: lower max_nb_states");
    const int per_cu = std::max(1, std::min(8, (int)((160 * 1024) / lds)));
    const int grid = (int)std::min<int64_t>(b.N, (int64_t)ctx->n_cu * per_cu * 2);
    a.ws_stride = 2 * (int64_t)xt_hist_parent_doubles(a.PC, D, K, a.HW);
    if (!a.par_lds) {
        extrack_ctx::ThSlot& sl = ctx->th_slot[0];  // the workspace of the threshold-fusion plan kernel, which never runs beside this one
        if ((rc = xt_grow_device(ctx, (void**)&sl.d_ws, &sl.ws_cap, (size_t)a.ws_stride * grid * sizeof(double), "histogram workspace"))) return rc;
        a.ws = sl.d_ws;
    }
    const int nbins = (L - 1) * S;
    if ((rc = xt_reserve_partials(ctx, (size_t)grid * nbins + nbins))) return rc;
    a.partials = ctx->d_partials;
    XT_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    const void* kp = kernel_of(D, K, threads);
    if (!kp) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "histogram kernel variant not built");
    hipError_t e = hipSuccess;
    if (lds > 64 * 1024) e = hipFuncSetAttribute(kp, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e == hipSuccess) {
        void* kargs[1] = {(void*)&a};
        e = hipLaunchKernel(kp, dim3(grid), dim3(threads), kargs, lds, ctx->stream);
        if (e == hipSuccess) e = hipGetLastError();
    }
    if (e != hipSuccess) return xt_fail(ctx, EXTRACK_E_HIP, std::string("histogram kernel launch: ") + hipGetErrorString(e));
    XT_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    ctx->timed = true;
    double* d_out = ctx->d_partials + (size_t)grid * nbins;
    XT_HIP(ctx, xt_hist_reduce_launch(ctx->stream, ctx->d_partials, grid, nbins, d_out));
    XT_HIP(ctx, hipMemcpyAsync(hist, d_out, (size_t)nbins * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    xt_set_launch_info(ctx, grid, threads, lds, 1, per_cu);
    return EXTRACK_OK;
}
#endif
