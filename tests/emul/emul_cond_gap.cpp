// TEST INFRASTRUCTURE ONLY: the fixed-state smoother body (xt_cond.h) with GAPS = true (missed detections: all-NaN rows) and, for the
// comparison on gap-free data, with GAPS = false, on CPU threads; one bucket per emulated launch, with the model tables built as the library
// builds them (xt_tables.h).  Built into its own library (run_emul_cond_gap.py).
#include <algorithm>
#include <cstring>
#include <vector>

#include "emul_ctx.h"
#include "../../extrack_amd/csrc/xt_cond.h"
#include "../../extrack_amd/csrc/xt_tables.h"

template <int D, int K, bool GAPS>
static void run_cond_g(const XtCondArgs& a, int nblocks, int threads, size_t ldsd)
{
    if (a.ws_global)
        th_emul_blocks(nblocks, threads, ldsd, [&](HostCtx& cx) { xt_cond_body<D, K, true, GAPS>(a, cx); });
    else
        th_emul_blocks(nblocks, threads, ldsd, [&](HostCtx& cx) { xt_cond_body<D, K, false, GAPS>(a, cx); });
}

static bool g_gaps = true;
template <int D, int K>
static void run_cond(const XtCondArgs& a, int nblocks, int threads, size_t ldsd)
{
    if (g_gaps) run_cond_g<D, K, true>(a, nblocks, threads, ldsd);
    else run_cond_g<D, K, false>(a, nblocks, threads, ldsd);
}

// tracks [N][L][D]; sigma: per-peak errors [N][L][KS] or null (locerr_mode 0); states int8 [N][L].  ws_global: rows in the output arrays
// (else in the emulated LDS).  gaps: the GAPS body (else the plain one).  mu [N][L][D], sig_out [N][L][K], logdens [N] or null.
extern "C" int xt_emul_cond_gap(const double* tracks, const double* sigma, const int8_t* states, long long N, int L, int D, int KS, int S, int locerr_mode,
                            int locerr_dims, const double* locerr, double slope, double offset, const double* ds, const double* Fs,
                            const double* TrMat, const double* p_stay, int nblocks, int tpb, int ws_global, int gaps, double* mu,
                            double* sig_out, double* logdens)
{
    g_gaps = gaps != 0;
    XtConfig cfg;
    if (!xt_build_config(S, 1, 2, cfg).empty()) return -1;
    XtModelHost m{S, 1, locerr_mode == 0 ? locerr_dims : 1, {0, 0, 0}, slope, offset, 0.0, ds, Fs, TrMat, p_stay};
    for (int k = 0; k < 3; ++k) m.locerr[k] = locerr[k];
    std::vector<double> blob;
    xt_build_blob(m, cfg, blob);
    const int K = locerr_mode == 0 ? locerr_dims : KS;
    if (tpb < 64 || tpb % 64 || tpb > 1024) return -2;
    XtCondArgs a;
    memset(&a, 0, sizeof(a));
    a.tracks = tracks;
    a.sigma = locerr_mode ? sigma : nullptr;
    a.states = states;
    a.mu = mu;
    a.sig_out = sig_out;
    a.logdens = logdens;
    a.N = N;
    a.L = L;
    a.S = S;
    a.TPB = tpb;
    a.locerr_mode = locerr_mode;
    a.ws_global = ws_global ? 1 : 0;
    for (int i = 0; i < 8; ++i) a.hdr[i] = blob[i];
    for (int i = 0; i < S * S; ++i) a.d2[i] = blob[(size_t)XT_BLOB_HDR + 4 * (size_t)S * S + i];
    const size_t ldsd = xt_cond_lds_doubles(S, L, D, K, tpb, ws_global != 0);
    if (D == 1 && K == 1) return run_cond<1, 1>(a, nblocks, tpb, ldsd), 0;
    if (D == 2 && K == 1) return run_cond<2, 1>(a, nblocks, tpb, ldsd), 0;
    if (D == 2 && K == 2) return run_cond<2, 2>(a, nblocks, tpb, ldsd), 0;
    if (D == 3 && K == 1) return run_cond<3, 1>(a, nblocks, tpb, ldsd), 0;
    if (D == 3 && K == 3) return run_cond<3, 3>(a, nblocks, tpb, ldsd), 0;
    return -3;
}
