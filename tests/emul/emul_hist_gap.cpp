// TEST INFRASTRUCTURE ONLY: the state-duration histogram body (xt_hist.h) with GAPS = true (missed detections: all-NaN interior rows) and, for
// the comparison on gap-free data, with GAPS = false, on CPU threads, one bucket per emulated launch.  Built into its own library
// (run_emul_hist_gap.py).
#include <cstring>
#include <vector>

#include "emul_ctx.h"
#include "../../extrack_amd/csrc/xt_hist.h"
#include "../../extrack_amd/csrc/xt_hist_host.h"

template <int D, int K>
static void run_hist(const XtHistArgs& a, int nblocks, int threads, size_t ldsd, bool gaps)
{
    if (gaps) th_emul_blocks(nblocks, threads, ldsd, [&](HostCtx& cx) { xt_hist_body<D, K, true>(a, cx); });
    else th_emul_blocks(nblocks, threads, ldsd, [&](HostCtx& cx) { xt_hist_body<D, K>(a, cx); });
}

// tracks [N][L][D] (NaN rows allowed with gaps), sigma [N][L][KS] or null; par_lds: parent buffers in the emulated LDS (else in a "global"
// region); hist [(L - 1)][S]: the per-block histograms summed in block order.
extern "C" int xt_emul_hist_gap(const double* tracks, const double* sigma, long long N, int L, int D, int KS, int S, int isBL, int min_l, int locerr_mode,
                                int locerr_dims, const double* locerr, double slope, double offset, double pBL, const double* ds, const double* Fs,
                                const double* TrMat, const double* p_stay, int max_nb_states, int nblocks, int threads, int par_lds, int gaps, double* hist)
{
    XtModelHost m{S, 1, locerr_dims, {0, 0, 0}, slope, offset, pBL, ds, Fs, TrMat, p_stay};
    for (int k = 0; k < 3; ++k) m.locerr[k] = locerr ? locerr[k < locerr_dims ? k : 0] : 0.0;
    std::vector<double> blob;
    xt_hist_build_blob(m, blob);
    const int K = locerr_mode == 0 ? locerr_dims : KS;
    XtHistArgs a;
    memset(&a, 0, sizeof(a));
    a.bits = S <= 2 ? 1 : (S <= 4 ? 2 : 3);
    a.HW = (L * a.bits + 63) / 64;
    if (a.HW > XT_HIST_MAXW) return -2;
    a.K = max_nb_states;
    a.PC = max_nb_states > S * S ? max_nb_states : S * S;
    a.NC = 1;
    while (a.NC < a.PC * S) a.NC <<= 1;
    a.tracks = tracks;
    a.sigma = locerr_mode ? sigma : nullptr;
    a.blob = blob.data();
    a.N = N;
    a.L = L;
    a.S = S;
    a.KS = KS;
    a.locerr_mode = locerr_mode;
    a.isBL = isBL;
    a.min_l = min_l;
    a.par_lds = par_lds;
    const int nbins = (L - 1) * S;
    std::vector<double> partials((size_t)nblocks * nbins, 0.0);
    a.partials = partials.data();
    a.ws_stride = 2 * (int64_t)xt_hist_parent_doubles(a.PC, D, K, a.HW);
    std::vector<double> ws(par_lds ? 1 : (size_t)a.ws_stride * nblocks, NAN);  // poisoned like the emulated LDS
    a.ws = ws.data();
    const size_t ldsd = xt_hist_lds_doubles(S, L, D, K, locerr_mode ? KS : 0, a.PC, a.NC, a.HW, threads, par_lds != 0);
    if (D == 1 && K == 1) run_hist<1, 1>(a, nblocks, threads, ldsd, gaps != 0);
    else if (D == 2 && K == 1) run_hist<2, 1>(a, nblocks, threads, ldsd, gaps != 0);
    else if (D == 2 && K == 2) run_hist<2, 2>(a, nblocks, threads, ldsd, gaps != 0);
    else if (D == 3 && K == 1) run_hist<3, 1>(a, nblocks, threads, ldsd, gaps != 0);
    else if (D == 3 && K == 3) run_hist<3, 3>(a, nblocks, threads, ldsd, gaps != 0);
    else return -3;
    for (int i = 0; i < nbins; ++i) {
        double s2 = 0.0;
        for (int b = 0; b < nblocks; ++b) s2 += partials[(size_t)b * nbins + i];
        hist[i] = s2;
    }
    return 0;
}
