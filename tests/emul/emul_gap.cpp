// TEST INFRASTRUCTURE ONLY: the gap-aware instantiations of the fixed-window body (xt_kernel.h, GAPS = true) on CPU threads, through the
// bucket-descriptor table (several length buckets in one emulated launch), likelihood and posteriors.  Built into its own library
// (run_emul_gap.py).
#include <algorithm>
#include <cstring>
#include <vector>

#include "emul_ctx.h"
#include "../../extrack_amd/csrc/xt_kernel.h"
#include "../../extrack_amd/csrc/xt_tables.h"

template <int G_, int D, int K>
static void run_gap(const XtKernelArgs& a, bool preds, bool gaps, int nblocks, int threads, size_t ldsd)
{
    th_emul_blocks(nblocks, threads, ldsd, [&](HostCtx& cx) {
        if (gaps) {
            if (preds) xt_track_body<G_, D, K, true, true>(a, cx);
            else xt_track_body<G_, D, K, false, true>(a, cx);
        } else {
            if (preds) xt_track_body<G_, D, K, true>(a, cx);
            else xt_track_body<G_, D, K, false>(a, cx);
        }
    });
}

template <int G_>
static bool gap_dk(int D, int K, const XtKernelArgs& a, bool preds, bool gaps, int nblocks, int threads, size_t ldsd)
{
    if (D == 1 && K == 1) return run_gap<G_, 1, 1>(a, preds, gaps, nblocks, threads, ldsd), true;
    if (D == 2 && K == 1) return run_gap<G_, 2, 1>(a, preds, gaps, nblocks, threads, ldsd), true;
    if (D == 2 && K == 2) return run_gap<G_, 2, 2>(a, preds, gaps, nblocks, threads, ldsd), true;
    if (D == 3 && K == 1) return run_gap<G_, 3, 1>(a, preds, gaps, nblocks, threads, ldsd), true;
    if (D == 3 && K == 3) return run_gap<G_, 3, 3>(a, preds, gaps, nblocks, threads, ldsd), true;
    return false;
}

// Buckets in LAUNCH order.  sigma[i]: per-peak errors [N][L][KS] or all null (locerr_mode 0).  ll_out[i]: [N]; preds_out[i]: [N][L][S] or
// null pointers (likelihood launch).  gaps = 0 runs the body without the flag on the same arguments.  info [3]: tracks per block, threads,
// LDS bytes.
extern "C" int xt_emul_gap(int nbuckets, const double** tracks, const double** sigma, const long long* Ns, const int* Ls, int D, int KS, int S, int F,
                           int max_len, int min_len, int locerr_mode, int locerr_dims, const double* locerr, double slope, double offset, double pBL,
                           const double* ds, const double* Fs, const double* TrMat, const double* p_stay, const int* blocks_per_bucket, int preds,
                           int gaps, double** ll_out, double** preds_out, double* total, int* info)
{
    if (nbuckets < 1 || nbuckets > XT_MAX_BUCKETS) return -4;
    XtConfig cfg;
    if (!xt_build_config(S, 1, F, cfg).empty()) return -1;
    XtModelHost m{S, 1, locerr_mode == 0 ? locerr_dims : 1, {0, 0, 0}, slope, offset, pBL, ds, Fs, TrMat, p_stay};
    for (int k = 0; k < 3; ++k) m.locerr[k] = locerr[k];
    std::vector<double> blob;
    xt_build_blob(m, cfg, blob);
    const int K = locerr_mode == 0 ? locerr_dims : KS;
    XtKernelArgs a;
    memset(&a, 0, sizeof(a));
    xt_fill_args_from_config(cfg, a);
    std::vector<XtBucketDesc> descs(nbuckets);
    int nblocks = 0;
    for (int i = 0; i < nbuckets; ++i) {
        descs[i] = XtBucketDesc{tracks[i], locerr_mode ? sigma[i] : nullptr, preds ? nullptr : ll_out[i], preds ? preds_out[i] : nullptr, Ns[i], Ls[i],
                                Ls[i] != max_len ? 1 : 0, -(double)(Ls[i] - 1) * D * 0.5 * XT_LOG2PI};
        nblocks += blocks_per_bucket[i];
        a.blk_end[i] = nblocks;
    }
    std::vector<double> partials(nblocks, 0.0);
    a.desc = descs.data();
    a.ndesc = nbuckets;
    a.blob = blob.data();
    a.base_tab = cfg.base_tab.data();
    a.off_tab = cfg.off_tab.data();
    a.partials = partials.data();
    a.min_len = min_len;
    a.locerr_mode = locerr_mode;
    a.KS = KS ? KS : 1;
    int tpb, threads;
    xt_geometry(cfg, D, K, tpb, threads);
    if (threads > 1024) return -2;
    a.TPB = tpb;
    const size_t lds = xt_lds_bytes(cfg, D, K, tpb);
    if (info) {
        info[0] = tpb;
        info[1] = threads;
        info[2] = (int)lds;
    }
    const bool ok = S == 2 ? gap_dk<2>(D, K, a, preds != 0, gaps != 0, nblocks, threads, lds / 8)
                           : (S == 3 ? gap_dk<3>(D, K, a, preds != 0, gaps != 0, nblocks, threads, lds / 8)
                                     : (S == 4 ? gap_dk<4>(D, K, a, preds != 0, gaps != 0, nblocks, threads, lds / 8) : false));
    if (!ok) return -3;
    double s = 0.0;
    for (double p : partials) s += p;
    if (total) *total = s;
    return 0;
}
