// TEST INFRASTRUCTURE ONLY: the PAIRS instantiations of the fixed-window body (xt_kernel.h) on CPU threads, through the bucket-descriptor
// table (several length buckets in one emulated launch), with and without GAPS, and the pair launch's geometry function (xt_pair_geom.h) as
// the library compiles it.  Built into its own library (run_emul_pairs.py).
#include <algorithm>
#include <cstring>
#include <vector>

#include "emul_ctx.h"
#include "../../extrack_amd/csrc/xt_kernel.h"
#include "../../extrack_amd/csrc/xt_tables.h"
#include "../../extrack_amd/csrc/xt_ll_geom.h"
#include "../../extrack_amd/csrc/xt_pair_geom.h"

template <int G_, int D, int K>
static void run_pairs(const XtKernelArgs& a, bool gaps, int nblocks, int threads, size_t ldsd)
{
    th_emul_blocks(nblocks, threads, ldsd, [&](HostCtx& cx) {
        if (gaps) xt_track_body<G_, D, K, true, true, true>(a, cx);
        else xt_track_body<G_, D, K, true, false, true>(a, cx);
    });
}

template <int G_>
static bool pairs_dk(int D, int K, const XtKernelArgs& a, bool gaps, int nblocks, int threads, size_t ldsd)
{
    if (D == 1 && K == 1) return run_pairs<G_, 1, 1>(a, gaps, nblocks, threads, ldsd), true;
    if (D == 2 && K == 1) return run_pairs<G_, 2, 1>(a, gaps, nblocks, threads, ldsd), true;
    if (D == 2 && K == 2) return run_pairs<G_, 2, 2>(a, gaps, nblocks, threads, ldsd), true;
    if (D == 3 && K == 1) return run_pairs<G_, 3, 1>(a, gaps, nblocks, threads, ldsd), true;
    if (D == 3 && K == 3) return run_pairs<G_, 3, 3>(a, gaps, nblocks, threads, ldsd), true;
    return false;
}

// Buckets in LAUNCH order.  sigma[i]: per-peak errors [N][L][KS] or all null (locerr_mode 0).  pairs_out[i]: [N][L-1][S][S] or null;
// counts_out[i]: [N][S][S] or null.  tpb > 0 overrides the tracks per block of xt_pair_pick (fewer only).  info [3]: tracks per block,
// threads, LDS bytes.
extern "C" int xt_emul_pairs(int nbuckets, const double** tracks, const double** sigma, const long long* Ns, const int* Ls, int D, int KS, int S, int F,
                             int max_len, int min_len, int locerr_mode, int locerr_dims, const double* locerr, double slope, double offset, double pBL,
                             const double* ds, const double* Fs, const double* TrMat, const double* p_stay, const int* blocks_per_bucket, int gaps,
                             int tpb, double** pairs_out, double** counts_out, int* info)
{
    if (nbuckets < 1 || nbuckets > XT_MAX_BUCKETS) return -4;
    XtConfig cfg;
    if (!xt_build_config(S, 1, F, cfg).empty()) return -1;
    XtModelHost m{S, 1, locerr_mode == 0 ? locerr_dims : 1, {0, 0, 0}, slope, offset, pBL, ds, Fs, TrMat, p_stay};
    for (int k = 0; k < 3; ++k) m.locerr[k] = locerr[k];
    std::vector<double> blob;
    xt_build_blob(m, cfg, blob);
    const int K = locerr_mode == 0 ? locerr_dims : KS;
    XtPairPick pk = xt_pair_pick(cfg, D, K);
    if (pk.refusal != XT_PAIR_FITS) return -2;
    if (tpb > 0 && tpb < pk.tpb) {
        pk.tpb = tpb;
        pk.threads = (tpb * cfg.NG + 63) / 64 * 64;
        pk.lds = xt_pair_lds_bytes(cfg, D, K, tpb);
    }
    XtKernelArgs a;
    memset(&a, 0, sizeof(a));
    xt_fill_args_from_config(cfg, a);
    std::vector<XtBucketDesc> descs(nbuckets);
    int nblocks = 0;
    for (int i = 0; i < nbuckets; ++i) {
        descs[i] = XtBucketDesc{tracks[i], locerr_mode ? sigma[i] : nullptr, nullptr, pairs_out[i], Ns[i], Ls[i], Ls[i] != max_len ? 1 : 0,
                                -(double)(Ls[i] - 1) * D * 0.5 * XT_LOG2PI};
        descs[i].scores_out = counts_out[i];
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
    a.TPB = pk.tpb;
    if (info) {
        info[0] = pk.tpb;
        info[1] = pk.threads;
        info[2] = (int)pk.lds;
    }
    const bool ok = S == 2 ? pairs_dk<2>(D, K, a, gaps != 0, nblocks, pk.threads, pk.lds / 8)
                           : (S == 3 ? pairs_dk<3>(D, K, a, gaps != 0, nblocks, pk.threads, pk.lds / 8)
                                     : (S == 4 ? pairs_dk<4>(D, K, a, gaps != 0, nblocks, pk.threads, pk.lds / 8) : false));
    return ok ? 0 : -3;
}

// xt_pair_pick at (S, nb_substeps, frame_len, D, K) beside xt_ll_pick for posteriors at the same point (with and without gaps, default
// context, one bucket).  out [12]: pair refusal, tpb, threads, lds, wide, sel; LDS bytes of a posterior launch of the same body at the pair
// launch's tracks per block (xt_lds_bytes); posterior launch with gaps (always that body): path, tpb, threads, lds; without gaps: path.
// Returns -1 where xt_build_config refuses the model.
extern "C" int xt_emul_pair_pick(int S, int NS, int F, int D, int K, int n_cu, long long* out)
{
    XtConfig cfg;
    if (!xt_build_config(S, NS, F, cfg).empty()) return -1;
    const XtPairPick p = xt_pair_pick(cfg, D, K);
    const XtLlPick q = xt_ll_pick(cfg, D, K, 0, true, false, false, 1, false, 32768, 1, n_cu);
    const XtLlPick g = xt_ll_pick(cfg, D, K, 0, true, false, true, 1, false, 32768, 1, n_cu);
    const long long v[12] = {p.refusal, p.tpb, p.threads, (long long)p.lds, p.wide, p.sel, (long long)xt_lds_bytes(cfg, D, K, p.tpb),
                             g.path, g.tpb, g.threads, (long long)g.lds, q.path};
    memcpy(out, v, sizeof(v));
    return 0;
}

extern "C" const char* xt_emul_pair_refusal_text(int r) { return xt_pair_refusal_text(r); }
