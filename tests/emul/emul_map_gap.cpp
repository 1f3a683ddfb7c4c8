// TEST INFRASTRUCTURE ONLY: the state-path decoder body (xt_map.h) with GAPS = true (missed detections: all-NaN rows) and, for the
// comparison on gap-free data, with GAPS = false, on CPU threads, through the bucket-descriptor table (several length buckets in one
// emulated launch).  Built into its own library (run_emul_map_gap.py).
#include <algorithm>
#include <cstring>
#include <vector>

#include "emul_ctx.h"
#include "../../extrack_amd/csrc/xt_map.h"
#include "../../extrack_amd/csrc/xt_tables.h"

// the context of emul_ctx.h plus the one primitive the GAPS body adds (device version: DevCtx in xt_host.h)
struct GapCtx : HostCtx {
    void atomic_add_i32(int* p, int v) { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
};

static bool g_gaps = true;
template <int G_, int D, int K>
static void run_map(const XtKernelArgs& a, const XtMapArgs& ma, int nblocks, int threads, size_t ldsd)
{
    if (g_gaps)
        th_emul_blocks(nblocks, threads, ldsd, [&](HostCtx& hx) {
            GapCtx cx{hx};
            xt_map_body<G_, D, K, true>(a, ma, cx);
        });
    else
        th_emul_blocks(nblocks, threads, ldsd, [&](HostCtx& cx) { xt_map_body<G_, D, K, false>(a, ma, cx); });
}

template <int G_>
static bool map_dk(int D, int K, const XtKernelArgs& a, const XtMapArgs& ma, int nblocks, int threads, size_t ldsd)
{
    if (D == 1 && K == 1) return run_map<G_, 1, 1>(a, ma, nblocks, threads, ldsd), true;
    if (D == 2 && K == 1) return run_map<G_, 2, 1>(a, ma, nblocks, threads, ldsd), true;
    if (D == 2 && K == 2) return run_map<G_, 2, 2>(a, ma, nblocks, threads, ldsd), true;
    if (D == 3 && K == 1) return run_map<G_, 3, 1>(a, ma, nblocks, threads, ldsd), true;
    if (D == 3 && K == 3) return run_map<G_, 3, 3>(a, ma, nblocks, threads, ldsd), true;
    return false;
}

// Buckets in LAUNCH order.  sigma[i]: per-peak errors [N][L][KS] or all null (locerr_mode 0).  bp_global: back-pointer words in a
// "global" region sized by the launched grid (else in the emulated LDS).  gaps: the GAPS body (else the plain one).  states[i]: int8
// [N][L]; scores[i]: [N].
extern "C" int xt_emul_map_gap(int nbuckets, const double** tracks, const double** sigma, const long long* Ns, const int* Ls, int D, int KS, int S, int F,
                           int max_len, int min_len, int locerr_mode, int locerr_dims, const double* locerr, double slope, double offset, double pBL,
                           const double* ds, const double* Fs, const double* TrMat, const double* p_stay, const int* blocks_per_bucket, int tpb,
                           int bp_global, int gaps, int8_t** states, double** scores)
{
    g_gaps = gaps != 0;
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
    std::vector<XtMapOut> outs(nbuckets);
    int nblocks = 0, Lmax = 0;
    for (int i = 0; i < nbuckets; ++i) {
        descs[i] = XtBucketDesc{tracks[i], locerr_mode ? sigma[i] : nullptr, nullptr, nullptr, Ns[i], Ls[i], Ls[i] != max_len ? 1 : 0,
                                -(double)(Ls[i] - 1) * D * 0.5 * XT_LOG2PI};
        outs[i] = XtMapOut{states[i], scores[i]};
        nblocks += blocks_per_bucket[i];
        a.blk_end[i] = nblocks;
        Lmax = std::max(Lmax, Ls[i]);
    }
    a.desc = descs.data();
    a.ndesc = nbuckets;
    a.blob = blob.data();
    a.base_tab = cfg.base_tab.data();
    a.off_tab = cfg.off_tab.data();
    a.min_len = min_len;
    a.locerr_mode = locerr_mode;
    a.KS = KS ? KS : 1;
    a.TPB = tpb;
    const int threads = (tpb * cfg.NG + 63) / 64 * 64;
    if (threads > 1024) return -2;
    XtMapArgs ma;
    memset(&ma, 0, sizeof(ma));
    ma.out = outs.data();
    ma.bp_words = xt_map_bp_words(Lmax, F);
    ma.Lmax = Lmax;
    // poisoned like the emulated LDS: a word read before it was written shows
    std::vector<uint32_t> ws(bp_global ? (size_t)nblocks * tpb * ma.bp_words * cfg.NG : 0, 0xFFFFFFFFu);
    if (bp_global) ma.bp_ws = ws.data();
    const size_t ldsd = xt_map_lds_doubles(S, cfg.EP, cfg.NG, D, K, Lmax, ma.bp_words, !bp_global, tpb);
    const bool ok = S == 2 ? map_dk<2>(D, K, a, ma, nblocks, threads, ldsd) : (S == 3 ? map_dk<3>(D, K, a, ma, nblocks, threads, ldsd)
                                                                           : (S == 4 ? map_dk<4>(D, K, a, ma, nblocks, threads, ldsd) : false));
    return ok ? 0 : -3;
}
