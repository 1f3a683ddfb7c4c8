// TEST INFRASTRUCTURE ONLY: the two forward-mode gradient bodies (xt_gradr.h, xt_grad.h) with and without their GAPS flag on CPU threads, through
// the bucket-descriptor table (several length buckets in one emulated launch) with the per-track score store.  Built into its own library
// (run_emul_grad_gap.py).
#include <algorithm>
#include <cstring>
#include <vector>

#include "emul_ctx.h"
#include "../../extrack_amd/csrc/xt_grad.h"
#include "../../extrack_amd/csrc/xt_grad_host.h"
#include "../../extrack_amd/csrc/xt_gradr.h"

template <int G_, int D, int K>
static void run_body(int npc, bool gaps, const XtKernelArgs& a, const XtGradArgs& ga, int nblocks, int threads, size_t ldsd)
{
    th_emul_blocks(nblocks, threads, ldsd + 16, [&](HostCtx& cx) {
        if (npc == 0) {
            if (gaps) xt_grad_body<G_, D, K, true>(a, ga, cx);
            else xt_grad_body<G_, D, K>(a, ga, cx);
        } else if (npc == 3) {
            if (gaps) xt_gradr_body<G_, D, K, 3, true>(a, ga, cx);
            else xt_gradr_body<G_, D, K, 3>(a, ga, cx);
        } else {
            if (gaps) xt_gradr_body<G_, D, K, 4, true>(a, ga, cx);
            else xt_gradr_body<G_, D, K, 4>(a, ga, cx);
        }
    });
}

template <int G_>
static bool body_dk(int D, int K, int npc, bool gaps, const XtKernelArgs& a, const XtGradArgs& ga, int nblocks, int threads, size_t ldsd)
{
    if (D == 1 && K == 1) return run_body<G_, 1, 1>(npc, gaps, a, ga, nblocks, threads, ldsd), true;
    if (D == 2 && K == 1) return run_body<G_, 2, 1>(npc, gaps, a, ga, nblocks, threads, ldsd), true;
    if (D == 2 && K == 2) return run_body<G_, 2, 2>(npc, gaps, a, ga, nblocks, threads, ldsd), true;
    if (D == 3 && K == 1) return run_body<G_, 3, 1>(npc, gaps, a, ga, nblocks, threads, ldsd), true;
    if (D == 3 && K == 3) return run_body<G_, 3, 3>(npc, gaps, a, ga, nblocks, threads, ldsd), true;
    return false;
}

// body: 0 = xt_grad.h (two tracks per workgroup, two lanes per group, passes of at most 16 directions), 3 / 4 = xt_gradr.h with that many
// directions per pass.  gaps = 0 runs the body without the flag on the same arguments.  Buckets in LAUNCH order; sigma[i]: per-peak errors
// [N][L][KS] or all null (locerr_mode 0); row0[i] = first row of bucket i in scores [sum N][n_dir]; ll_out[i]: [N].
// tangents: n_dir rows of [locerr(3), slope, offset, pBL, ds2(S), Fs(S), TrMat(S*S), p_stay(S)].  out: [1 + n_dir] = {sum LL, gradient}.
extern "C" int xt_emul_grad_gap(int body, int gaps, int nbuckets, const double** tracks, const double** sigma, const long long* Ns, const int* Ls,
                                const long long* row0, int D, int KS, int S, int F, int max_len, int min_len, int locerr_mode, int locerr_dims,
                                const double* locerr, double slope, double offset, double pBL, const double* ds, const double* Fs, const double* TrMat,
                                const double* p_stay, int n_dir, const double* tangents, const int* blocks_per_bucket, double** ll_out, double* scores,
                                double* out)
{
    if (nbuckets < 1 || nbuckets > XT_MAX_BUCKETS || n_dir < 1 || (body != 0 && body != 3 && body != 4)) return -4;
    XtConfig cfg;
    if (!xt_build_config(S, 1, F, cfg).empty()) return -1;
    XtModelHost m{S, 1, locerr_mode == 0 ? locerr_dims : 1, {0, 0, 0}, slope, offset, pBL, ds, Fs, TrMat, p_stay};
    for (int k = 0; k < 3; ++k) m.locerr[k] = locerr[k];
    std::vector<double> blob;
    xt_build_blob(m, cfg, blob);
    const int K = locerr_mode == 0 ? locerr_dims : KS;
    const int TB = xt_grad_tb_doubles(S, cfg.G);
    const int row = 6 + 2 * S + S * S + cfg.G;
    std::vector<double> dblob((size_t)n_dir * TB, 0.0);
    for (int i = 0; i < n_dir; ++i) {
        const double* r = tangents + (size_t)i * row;
        extrack_model_tangent t;
        for (int k = 0; k < 3; ++k) t.locerr[k] = r[k];
        t.slope = r[3];
        t.offset = r[4];
        t.pBL = r[5];
        t.ds2 = r + 6;
        t.Fs = r + 6 + S;
        t.TrMat = r + 6 + 2 * S;
        t.p_stay = r + 6 + 2 * S + S * S;
        xt_build_tangent_block(m, t, cfg, locerr_mode, dblob.data() + (size_t)i * TB);
    }
    XtKernelArgs a;
    memset(&a, 0, sizeof(a));
    xt_fill_args_from_config(cfg, a);
    std::vector<XtBucketDesc> descs(nbuckets);
    int nblocks = 0;
    for (int i = 0; i < nbuckets; ++i) {
        descs[i] = XtBucketDesc{tracks[i], locerr_mode ? sigma[i] : nullptr, ll_out[i], nullptr, Ns[i], Ls[i], Ls[i] != max_len ? 1 : 0,
                                -(double)(Ls[i] - 1) * D * 0.5 * XT_LOG2PI};
        descs[i].scores_out = scores + (size_t)row0[i] * n_dir;
        nblocks += blocks_per_bucket[i];
        a.blk_end[i] = nblocks;
    }
    a.desc = descs.data();
    a.ndesc = nbuckets;
    a.blob = blob.data();
    a.base_tab = cfg.base_tab.data();
    a.off_tab = cfg.off_tab.data();
    a.min_len = min_len;
    a.locerr_mode = locerr_mode;
    a.KS = KS ? KS : 1;
    XtGradArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.TB = TB;
    ga.score_ld = n_dir;
    for (int i = 0; i <= n_dir; ++i) out[i] = 0.0;
    int per, threads, tpb;
    if (body == 0) {
        const int npass = (n_dir + 15) / 16;
        per = (n_dir + npass - 1) / npass;
        tpb = 2;
        ga.PJ = 2;
        ga.tan_lds = 1;
        threads = (tpb * cfg.NG * ga.PJ + 63) / 64 * 64;
        if (threads > 1024) return -2;
    } else {
        if (cfg.NG > 256) return -2;
        per = body;
        tpb = std::max(1, 256 / cfg.NG);
        threads = (tpb * cfg.NG + 63) / 64 * 64;
    }
    a.TPB = tpb;
    for (int p0 = 0; p0 < n_dir; p0 += per) {
        const int NP = std::min(per, n_dir - p0);
        std::vector<double> gp((size_t)nblocks * (NP + 1), 0.0);
        ga.dblob = dblob.data() + (size_t)p0 * TB;
        ga.gpartials = gp.data();
        ga.NP = NP;
        ga.score_col0 = p0;
        size_t ldsd;
        if (body == 0) {
            ldsd = (size_t)((xt_tab_doubles(S, cfg.G) + 1) & ~1) + (size_t)((NP * TB + 1) & ~1) +
                   (size_t)tpb * ((size_t)xt_grad_region_doubles(cfg.EP, D, K, NP) + xt_grad_acc_doubles(NP, cfg.NG) + xt_stage_doubles(D));
        } else {
            ldsd = xt_gradr_lds_bytes(S, cfg.G, cfg.E, cfg.EP, cfg.NG, cfg.P, D, K, NP, tpb) / 8;
        }
        const bool ok = S == 2 ? body_dk<2>(D, K, body, gaps != 0, a, ga, nblocks, threads, ldsd)
                               : (S == 3 ? body_dk<3>(D, K, body, gaps != 0, a, ga, nblocks, threads, ldsd)
                                         : (S == 4 ? body_dk<4>(D, K, body, gaps != 0, a, ga, nblocks, threads, ldsd) : false));
        if (!ok) return -3;
        for (int b = 0; b < nblocks; ++b) {
            if (p0 == 0) out[0] += gp[(size_t)b * (NP + 1)];
            for (int c = 0; c < NP; ++c) out[1 + p0 + c] += gp[(size_t)b * (NP + 1) + 1 + c];
        }
    }
    return 0;
}
