// TEST INFRASTRUCTURE ONLY: the per-track score store of the forward-mode gradient bodies (xt_reg2.h, xt_gradr.h, xt_grad.h) on CPU threads,
// through the bucket-descriptor table as the product launches them (XtBucketDesc::scores_out, XtGradArgs::score_*).  Built into its own
// library (run_emul_scores.py) next to libxt_emul.so; emul_r2.cpp and emul_gradr.cpp are linked in unchanged.
#include <algorithm>
#include <cstring>
#include <vector>

#include "emul_ctx.h"
#include "../../extrack_amd/csrc/xt_grad.h"
#include "../../extrack_amd/csrc/xt_grad_host.h"
#include "../../extrack_amd/csrc/xt_gradr.h"
#include "../../extrack_amd/csrc/xt_reg2.h"

bool emul_r2(int F, int D, int K, int KS, int NP, const XtKernelArgs& a, const XtGradArgs& ga, int nblocks);  // emul_r2.cpp
bool emul_gradr(int G, int D, int K, int NPC, const XtKernelArgs& a, const XtGradArgs& ga, int nblocks, int threads, size_t lds_doubles);  // emul_gradr.cpp

template <int G_, int D, int K>
static void run_lds(const XtKernelArgs& a, const XtGradArgs& ga, int nblocks, int threads, size_t ldsd)
{
    th_emul_blocks(nblocks, threads, ldsd + 16, [&](HostCtx& cx) { xt_grad_body<G_, D, K>(a, ga, cx); });
}
template <int G_>
static bool lds_dk(int D, int K, const XtKernelArgs& a, const XtGradArgs& ga, int nblocks, int threads, size_t ldsd)
{
    if (D == 2 && K == 1) return run_lds<G_, 2, 1>(a, ga, nblocks, threads, ldsd), true;
    if (D == 2 && K == 2) return run_lds<G_, 2, 2>(a, ga, nblocks, threads, ldsd), true;
    return false;
}

// family: 2 = xt_reg2.h, 3 / 4 = xt_gradr.h with that many directions per pass, 0 = xt_grad.h (all directions in one pass), 1 = xt_grad.h in two passes.
// Buckets in LAUNCH order; row0[i] = first row of bucket i in scores [sum N][n_dir] (with_scores == 0: no score pointer at all).
// tangents: n_dir rows of [locerr(3), slope, offset, pBL, ds2(S), Fs(S), TrMat(S*S), p_stay(G)].  out: [1 + n_dir] = {sum LL, gradient}.
extern "C" int xt_emul_scores(int family, int nbuckets, const double** tracks, const long long* Ns, const int* Ls, const long long* row0, int D, int S,
                              int NS, int F, int max_len, int min_len, int locerr_dims, const double* locerr, double pBL, const double* ds,
                              const double* Fs, const double* TrMat, const double* p_stay, int n_dir, const double* tangents,
                              const int* blocks_per_bucket, int with_scores, double* scores, double* out)
{
    if (nbuckets < 1 || nbuckets > XT_MAX_BUCKETS || n_dir < 1) return -4;
    XtConfig cfg;
    if (!xt_build_config(S, NS, F, cfg).empty()) return -1;
    XtModelHost m{S, NS, locerr_dims, {0, 0, 0}, 0.0, 0.0, pBL, ds, Fs, TrMat, p_stay};
    for (int k = 0; k < 3; ++k) m.locerr[k] = locerr[k < locerr_dims ? k : 0];
    std::vector<double> blob;
    xt_build_blob(m, cfg, blob);
    const int K = locerr_dims;
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
        xt_build_tangent_block(m, t, cfg, 0, dblob.data() + (size_t)i * TB);
    }
    // launch-order score matrix [sum N][W] (W >= n_dir: the emulated 2-state passes are padded with zero directions); col_of[c] = caller's direction or -1
    long long n_total = 0;
    for (int i = 0; i < nbuckets; ++i) n_total += Ns[i];
    int W = n_dir;
    std::vector<int> full, uni;
    if (family == 2) {
        if (!xt_use_reg2(S, NS, F)) return -5;
        for (int i = 0; i < n_dir; ++i)
            ((int)uni.size() < XT_R2_MAXU && xt_r2_uniform_direction(dblob.data() + (size_t)i * TB) ? uni : full).push_back(i);
        if (full.empty()) {
            full.push_back(uni.back());
            uni.pop_back();
        }
        W = 0;
        for (int p0 = 0; p0 < (int)full.size();) {
            const int NPp = (int)full.size() - p0 > 3 ? 8 : 3;
            W += NPp;
            p0 += std::min(NPp, (int)full.size() - p0);
        }
        W += (int)uni.size();
    }
    std::vector<int> col_of(W, -1);
    std::vector<double> raw((size_t)n_total * W, -12345.0);
    XtKernelArgs a;
    memset(&a, 0, sizeof(a));
    xt_fill_args_from_config(cfg, a);
    std::vector<XtBucketDesc> descs(nbuckets);
    int nblocks = 0;
    for (int i = 0; i < nbuckets; ++i) {
        descs[i] = XtBucketDesc{tracks[i], nullptr, nullptr, nullptr, Ns[i], Ls[i], Ls[i] != max_len ? 1 : 0, -(double)(Ls[i] - 1) * D * 0.5 * XT_LOG2PI};
        if (with_scores) descs[i].scores_out = raw.data() + (size_t)row0[i] * W;
        nblocks += blocks_per_bucket[i];
        a.blk_end[i] = nblocks;
    }
    a.desc = descs.data();
    a.ndesc = nbuckets;
    a.blob = blob.data();
    a.base_tab = cfg.base_tab.data();
    a.off_tab = cfg.off_tab.data();
    a.min_len = min_len;
    a.locerr_mode = 0;
    a.KS = 1;
    XtGradArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.TB = TB;
    ga.score_ld = W;
    for (int i = 0; i <= n_dir; ++i) out[i] = 0.0;
    auto collect = [&](const std::vector<double>& gp, int ncol, bool first, const std::vector<int>& dir_of_col) {
        for (int b = 0; b < nblocks; ++b) {
            if (first) out[0] += gp[(size_t)b * (ncol + 1)];
            for (int c = 0; c < ncol; ++c)
                if (dir_of_col[c] >= 0) out[1 + dir_of_col[c]] += gp[(size_t)b * (ncol + 1) + 1 + c];
        }
    };
    if (family == 2) {
        double lo = INFINITY, hi = -INFINITY;
        for (int k = 0; k < locerr_dims && k < 3; ++k) {
            lo = std::min(lo, m.locerr[k] * m.locerr[k]);
            hi = std::max(hi, m.locerr[k] * m.locerr[k]);
        }
        a.well_scaled = xt_model_well_scaled(blob, lo, hi) ? 1 : 0;
        a.TPB = (64 >> (F - 1)) * XT_F2_WAVES;
        const int NF = (int)full.size(), NUn = (int)uni.size();
        std::vector<double> ublob(std::max<size_t>(1, uni.size()) * TB, 0.0);
        for (size_t i = 0; i < uni.size(); ++i) memcpy(ublob.data() + i * TB, dblob.data() + (size_t)uni[i] * TB, TB * sizeof(double));
        for (int i = 0; i < NUn; ++i) col_of[W - NUn + i] = uni[i];
        int c0 = 0;
        for (int p0 = 0; p0 < NF;) {
            const int NPp = NF - p0 > 3 ? 8 : 3, real = std::min(NPp, NF - p0), NU = p0 == 0 ? NUn : 0, NPT = NPp + NU;
            std::vector<double> gp((size_t)nblocks * (NPT + 1), 0.0), pad((size_t)NPp * TB, 0.0);
            std::vector<int> dir_of_col(NPT, -1);
            for (int i = 0; i < real; ++i) {
                memcpy(pad.data() + (size_t)i * TB, dblob.data() + (size_t)full[p0 + i] * TB, (size_t)TB * sizeof(double));
                dir_of_col[i] = col_of[c0 + i] = full[p0 + i];
            }
            for (int i = 0; i < NU; ++i) dir_of_col[NPp + i] = uni[i];
            ga.dblob = pad.data();
            ga.udblob = ublob.data();
            ga.NU = NU;
            ga.NP = NPp;
            ga.gpartials = gp.data();
            ga.score_col0 = c0;
            ga.score_ucol0 = W - NUn;
            if (!emul_r2(F, D, K, 0, NPp, a, ga, nblocks)) return -3;
            collect(gp, NPT, p0 == 0, dir_of_col);
            c0 += NPp;
            p0 += real;
        }
    } else if (family == 3 || family == 4) {
        if (cfg.G < 2 || cfg.G > 4 || cfg.NG > 256) return -5;
        const int tpb = std::max(1, 256 / cfg.NG), thr = (tpb * cfg.NG + 63) / 64 * 64;
        a.TPB = tpb;
        for (int p0 = 0; p0 < n_dir; p0 += family) {
            const int NPp = std::min(family, n_dir - p0);
            std::vector<double> gp((size_t)nblocks * (NPp + 1), 0.0);
            std::vector<int> dir_of_col(NPp);
            for (int i = 0; i < NPp; ++i) dir_of_col[i] = col_of[p0 + i] = p0 + i;
            ga.dblob = dblob.data() + (size_t)p0 * TB;
            ga.gpartials = gp.data();
            ga.NP = NPp;
            ga.score_col0 = p0;
            const size_t ldsd = xt_gradr_lds_bytes(S, cfg.G, cfg.E, cfg.EP, cfg.NG, cfg.P, D, K, NPp, tpb) / 8;
            if (!emul_gradr(cfg.G, D, K, family, a, ga, nblocks, thr, ldsd)) return -3;
            collect(gp, NPp, p0 == 0, dir_of_col);
        }
    } else {
        const int tpb = 2, PJ = 2;
        const int threads = (tpb * cfg.NG * PJ + 63) / 64 * 64;
        if (threads > 1024) return -2;
        a.TPB = tpb;
        const int per = family == 1 ? (n_dir + 1) / 2 : n_dir;
        for (int p0 = 0; p0 < n_dir; p0 += per) {
            const int NPp = std::min(per, n_dir - p0);
            std::vector<double> gp((size_t)nblocks * (NPp + 1), 0.0);
            std::vector<int> dir_of_col(NPp);
            for (int i = 0; i < NPp; ++i) dir_of_col[i] = col_of[p0 + i] = p0 + i;
            ga.dblob = dblob.data() + (size_t)p0 * TB;
            ga.gpartials = gp.data();
            ga.NP = NPp;
            ga.tan_lds = 1;
            ga.PJ = PJ;
            ga.score_col0 = p0;
            size_t d = (size_t)((xt_tab_doubles(S, cfg.G) + 1) & ~1) + (size_t)((NPp * TB + 1) & ~1);
            d += (size_t)tpb * ((size_t)xt_grad_region_doubles(cfg.EP, D, K, NPp) + xt_grad_acc_doubles(NPp, cfg.NG) + xt_stage_doubles(D));
            bool ok = cfg.G == 2 ? lds_dk<2>(D, K, a, ga, nblocks, threads, d) : (cfg.G == 3 ? lds_dk<3>(D, K, a, ga, nblocks, threads, d) : false);
            if (!ok) return -3;
            collect(gp, NPp, p0 == 0, dir_of_col);
        }
    }
    if (with_scores && scores)
        for (long long r = 0; r < n_total; ++r)
            for (int c = 0; c < W; ++c)
                if (col_of[c] >= 0) scores[(size_t)r * n_dir + col_of[c]] = raw[(size_t)r * W + c];
    return 0;
}
