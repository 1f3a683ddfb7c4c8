// TEST INFRASTRUCTURE ONLY: the reverse-mode gradient body (xt_rev.h) with and without its GAPS flag on CPU threads, through the bucket-descriptor
// table (several length buckets in one emulated launch), and the launcher's third decision of a gapped group (xt_grad_gap_rev, xt_grad_geom.h).
// Built into its own library (run_emul_rev_gap.py).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "emul_ctx.h"
#include "../../extrack_amd/csrc/xt_grad_geom.h"
#include "../../extrack_amd/csrc/xt_grad_host.h"
#include "../../extrack_amd/csrc/xt_rev.h"

template <int G_, int D, int K, int NBUF>
static void run_body(bool gaps, const XtKernelArgs& a, const XtRevArgs& ra, int nblocks, int threads, size_t ldsd)
{
    th_emul_blocks(nblocks, threads, ldsd + 8, [&](HostCtx& cx) {
        if (gaps) xt_rev_body<G_, D, K, NBUF, true>(a, ra, cx);
        else xt_rev_body<G_, D, K, NBUF>(a, ra, cx);
    });
}

template <int G_, int NBUF>
static bool body_dk(int D, int K, bool gaps, const XtKernelArgs& a, const XtRevArgs& ra, int nblocks, int threads, size_t ldsd)
{
    if (D == 1 && K == 1) return run_body<G_, 1, 1, NBUF>(gaps, a, ra, nblocks, threads, ldsd), true;
    if (D == 2 && K == 1) return run_body<G_, 2, 1, NBUF>(gaps, a, ra, nblocks, threads, ldsd), true;
    if (D == 2 && K == 2) return run_body<G_, 2, 2, NBUF>(gaps, a, ra, nblocks, threads, ldsd), true;
    if (D == 3 && K == 1) return run_body<G_, 3, 1, NBUF>(gaps, a, ra, nblocks, threads, ldsd), true;
    if (D == 3 && K == 3) return run_body<G_, 3, 3, NBUF>(gaps, a, ra, nblocks, threads, ldsd), true;
    return false;
}
template <int G_>
static bool body_nbuf(int nbuf, int D, int K, bool gaps, const XtKernelArgs& a, const XtRevArgs& ra, int nblocks, int threads, size_t ldsd)
{
    return nbuf == 1 ? body_dk<G_, 1>(D, K, gaps, a, ra, nblocks, threads, ldsd) : body_dk<G_, 2>(D, K, gaps, a, ra, nblocks, threads, ldsd);
}

// nbuf: exchange buffers per track (1 | 2).  gaps = 0 runs the body without the flag on the same arguments.  Buckets in LAUNCH order (longest
// first: the log stride is that of the first); sigma[i]: per-peak errors [N][L][KS] or all null (locerr_mode 0); ll_out[i]: [N].
// tangents: n_dir rows of [locerr(3), slope, offset, pBL, ds2(S), Fs(S), TrMat(S*S), p_stay(S)].  out: [1 + n_dir] = {sum LL, gradient}: the
// per-block partials added in block order, the adjoint of the model blob contracted with the tangent blocks here (the product: two small kernels).
extern "C" int xt_emul_rev_gap(int nbuf, int gaps, int nbuckets, const double** tracks, const double** sigma, const long long* Ns, const int* Ls, int D,
                               int KS, int S, int F, int max_len, int min_len, int locerr_mode, int locerr_dims, const double* locerr, double slope,
                               double offset, double pBL, const double* ds, const double* Fs, const double* TrMat, const double* p_stay, int n_dir,
                               const double* tangents, const int* blocks_per_bucket, double** ll_out, double* out)
{
    if (nbuckets < 1 || nbuckets > XT_MAX_BUCKETS || n_dir < 1 || (nbuf != 1 && nbuf != 2)) return -4;
    XtConfig cfg;
    if (!xt_build_config(S, 1, F, cfg).empty()) return -1;
    if (!xt_rev_supported(cfg.G, cfg.NG)) return -5;
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
    int nblocks = 0, Lmax = 2;
    for (int i = 0; i < nbuckets; ++i) {
        descs[i] = XtBucketDesc{tracks[i], locerr_mode ? sigma[i] : nullptr, ll_out[i], nullptr, Ns[i], Ls[i], Ls[i] != max_len ? 1 : 0,
                                -(double)(Ls[i] - 1) * D * 0.5 * XT_LOG2PI};
        nblocks += blocks_per_bucket[i];
        a.blk_end[i] = nblocks;
        Lmax = std::max(Lmax, Ls[i]);
    }
    const int tpb = std::max(1, 256 / cfg.NG), threads = (tpb * cfg.NG + 63) / 64 * 64;
    a.desc = descs.data();
    a.ndesc = nbuckets;
    a.blob = blob.data();
    a.TPB = tpb;
    a.min_len = min_len;
    a.locerr_mode = locerr_mode;
    a.KS = KS ? KS : 1;
    XtRevArgs ra;
    memset(&ra, 0, sizeof(ra));
    std::vector<double> gp((size_t)nblocks * (1 + TB), 0.0);
    ra.log_stride = (int64_t)std::max(Lmax - 2, 1) * xt_rev_step_doubles(cfg.NG, D, K);
    std::vector<double> logbuf((size_t)nblocks * tpb * ra.log_stride, xt_emul_poison() ? NAN : 0.0);
    ra.gpartials = gp.data();
    ra.log = logbuf.data();
    ra.TB = TB;
    const size_t ldsd = xt_rev_lds_bytes(S, cfg.G, cfg.EP, D, K, tpb, threads, nbuf) / 8;
    const bool ok = S == 2 ? body_nbuf<2>(nbuf, D, K, gaps != 0, a, ra, nblocks, threads, ldsd)
                           : (S == 3 ? body_nbuf<3>(nbuf, D, K, gaps != 0, a, ra, nblocks, threads, ldsd)
                                     : (S == 4 ? body_nbuf<4>(nbuf, D, K, gaps != 0, a, ra, nblocks, threads, ldsd) : false));
    if (!ok) return -3;
    std::vector<double> adj(TB, 0.0);
    out[0] = 0.0;
    for (int b = 0; b < nblocks; ++b) {
        out[0] += gp[(size_t)b * (1 + TB)];
        for (int c = 0; c < TB; ++c) adj[c] += gp[(size_t)b * (1 + TB) + 1 + c];
    }
    for (int i = 0; i < n_dir; ++i) {
        double s = 0.0;
        for (int c = 0; c < TB; ++c) s = __builtin_fma(adj[c], dblob[(size_t)i * TB + c], s);
        out[1 + i] = s;
    }
    return 0;
}

// The decisions of a gapped launch group in the launcher's order.  in: S, nb_substeps, frame_len, D, K, locerr_mode, n_dir, Lmax, nbuckets, n_cu,
// gaps, scores, grad_reg2, grad_rev, rev_log_mb, fmask.  out: 4 picks of 9 fields {path, refusal, tpb, threads, lds, nbuf, max_blocks, log_stride,
// NPC}: xt_grad_pick, after xt_grad_gap_reg2, after xt_grad_gap_rev, and xt_grad_pick of the gap-free twin (gaps = scores = false).
extern "C" int xt_emul_grad_gap_rev(const long long* in, long long* out)
{
    XtConfig c;
    if (!xt_build_config((int)in[0], (int)in[1], (int)in[2], c).empty()) return -1;
    const int D = (int)in[3], K = (int)in[4], mode = (int)in[5], n_dir = (int)in[6], Lmax = (int)in[7], nbk = (int)in[8], n_cu = (int)in[9];
    const bool gaps = in[10] != 0, scores = in[11] != 0;
    XtGradKnobs kn;
    kn.grad_reg2 = (int)in[12], kn.grad_rev = (int)in[13], kn.rev_log_mb = (size_t)in[14];
    const XtGradPick p0 = xt_grad_pick(c, D, K, mode, n_dir, Lmax, nbk, n_cu, gaps, scores, kn);
    const XtGradPick p1 = xt_grad_gap_reg2(p0, c, D, K, mode, n_dir, Lmax, gaps, kn, (int)in[15]);
    const XtGradPick p2 = xt_grad_gap_rev(p1, c, D, K, mode, n_dir, Lmax, nbk, n_cu, gaps, scores, kn);
    const XtGradPick tw = xt_grad_pick(c, D, K, mode, n_dir, Lmax, nbk, n_cu, false, false, kn);
    const XtGradPick* ps[4] = {&p0, &p1, &p2, &tw};
    for (int i = 0; i < 4; ++i) {
        const XtGradPick& p = *ps[i];
        const long long o[9] = {p.path, p.refusal, p.tpb, p.threads, (long long)p.lds, p.nbuf, (long long)p.max_blocks, (long long)p.log_stride, p.NPC};
        for (int j = 0; j < 9; ++j) out[i * 9 + j] = o[j];
    }
    return 0;
}
