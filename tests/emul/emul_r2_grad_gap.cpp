// TEST INFRASTRUCTURE ONLY: the gap-aware GRADIENT instantiation of the register-resident 2-state body (extrack_amd/csrc/xt_reg2.h:
// xt_r2_body<.., NP > 0, .., GAPS>) on CPU threads, under the PRODUCT's own decisions - xt_grad_pick(gaps), xt_grad_gap_reg2,
// xt_grad_gap_reg2_lazy (csrc/xt_grad_geom.h), the uniform / full split and the pass sizes of xt_grad_run_reg2 - which are reported back so that a
// test can assert that the launch was upgraded; and a binding of the upgrade decision alone.  One frame_len per library (-DXT_EMUL_F=4..7, every
// instance unrolls the whole step loop), with the track dimensionality of the test cases: (F, D) = (4, 1), (5, 2), (6, 2), (7, 3).  Built by
// tests/test_emul_r2_grad_gaps.py / tests/test_grad_gap_reg2_cpu.py.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

// what the staging leaves in LDS in place of a NaN coordinate (NaN: the product's behaviour); rows are classified from the input as always
static double g_gap_fill = NAN;
#define XT_R2_GAP_STAGED(v) ((v) != (v) ? g_gap_fill : (v))
extern "C" void xt_emul_r2gg_set_fill(double v) { g_gap_fill = v; }

#include "emul_ctx.h"
#include "../../extrack_amd/csrc/xt_grad_geom.h"
#include "../../extrack_amd/csrc/xt_grad_host.h"
#include "../../extrack_amd/csrc/xt_reg2.h"
#include "../../extrack_amd/csrc/xt_tables.h"

#ifndef XT_EMUL_F
#define XT_EMUL_F 6
#endif
#define XT_EMUL_D (XT_EMUL_F == 4 ? 1 : (XT_EMUL_F == 7 ? 3 : 2))

// NP directions per pass are compile-time: 1, 3, 5 and 8 are instantiated; the caller pads a pass with zero directions
template <int NP, bool GAPS>
static void r2gg_run(const XtKernelArgs& a, const XtGradArgs& ga, int nblocks, size_t lds_bytes)
{
    th_emul_blocks(nblocks, 64 * XT_F2_WAVES, lds_bytes / 8 + 8, [&](HostCtx& cx) { xt_r2_body<XT_EMUL_F, XT_EMUL_D, 1, NP, 0, GAPS>(a, ga, cx); });
}
static int r2gg_np(int real) { return real <= 1 ? 1 : (real <= 3 ? 3 : (real <= 5 ? 5 : 8)); }
static bool r2gg(int NP, bool gaps, const XtKernelArgs& a, const XtGradArgs& ga, int nblocks, size_t lds_bytes)
{
#define XT_GG(N)                                                  \
    if (NP == N) {                                                \
        if (gaps) r2gg_run<N, true>(a, ga, nblocks, lds_bytes);   \
        else r2gg_run<N, false>(a, ga, nblocks, lds_bytes);       \
        return true;                                              \
    }
    XT_GG(1)
    XT_GG(3)
    XT_GG(5)
    XT_GG(8)
#undef XT_GG
    return false;
}

extern "C" int xt_emul_r2gg_frame_len() { return XT_EMUL_F; }
extern "C" int xt_emul_r2gg_dims() { return XT_EMUL_D; }
extern "C" int xt_emul_r2gg_block_bytes(int NPT, int D, int tpw, int gaps) { return gaps ? xt_r2_grad_gap_block_bytes(NPT, D, tpw) : xt_r2_block_bytes(NPT, D, 0, tpw); }

// Buckets in LAUNCH order (one launch group), one global localisation error; row0[i] = first row of bucket i in scores [sum N][n_dir]; ll_out[i]: [N].
// tangents: n_dir rows of [locerr(3), slope, offset, pBL, ds2(2), Fs(2), TrMat(4), p_stay(2)].  out: [1 + n_dir] = {sum LL, gradient}.
// gaps != 0: the launch of extrack_loglik_scores_gaps - knobs = {grad_reg2, r2_maxnp, frame_len mask, variant: 0 as the product decides, 1 guarded forced};
// info = {path after xt_grad_gap_reg2, lazy variant ran, tracks per block, threads, passes, LDS bytes of the first pass}; the body runs only when the
// launch was upgraded (path XT_GRAD_GAPS_REG2), else the call returns 1 with info filled.  gaps == 0: the plain NP > 0 body on the same input with the
// same passes (path XT_GRAD_REG2), for the gap-free comparison.
extern "C" int xt_emul_r2_grad_gap(int gaps, int nbuckets, const double** tracks, const long long* Ns, const int* Ls, const long long* row0, int D, int max_len,
                                   int min_len, double locerr, double pBL, const double* ds, const double* Fs, const double* TrMat, const double* p_stay,
                                   int n_dir, const double* tangents, const int* blocks_per_bucket, const int* knobs, double** ll_out, double* scores,
                                   double* out, int* info)
{
    const int F = XT_EMUL_F, S = 2;
    if (nbuckets < 1 || nbuckets > XT_MAX_BUCKETS || n_dir < 1 || D != XT_EMUL_D) return -4;
    XtConfig cfg;
    if (!xt_build_config(S, 1, F, cfg).empty() || !xt_use_reg2(S, 1, F)) return -1;
    XtModelHost m{S, 1, 1, {locerr, locerr, locerr}, 0.0, 0.0, pBL, ds, Fs, TrMat, p_stay};
    std::vector<double> blob;
    xt_build_blob(m, cfg, blob);
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
    // ---- the product's two decisions
    int Lmax = 0;
    for (int i = 0; i < nbuckets; ++i) Lmax = std::max(Lmax, Ls[i]);
    XtGradKnobs kn;
    kn.grad_reg2 = knobs[0], kn.r2_maxnp = knobs[1];
    XtGradPick pk = xt_grad_pick(cfg, D, 1, 0, n_dir, Lmax, nbuckets, 256, gaps != 0, scores != nullptr, kn);
    pk = xt_grad_gap_reg2(pk, cfg, D, 1, 0, n_dir, Lmax, gaps != 0, kn, knobs[2]);
    const bool ws = xt_model_well_scaled(blob, locerr * locerr, locerr * locerr);
    const bool lazy = gaps ? (knobs[3] == 0 && xt_grad_gap_reg2_lazy(ws, Lmax, blob[7])) : (knobs[3] == 0 && ws);
    if (info) info[0] = pk.path, info[1] = lazy, info[2] = pk.tpb, info[3] = pk.threads, info[4] = 0, info[5] = 0;
    if (pk.path != (gaps ? XT_GRAD_GAPS_REG2 : XT_GRAD_REG2)) return 1;
    // ---- xt_grad_run_reg2: uniform directions ride along with the first pass, the full ones go in passes of at most maxnp
    std::vector<int> full, uni;
    for (int i = 0; i < n_dir; ++i) ((int)uni.size() < XT_R2_MAXU && xt_r2_uniform_direction(dblob.data() + (size_t)i * TB) ? uni : full).push_back(i);
    if (full.empty()) {
        full.push_back(uni.back());
        uni.pop_back();
    }
    const int NF = (int)full.size(), NUn = (int)uni.size();
    const int npass = (NF + pk.maxnp - 1) / pk.maxnp, per = (NF + npass - 1) / npass;
    XtKernelArgs a;
    memset(&a, 0, sizeof(a));
    xt_fill_args_from_config(cfg, a);
    long long n_total = 0;
    for (int i = 0; i < nbuckets; ++i) n_total += Ns[i];
    int W = NUn;  // launch-order score matrix [sum N][W]: the passes padded with zero directions, then the uniform columns
    for (int p0 = 0; p0 < NF; p0 += per) W += r2gg_np(std::min(per, NF - p0));
    std::vector<int> col_of(W, -1);
    std::vector<double> raw((size_t)n_total * W, -12345.0);
    std::vector<XtBucketDesc> descs(nbuckets);
    int nblocks = 0;
    for (int i = 0; i < nbuckets; ++i) {
        descs[i] = XtBucketDesc{tracks[i], nullptr, ll_out ? ll_out[i] : nullptr, nullptr, Ns[i], Ls[i], Ls[i] != max_len ? 1 : 0, -(double)(Ls[i] - 1) * D * 0.5 * XT_LOG2PI};
        if (scores) descs[i].scores_out = raw.data() + (size_t)row0[i] * W;
        nblocks += blocks_per_bucket[i];
        a.blk_end[i] = nblocks;
    }
    a.desc = descs.data();
    a.ndesc = nbuckets;
    a.blob = blob.data();
    a.min_len = min_len;
    a.locerr_mode = 0;
    a.KS = 1;
    a.well_scaled = lazy ? 1 : 0;
    a.TPB = pk.tpb;
    XtGradArgs ga;
    memset(&ga, 0, sizeof(ga));
    ga.TB = TB;
    ga.score_ld = W;
    for (int i = 0; i <= n_dir; ++i) out[i] = 0.0;
    std::vector<double> ublob(std::max<size_t>(1, uni.size()) * TB, 0.0);
    for (size_t i = 0; i < uni.size(); ++i) memcpy(ublob.data() + i * TB, dblob.data() + (size_t)uni[i] * TB, TB * sizeof(double));
    for (int i = 0; i < NUn; ++i) col_of[W - NUn + i] = uni[i];
    int c0 = 0, passes = 0;
    for (int p0 = 0; p0 < NF; p0 += per, ++passes) {
        const int real = std::min(per, NF - p0), NPp = r2gg_np(real), NU = p0 == 0 ? NUn : 0, NPT = NPp + NU;
        std::vector<double> gp((size_t)nblocks * (NPT + 1), 0.0), pad((size_t)NPp * TB, 0.0);
        for (int i = 0; i < real; ++i) {
            memcpy(pad.data() + (size_t)i * TB, dblob.data() + (size_t)full[p0 + i] * TB, (size_t)TB * sizeof(double));
            col_of[c0 + i] = full[p0 + i];
        }
        ga.dblob = pad.data();
        ga.udblob = ublob.data();
        ga.NU = NU;
        ga.NP = NPp;
        ga.gpartials = gp.data();
        ga.score_col0 = c0;
        ga.score_ucol0 = W - NUn;
        const size_t lds = gaps ? (size_t)xt_r2_grad_gap_block_bytes(NPT, D, pk.tpw) : (size_t)xt_r2_block_bytes(NPT, D, 0, pk.tpw);
        if (info && p0 == 0) info[5] = (int)lds;
        if (!r2gg(NPp, gaps != 0, a, ga, nblocks, lds)) return -3;
        for (int b = 0; b < nblocks; ++b) {
            if (p0 == 0) out[0] += gp[(size_t)b * (NPT + 1)];
            for (int i = 0; i < real; ++i) out[1 + full[p0 + i]] += gp[(size_t)b * (NPT + 1) + 1 + i];
            for (int i = 0; i < NU; ++i) out[1 + uni[i]] += gp[(size_t)b * (NPT + 1) + 1 + NPp + i];
        }
        c0 += NPp;
    }
    if (info) info[4] = passes;
    if (scores)
        for (long long r = 0; r < n_total; ++r)
            for (int c = 0; c < W; ++c)
                if (col_of[c] >= 0) scores[(size_t)r * n_dir + col_of[c]] = raw[(size_t)r * W + c];
    return 0;
}

// xt_grad_gap_reg2 after xt_grad_pick at one point.  in [12]: S, NS, F, D, K, locerr_mode, n_dir, Lmax, gaps, grad_reg2, r2_maxnp, frame_len mask;
// out [2][7]: {path, refusal, tpb, threads, lds, tpw, maxnp} first as xt_grad_pick left them, then after the second decision.  -1: a model
// xt_build_config refuses.
extern "C" int xt_emul_grad_gap_reg2(const long long* in, long long* out)
{
    static XtConfig c;
    if ((c.S != in[0] || c.NS != in[1] || c.F != in[2]) && !xt_build_config((int)in[0], (int)in[1], (int)in[2], c).empty()) return -1;
    XtGradKnobs kn;
    kn.grad_reg2 = (int)in[9], kn.r2_maxnp = (int)in[10];
    const XtGradPick p0 = xt_grad_pick(c, (int)in[3], (int)in[4], (int)in[5], (int)in[6], (int)in[7], 1, 256, in[8] != 0, false, kn);
    const XtGradPick p1 = xt_grad_gap_reg2(p0, c, (int)in[3], (int)in[4], (int)in[5], (int)in[6], (int)in[7], in[8] != 0, kn, (int)in[11]);
    const XtGradPick* ps[2] = {&p0, &p1};
    for (int i = 0; i < 2; ++i) {
        const XtGradPick& p = *ps[i];
        const long long o[7] = {p.path, p.refusal, p.tpb, p.threads, (long long)p.lds, p.tpw, p.maxnp};
        for (int j = 0; j < 7; ++j) out[i * 7 + j] = o[j];
    }
    return 0;
}
extern "C" int xt_emul_grad_gap_reg2_lazy(int well_scaled, int Lmax, double d2max) { return xt_grad_gap_reg2_lazy(well_scaled != 0, Lmax, d2max) ? 1 : 0; }
