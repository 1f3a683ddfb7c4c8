// TEST INFRASTRUCTURE ONLY: the gap-aware likelihood-only register-resident 2-state body (extrack_amd/csrc/xt_reg2.h: xt_r2_body<.., GAPS>) on
// CPU threads, under the PRODUCT's own decisions - xt_ll_pick(gaps), xt_launch_scaling, xt_ll_gap_reg2 (csrc/xt_ll_geom.h) - which are reported
// back so that a test can assert that the launch was upgraded and ran g-form steps; and a binding of that second decision alone.  Built into
// its own library by tests/test_emul_r2_gaps.py / tests/test_ll_gap_reg2_cpu.py.
#include "emul_ctx.h"
#include "../../extrack_amd/csrc/xt_ll_geom.h"
#include "../../extrack_amd/csrc/xt_reg2.h"
#include "../../extrack_amd/csrc/xt_tables.h"

template <int F, int D, bool GAPS>
static void r2gap_run(const XtKernelArgs& a, int nblocks, int threads, size_t lds_bytes)
{
    XtGradArgs ga;
    memset(&ga, 0, sizeof(ga));
    th_emul_blocks(nblocks, threads, lds_bytes / 8 + 8, [&](HostCtx& cx) { xt_r2_body<F, D, 1, 0, 0, GAPS>(a, ga, cx); });
}
template <int F>
static bool r2gap_d(int D, bool gaps, const XtKernelArgs& a, int nblocks, int threads, size_t lds_bytes)
{
#define XT_RG_D(DD)                                                  \
    if (D == DD) {                                                   \
        if (gaps) r2gap_run<F, DD, true>(a, nblocks, threads, lds_bytes);  \
        else r2gap_run<F, DD, false>(a, nblocks, threads, lds_bytes);      \
        return true;                                                 \
    }
    XT_RG_D(1)
    XT_RG_D(2)
    XT_RG_D(3)
#undef XT_RG_D
    return false;
}

// One bucket of N tracks of length L with one global localisation error; fmask: the frame lengths the context upgrades.  gaps != 0: the
// launch of extrack_loglik_gaps - info = {path after xt_ll_gap_reg2, scaling, tracks per block, LDS bytes}; the body runs only when the launch was upgraded (path XT_LL_GAPS_REG2), else the call
// returns 1 with info filled.  gaps == 0: the plain likelihood-only body (xt_ll_r2_kernel's) on the same input, for the gap-free comparison.
extern "C" int xt_emul_r2_gap_run(const double* tracks, long long N, int L, int D, int F, int isBL, int min_len, double locerr, double pBL,
                                  const double* ds, const double* Fs, const double* TrMat, const double* p_stay, int nblocks, int gaps,
                                  int ll_reg2, int fmask, double* ll_out, double* total, int* info)
{
    XtConfig cfg;
    if (!xt_build_config(2, 1, F, cfg).empty() || !xt_use_reg2(2, 1, F)) return -1;
    XtModelHost m{2, 1, 1, {locerr, locerr, locerr}, 0.0, 0.0, pBL, ds, Fs, TrMat, p_stay};
    std::vector<double> blob;
    xt_build_blob(m, cfg, blob);
    const int scaling = xt_launch_scaling(blob, locerr * locerr, locerr * locerr, true);
    XtLlPick pk = xt_ll_pick(cfg, D, 1, 0, false, false, gaps != 0, ll_reg2, false, 32768, 1, 256);
    if (gaps) pk = xt_ll_gap_reg2(pk, cfg, D, 1, 0, false, ll_out != nullptr, ll_reg2, scaling, L, blob[7], fmask);
    if (info) info[0] = pk.path, info[1] = scaling, info[2] = pk.tpb, info[3] = (int)pk.lds;
    if (pk.path != (gaps ? XT_LL_GAPS_REG2 : XT_LL_REG2)) return 1;
    XtKernelArgs a;
    memset(&a, 0, sizeof(a));
    xt_fill_args_from_config(cfg, a);
    std::vector<double> partials(nblocks, 0.0);
    a.tracks = tracks;
    a.blob = blob.data();
    a.ll_out = ll_out;
    a.partials = partials.data();
    a.N = N;
    a.L = L;
    a.TPB = pk.tpb;
    a.isBL = isBL;
    a.min_len = min_len;
    a.locerr_mode = 0;
    a.KS = 1;
    a.ll_const = -(double)(L - 1) * D * 0.5 * XT_LOG2PI;
    a.well_scaled = scaling;
    bool ok = false;
    if (F == 4) ok = r2gap_d<4>(D, gaps != 0, a, nblocks, pk.threads, pk.lds);
    if (F == 5) ok = r2gap_d<5>(D, gaps != 0, a, nblocks, pk.threads, pk.lds);
    if (F == 6) ok = r2gap_d<6>(D, gaps != 0, a, nblocks, pk.threads, pk.lds);
    if (F == 7) ok = r2gap_d<7>(D, gaps != 0, a, nblocks, pk.threads, pk.lds);
    if (!ok) return -3;
    double s = 0.0;
    for (double p : partials) s += p;
    if (total) *total = s;
    return 0;
}

// xt_ll_gap_reg2 after xt_ll_pick at one point.  in: S, NS, F, D, K, KS, preds, per_track, ll_reg2, scaling, Lmax, gaps, frame_len mask (< 0: the
// function's default); out: the nine fields of the pick (as xt_emul_ll_pick of emul.cpp) first as xt_ll_pick left them, then after the second decision.
extern "C" int xt_emul_ll_gap_reg2(const long long* in, double d2max, long long* out)
{
    XtConfig c;
    if (!xt_build_config((int)in[0], (int)in[1], (int)in[2], c).empty()) return -1;
    const XtLlPick p0 = xt_ll_pick(c, (int)in[3], (int)in[4], (int)in[5], in[6] != 0, false, in[11] != 0, (int)in[8], false, 32768, 1, 256);
    const XtLlPick p1 = xt_ll_gap_reg2(p0, c, (int)in[3], (int)in[4], (int)in[5], in[6] != 0, in[7] != 0, (int)in[8], (int)in[9], (int)in[10], d2max, in[12] < 0 ? XT_LL_GAP_REG2_F_DEFAULT : (int)in[12]);
    const XtLlPick* ps[2] = {&p0, &p1};
    for (int i = 0; i < 2; ++i) {
        const XtLlPick& p = *ps[i];
        const long long o[9] = {p.path, p.refusal, p.tpb, p.threads, (long long)p.lds, p.wide, p.sel, p.ws_stride, (long long)p.max_blocks};
        for (int j = 0; j < 9; ++j) out[i * 9 + j] = o[j];
    }
    return 0;
}
extern "C" int xt_emul_r2_gap_block_bytes(int D, int tpw) { return xt_r2_gap_block_bytes(D, tpw); }
extern "C" int xt_emul_r2_block_bytes(int D, int tpw) { return xt_r2_block_bytes(0, D, 0, tpw); }
