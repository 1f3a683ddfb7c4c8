// TEST INFRASTRUCTURE ONLY: the likelihood-only register-resident 2-state body (extrack_amd/csrc/xt_reg2.h) on CPU threads with the
// PRODUCT's per-launch scaling decision (xt_launch_scaling: 0 guarded steps, 1 well scaled, 2 well scaled + g-form steps), which is
// reported back so that a test can assert which steps ran.  Built into its own library by tests/test_emul_r2_gform.py.
#include "emul_ctx.h"
#include "../../extrack_amd/csrc/xt_reg2.h"
#include "../../extrack_amd/csrc/xt_tables.h"

template <int F, int D, int K>
static void gform_run(const XtKernelArgs& a, int nblocks, size_t lds_bytes)
{
    XtGradArgs ga;
    memset(&ga, 0, sizeof(ga));
    th_emul_blocks(nblocks, 64 * XT_F2_WAVES, lds_bytes / 8 + 8, [&](HostCtx& cx) { xt_r2_body<F, D, K, 0>(a, ga, cx); });
}
template <int F>
static bool gform_dk(int D, int K, const XtKernelArgs& a, int nblocks, size_t lds_bytes)
{
#define XT_GF_DK(DD, KK)                         \
    if (D == DD && K == KK) {                    \
        gform_run<F, DD, KK>(a, nblocks, lds_bytes); \
        return true;                             \
    }
    XT_GF_DK(1, 1)
    XT_GF_DK(2, 1)
    XT_GF_DK(2, 2)
    XT_GF_DK(3, 1)
    XT_GF_DK(3, 3)
#undef XT_GF_DK
    return false;
}

// One bucket of N tracks of length L.  sigma: per-peak errors [N][L][KS] (locerr_mode 1) or null (locerr_mode 0: locerr[locerr_dims]).
// guarded != 0 forces the fully guarded steps (the general algebra).  scaling_out: the value of XtKernelArgs::well_scaled the launch ran with.
extern "C" int xt_emul_gform_run(const double* tracks, const double* sigma, long long N, int L, int D, int KS, int F, int isBL, int min_len,
                                 int locerr_mode, int locerr_dims, const double* locerr, double pBL, const double* ds, const double* Fs,
                                 const double* TrMat, const double* p_stay, int nblocks, int guarded, double* ll_out, double* total,
                                 int* scaling_out)
{
    XtConfig cfg;
    if (!xt_build_config(2, 1, F, cfg).empty() || !xt_use_reg2(2, 1, F)) return -1;
    XtModelHost m{2, 1, locerr_dims, {0, 0, 0}, 0.0, 0.0, pBL, ds, Fs, TrMat, p_stay};
    for (int k = 0; k < 3; ++k) m.locerr[k] = locerr ? locerr[k < locerr_dims ? k : 0] : 0.0;
    std::vector<double> blob;
    xt_build_blob(m, cfg, blob);
    const int K = locerr_mode == 0 ? locerr_dims : KS;
    XtKernelArgs a;
    memset(&a, 0, sizeof(a));
    xt_fill_args_from_config(cfg, a);
    std::vector<double> partials(nblocks, 0.0);
    a.tracks = tracks;
    a.sigma = locerr_mode ? sigma : nullptr;
    a.blob = blob.data();
    a.ll_out = ll_out;
    a.partials = partials.data();
    a.N = N;
    a.L = L;
    a.TPB = (64 >> (F - 1)) * XT_F2_WAVES;
    a.isBL = isBL;
    a.min_len = min_len;
    a.locerr_mode = locerr_mode;
    a.KS = KS;
    a.ll_const = -(double)(L - 1) * D * 0.5 * XT_LOG2PI;
    double lo = INFINITY, hi = -INFINITY;  // range of the localisation variance over the launch, as xt_launch_group takes it
    if (locerr_mode == 0) {
        for (int k = 0; k < locerr_dims && k < 3; ++k) {
            lo = std::min(lo, m.locerr[k] * m.locerr[k]);
            hi = std::max(hi, m.locerr[k] * m.locerr[k]);
        }
    } else {
        for (long long i = 0; i < N * L * KS; ++i)
            if (sigma[i] == sigma[i]) {
                lo = std::min(lo, sigma[i] * sigma[i]);
                hi = std::max(hi, sigma[i] * sigma[i]);
            }
    }
    a.well_scaled = guarded ? 0 : xt_launch_scaling(blob, lo, hi, locerr_mode == 0 && K == 1);
    if (scaling_out) *scaling_out = a.well_scaled;
    const size_t lds = (size_t)xt_r2_block_bytes(0, D, locerr_mode ? KS : 0, 64 >> (F - 1));
    bool ok = false;
    if (F == 4) ok = gform_dk<4>(D, K, a, nblocks, lds);
    if (F == 5) ok = gform_dk<5>(D, K, a, nblocks, lds);
    if (F == 6) ok = gform_dk<6>(D, K, a, nblocks, lds);
    if (F == 7) ok = gform_dk<7>(D, K, a, nblocks, lds);
    if (!ok) return -3;
    double s = 0.0;
    for (double p : partials) s += p;
    if (total) *total = s;
    return 0;
}
