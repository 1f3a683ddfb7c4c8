// libextrack_hip.so: the gap-aware instantiations of the fixed-window body (xt_kernel.h, GAPS = true) behind extrack_loglik_gaps /
// extrack_predict_gaps, and their lookup.  The launch sites live in extrack_ll.hip (xt_launch_group), which gives them the geometry of
// xt_track_kernel; the definition of a gap is in DESIGN.md section 18.
#include "xt_host.h"

// Waves per SIMD asked of the register allocator: the values of xt_track_kernel (extrack_ll.hip, measured there).  The gap branch adds a
// handful of LDS stores and no live value across the step, so the same bounds are taken over unmeasured.
#ifndef XT_LL_WAVES
#define XT_LL_WAVES 4
#endif
#ifndef XT_G4_WAVES
#define XT_G4_WAVES 1
#endif
#ifndef XT_PREDS_WAVES
#define XT_PREDS_WAVES 3
#endif
template <int G_, int D, int K, bool PREDS, int MAXT>
__global__ void __launch_bounds__(MAXT, (MAXT == 256 && !PREDS ? (G_ != 4 ? XT_LL_WAVES : XT_G4_WAVES) : (MAXT == 256 && PREDS ? XT_PREDS_WAVES : 1))) xt_gap_kernel(XtKernelArgs a)
{
    DevCtx cx;
    xt_track_body<G_, D, K, PREDS, true>(a, cx);
    if (!PREDS) xt_fused_total(a);
}

template <int G_, int D, int K>
static const void* gap_ptr(bool preds, bool wide)
{
    if (preds) return wide ? (const void*)xt_gap_kernel<G_, D, K, true, 1024> : (const void*)xt_gap_kernel<G_, D, K, true, 256>;
    return wide ? (const void*)xt_gap_kernel<G_, D, K, false, 1024> : (const void*)xt_gap_kernel<G_, D, K, false, 256>;
}

template <int G_>
static const void* gap_dk(int D, int K, bool preds, bool wide)
{
    if (D == 1 && K == 1) return gap_ptr<G_, 1, 1>(preds, wide);
    if (D == 2 && K == 1) return gap_ptr<G_, 2, 1>(preds, wide);
    if (D == 2 && K == 2) return gap_ptr<G_, 2, 2>(preds, wide);
    if (D == 3 && K == 1) return gap_ptr<G_, 3, 1>(preds, wide);
    if (D == 3 && K == 3) return gap_ptr<G_, 3, 3>(preds, wide);
    return nullptr;
}

// Kernel address for (members per group = n_states at nb_substeps 1, dims, loc.-error dims, posteriors, more than 256 threads per workgroup).
// Built where xt_ll_gap_built (xt_ll_geom.h) holds.
const void* xt_gap_kernel_ptr(int G, int D, int K, bool preds, bool wide)
{
    if (G == 2) return gap_dk<2>(D, K, preds, wide);
    if (G == 3) return gap_dk<3>(D, K, preds, wide);
    if (G == 4) return gap_dk<4>(D, K, preds, wide);
    return nullptr;
}
