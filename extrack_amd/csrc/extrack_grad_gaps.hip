// libextrack_hip.so: the gap-aware instantiations of the two forward-mode gradient bodies (xt_gradr.h and xt_grad.h, GAPS = true) behind
// extrack_loglik_grad_gaps / extrack_loglik_scores_gaps, and their lookup.  The launch sites live in extrack_grad.hip (xt_grad_enqueue),
// which gives them the geometry of their plain twins; the tangent rule of a gap step is in DESIGN.md section 21.
#include "xt_host.h"

#include "xt_gradr.h"

// Launch bounds: those of the plain twins (xt_gradr_kernel in extrack_gradr.hip, xt_grad_kernel in extrack_grad.hip, measured there), taken
// over UNMEASURED for the gap variants.
#ifndef XT_GRAD_WAVES
#define XT_GRAD_WAVES 3
#endif
template <int G_, int D, int K, int NPC>
__global__ void __launch_bounds__(256, 2) xt_gradr_gap_kernel(XtKernelArgs a, XtGradArgs ga)
{
    DevCtx cx;
    xt_gradr_body<G_, D, K, NPC, true>(a, ga, cx);
}

template <int G_, int D, int K, int MAXT>
__global__ void __launch_bounds__(MAXT, (MAXT == 256 ? XT_GRAD_WAVES : 1)) xt_grad_gap_kernel(XtKernelArgs a, XtGradArgs ga)
{
    DevCtx cx;
    xt_grad_body<G_, D, K, true>(a, ga, cx);
}

template <int G_, int NPC>
static const void* gradr_gap_dk(int D, int K)
{
    if (D == 1 && K == 1) return (const void*)xt_gradr_gap_kernel<G_, 1, 1, NPC>;
    if (D == 2 && K == 1) return (const void*)xt_gradr_gap_kernel<G_, 2, 1, NPC>;
    if (D == 2 && K == 2) return (const void*)xt_gradr_gap_kernel<G_, 2, 2, NPC>;
    if (D == 3 && K == 1) return (const void*)xt_gradr_gap_kernel<G_, 3, 1, NPC>;
    if (D == 3 && K == 3) return (const void*)xt_gradr_gap_kernel<G_, 3, 3, NPC>;
    return nullptr;
}

// Kernel address for (members per group = n_states at nb_substeps 1, dims, loc.-error dims, directions per pass: 3 or 4); nullptr: not built.
// Built where xt_gradr_built (xt_grad_geom.h) holds.
const void* xt_gradr_gap_kernel_ptr(int G, int D, int K, int NPC)
{
    if (NPC == 4) {
        if (G == 2) return gradr_gap_dk<2, 4>(D, K);
        if (G == 3) return gradr_gap_dk<3, 4>(D, K);
        if (G == 4) return gradr_gap_dk<4, 4>(D, K);
    } else if (NPC == 3) {
        if (G == 2) return gradr_gap_dk<2, 3>(D, K);
        if (G == 3) return gradr_gap_dk<3, 3>(D, K);
        if (G == 4) return gradr_gap_dk<4, 3>(D, K);
    }
    return nullptr;
}

template <int G_>
static const void* grad_gap_dk(int D, int K, bool wide)
{
#define XT_GG(DD, KK) (wide ? (const void*)xt_grad_gap_kernel<G_, DD, KK, 1024> : (const void*)xt_grad_gap_kernel<G_, DD, KK, 256>)
    if (D == 1 && K == 1) return XT_GG(1, 1);
    if (D == 2 && K == 1) return XT_GG(2, 1);
    if (D == 2 && K == 2) return XT_GG(2, 2);
    if (D == 3 && K == 1) return XT_GG(3, 1);
    if (D == 3 && K == 3) return XT_GG(3, 3);
#undef XT_GG
    return nullptr;
}

// The LDS-resident body (up to 1024 groups per track); wide: more than 256 threads per workgroup.  Built where xt_grad_lds_built(gaps = true) holds.
const void* xt_grad_gap_kernel_ptr(int G, int D, int K, bool wide)
{
    if (G == 2) return grad_gap_dk<2>(D, K, wide);
    if (G == 3) return grad_gap_dk<3>(D, K, wide);
    if (G == 4) return grad_gap_dk<4>(D, K, wide);
    return nullptr;
}
