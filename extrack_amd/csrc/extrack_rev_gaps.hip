// libextrack_hip.so, translation unit: the gap-aware instantiations of the reverse-mode gradient body (xt_rev.h, GAPS = true; DESIGN.md
// section 28), for models with 2, 3 or 4 members per group.  Launched from extrack_grad.hip (extrack_loglik_grad_gaps) where
// xt_grad_gap_rev (xt_grad_geom.h) says so; launch bounds, geometry, log regions and the projection kernel are those of extrack_rev.hip.
#include "xt_host.h"

#include "xt_rev.h"

#ifndef XT_REV_WAVES
#define XT_REV_WAVES 2
#endif
template <int G_, int D, int K, int NBUF>
__global__ void __launch_bounds__(256, XT_REV_WAVES) xt_rev_gap_kernel(XtKernelArgs a, XtRevArgs ra)
{
    DevCtx cx;
    xt_rev_body<G_, D, K, NBUF, true>(a, ra, cx);
}

template <int G_, int NBUF>
static const void* rev_gap_dk(int D, int K)
{
    if (D == 1 && K == 1) return (const void*)xt_rev_gap_kernel<G_, 1, 1, NBUF>;
    if (D == 2 && K == 1) return (const void*)xt_rev_gap_kernel<G_, 2, 1, NBUF>;
    if (D == 2 && K == 2) return (const void*)xt_rev_gap_kernel<G_, 2, 2, NBUF>;
    if (D == 3 && K == 1) return (const void*)xt_rev_gap_kernel<G_, 3, 1, NBUF>;
    if (D == 3 && K == 3) return (const void*)xt_rev_gap_kernel<G_, 3, 3, NBUF>;
    return nullptr;
}

// Kernel address for (members per group, dims, loc.-error dims, exchange buffers per track: 1 | 2); nullptr: not built.  Built where xt_rev_built (xt_grad_geom.h) holds.
const void* xt_rev_gap_kernel_ptr(int G, int D, int K, int nbuf)
{
    if (nbuf == 2) {
        if (G == 2) return rev_gap_dk<2, 2>(D, K);
        if (G == 3) return rev_gap_dk<3, 2>(D, K);
        if (G == 4) return rev_gap_dk<4, 2>(D, K);
    } else if (nbuf == 1) {
        if (G == 2) return rev_gap_dk<2, 1>(D, K);
        if (G == 3) return rev_gap_dk<3, 1>(D, K);
        if (G == 4) return rev_gap_dk<4, 1>(D, K);
    }
    return nullptr;
}
