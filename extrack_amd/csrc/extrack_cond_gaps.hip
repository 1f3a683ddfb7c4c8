// libextrack_hip.so, translation unit: the gap-aware instantiations of the fixed-state smoother (xt_cond.h, GAPS = true) behind
// extrack_refine_fixed_states_gaps, and their lookup.  The launch path is that of extrack_refine_fixed_states
// (xt_refine_fixed_states_launch, extrack_cond.hip); the definition of a gap is in DESIGN.md sections 18 and 19.
#include "xt_host.h"

#include "xt_cond.h"

template <int D, int K, bool WS_GLOBAL>
__global__ void __launch_bounds__(256) xt_cond_gap_kernel(XtCondArgs a)
{
    DevCtx cx;
    xt_cond_body<D, K, WS_GLOBAL, true>(a, cx);
}

template <int D, int K>
static const void* cond_gap_w(bool ws_global)
{
    return ws_global ? (const void*)xt_cond_gap_kernel<D, K, true> : (const void*)xt_cond_gap_kernel<D, K, false>;
}

const void* xt_cond_gap_kernel_ptr(int D, int K, bool ws_global)
{
    if (D == 1 && K == 1) return cond_gap_w<1, 1>(ws_global);
    if (D == 2 && K == 1) return cond_gap_w<2, 1>(ws_global);
    if (D == 2 && K == 2) return cond_gap_w<2, 2>(ws_global);
    if (D == 3 && K == 1) return cond_gap_w<3, 1>(ws_global);
    if (D == 3 && K == 3) return cond_gap_w<3, 3>(ws_global);
    return nullptr;
}

extern "C" int extrack_refine_fixed_states_gaps(extrack_ctx* ctx, const extrack_model* m, int32_t bucket_id, const int8_t* states, double* mu,
                                                double* sigma, double* logdens)
{
    return xt_refine_fixed_states_launch(ctx, m, bucket_id, states, mu, sigma, logdens, true);
}
