// libextrack_hip.so, translation unit: the gap-aware instantiations of the state-duration histogram body (xt_hist.h, GAPS = true) behind
// extrack_segment_len_hist_gaps.  The host path is that of extrack_segment_len_hist (xt_hist_run, xt_hist_host.h); the definition of a
// gap is in DESIGN.md sections 18 and 24.
#include "xt_host.h"

#include "xt_hist.h"
#include "xt_hist_host.h"

// The register bound of xt_hist_kernel (XT_HIST_WAVES, measured there): the gap branch adds no value that lives across a step.
template <int D, int K, int MAXT>
__global__ void __launch_bounds__(MAXT, (MAXT == 256 ? XT_HIST_WAVES : 1)) xt_hist_gap_kernel(XtHistArgs a)
{
    DevCtx cx;
    xt_hist_body<D, K, true>(a, cx);
}

template <int D, int K>
static const void* hist_gap_t(int threads)
{
    return threads > 256 ? (const void*)xt_hist_gap_kernel<D, K, 512> : (const void*)xt_hist_gap_kernel<D, K, 256>;
}

static const void* xt_hist_gap_kernel_ptr(int D, int K, int threads)
{
    if (D == 1 && K == 1) return hist_gap_t<1, 1>(threads);
    if (D == 2 && K == 1) return hist_gap_t<2, 1>(threads);
    if (D == 2 && K == 2) return hist_gap_t<2, 2>(threads);
    if (D == 3 && K == 1) return hist_gap_t<3, 1>(threads);
    if (D == 3 && K == 3) return hist_gap_t<3, 3>(threads);
    return nullptr;
}

extern "C" int extrack_segment_len_hist_gaps(extrack_ctx* ctx, const extrack_model* m, int32_t bucket_id, int32_t max_nb_states, double* hist)
{
    return xt_hist_run(ctx, m, bucket_id, max_nb_states, hist, xt_hist_gap_kernel_ptr);
}
