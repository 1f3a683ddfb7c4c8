// libextrack_hip.so, translation unit 3: state-duration histograms (xt_hist.h) behind extrack_segment_len_hist; the host path both
// histogram entry points share is xt_hist_run (xt_hist_host.h), the gap-aware kernels are in extrack_hist_gaps.hip.
#include "xt_host.h"

#include "xt_hist.h"
#include "xt_hist_host.h"

// Waves per SIMD asked of the register allocator (256-thread workgroups): unbounded the kernel takes 136 VGPRs = 3 workgroups per CU; measured r03
// (1e5 x 30, max_nb_states 500 / 120): 3 -> 68.2 / 24.8 ms, 4 -> 62.0 / 21.2, 5 -> 61.4 / 19.9, 6 -> 74.0 / 21.8.  XT_HIST_WAVES itself is set in
// xt_hist_host.h: the host path weighs it against the LDS footprint when it places the parent buffers, and the gap-aware kernels
// (extrack_hist_gaps.hip) are built with the same bound.
template <int D, int K, int MAXT>
__global__ void __launch_bounds__(MAXT, (MAXT == 256 ? XT_HIST_WAVES : 1)) xt_hist_kernel(XtHistArgs a)
{
    DevCtx cx;
    xt_hist_body<D, K>(a, cx);
}

// Sum of the per-block histograms in a fixed order: one thread per bin.
__global__ void __launch_bounds__(256) xt_hist_reduce(const double* __restrict__ partials, int nblocks, int nbins, double* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= nbins) return;
    double s = 0.0;
    for (int b = 0; b < nblocks; ++b) s += partials[(size_t)b * nbins + i];
    out[i] = s;
}

hipError_t xt_hist_reduce_launch(hipStream_t stream, const double* partials, int nblocks, int nbins, double* out)
{
    hipLaunchKernelGGL(xt_hist_reduce, dim3((nbins + 255) / 256), dim3(256), 0, stream, partials, nblocks, nbins, out);
    return hipGetLastError();
}

template <int D, int K>
static const void* hist_t(int threads)
{
    return threads > 256 ? (const void*)xt_hist_kernel<D, K, 512> : (const void*)xt_hist_kernel<D, K, 256>;
}

static const void* xt_hist_kernel_ptr(int D, int K, int threads)
{
    if (D == 1 && K == 1) return hist_t<1, 1>(threads);
    if (D == 2 && K == 1) return hist_t<2, 1>(threads);
    if (D == 2 && K == 2) return hist_t<2, 2>(threads);
    if (D == 3 && K == 1) return hist_t<3, 1>(threads);
    if (D == 3 && K == 3) return hist_t<3, 3>(threads);
    return nullptr;
}

extern "C" int extrack_segment_len_hist(extrack_ctx* ctx, const extrack_model* m, int32_t bucket_id, int32_t max_nb_states, double* hist)
{
    return xt_hist_run(ctx, m, bucket_id, max_nb_states, hist, xt_hist_kernel_ptr);
}
