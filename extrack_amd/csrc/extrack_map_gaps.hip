// libextrack_hip.so, translation unit: the gap-aware instantiations of the state-path decoder (xt_map.h, GAPS = true) behind
// extrack_map_states_gaps, and their lookup.  The launch path is that of extrack_map_states (xt_map_states_launch, extrack_map.hip); the
// definition of a gap is in DESIGN.md sections 18 and 19.
#include "xt_host.h"

#include "xt_map.h"

// Waves per SIMD asked of the register allocator: the value of xt_map_kernel (extrack_map.hip, measured there).  The gap branch adds a
// handful of LDS stores and no live value across the step, so the same bound is taken over.
#ifndef XT_MAP_WAVES
#define XT_MAP_WAVES 3
#endif
template <int G_, int D, int K, int MAXT>
__global__ void __launch_bounds__(MAXT, (MAXT == 256 && XT_MAP_WAVES ? XT_MAP_WAVES : 1)) xt_map_gap_kernel(XtKernelArgs a, XtMapArgs ma)
{
    DevCtx cx;
    xt_map_body<G_, D, K, true>(a, ma, cx);
}

template <int G_, int D, int K>
static const void* map_gap_t(int threads)
{
    return threads <= 256 ? (const void*)xt_map_gap_kernel<G_, D, K, 256> : (const void*)xt_map_gap_kernel<G_, D, K, 1024>;
}

template <int G_>
static const void* map_gap_dk(int D, int K, int threads)
{
    if (D == 1 && K == 1) return map_gap_t<G_, 1, 1>(threads);
    if (D == 2 && K == 1) return map_gap_t<G_, 2, 1>(threads);
    if (D == 2 && K == 2) return map_gap_t<G_, 2, 2>(threads);
    if (D == 3 && K == 1) return map_gap_t<G_, 3, 1>(threads);
    if (D == 3 && K == 3) return map_gap_t<G_, 3, 3>(threads);
    return nullptr;
}

const void* xt_map_gap_kernel_ptr(int S, int D, int K, int threads)
{
    if (S == 2) return map_gap_dk<2>(D, K, threads);
    if (S == 3) return map_gap_dk<3>(D, K, threads);
    if (S == 4) return map_gap_dk<4>(D, K, threads);
    return nullptr;
}

extern "C" int extrack_map_states_gaps(extrack_ctx* ctx, const extrack_model* m, int32_t bucket_id, int8_t* states, double* score)
{
    return xt_map_states_launch(ctx, m, bucket_id, states, score, true);
}
