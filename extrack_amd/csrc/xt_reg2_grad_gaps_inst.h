// Instantiation table of the gap-aware register-resident 2-state GRADIENT kernels (xt_reg2.h: xt_r2_body<.., NP > 0, .., GAPS = true>; DESIGN.md
// section 27) for ONE frame_len: included by extrack_reg2_grad_gaps_f{4..7}.hip with XT_R2_F defined, as xt_reg2_inst.h is by the plain ones.
#include "xt_host.h"

#include "xt_reg2.h"

// Waves per SIMD asked of the register allocator: the rule of the plain twins (xt_reg2_inst.h: xt_r2_waves, measured there), restated here and taken
// over UNMEASURED - the gap step adds one vector register across the step loop (the track's mask of missed rows) and selects inside it.
XT_HD constexpr int xt_r2_gap_grad_waves(int NP, int D, int K) { return (NP * (1 + D + K) * 4 > 40) ? 2 : 3; }

template <int F, int D, int K, int NP, int WV>
__global__ void __launch_bounds__(64 * XT_F2_WAVES, WV) xt_grad_r2_gap_kernel(XtKernelArgs a, XtGradArgs ga)
{
    DevCtx cx;
    xt_r2_body<F, D, K, NP, 0, true>(a, ga, cx);
}

template <int F, int D>
static const void* r2_grad_gap_np(int NP)
{
    switch (NP) {
#define XT_R2_NP(N) \
    case N: return (const void*)xt_grad_r2_gap_kernel<F, D, 1, N, xt_r2_gap_grad_waves(N, D, 1)>;
        XT_R2_NP(1)
        XT_R2_NP(2)
        XT_R2_NP(3)
        XT_R2_NP(4)
        XT_R2_NP(5)
        XT_R2_NP(6)
        XT_R2_NP(7)
        XT_R2_NP(8)
#undef XT_R2_NP
    }
    return nullptr;
}

// Kernel address for (dims, directions per pass) at frame_len XT_R2_F (one global localisation error: K = 1); nullptr: not built.
#define XT_R2_CAT_(a, b) a##b
#define XT_R2_CAT(a, b) XT_R2_CAT_(a, b)
const void* XT_R2_CAT(xt_r2_grad_gap_kernel_f, XT_R2_F)(int D, int NP)
{
    if (D == 1) return r2_grad_gap_np<XT_R2_F, 1>(NP);
    if (D == 2) return r2_grad_gap_np<XT_R2_F, 2>(NP);
    if (D == 3) return r2_grad_gap_np<XT_R2_F, 3>(NP);
    return nullptr;
}
