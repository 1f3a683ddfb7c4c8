// Instantiation table of the gap-aware register-resident 2-state likelihood kernels (xt_reg2.h: xt_r2_body<.., GAPS = true>; DESIGN.md section
// 25) for ONE frame_len: included by extrack_reg2_gaps_f{4..7}.hip with XT_R2_F defined, as xt_reg2_inst.h is by the plain ones.
#include "xt_host.h"

#include "xt_reg2.h"

// Waves per SIMD asked of the register allocator: the value of xt_ll_r2_kernel (xt_reg2_inst.h, measured there), taken over unmeasured - the gap
// step adds one vector register across the step loop (the track's mask of missed rows) and selects inside it.
#ifndef XT_R2_GAP_WAVES
#define XT_R2_GAP_WAVES 4
#endif
template <int F, int D>
__global__ void __launch_bounds__(64 * XT_F2_WAVES, XT_R2_GAP_WAVES) xt_ll_r2_gap_kernel(XtKernelArgs a)
{
    DevCtx cx;
    XtGradArgs ga;
    ga.dblob = nullptr;
    ga.gpartials = nullptr;
    xt_r2_body<F, D, 1, 0, 0, true>(a, ga, cx);
    xt_fused_total(a);
}

// Kernel address for track dimensionality D at frame_len XT_R2_F (one global localisation error: K = 1); nullptr: not built.
#define XT_R2_CAT_(a, b) a##b
#define XT_R2_CAT(a, b) XT_R2_CAT_(a, b)
const void* XT_R2_CAT(xt_r2_gap_kernel_f, XT_R2_F)(int D)
{
    if (D == 1) return (const void*)xt_ll_r2_gap_kernel<XT_R2_F, 1>;
    if (D == 2) return (const void*)xt_ll_r2_gap_kernel<XT_R2_F, 2>;
    if (D == 3) return (const void*)xt_ll_r2_gap_kernel<XT_R2_F, 3>;
    return nullptr;
}
