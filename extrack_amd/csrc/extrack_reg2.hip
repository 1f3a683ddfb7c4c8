// libextrack_hip.so: lookup of the register-resident 2-state kernels (xt_reg2.h), instantiated per frame_len in extrack_reg2_f{4..7}.hip.
// The launch sites live in extrack_ll.hip (extrack_loglik*) and extrack_grad.hip (extrack_loglik_grad).
const void* xt_r2_kernel_f4(int D, int K, int NP);
const void* xt_r2_kernel_f5(int D, int K, int NP);
const void* xt_r2_kernel_f6(int D, int K, int NP);
const void* xt_r2_kernel_f7(int D, int K, int NP);

// Kernel address for (frame_len, dims, loc.-error dims, directions per pass); NP = 0: the likelihood-only kernel.  nullptr: not built.  The gradient
// kernels (NP >= 1) are built where xt_r2_built (xt_grad_geom.h) holds.
const void* xt_r2_kernel(int F, int D, int K, int NP)
{
    if (F == 4) return xt_r2_kernel_f4(D, K, NP);
    if (F == 5) return xt_r2_kernel_f5(D, K, NP);
    if (F == 6) return xt_r2_kernel_f6(D, K, NP);
    if (F == 7) return xt_r2_kernel_f7(D, K, NP);
    return nullptr;
}

// The gap-aware likelihood-only kernels (extrack_reg2_gaps_f{4..7}.hip): kernel address for (frame_len, dims); one global localisation error.
const void* xt_r2_gap_kernel_f4(int D);
const void* xt_r2_gap_kernel_f5(int D);
const void* xt_r2_gap_kernel_f6(int D);
const void* xt_r2_gap_kernel_f7(int D);
const void* xt_r2_gap_kernel(int F, int D)
{
    if (F == 4) return xt_r2_gap_kernel_f4(D);
    if (F == 5) return xt_r2_gap_kernel_f5(D);
    if (F == 6) return xt_r2_gap_kernel_f6(D);
    if (F == 7) return xt_r2_gap_kernel_f7(D);
    return nullptr;
}

// The gap-aware gradient kernels (extrack_reg2_grad_gaps_f{4..7}.hip): kernel address for (frame_len, dims, directions per pass); one global
// localisation error.  Built where xt_r2_gap_grad_built (xt_grad_geom.h) holds.
const void* xt_r2_grad_gap_kernel_f4(int D, int NP);
const void* xt_r2_grad_gap_kernel_f5(int D, int NP);
const void* xt_r2_grad_gap_kernel_f6(int D, int NP);
const void* xt_r2_grad_gap_kernel_f7(int D, int NP);
const void* xt_r2_grad_gap_kernel(int F, int D, int NP)
{
    if (F == 4) return xt_r2_grad_gap_kernel_f4(D, NP);
    if (F == 5) return xt_r2_grad_gap_kernel_f5(D, NP);
    if (F == 6) return xt_r2_grad_gap_kernel_f6(D, NP);
    if (F == 7) return xt_r2_grad_gap_kernel_f7(D, NP);
    return nullptr;
}
