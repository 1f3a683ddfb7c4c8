// Micro-benchmark: issue cost (cycles per wave64 instruction per SIMD) of the fp64 / int VALU instructions used by the
// track-likelihood kernels on gfx950.  4 waves per SIMD, 8 independent chains per wave, s_memtime-free: wall clock only.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

#define ITER 32768
#define CH 8

template <int OP>
__global__ void __launch_bounds__(256) k(double* out, double seed, int n, double c0 = 0.5, double c1 = 0.25)
{
    double x[CH];
    int y[CH];
    for (int c = 0; c < CH; ++c) {
        x[c] = seed + threadIdx.x * 1e-3 + c;
        y[c] = threadIdx.x + c;
    }
    for (int i = 0; i < n; ++i) {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            if (OP == 0) x[c] = __builtin_fma(x[c], 1.0000001, 1e-9);
            if (OP == 1) x[c] = x[c] * 1.0000001;
            if (OP == 2) x[c] = x[c] + 1e-9;
            if (OP == 3) x[c] = __builtin_amdgcn_ldexp(x[c], y[c] & 1);
            if (OP == 4) x[c] = __builtin_amdgcn_frexp_mant(x[c]) + 1.0;
            if (OP == 5) y[c] += __builtin_amdgcn_frexp_exp(x[c] + y[c]);
            if (OP == 6) x[c] = __builtin_rint(x[c]) + 0.3;
            if (OP == 7) y[c] += (int)x[c];
            if (OP == 8) x[c] = __builtin_amdgcn_rcp(x[c]) + 1.0;
            if (OP == 9) x[c] = fmax(x[c], (double)y[c]);
            if (OP == 10) y[c] = (x[c] < (double)i) ? y[c] + 1 : y[c];
            if (OP == 11) y[c] = y[c] * 3 + 1;             // v_mul_lo/mad u32
            if (OP == 12) y[c] = (y[c] + i) ^ c;           // add + xor
            if (OP == 13) y[c] = __shfl_xor(y[c], 1, 64);  // ds_bpermute / dpp
            if (OP == 14) x[c] = sqrt(x[c]) + 1.0;
            if (OP == 15) { asm volatile("v_add_f64 %0, %0, 1.0" : "+v"(x[c])); }
            if (OP == 16) x[c] = __builtin_fma(x[c], 0.999, c0);               // fma with an SGPR-pair constant + literal
            if (OP == 17) x[c] = __builtin_fma(x[c], c1, c0);                  // two SGPR-pair constants
            if (OP == 18) x[c] = __builtin_fma(x[c], x[(c + 1) % CH], 0.5);    // inline constant
            if (OP == 19) y[c] = y[c] > i ? y[c] : x[c] > 1.0;                 // cmp/cndmask mix
            if (OP == 20) x[c] = __builtin_fma(x[c], x[(c + 1) % CH], x[(c + 2) % CH]);  // 3 VGPR-pair sources
            // ---- the lane exchange and the selects of the 2-state step (xt_host.h: xor_i32 / pair_exchange_i32), and bare 64-bit instructions
            if (OP == 21) y[c] = __builtin_amdgcn_update_dpp(y[c], y[c], 0xB1, 0xf, 0xf, false);   // v_mov_b32_dpp quad_perm:[1,0,3,2]
            if (OP == 22) y[c] = __builtin_amdgcn_update_dpp(y[c], y[c], 0x128, 0xf, 0xf, false);  // v_mov_b32_dpp row_ror:8
            if (OP == 23) {                                                                        // the bit-2 exchange: two moves under bank masks
                const int r = __builtin_amdgcn_update_dpp(y[c], y[c], 0x104, 0xf, 0x5, false);
                y[c] = __builtin_amdgcn_update_dpp(r, y[c], 0x114, 0xf, 0xA, false);
            }
            if (OP == 24 && (c & 1) == 0) {  // one swap serves two chains
                const auto r = __builtin_amdgcn_permlane16_swap((unsigned)y[c], (unsigned)y[c + 1], false, false);
                y[c] = (int)r[0], y[c + 1] = (int)r[1];
            }
            if (OP == 25 && (c & 1) == 0) {
                const auto r = __builtin_amdgcn_permlane32_swap((unsigned)y[c], (unsigned)y[c + 1], false, false);
                y[c] = (int)r[0], y[c + 1] = (int)r[1];
            }
            if (OP == 26) { asm volatile("v_cndmask_b32 %0, %0, %1, vcc" : "+v"(y[c]) : "v"(n)); }  // whatever vcc holds
            if (OP == 32) { asm volatile("v_cmp_lt_u32 vcc, %0, %1\n\tv_cndmask_b32 %0, %0, %1, vcc" : "+v"(y[c]) : "v"(n) : "vcc"); }
            if (OP == 33) { asm volatile("v_cmp_lt_u32 vcc, %0, %1" : : "v"(y[c]), "v"(n) : "vcc"); }
            if (OP == 27) { asm volatile("v_bfe_u32 %0, %0, 1, 31" : "+v"(y[c])); }
            if (OP == 28) { asm volatile("v_alignbit_b32 %0, %0, %1, 3" : "+v"(y[c]) : "v"(n)); }
            if (OP == 29) { asm volatile("v_rcp_f64 %0, %0" : "+v"(x[c])); }
            if (OP == 30) { asm volatile("v_ldexp_f64 %0, %0, 0" : "+v"(x[c])); }
            if (OP == 31) { asm volatile("v_min_f64 %0, %0, %1" : "+v"(x[c]) : "v"(seed)); }
        }
    }
    double s = 0;
    for (int c = 0; c < CH; ++c) s += x[c] + y[c];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <int OP>
double run(const char* name, double* d, int extra_per_iter)
{
    const int blocks = 256 * 4;  // 4 blocks x 4 waves per CU = 4 waves per SIMD
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    k<OP><<<blocks, 256>>>(d, 1.5, 64);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    k<OP><<<blocks, 256>>>(d, 1.5, ITER);
    hipEventRecord(e1);
    hipEventSynchronize(e1);
    float ms;
    hipEventElapsedTime(&ms, e0, e1);
    // instructions per SIMD = 4 waves * ITER * CH * (1 + extra)
    const double inst = 4.0 * ITER * CH;
    const double cyc = ms * 1e-3 * 2.4e9 / inst;
    printf("%-28s %8.3f ms  %6.2f cycles per (op%s) at 2.4 GHz nominal\n", name, ms, cyc, extra_per_iter ? " + helper" : "");
    return cyc;
}

int main()
{
    double* d;
    hipMalloc(&d, 256 * 4 * 256 * sizeof(double));
    run<0>("v_fma_f64", d, 0);
    run<1>("v_mul_f64", d, 0);
    run<2>("v_add_f64", d, 0);
    run<15>("v_add_f64 (asm)", d, 0);
    run<3>("v_ldexp_f64 (+and)", d, 1);
    run<4>("v_frexp_mant_f64 (+add_f64)", d, 1);
    run<5>("v_frexp_exp_i32_f64 (+2)", d, 1);
    run<6>("v_rndne_f64 (+add_f64)", d, 1);
    run<7>("v_cvt_i32_f64 (+add_u32)", d, 1);
    run<8>("v_rcp_f64 (+add_f64)", d, 1);
    run<9>("v_max_f64 (+cvt_f64_i32)", d, 1);
    run<10>("v_cmp_lt_f64+cndmask(+cvt)", d, 1);
    run<11>("v_mad_u32", d, 0);
    run<12>("v_add_u32+v_xor", d, 1);
    run<13>("shfl_xor 1 (dpp/bpermute)", d, 0);
    run<14>("sqrt f64 (+add)", d, 1);
    run<16>("v_fma_f64 v, literal, sgpr", d, 0);
    run<17>("v_fma_f64 v, sgpr, sgpr", d, 0);
    run<18>("v_fma_f64 v, v, inline", d, 0);
    run<20>("v_fma_f64 v, v, v", d, 0);
    for (int rep = 0; rep < 3; ++rep) run<0>("v_fma_f64 (repeat, warm)", d, 0);
    // lane exchange, selects and bare 64-bit instructions (profiles/readout_valu_rates.txt); the permlane rows: cycles per swap = 2 x the figure
    run<21>("v_mov_b32_dpp quad_perm", d, 0);
    run<22>("v_mov_b32_dpp row_ror:8", d, 0);
    run<23>("bit-2 exch. (2 dpp + 1 mov)", d, 0);
    run<24>("v_permlane16_swap_b32 / 2", d, 0);
    run<25>("v_permlane32_swap_b32 / 2", d, 0);
    run<26>("v_cndmask_b32", d, 0);
    run<32>("v_cmp_lt_u32 + v_cndmask_b32", d, 1);
    run<33>("v_cmp_lt_u32 alone", d, 0);
    run<27>("v_bfe_u32", d, 0);
    run<28>("v_alignbit_b32", d, 0);
    run<29>("v_rcp_f64 (bare)", d, 0);
    run<30>("v_ldexp_f64 (bare)", d, 0);
    run<31>("v_min_f64", d, 0);
    run<0>("v_fma_f64 (closing)", d, 0);
    return 0;
}
