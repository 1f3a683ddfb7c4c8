// Position refinement along a given state path (fixed-state Kalman / Rauch-Tung-Striebel smoother): the kernel body behind
// extrack_refine_fixed_states, shared by the HIP kernels (extrack_cond.hip) and by the CPU-thread emulator used in tests
// (tests/emul/emul_cond.cpp).
//
// What it computes (what get_pos_PDF_fixedBs / get_LC_Km_Ks_fixed_Bs, extrack/refined_localization.py:414-519, were written to compute;
// exact statement and the evidence about that function in DESIGN.md section 17): given the state b[t] of every position the model is
// linear-Gaussian per dimension - flat prior on r[0], r[t+1] - r[t] ~ N(0, q[t]) with q[t] = d2[b[t]][b[t+1]] (the step-variance table of
// the likelihood's model blob), c[t] ~ N(r[t], l2[t]) - and the kernel returns the posterior mean and standard deviation of every r[t]
// given the whole track, and the log density of the observed displacements.  Per error channel (K = 1: one for all dimensions, K = D):
//   forward   f[0] = c[0], a[0] = l2[0];  p = a[t-1] + q[t-1], w = p + l2[t], g = p / w, r = c[t] - f[t-1]:
//             f[t] = f[t-1] + g r, a[t] = g l2[t], logdens += -log(2 pi w) / 2 - r^2 / (2 w) per dimension
//   backward  mu[L-1] = f[L-1], v[L-1] = a[L-1];  J = a[t] / (a[t] + q[t]):
//             mu[t] = f[t] + J (mu[t+1] - f[t]), v[t] = a[t] + J^2 (v[t+1] - a[t] - q[t]);  sigma = sqrt(v)
// The sum of log w is carried as a product (mantissa in [0.5, 1) and an integer exponent): one logarithm per track.
//
// Organisation: one lane per track, no communication between lanes.  A block owns TPB consecutive tracks of the bucket, so its
// positions, per-peak errors and states are each ONE contiguous run of the input arrays.  Two placements of the per-track rows:
//   * LDS: the runs are staged with coalesced loads into rows of xt_cond_row_doubles (odd: lane l reads position t at
//     l * row + t, distinct banks over a half wave for the 8-byte accesses), both sweeps run in place - f[t] overwrites c[t], a[t] the
//     error of position t (or fills the [L][K] part of the row when the error is global), the backward sweep overwrites both with mu and
//     sigma - and the block writes its rows out coalesced;
//   * global (rows of 64 tracks beyond the LDS of a CU): each lane reads its own rows of the inputs and uses its own rows of the OUTPUT
//     arrays mu / sigma as the workspace between the sweeps - nothing is allocated for it.
// Both run the same operations in the same order on the same values: the results are bit-identical.
//
// GAPS (compile-time, default off: the instantiations without it are unchanged; DESIGN.md sections 18 and 19): a row whose coordinates are
// all NaN is a missed detection, an observation of infinite error.  The forward sweep predicts through it - p = a[t-1] + q[t-1], f[t] =
// f[t-1], a[t] = p, nothing added to the log density - without reading its position or its error (the error slot of the row, which may
// hold NaN, is overwritten by a[t] as at any row); the backward sweep is unchanged and returns the interpolated posterior at the row.  The
// first and the last row must be observed and a row with only some NaN coordinates is no gap: both poison the track.  The constant of the
// log density counts the observed rows: -(n_observed - 1) * D/2 * log(2 pi).
#pragma once
#include <stddef.h>

#include "xt_kernel.h"

struct XtCondArgs {
    const double* tracks;  // [N][L][D]
    const double* sigma;   // [N][L][K] per-peak localisation errors (std), or nullptr (locerr_mode 0)
    const int8_t* states;  // [N][L]
    double* mu;            // [N][L][D]
    double* sig_out;       // [N][L][K]
    double* logdens;       // [N] or nullptr
    int64_t N;
    int32_t L, S;
    int32_t TPB;           // tracks per block = threads per block
    int32_t locerr_mode;   // as XtKernelArgs
    int32_t ws_global;     // 1: rows in global memory (the kernel instantiated for it), 0: in LDS
    int32_t pad_;
    double hdr[8];         // the model blob's header: [0..2] global l2 per dimension, [3] slope, [4] offset
    double d2[XT_MAX_STATES * XT_MAX_STATES];  // the model blob's step-variance table [from][to], nb_substeps 1
};

// Doubles per track row in LDS, odd.
XT_HD int xt_cond_row_doubles(int L, int D, int K) { return (L * (D + K)) | 1; }
// Bytes per track row of staged states: a multiple of 4 with an odd number of dwords.
XT_HD int xt_cond_srow_bytes(int L) { return 4 * (((L + 3) / 4) | 1); }
XT_HD int xt_cond_tab_doubles(int S) { return (S * S + 1) & ~1; }
// LDS footprint in doubles.  Layout: [d2 table][rows x TPB][state rows x TPB]; the global placement keeps the table only.
XT_HD size_t xt_cond_lds_doubles(int S, int L, int D, int K, int tpb, bool ws_global)
{
    size_t n = (size_t)xt_cond_tab_doubles(S);
    if (!ws_global) n += (size_t)tpb * xt_cond_row_doubles(L, D, K) + ((size_t)tpb * xt_cond_srow_bytes(L) + 7) / 8;
    return n;
}

// The step-variance table of a launch: read through the kernarg segment on the device (the arguments are the kernel's only parameter), so
// that a per-lane index does not turn the by-value struct into a scratch copy (as xt_blob_ptr).
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ const double* xt_cond_d2_ptr(const XtCondArgs&)
{
    return (const double*)((const char*)__builtin_amdgcn_kernarg_segment_ptr() + __builtin_offsetof(XtCondArgs, d2));
}
#else
inline const double* xt_cond_d2_ptr(const XtCondArgs& a) { return a.d2; }
#endif

template <int D, int K, bool WS_GLOBAL, bool GAPS = false, class Ctx>
XT_HD void xt_cond_body(const XtCondArgs& a, Ctx& cx)
{
    static_assert(K == 1 || K == D, "one error channel, or one per dimension");
    const int S = a.S, L = a.L, TPB = a.TPB;
    const int tid = cx.tid(), T = cx.nthreads();
    const int LD = L * D, LK = L * K;
    const int RS = xt_cond_row_doubles(L, D, K), SB = xt_cond_srow_bytes(L);
    double* smem = cx.smem();
    double* d2 = smem;
    double* rows = smem + xt_cond_tab_doubles(S);
    int8_t* srows = (int8_t*)(rows + (size_t)TPB * RS);

    {
        const double* src = xt_cond_d2_ptr(a);
        for (int i = tid; i < S * S; i += T) d2[i] = src[i];
    }
    double l2g[K];
    XT_UNROLL
    for (int k = 0; k < K; ++k) l2g[k] = a.hdr[k];
    const double slope = a.hdr[3], offset = a.hdr[4];
    const int mode = a.locerr_mode;
    cx.sync();

    const int64_t nbatch = (a.N + TPB - 1) / TPB;
    for (int64_t batch = cx.block(); batch < nbatch; batch += cx.nblocks()) {
        const int64_t trk0 = batch * TPB;
        const int nt = a.N - trk0 < TPB ? (int)(a.N - trk0) : TPB;
        const int64_t trk = trk0 + tid;
        const bool act = tid < nt;

        if (!WS_GLOBAL) {
            // ---- the block's runs of positions / errors / states -> LDS rows (consecutive threads, consecutive addresses)
            auto stage = [&](const double* src, int n, int len, int col0) XT_INL {
                int row = tid / len, col = tid - row * len;
                const int qT = T / len, rT = T - qT * len;
                for (int e = tid; e < n; e += T) {
                    rows[row * RS + col0 + col] = src[e];
                    row += qT;
                    col += rT;
                    if (col >= len) {
                        col -= len;
                        ++row;
                    }
                }
            };
            stage(a.tracks + trk0 * LD, nt * LD, LD, 0);
            if (mode != 0) stage(a.sigma + trk0 * LK, nt * LK, LK, LD);
            {
                const int8_t* src = a.states + trk0 * L;
                int row = tid / L, col = tid - row * L;
                const int qT = T / L, rT = T - qT * L;
                for (int e = tid; e < nt * L; e += T) {
                    srows[row * SB + col] = src[e];
                    row += qT;
                    col += rT;
                    if (col >= L) {
                        col -= L;
                        ++row;
                    }
                }
            }
            cx.sync();
        }

        if (act) {
            // the lane's rows: read c at pc, the error (std) at pe, the state at ps; keep f / mu at pf and a / sigma at pa
            const double* pc = WS_GLOBAL ? a.tracks + trk * LD : rows + tid * RS;
            double* pf = WS_GLOBAL ? a.mu + trk * LD : rows + tid * RS;
            const double* pe = WS_GLOBAL ? (mode != 0 ? a.sigma + trk * LK : nullptr) : rows + tid * RS + LD;
            double* pa = WS_GLOBAL ? a.sig_out + trk * LK : rows + tid * RS + LD;
            const int8_t* ps = WS_GLOBAL ? a.states + trk * L : srows + tid * SB;

            bool bad = false;
            auto state_at = [&](int t) XT_INL {  // a table is never indexed with a state outside [0, S)
                const int b = ps[t];
                const bool ok = b >= 0 && b < S;
                bad = bad || !ok;
                return ok ? b : 0;
            };
            auto l2_at = [&](int t, double* l2) XT_INL {
                XT_UNROLL
                for (int k = 0; k < K; ++k) {
                    if (mode == 0) {
                        l2[k] = l2g[k];
                    } else {
                        double s = pe[t * K + k];
                        bad = bad || s != s;
                        if (mode == 2) {
                            s = xt_fma(s, slope, offset);
                            s = s < 1e-6 ? 1e-6 : s;
                        }
                        l2[k] = s * s;
                    }
                }
            };

            // ---- forward sweep
            double f[D], av[K];
            int bp = state_at(0);
            XT_UNROLL
            for (int d = 0; d < D; ++d) {
                f[d] = pc[d];
                bad = bad || f[d] != f[d];
                if (WS_GLOBAL) pf[d] = f[d];
            }
            l2_at(0, av);
            XT_UNROLL
            for (int k = 0; k < K; ++k) pa[k] = av[k];
            double quad = 0.0, lm = 1.0;  // sum of r^2 / w;  prod of w = lm * 2^le
            int le = 0;
            int ngap = 0;  // GAPS: missed detections of the track
            for (int t = 1; t < L; ++t) {
                const int bc = state_at(t);
                const double q = d2[bp * S + bc];
                bp = bc;
                if (GAPS) {
                    int nn = 0;
                    XT_UNROLL
                    for (int d = 0; d < D; ++d) nn += pc[t * D + d] != pc[t * D + d] ? 1 : 0;
                    if (nn == D) {  // a missed detection: predict through it (some NaN coordinates: no gap, the row poisons the track below)
                        bad = bad || t == L - 1;
                        ++ngap;
                        XT_UNROLL
                        for (int k = 0; k < K; ++k) {
                            av[k] = av[k] + q;
                            pa[t * K + k] = av[k];
                        }
                        XT_UNROLL
                        for (int d = 0; d < D; ++d) pf[t * D + d] = f[d];
                        continue;
                    }
                }
                double l2[K], g[K], rw[K];
                l2_at(t, l2);
                XT_UNROLL
                for (int k = 0; k < K; ++k) {
                    const double p = av[k] + q;
                    const double w = p + l2[k];
                    rw[k] = xt_rcp(w);
                    g[k] = p * rw[k];
                    av[k] = g[k] * l2[k];
                    pa[t * K + k] = av[k];
                    lm *= w;
                    le += xt_frexp_exp(lm);
                    lm = xt_frexp_mant(lm);
                }
                XT_UNROLL
                for (int d = 0; d < D; ++d) {
                    const int k = K == 1 ? 0 : d;
                    const double c = pc[t * D + d];
                    bad = bad || c != c;
                    const double r = c - f[d];
                    f[d] = xt_fma(g[k], r, f[d]);
                    pf[t * D + d] = f[d];
                    quad = xt_fma(r * r, rw[k], quad);
                }
            }

            // ---- backward sweep (bp is the state of position L - 1; f and av hold f[L-1] and a[L-1])
            if (bad) {
                for (int i = 0; i < LD; ++i) pf[i] = NAN;
                for (int i = 0; i < LK; ++i) pa[i] = NAN;
            } else {
                XT_UNROLL
                for (int k = 0; k < K; ++k) pa[(L - 1) * K + k] = sqrt(av[k]);
                for (int t = L - 2; t >= 0; --t) {
                    const int bc = state_at(t);
                    const double q = d2[bc * S + bp];
                    bp = bc;
                    double J[K];
                    XT_UNROLL
                    for (int k = 0; k < K; ++k) {
                        const double at = pa[t * K + k];
                        const double p = at + q;
                        J[k] = at * xt_rcp(p);
                        av[k] = xt_fma(J[k] * J[k], av[k] - p, at);
                        pa[t * K + k] = sqrt(av[k]);
                    }
                    XT_UNROLL
                    for (int d = 0; d < D; ++d) {
                        const double ft = pf[t * D + d];
                        f[d] = xt_fma(J[K == 1 ? 0 : d], f[d] - ft, ft);
                        pf[t * D + d] = f[d];
                    }
                }
            }
            if (a.logdens) {
                const double logw = log(lm) + (double)le * XT_LN2;  // sum over steps and channels of log w
                a.logdens[trk] = bad ? NAN : -0.5 * ((K == 1 ? (double)D : 1.0) * logw + quad) - (double)(GAPS ? L - 1 - ngap : L - 1) * D * 0.5 * XT_LOG2PI;
            }
        }

        if (!WS_GLOBAL) {
            cx.sync();
            // ---- rows -> the block's runs of mu and sigma
            auto unstage = [&](double* dst, int n, int len, int col0) XT_INL {
                int row = tid / len, col = tid - row * len;
                const int qT = T / len, rT = T - qT * len;
                for (int e = tid; e < n; e += T) {
                    dst[e] = rows[row * RS + col0 + col];
                    row += qT;
                    col += rT;
                    if (col >= len) {
                        col -= len;
                        ++row;
                    }
                }
            };
            unstage(a.mu + trk0 * LD, nt * LD, LD, 0);
            unstage(a.sig_out + trk0 * LK, nt * LK, LK, LD);
            cx.sync();  // the rows are re-used by the next batch
        }
    }
}
