// Path choice and launch geometry of the fixed-window likelihood / posterior / sequence-matrix path (host only, no HIP calls, no context, no
// environment: the library and tests/emul compile the same function; tests/test_ll_geom_cpu.py).  xt_ll_pick is the ONE place where a launch
// group of extrack_loglik* / extrack_predict* / extrack_sequence_matrix gets its kernel family or is refused: called by the launcher
// (extrack_ll.hip: xt_ll_launch) and by xt_gaps_check.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "xt_big.h"
#include "xt_entry.h"
#include "xt_fast2.h"
#include "xt_grad_geom.h"
#include "xt_reg2.h"
#include "xt_tables.h"

// ---- which instantiations exist: the domains of the kernel-address lookups, restated as pure functions (a lookup that returns nullptr where
// its predicate holds is caught by the launcher's nullptr guard)
// xt_track_kernel through xt_dispatch: G = 0 is the runtime-G instantiation, posteriors need a compile-time G
static inline bool xt_ll_general_built(int G, int D, int K, bool preds) { return (preds ? G >= 2 && G <= 6 : G == 0 || (G >= 2 && G <= 4)) && xt_grad_dk_built(D, K); }
static inline bool xt_ll_gap_built(int G, int D, int K) { return G >= 2 && G <= 4 && xt_grad_dk_built(D, K); }  // xt_gap_kernel_ptr (extrack_gaps.hip)
static inline bool xt_ll_entry_built(int GP, int D, int K) { return GP >= 4 && GP <= 64 && (GP & (GP - 1)) == 0 && xt_grad_dk_built(D, K); }  // xt_dispatch_entry
static inline bool xt_ll_f2_built(int F, int D, int K) { return F >= 4 && F <= 7 && xt_grad_dk_built(D, K); }  // xt_dispatch_f2, xt_r2_kernel(.., NP = 0)
static inline bool xt_ll_big_built(int D, int K) { return xt_grad_dk_built(D, K); }  // xt_big_kernel_dk

enum XtLlPath { XT_LL_NONE = 0, XT_LL_REG2, XT_LL_FAST2, XT_LL_ENTRY, XT_LL_GENERAL, XT_LL_GAPS, XT_LL_BIG, XT_LL_GAPS_REG2 };
// what extrack_last_ll_path reports as text (extrack_amd._lib.LL_PATH_NAMES is the same list)
static inline const char* xt_ll_path_name(int p)
{
    static const char* const n[] = {"none", "reg2", "fast2", "entry", "general", "gaps", "big", "gaps_reg2"};
    return p >= 0 && p <= XT_LL_GAPS_REG2 ? n[p] : "none";
}
// why no kernel serves the group (all EXTRACK_E_UNSUPPORTED)
enum XtLlRefusal { XT_LL_FITS = 0, XT_LL_NO_GAPS_BIG, XT_LL_NO_SEQ_BIG, XT_LL_NO_PREDS_F15, XT_LL_NO_BUDGET, XT_LL_NO_PREDS_G, XT_LL_NO_VARIANT };
static inline const char* xt_ll_refusal_text(int r)
{
    switch (r) {
    case XT_LL_NO_GAPS_BIG: return "missed detections: the global-state kernel for big models has no gap-aware variant";
    case XT_LL_NO_SEQ_BIG: return "sequence matrix: n_states^frame_len sequences per track do not fit a workgroup";
    case XT_LL_NO_PREDS_F15: return "posteriors: frame_len > 15";
    case XT_LL_NO_BUDGET: return "n_states^frame_len sequences per track: the state of one workgroup per bucket exceeds the scratch budget (EXTRACK_BIG_WS_MB)";
    case XT_LL_NO_PREDS_G: return "posteriors are built for n_states <= 6";
    default: return "kernel variant not built";
    }
}

// What the launcher needs of a launch group before it asks the device anything (occupancy and the grid split stay with the launcher).
struct XtLlPick {
    int path = XT_LL_NONE, refusal = XT_LL_FITS;
    int tpb = 0, threads = 0;
    size_t lds = 0;
    bool wide = false;      // more than 256 threads: the 1024-thread instantiation
    int sel = 0;            // template selector of the family: G as xt_dispatch maps it (general, gaps), frame_len (reg2, fast2), xt_entry_gp(G) (entry)
    int64_t ws_stride = 0;  // big: doubles of one wavefront's sequence state
    size_t max_blocks = 0;  // big: upper bound of the grid (scratch budget)
};

// KS: sigma dims of the buckets in the per-peak modes, else 0.  preds: posteriors; seq: the general kernel writes the log-weight of every
// sequence of the last position, without the leaving term (extrack_sequence_matrix); gaps: the general body's gap-aware instantiations only
// (extrack_gaps.hip), two states included.  ll_reg2: extrack_ctx::ll_reg2; force_big / big_budget_mb: EXTRACK_FORCE_BIG / EXTRACK_BIG_WS_MB.
static inline XtLlPick xt_ll_pick(const XtConfig& c, int D, int K, int KS, bool preds, bool seq, bool gaps, int ll_reg2, bool force_big,
                                  size_t big_budget_mb, int nbuckets, int n_cu)
{
    XtLlPick p, none;
    int tpb, threads;
    size_t lds;
    const bool fast2 = !seq && !gaps && xt_use_fast2(c.S, c.NS, c.F, preds);
    const bool entry = !seq && !gaps && !fast2 && xt_use_entry(c.NS, c.G, c.NG, preds);
    if (entry) {
        xt_entry_geometry(c.S, c.G, c.E, c.NG, D, K, tpb, threads, lds);
    } else if (fast2) {
        const int tpw = 64 >> (c.F - 1);
        tpb = tpw * XT_F2_WAVES;
        threads = 64 * XT_F2_WAVES;
        lds = ll_reg2 ? (size_t)xt_r2_block_bytes(0, D, KS, tpw) : (size_t)xt_f2_block_bytes(D, K, KS, tpw);
    } else {
        xt_geometry(c, D, K, tpb, threads);
        lds = xt_lds_bytes(c, D, K, tpb);
    }
    // the sequence state of a track does not fit a workgroup (more than 1024 groups, more than the CU's LDS, posteriors beyond the built group
    // sizes): one lane per track with the state in global memory (xt_big.h)
    bool big = lds > 160 * 1024 || (!fast2 && !entry && (threads > 1024 || (preds && c.G > 6)));
    big = big || (force_big && !seq && !gaps);
    if (big && gaps) return none.refusal = XT_LL_NO_GAPS_BIG, none;
    if (big) {
        if (seq) return none.refusal = XT_LL_NO_SEQ_BIG, none;
        if (preds && c.F > 15) return none.refusal = XT_LL_NO_PREDS_F15, none;
        const int NW = 4;
        threads = 64 * NW;
        tpb = threads;
        lds = (size_t)(((xt_tab_doubles(c.S, c.G) + 1) & ~1) + threads) * sizeof(double);
        p.ws_stride = xt_big_ws_doubles(c.E, D, K);
        const size_t per_block = (size_t)p.ws_stride * sizeof(double) * NW;
        const size_t maxb = std::max<size_t>(1, (big_budget_mb << 20) / per_block);
        if (maxb < (size_t)nbuckets) return none.refusal = XT_LL_NO_BUDGET, none;
        // the grid never exceeds max_blocks (xt_split_blocks); the scratch is reserved for the grid actually launched
        p.max_blocks = std::min<size_t>(maxb, (size_t)n_cu * 8);
    }
    p.tpb = tpb, p.threads = threads, p.lds = lds, p.wide = threads > 256;
    bool built;
    if (big) {
        p.path = XT_LL_BIG;
        built = xt_ll_big_built(D, K);
    } else if (gaps) {
        p.path = XT_LL_GAPS, p.sel = c.NS == 1 ? c.G : 0;
        built = xt_ll_gap_built(p.sel, D, K);
    } else if (fast2) {
        p.path = ll_reg2 ? XT_LL_REG2 : XT_LL_FAST2, p.sel = c.F;
        built = xt_ll_f2_built(p.sel, D, K);
    } else if (entry) {
        p.path = XT_LL_ENTRY, p.sel = xt_entry_gp(c.G);
        built = xt_ll_entry_built(p.sel, D, K);
    } else {
        p.path = XT_LL_GENERAL, p.sel = preds || (c.G >= 2 && c.G <= 4) ? c.G : 0;
        built = xt_ll_general_built(p.sel, D, K, preds);
    }
    if (!built) return none.refusal = preds ? XT_LL_NO_PREDS_G : XT_LL_NO_VARIANT, none;
    return p;
}

// ---- missed detections on the register-resident 2-state kernel (xt_reg2.h: xt_r2_body<.., GAPS>)
static inline bool xt_ll_gap_reg2_built(int F, int D) { return F >= 4 && F <= 7 && D >= 1 && D <= 3; }  // xt_r2_gap_kernel (extrack_reg2.hip)

// Range of the g-form steps under gaps.  `scaling == 2` (xt_launch_scaling) says: fractions and weights in [1e-20, 1], one global l2 >= 1e-12,
// l2 + d2min >= 1e-12 and 2 l2 + d2max <= 1e4 - derived with u <= l2, i.e. v = l2 + u <= 2 l2.  A missed frame adds d2 to the carried variance
// instead of shrinking it, and a track of the group has at most Lmax - 2 of them, so v <= 2 l2 + (Lmax - 2) d2max and
//     den = d2 + v <= (2 l2 + d2max) + (Lmax - 2) d2max <= 1e4 + (Lmax - 2) d2max.
// The upgrade asks for (Lmax - 2) d2max <= 1e4: den in [1e-12, 2e4].  What xt_r2_step_g, xt_r2_chain_g and the read-out need then:
//   * g = l2 / den in [5e-17, 1] at an observed step (1e-16 before), so the lazy mantissa picks up at least (5e-17)^(3/2) = 3.5e-25 per step
//     (1e-24 before); a missed step multiplies it by exactly 1 (no Gaussian factor) - three un-normalised steps stay within [4e-74, 8];
//   * Ws Dq0 Dq1 = W^3 den^2 in [6e-245, 2e11]; h_q <= 1 / (W_min^2 den_min) = 6e158; k_q = g_q / Ws (observed) or 1 / Ws (missed) <= 2.5e73;
//     v_q = Dq_q / Ws = den_q <= 2e4 at a missed step - the product R (Dq0 Dq1) Dq_q is formed as (R Dq0 Dq1) Dq_q, each factor in range;
//   * the chain: at most F - 2 = 5 positions, y >= (3.5e-25)^5 = 5e-123 times the initial fraction;
//   * the read-out: the product of its four den <= 1.6e17, >= 1e-48;
//   * lambda: a missed step adds -2 lnT' only (|.| <= 2 * 46 + D * 28), the re-centring is unchanged.
// All far inside the fp64 range, as in the gap-free derivation (xt_tables.h: xt_build_blob; xt_reg2.h: xt_r2_step_g).
static inline bool xt_ll_gap_reg2_range(int scaling, int Lmax, double d2max)
{
    return scaling == 2 && d2max == d2max && (double)(Lmax > 2 ? Lmax - 2 : 0) * d2max <= 1e4;
}

// Frame lengths upgraded (bit F of the mask).  Default: 5, 6, 7.  Frame_len 4 is built, tested and measured faster than the general gap body
//  but is upgraded only on request (EXTRACK_GAP_REG2_F=4,5,6,7 | all when the context is created): the recorded launch geometry
// that tests/test_hip_parity.py compares a default context's two-state, frame_len 4 gapped launch with is that of the general gap body.
#define XT_LL_GAP_REG2_F_DEFAULT ((1 << 5) | (1 << 6) | (1 << 7))
#define XT_LL_GAP_REG2_F_ALL ((1 << 4) | XT_LL_GAP_REG2_F_DEFAULT)

// The second decision of a gapped launch group, after xt_ll_pick and once the group's scaling is known (xt_launch_scaling of the model and its
// one localisation variance): either `pk` unchanged (the general gap body) or the geometry of the gap-aware register-resident kernel.
// Upgraded: likelihood (with or without per-track output), S = 2, nb_substeps = 1, frame_len 4..7, ll_reg2 (EXTRACK_LL_PATH=lds keeps the
// general body), one global scalar error (KS == 0: locerr_mode 0; K == 1), scaling 2 under the gap-extended bound above; fmask: the frame
// lengths the context upgrades (extrack_ctx::gap_reg2_fmask).
static inline XtLlPick xt_ll_gap_reg2(const XtLlPick& pk, const XtConfig& c, int D, int K, int KS, bool preds, bool per_track, int ll_reg2, int scaling,
                                      int Lmax, double d2max, int fmask = XT_LL_GAP_REG2_F_DEFAULT)
{
    (void)per_track;
    if (c.F < 0 || c.F > 30 || !((fmask >> c.F) & 1)) return pk;
    if (pk.path != XT_LL_GAPS || preds || !xt_use_reg2(c.S, c.NS, c.F) || ll_reg2 != 1 || KS != 0 || K != 1) return pk;
    if (!xt_ll_gap_reg2_built(c.F, D) || !xt_ll_gap_reg2_range(scaling, Lmax, d2max)) return pk;
    XtLlPick p;
    const int tpw = 64 >> (c.F - 1);
    p.path = XT_LL_GAPS_REG2, p.sel = c.F;
    p.tpb = tpw * XT_F2_WAVES, p.threads = 64 * XT_F2_WAVES;
    p.lds = (size_t)xt_r2_gap_block_bytes(D, tpw);
    return p;
}
