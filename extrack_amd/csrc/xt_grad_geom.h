// Path choice and launch geometry of the gradient path (host only, no HIP calls, no context, no environment: the library and tests/emul
// compile the same functions; tests/test_grad_geom_cpu.py).  xt_grad_pick is the ONE place where a launch group of extrack_loglik_grad /
// _scores (and their _gaps forms) gets its kernel family - reverse mode (xt_rev.h), register-resident 2-state (xt_reg2.h), register + LDS
// exchange (xt_gradr.h), LDS-resident (xt_grad.h) - or is refused: called by the launcher (extrack_grad.hip) and by xt_grad_gaps_check.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "xt_grad.h"
#include "xt_gradr.h"
#include "xt_reg2.h"
#include "xt_rev.h"
#include "xt_tables.h"

// Tuning knobs of the context (extrack_create reads them from the environment once).
struct XtGradKnobs {
    int grad_reg2 = 1;  // 1 = register-resident kernels where built (xt_reg2.h for 2 states, else xt_gradr.h), 0 = the LDS-resident xt_grad.h
                        // only, 2 = xt_gradr.h before xt_reg2.h (tests); EXTRACK_GRAD_PATH = reg2 | lds | gradr
    int grad_rev = 1;   // reverse-mode kernels (xt_rev.h): 1 = where they win, 0 = never, 2 = wherever built; EXTRACK_GRAD_PATH = rev | auto
    int gradr_npc = 0;  // directions per pass of the xt_gradr.h kernels (0: chosen here; EXTRACK_GRADR_NPC = 3 | 4 also forces these kernels for small models)
    size_t rev_log_mb = 16384;  // budget of the reverse-mode log regions (EXTRACK_REV_LOG_MB): the launch uses fewer blocks to stay within it
    int oversub = 8;            // block generations per CU of the xt_reg2.h launches (EXTRACK_OVERSUB, the likelihood's knob)
    int rev_oversub = 16;       // ... of the reverse-mode launch (EXTRACK_REV_OVERSUB; each block owns a log region: fewer blocks, smaller cache footprint)
    int lds_pj = 0;             // lanes per group of the LDS-resident kernel (EXTRACK_GRAD_PJ = 1 | 2 | 4 | 8; 0: chosen here)
    int r2_maxnp = 8;           // most directions per pass of the xt_reg2.h kernels (EXTRACK_R2_MAXNP = 1 .. 8)
};

// ---- which instantiations exist: the domains of the kernel-address tables, restated as pure functions (a table that returns nullptr where
// its predicate holds is caught by the launcher's "gradient kernel variant not built" guard)
static inline bool xt_grad_dk_built(int D, int K) { return (K == 1 && D >= 1 && D <= 3) || (K == D && (D == 2 || D == 3)); }
static inline bool xt_rev_built(int G, int D, int K, int nbuf) { return G >= 2 && G <= 4 && (nbuf == 1 || nbuf == 2) && xt_grad_dk_built(D, K); }
static inline bool xt_gradr_built(int G, int D, int K, int NPC) { return G >= 2 && G <= 4 && (NPC == 3 || NPC == 4) && xt_grad_dk_built(D, K); }
static inline bool xt_r2_built(int F, int D, int K, int NP) { return F >= 4 && F <= 7 && NP >= 1 && NP <= 8 && xt_grad_dk_built(D, K); }
// the gap-aware gradient kernels of xt_reg2.h (xt_r2_grad_gap_kernel, extrack_reg2.hip): one scalar localisation error
static inline bool xt_r2_gap_grad_built(int F, int D, int K, int NP) { return F >= 4 && F <= 7 && NP >= 1 && NP <= 8 && K == 1 && D >= 1 && D <= 3; }
// the LDS-resident kernel: any G without gaps (G outside 2 .. 4 runs the generic instantiation 0); both workgroup sizes
static inline bool xt_grad_lds_built(int G, int D, int K, bool gaps) { return (!gaps || (G >= 2 && G <= 4)) && xt_grad_dk_built(D, K); }

// LDS bytes of a block of tpb tracks with NP directions
static inline size_t xt_grad_lds_bytes(const XtConfig& c, int D, int K, int NP, int tpb, bool tan_lds)
{
    size_t d = (size_t)((xt_tab_doubles(c.S, c.G) + 1) & ~1);
    if (tan_lds) d += (size_t)((NP * xt_grad_tb_doubles(c.S, c.G) + 1) & ~1);
    d += (size_t)tpb * ((size_t)xt_grad_region_doubles(c.EP, D, K, NP) + xt_grad_acc_doubles(NP, c.NG) + xt_stage_doubles(D));
    return d * sizeof(double);
}

// Geometry of one pass of the LDS-resident kernel (xt_grad.h) with NP directions
struct XtGradLdsGeom {
    bool tan_lds;
    int PJ, tpb, threads;
    size_t lds;
};
static inline XtGradLdsGeom xt_grad_lds_geometry(const XtConfig& c, int D, int K, int NP, int lds_pj)
{
    XtGradLdsGeom o;
    o.tan_lds = (size_t)NP * xt_grad_tb_doubles(c.S, c.G) * 8 <= 16 * 1024;
    const size_t per_track = xt_grad_lds_bytes(c, D, K, NP, 1, o.tan_lds) - xt_grad_lds_bytes(c, D, K, NP, 0, o.tan_lds);
    const size_t fixed = xt_grad_lds_bytes(c, D, K, NP, 0, o.tan_lds);
    const size_t budget = 64 * 1024;
    // PJ lanes per group: about two directions per lane, as long as a track's threads fit a workgroup
    int PJ = 1;
    while (PJ < 8 && PJ * 2 <= NP && NP > 2 * PJ - 1 && c.NG * PJ * 2 <= 1024) PJ *= 2;
    if (lds_pj && c.NG * lds_pj <= 1024) PJ = lds_pj;
    const int NT = c.NG * PJ;
    const int by_threads = NT >= 256 ? 1 : 256 / NT;
    const int by_lds = budget > fixed + per_track ? (int)((budget - fixed) / per_track) : 1;
    o.PJ = PJ;
    o.tpb = std::max(1, std::min(by_threads, by_lds));
    o.threads = (o.tpb * NT + 63) / 64 * 64;
    o.lds = xt_grad_lds_bytes(c, D, K, NP, o.tpb, o.tan_lds);
    return o;
}
// directions per pass of the LDS-resident kernel: as many as keep one track's state within the LDS of a CU (all of them for the usual models)
static inline int xt_grad_lds_npass_dir(const XtConfig& c, int D, int K, int n_dir)
{
    int npass_dir = std::max(n_dir, 1);
    while (npass_dir > 1 && (npass_dir > 16 || xt_grad_lds_bytes(c, D, K, npass_dir, 1, false) > 150 * 1024)) npass_dir = (npass_dir + 1) / 2;
    return npass_dir;
}
// directions per pass (and the compile-time NPC) of the register-resident kernel (xt_gradr.h)
static inline int xt_gradr_per_pass(int gradr_npc, int n_dir, int* NPC_out)
{
    // 4 directions per pass: with 6 the register allocator spills inside the step loop (3 states: 917 GB of scratch traffic per C3
    // launch, r03 PMC) and the pass count saved does not pay for it; 3 per pass when that needs no more passes
    int NPC = gradr_npc ? gradr_npc : 4;
    const int npass = (n_dir + NPC - 1) / NPC, per = (n_dir + npass - 1) / npass;
    if (per <= 3 && !gradr_npc) NPC = 3;
    *NPC_out = NPC;
    return per;
}

enum XtGradPath { XT_GRAD_NONE = 0, XT_GRAD_REV, XT_GRAD_REG2, XT_GRAD_GRADR, XT_GRAD_LDS, XT_GRAD_GAPS_REG2, XT_GRAD_GAPS_REV };
// what extrack_last_grad_path reports as text (extrack_amd._lib.GRAD_PATH_NAMES is the same list)
static inline const char* xt_grad_path_name(int p)
{
    static const char* const n[] = {"none", "rev", "reg2", "gradr", "lds", "gaps_reg2", "gaps_rev"};
    return p >= 0 && p <= XT_GRAD_GAPS_REV ? n[p] : "none";
}
// why no kernel serves the group (all EXTRACK_E_UNSUPPORTED)
enum XtGradRefusal { XT_GRAD_FITS = 0, XT_GRAD_NO_ONE_DIR, XT_GRAD_NO_GROUPS, XT_GRAD_NO_LDS, XT_GRAD_NO_VARIANT, XT_GRAD_NO_NP16 };
static inline const char* xt_grad_refusal_text(int r)
{
    switch (r) {
    case XT_GRAD_NO_ONE_DIR: return "sequence state with one tangent direction does not fit the 160 KiB LDS of a CU";
    case XT_GRAD_NO_GROUPS: return "n_states^(frame_len-nb_substeps) > 1024 groups per track is not built";
    case XT_GRAD_NO_LDS: return "sequence state does not fit the 160 KiB LDS of a CU";
    case XT_GRAD_NO_NP16: return "more than 16 directions per pass";
    default: return "gradient kernel variant not built";
    }
}

// What the launcher needs of a launch group before it asks the device anything (occupancy and the grid split stay with the launcher).
struct XtGradPick {
    int path = XT_GRAD_NONE, refusal = XT_GRAD_FITS;
    int tpb = 0, threads = 0;  // rev, reg2, gradr (lds: per pass, gm[])
    size_t lds = 0;            // rev, gradr (reg2: depends on the uniform directions of the pass, xt_r2_block_bytes)
    int nbuf = 0;              // rev: exchange buffers per track
    size_t max_blocks = 0;     // rev: log regions the budget pays for
    int64_t log_stride = 0;    // rev: doubles per track slot
    int tpw = 0, maxnp = 0;    // reg2: tracks per wavefront, most directions per pass
    int NPC = 0, per = 0;      // gradr: compile-time and actual directions per pass
    int npass_dir = 0, rem = 0;  // lds: directions per pass, directions of the last pass when it is a shorter one (else 0)
    XtGradLdsGeom gm[2] = {};    // lds: geometry of a pass of npass_dir directions / of rem directions
};

// Lmax / nbuckets: longest track length and bucket count of the group; scores: a per-track scores evaluation; gaps: missed detections.
// Order of trial: rev, reg2, gradr, lds.
static inline XtGradPick xt_grad_pick(const XtConfig& c, int D, int K, int locerr_mode, int n_dir, int Lmax, int nbuckets, int n_cu, bool gaps,
                                      bool scores, const XtGradKnobs& kn)
{
    XtGradPick p;
    // ---- two-state models: register-resident kernels (xt_reg2.h), <= 8 directions per pass, tangents in VGPRs
    const bool r2 = !gaps && kn.grad_reg2 == 1 && xt_use_reg2(c.S, c.NS, c.F) && locerr_mode == 0 && n_dir > 0 && xt_r2_built(c.F, D, K, 1);
    // ---- reverse mode (xt_rev.h): one forward + one backward sweep whatever the number of directions; the adjoint of the model blob
    // is contracted with the tangent blocks by a small kernel.  3 / 4 members per group by default (r03: C3, 13 directions)
    {
        const int tpb = std::max(1, 256 / c.NG), threads = (tpb * c.NG + 63) / 64 * 64;
        // one exchange buffer (two barriers per step) where two do not leave room for a second workgroup on the CU
        const size_t lds2 = xt_rev_lds_bytes(c.S, c.G, c.EP, D, K, tpb, threads, 2), lds1 = xt_rev_lds_bytes(c.S, c.G, c.EP, D, K, tpb, threads, 1);
        const int nbuf = (2 * lds2 > 160 * 1024 && 2 * lds1 <= 160 * 1024) ? 1 : 2;
        const size_t lds = nbuf == 1 ? lds1 : lds2;
        const bool built = n_dir > 0 && xt_rev_supported(c.G, c.NG) && xt_rev_built(c.G, D, K, nbuf);
        // the merged-state logs (one region per track slot of every block) must fit the budget with at least one block per two CUs:
        // very long tracks go to the forward-mode kernels instead
        const int64_t log_stride = (int64_t)std::max(std::max(Lmax, 2) - 2, 1) * xt_rev_step_doubles(c.NG, D, K);
        const size_t max_blocks = (kn.rev_log_mb << 20) / ((size_t)tpb * (size_t)log_stride * sizeof(double));
        if (!gaps && !scores && built && lds <= 160 * 1024 && max_blocks >= std::max((size_t)n_cu / 2, (size_t)nbuckets) &&
            (kn.grad_rev == 2 || (kn.grad_rev == 1 && kn.grad_reg2 == 1 && !r2))) {
            p.path = XT_GRAD_REV;
            p.tpb = tpb, p.threads = threads, p.nbuf = nbuf, p.lds = lds, p.max_blocks = max_blocks, p.log_stride = log_stride;
            return p;
        }
    }
    if (r2) {
        p.path = XT_GRAD_REG2;
        p.tpw = 64 >> (c.F - 1), p.tpb = p.tpw * XT_F2_WAVES, p.threads = 64 * XT_F2_WAVES, p.maxnp = kn.r2_maxnp;
        return p;
    }
    // ---- 2 - 4 members per group, <= 256 groups per track: state and tangents in registers, LDS as the exchange medium (xt_gradr.h)
    // Measured against the LDS-resident kernel below (r03): C3 (3 states, 13 directions) frame_len 6 601 ms vs 1 960 ms, frame_len 4 63 vs 79 ms;
    // C2-type data through the general kernels (2 states with per-peak errors; in the order rev -> reg2 -> gradr -> lds the reverse-mode
    // kernels above now take those models first) frame_len 6 43.8 vs 52.9 ms, frame_len 4 16.1 vs 16.4 ms.
    if (kn.grad_reg2 && n_dir > 0 && c.G >= 2 && c.G <= 4 && c.NG <= 256 && xt_gradr_built(c.G, D, K, 4)) {
        const int tpb = std::max(1, 256 / c.NG), threads = (tpb * c.NG + 63) / 64 * 64;
        int NPC;
        const int per = xt_gradr_per_pass(kn.gradr_npc, n_dir, &NPC);
        const size_t lds = xt_gradr_lds_bytes(c.S, c.G, c.E, c.EP, c.NG, c.P, D, K, per, tpb);
        if (xt_gradr_built(c.G, D, K, NPC) && lds <= 160 * 1024) {
            p.path = XT_GRAD_GRADR;
            p.tpb = tpb, p.threads = threads, p.NPC = NPC, p.per = per, p.lds = lds;
            return p;
        }
    }
    // ---- everything else: the LDS-resident kernel (xt_grad.h)
    p.npass_dir = xt_grad_lds_npass_dir(c, D, K, n_dir);
    p.rem = n_dir > p.npass_dir ? n_dir % p.npass_dir : 0;
    if (xt_grad_lds_bytes(c, D, K, std::min(p.npass_dir, std::max(n_dir, 0)), 1, false) > 160 * 1024) {
        p.refusal = XT_GRAD_NO_ONE_DIR;
        return p;
    }
    for (int i = 0; i < (p.rem ? 2 : 1); ++i) {
        const int NP = i ? p.rem : std::min(p.npass_dir, n_dir);
        const XtGradLdsGeom& gm = p.gm[i] = xt_grad_lds_geometry(c, D, K, NP, kn.lds_pj);
        if (gm.threads > 1024) p.refusal = XT_GRAD_NO_GROUPS;
        else if (gm.lds > 160 * 1024) p.refusal = XT_GRAD_NO_LDS;
        else if (!xt_grad_lds_built(c.G, D, K, gaps)) p.refusal = XT_GRAD_NO_VARIANT;
        else if (NP > 16) p.refusal = XT_GRAD_NO_NP16;
        if (p.refusal) return p;
    }
    p.path = XT_GRAD_LDS;
    return p;
}

// ---- missed detections on the register-resident 2-state gradient kernels (xt_reg2.h: xt_r2_body<.., NP > 0, .., GAPS>)

// Range of the LAZY variant of xt_r2_step (well_scaled != 0: mantissas re-normalised every XT_F2_RENORM = 3 phases) under gaps.
// xt_model_well_scaled says: fractions and weights T, T * stay in [1e-20, 1], l2 + d2min >= 1e-12 and 2 l2 + d2max <= 1e4 - derived with
// u <= l2, so that den = l2 + d2 + u is in [1e-12, 1e4].  A missed frame carries u' = u_bar + d2 forward instead of l2 tt <= l2, and a track
// of the group has at most Lmax - 2 of them: u <= l2 + (Lmax - 2) d2max, den <= 1e4 + (Lmax - 2) d2max.  The lazy variant is launched only
// when (Lmax - 2) d2max <= 1e4 as well: den in [1e-12, 2e4].  What the step needs then:
//   * an observed step multiplies a mantissa by T den^(-D/2) e^x 2^(-n) with den^(-D/2) in [3.5e-7, 1e18] (1e-6 before) and the exponential's
//     mantissa in [0.5, 1]; a missed step by T alone, in [1e-20, 1] - inside the observed step's interval.  Three un-normalised steps and two
//     merges keep a mantissa within [1e-82, 4e54] ([1e-80, 1e55] before);
//   * the shared reciprocal's argument Ws Dq0 Dq1 = W^3 den^2 is in [1e-270, 3e172]; rW = R d01 = 1 / Ws <= 1e82;
//   * u'_q = U rW + d2_q = u_bar + d2_q <= 2e4 at a missed step, m'_q = M rW = m_bar; the read-out's den <= 2e4;
//   * tangents are formed on normalised quantities (a_j = w_j / W, rq = 1 / den <= 1e12, tt in [0, 1)): a missed step adds d log T and dd2
//     only.  ZF is off in both gradient variants, so a zero weight is handled as without gaps.
// All far inside the fp64 range.  Beyond the bound the GUARDED variant runs (every mantissa normalised in every step, integer exponents:
// nothing to bound); the upgrade is never refused for range.
static inline bool xt_grad_gap_reg2_lazy(bool well_scaled, int Lmax, double d2max)
{
    return well_scaled && d2max == d2max && (double)(Lmax > 2 ? Lmax - 2 : 0) * d2max <= 1e4;
}

// The second decision of a gapped launch group, after xt_grad_pick (whose outputs do not change: a gapped two-state group still comes back as
// XT_GRAD_GRADR): either `pk` unchanged or the geometry of the register-resident kernels as path XT_GRAD_GAPS_REG2.  Upgraded exactly when:
// gaps and the pick is XT_GRAD_GRADR; S = 2, nb_substeps = 1, frame_len in fmask (extrack_ctx::gap_reg2_fmask: 5, 6, 7 by default, 4 under
// EXTRACK_GAP_REG2_F=all - frame_len 4 of a default context keeps the geometry tests/test_hip_grad.py pins); kn.grad_reg2 == 1
// (EXTRACK_GRAD_PATH=gradr | lds keep today's kernels); one global scalar error (locerr_mode 0, K = 1); n_dir > 0; the kernel is built.
// Lmax is not part of the decision (the range only picks the variant, xt_grad_gap_reg2_lazy); it is an argument so that the launcher hands both
// decisions the same group.
static inline XtGradPick xt_grad_gap_reg2(const XtGradPick& pk, const XtConfig& c, int D, int K, int locerr_mode, int n_dir, int Lmax, bool gaps,
                                          const XtGradKnobs& kn, int fmask)
{
    (void)Lmax;
    if (!gaps || pk.path != XT_GRAD_GRADR) return pk;
    if (c.F < 0 || c.F > 30 || !((fmask >> c.F) & 1) || !xt_use_reg2(c.S, c.NS, c.F)) return pk;
    if (kn.grad_reg2 != 1 || locerr_mode != 0 || K != 1 || n_dir <= 0 || !xt_r2_gap_grad_built(c.F, D, K, 1)) return pk;
    XtGradPick p;
    p.path = XT_GRAD_GAPS_REG2;
    p.tpw = 64 >> (c.F - 1), p.tpb = p.tpw * XT_F2_WAVES, p.threads = 64 * XT_F2_WAVES, p.maxnp = kn.r2_maxnp;
    return p;
}

// ---- missed detections on the reverse-mode kernels (xt_rev.h: xt_rev_body<.., GAPS = true>)

// The third decision of a gapped launch group, applied to the result of xt_grad_gap_reg2 (xt_grad_pick's outputs do not change): gapped data go
// where their gap-free twin would go.  Upgraded to XT_GRAD_GAPS_REV exactly when
//   * gaps and not a per-track scores evaluation (reverse mode accumulates its adjoints across tracks);
//   * pk.path is XT_GRAD_GRADR or XT_GRAD_LDS, or it is XT_GRAD_GAPS_REG2 and kn.grad_rev == 2 (EXTRACK_GRAD_PATH=rev: wherever built);
//   * xt_grad_pick of the same group with gaps = false, scores = false returns XT_GRAD_REV: the kernel is built, the LDS fits, the log budget
//     pays for max(n_cu / 2, nbuckets) blocks, and the knobs send the plain data to reverse mode (so EXTRACK_GRAD_PATH = gradr | lds | reg2
//     keep the forward-mode kernels, and a two-state model with one global scalar error stays on gaps_reg2 / gradr).
// The upgraded pick has that twin's geometry (tpb, threads, nbuf, lds, max_blocks, log_stride).  A refused group (XT_GRAD_NONE) stays refused.
static inline XtGradPick xt_grad_gap_rev(const XtGradPick& pk, const XtConfig& c, int D, int K, int locerr_mode, int n_dir, int Lmax, int nbuckets,
                                         int n_cu, bool gaps, bool scores, const XtGradKnobs& kn)
{
    if (!gaps || scores) return pk;
    if (pk.path != XT_GRAD_GRADR && pk.path != XT_GRAD_LDS && !(pk.path == XT_GRAD_GAPS_REG2 && kn.grad_rev == 2)) return pk;
    XtGradPick tw = xt_grad_pick(c, D, K, locerr_mode, n_dir, Lmax, nbuckets, n_cu, false, false, kn);
    if (tw.path != XT_GRAD_REV) return pk;
    tw.path = XT_GRAD_GAPS_REV;
    return tw;
}
