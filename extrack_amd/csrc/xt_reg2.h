// Register-resident path of the track-likelihood recursion for TWO-STATE models with one substep (S = 2, ns = 1,
// frame_len 4..7): log-likelihood (NP = 0) and log-likelihood + exact gradient along NP model directions (NP > 0).
// GAPS (compile-time, default off: the instantiations without it are unchanged): missed detections (all-NaN rows) -
// the likelihood-only g-form path (section 25: xt_r2_step_g, xt_r2_chain_g and the staging in xt_r2_body) and, for one scalar localisation
// error, the gradient path (NP > 0, section 27: xt_r2_step<.., GAPS> and the staging of absolute positions in xt_r2_body).
//
// Reference: extrack/tracking.py:109-318 (P_Cs_inter_bound_stats), :76-98 (log_integrale_dif), :361-423 (fuse_tracks_general);
// the gradient replaces the finite differences lmfit's BFGS takes around cum_Proba_Cs (tracking.py:1371).  Same mathematics as
// xt_fast2.h (primal) and xt_grad.h (tangents: rz = d log z, dm, du); what differs is where the state lives:
//
//   * a lane owns one GROUP = the two sequences that differ only in their OLDEST state digit, held in VGPRs
//     {z, e, m[D], u[K]} x 2 (+ per direction {rz, dm[D], du[K]} x 2).  The other F - 1 digits of the lane's sequences are lane-id
//     bits.  A step merges the two members (the oldest digit is fused away), expands by the new digit q in {0, 1} and integrates
//     the position: the lane now holds two sequences that differ in their NEWEST digit;
//   * then ONE lane exchange over the lane bit that holds the oldest remaining digit brings that digit into the registers and
//     parks the newest one in the lane bit (a 2 x 2 transpose between the two lanes of a pair).  The exchanged bit rotates through
//     the F - 1 group bits, so the step loop is unrolled over F - 1 phases with compile-time exchange instructions:
//       lane bits 0, 1, 3  -> one DPP move per dword (quad_perm / row_ror:8): the lane computes the output it KEEPS (new digit =
//                             its own bit) and the one it SENDS (the other digit) - no selects;
//       lane bit 2         -> two DPP moves (row_shl:4 / row_shr:4 under bank masks); only frame_len 7 uses it;
//       lane bits 4, 5     -> v_permlane16_swap / v_permlane32_swap (gfx950): the transpose itself, outputs in natural order;
//   * nothing of the recursion goes through LDS: xt_fast2.h's step pays 10 ds_read + 10 ds_write per wave-step (a
//     ds_write_b64 occupies the CU's LDS pipe for ~6 cycles), and tangents in LDS (xt_grad.h) are LDS-bandwidth bound: 8 doubles
//     per direction and group there and back ~ 64 LDS cycles against ~40 fp64 operations.  LDS only holds the model tables
//     (read per step at lane-dependent [prev][q] addresses), the staged positions and the per-slot accumulators.
//
// Digit bookkeeping: step t (position t) exchanges group bit GB[(t-1) mod (F-1)]; the newest old digit ("prev" of the transition)
// sits in GB[(t-2) mod (F-1)].  Position 0 puts the initial state into GB[F-2]; dummy digits (time < 0) are zero-weight.
#pragma once
#include "xt_fast2.h"
#include "xt_grad.h"


template <int F>
struct XtR2Geom {
    static constexpr int NGB = F - 1;     // group bits
    static constexpr int NG = 1 << NGB;   // lanes per track
    static constexpr int TPW = 64 / NG;   // tracks per wave
};
// lane bit of group bit i (i = exchange order).  frame_len 7 needs all six lane bits; shorter windows skip bit 2 (two DPP moves).
XT_HD constexpr int xt_r2_gbit(int F, int i) { return F == 7 ? i : (i < 2 ? i : i + 1); }
XT_HD constexpr int xt_r2_gmask(int F) { return F == 7 ? 63 : (F == 6 ? 0x3b : (F == 5 ? 0x1b : 0x0b)); }
template <int F>
XT_HD int xt_r2_slot(int lane)
{
    if (F == 7) return 0;
    int ts = (lane >> 2) & 1;
    if (F == 5) ts |= ((lane >> 5) & 1) << 1;
    if (F == 4) ts |= ((lane >> 4) & 3) << 1;
    return ts;
}

// LDS map (bytes): [model blob 1 KiB (as xt_fast2.h: tables, T64, NaN flags)] [1024-entry exp table 8 KiB] [tangent blocks NP x TB] [staged positions] [accumulators]
#define XT_R2_TAN0 XT_F2_TAB_BYTES
#define XT_R2_TB 36  // xt_grad_tb_doubles(2, 2)
#define XT_R2_MAXU 4  // uniform directions served by one launch (on top of its NP full ones)
XT_HD int xt_r2_pos0(int NP) { return XT_R2_TAN0 + NP * XT_R2_TB * 8; }
XT_HD int xt_r2_acc0(int NP, int D, int KS, int tpw) { return xt_r2_pos0(NP) + XT_F2_WAVES * tpw * XT_F2_CHUNK * (D + KS) * 8; }
// likelihood-only launches (NP == 0), after the accumulators: the re-centring cells of the log-carried g-form step (xt_r2_step_g), one
// 8-byte cell per lane each (an int in it) - [largest base of the track, in the cell of the track's first lane][accumulated shift of the
// track in flight] - and per (wave, slot) a double: the shifts of the finished tracks
#define XT_R2_RC_ARR (XT_F2_WAVES * 64 * 8)
XT_HD int xt_r2_rc0(int D, int KS, int tpw) { return xt_r2_acc0(0, D, KS, tpw) + XT_F2_WAVES * 8 * 3 * 8; }
XT_HD int xt_r2_block_bytes(int NP, int D, int KS, int tpw)
{
    return xt_r2_acc0(NP, D, KS, tpw) + XT_F2_WAVES * 8 * (NP + 3) * 8 + (NP == 0 ? 2 * XT_R2_RC_ARR + XT_F2_WAVES * 8 * 8 : 0);
}
// Gap-aware likelihood-only launches (xt_r2_body<.., GAPS = true>), after everything above: per (wave, slot) 16 bytes -
// {u32 rows of the staged chunk with a NaN coordinate, then: rows that are missed frames; u32 rows with a finite coordinate; int last observed
// row before the chunk; int missed rows of the track so far}
XT_HD int xt_r2_gap0(int D, int tpw) { return xt_r2_block_bytes(0, D, 0, tpw); }
XT_HD int xt_r2_gap_block_bytes(int D, int tpw) { return xt_r2_gap0(D, tpw) + XT_F2_WAVES * 8 * 16; }
// Gap-aware gradient launches (xt_r2_body<.., NP > 0, .., GAPS = true>), after everything xt_r2_block_bytes(NPT, D, 0, tpw)
// counts (NPT = the pass's full + uniform directions): per (wave, slot) 16 bytes - {u32 rows of the staged chunk with a NaN coordinate, then:
// rows that are missed frames; u32 rows with a finite coordinate; unused; int missed rows of the track so far}
XT_HD int xt_r2_grad_gap0(int NPT, int D, int tpw) { return xt_r2_block_bytes(NPT, D, 0, tpw); }
XT_HD int xt_r2_grad_gap_block_bytes(int NPT, int D, int tpw) { return xt_r2_grad_gap0(NPT, D, tpw) + XT_F2_WAVES * 8 * 16; }
#define XT_R2_TAB0 (XT_BLOB_HDR * 8)  // byte address of table v = 0; table v at + v * 32, entry [prev][q] at + (prev * 2 + q) * 8
// Derived constants of the g-form step (xt_r2_step_g), built per workgroup in the two gaps of the blob's 1 KiB that nothing else uses (the blob
// ends at byte 800, the NaN flags take 832 .. 959): {-1 / (2 l2) (kept in the map; the ratio form of the step no longer reads it), 2 l2} and LT2[v][prev][q] = -2 lnT' = -2 (ln TAB[v][prev][q] - D/2 ln l2), v = 0 (T), 1 (T * stay)
// - at a fixed distance from the entry of table v, so that the step reaches it from the same `tab + [prev][q]` address.
#define XT_R2_GC_OFF 800
#define XT_R2_LNT_OFF 960
#define XT_R2_LNT_REL (XT_R2_LNT_OFF - XT_R2_TAB0)
static_assert(XT_R2_GC_OFF >= (XT_BLOB_HDR + XT_NTAB * 4 + 64) * 8 && XT_R2_GC_OFF + 16 <= XT_F2_NAN_OFF, "g-form constants overlap the blob / the NaN flags");
static_assert(XT_R2_LNT_OFF >= XT_F2_NAN_OFF + XT_F2_WAVES * 8 * 4 && XT_R2_LNT_OFF + 64 <= XT_F2_EXPB_OFF, "lnT' overlaps the NaN flags / the exp table");

static inline bool xt_use_reg2(int S, int NS, int F) { return S == 2 && NS == 1 && F >= 4 && F <= 7; }

template <int D, int K, int NP>
struct XtR2Lane {
    double z[2];
    int e[2];
    double m[2][D], u[2][K];
    double rz[NP ? NP : 1][2], dm[NP ? NP : 1][2][D], du[NP ? NP : 1][2][K];
};

// One recursion step at compile-time phase H (the loop is unrolled over the F - 1 phases: every exchange instruction and lane bit is an
// immediate).  tab: byte address of the transition table in use (T or T * stay).  A variant with a run-time phase - one step body, the
// exchange picked by a switch - was measured 1.8x SLOWER with 7 directions (16.4 -> 43.8 ms on C2: the switches cut the step into
// basic blocks the scheduler cannot overlap).
// FIRST: step F - 1 right after the warm-up chain (xt_r2_chain; likelihood only, zero-free): member 1 is dead and member 0 holds a
// normalised mantissa, so there is nothing to merge - the step runs on member 0 at unit weight scale (W = 1, M = m0, U = u0; Wm, We = z0, e0)
// and its shared reciprocal covers Dq[0] Dq[1] only.
// GAPS (gradient launches with one scalar localisation error; DESIGN.md sections 21, 27): `gap` = position t of this lane's track is a missed
// frame.  The gap step is the observed step at the l2 -> infinity limit of its per-child factors: no Gaussian factor (z'_q = Wm TT[q] at exponent
// We), gain tt_q -> 0 (m'_q = M rW), l2 tt_q -> d2_q + u_bar (u'_q = U rW + TD2[q]); tangents rz'_q = R + dlogT[q] (0 in a dead group),
// dm'_q = dmb, du'_q = dd2_q + dub.  Per-lane SELECTS, no branch: the tracks of a wave (64 >> (F - 1) of them) miss different rows, and a branch
// would cut the unrolled phase into basic blocks (see above what that cost once).  The selects sit where the fewest are needed - on the step's
// SHARED factors rather than on every direction's results:
//   * c - m_bar (dmW) := 0: the one place the position enters.  The staged position of a missed row is NaN; after this select nothing of the
//     step depends on it (dn = 0, hd = 0, x = 0: a NaN and any number as the coordinate give the same bits);
//   * tt_q := 0 and rq_q = 1 / den_q := 0 (hence Aq_q = 0, dtt_q = 0): with dn = 0 the tangent formulas below then give rz' = R + dlogT and
//     dm' = dmb by themselves (fma(0, finite, x) = x: l2, dl are the model's ONE variance and the direction's constant, finite by validation);
//   * the three results that the limit 0 * infinity hides are selected outright: z'_q (and its exponent increment n_q), u'_q, du'_q.
// D + 8 double selects (and two integer ones) per step and 2 per direction, against 2 (2 + D) per step and as many per direction on the results.
template <int F, int D, int K, int NP, int H, bool ZF, bool LAZY, int VAR, bool FIRST = false, bool GAPS = false, class Ctx>
XT_HD void xt_r2_step(Ctx& cx, char* lds, XtR2Lane<D, K, NP>& s, int tab, const double* c, const double* l2, bool gap = false)
{
    static_assert(!FIRST || (NP == 0 && ZF && LAZY), "the merge-free first step is a step of the zero-free likelihood-only loop");
    static_assert(!GAPS || (NP > 0 && K == 1 && !FIRST), "the gap-aware non-g-form step is the gradient step with one scalar localisation error");
    constexpr int NGB = F - 1;
    constexpr int XB = xt_r2_gbit(F, H), PB = xt_r2_gbit(F, (H + NGB - 1) % NGB);
    const int lane = xt_opaque(cx.lane());  // keeps the per-phase constants (prev, qa, table offsets) out of the loop-invariant registers
    const int prev = (lane >> PB) & 1;
    const int qa = Ctx::template pair_natural<XB>() ? 0 : (lane >> XB) & 1;
    const int io[2] = {(prev * 2 + qa) * 8, (prev * 2 + (qa ^ 1)) * 8};  // [prev][q] byte offsets of the two outputs
    double TT[2], TD2[2];
    XT_UNROLL
    for (int q = 0; q < 2; ++q) {
        TT[q] = xt_at<double>(lds, tab + io[q]);
        TD2[q] = xt_at<double>(lds, XT_R2_TAB0 + 4 * 32 + io[q]);
    }

    // ---- primal: merge, expand, integrate (xt_f2_step with the members in registers)
    const int e0 = s.e[0], e1 = s.e[1];
    const int emax = e0 > e1 ? e0 : e1;
    const double w0 = FIRST ? 1.0 : xt_ldexp(s.z[0], e0 - emax), w1 = FIRST ? 0.0 : xt_ldexp(s.z[1], e1 - emax);
    const double W = FIRST ? 1.0 : w0 + w1;
    double M[D], U[K];
    XT_UNROLL
    for (int d = 0; d < D; ++d) M[d] = FIRST ? s.m[0][d] : xt_fma(w1, s.m[1][d], w0 * s.m[0][d]);
    XT_UNROLL
    for (int k = 0; k < K; ++k) U[k] = FIRST ? s.u[0][k] : xt_fma(w1, s.u[1][k], w0 * s.u[0][k]);
    const bool live = ZF ? true : W > 0.0;
    const double Ws = ZF ? W : (live ? W : 1.0);
    constexpr bool RN = !LAZY || (H % XT_F2_RENORM) == 0;
    const double Wm = FIRST ? s.z[0] : (RN ? xt_frexp_mant(W) : W);
    const int We = FIRST ? e0 : (live ? (RN ? emax + xt_frexp_exp(W) : emax) : XT_EMIN);

    double Dq[2][K];
    XT_UNROLL
    for (int q = 0; q < 2; ++q)
        XT_UNROLL
        for (int k = 0; k < K; ++k) Dq[q][k] = xt_fma(Ws, l2[k] + TD2[q], U[k]);
    double rD[2][K], rW;
    if (K == 1) {
        const double d01 = Dq[0][0] * Dq[1][0];
        const double R = xt_rcp(Ws * d01);
        const double RW = R * Ws;
        rW = FIRST ? 1.0 : R * d01;
        rD[0][0] = RW * Dq[1][0];
        rD[1][0] = RW * Dq[0][0];
    } else {
        double f[2 * K + 1], pre[2 * K + 2], suf[2 * K + 2];
        f[0] = Ws;
        XT_UNROLL
        for (int q = 0; q < 2; ++q)
            XT_UNROLL
            for (int k = 0; k < K; ++k) f[1 + q * K + k] = Dq[q][k];
        pre[0] = 1.0;
        XT_UNROLL
        for (int i = 0; i < 2 * K + 1; ++i) pre[i + 1] = pre[i] * f[i];
        suf[2 * K + 1] = 1.0;
        XT_UNROLL
        for (int i = 2 * K; i >= 0; --i) suf[i] = suf[i + 1] * f[i];
        const double R = xt_rcp(pre[2 * K + 1]);
        rW = FIRST ? 1.0 : R * suf[1];
        XT_UNROLL
        for (int q = 0; q < 2; ++q)
            XT_UNROLL
            for (int k = 0; k < K; ++k) rD[q][k] = R * pre[1 + q * K + k] * suf[2 + q * K + k];
    }
    double dmW[D], dsqW = 0.0;
    XT_UNROLL
    for (int d = 0; d < D; ++d) {
        dmW[d] = xt_fma(c[d], Ws, -M[d]);
        if constexpr (GAPS) dmW[d] = gap ? 0.0 : dmW[d];
        if (K == 1) dsqW = xt_fma(dmW[d], dmW[d], dsqW);
    }
    double x[2], gf[2], tt[2][K];
    const double A = -0.5 * rW * dsqW;
    XT_UNROLL
    for (int q = 0; q < 2; ++q) {
        if (K == 1) {
            x[q] = A * rD[q][0];
            tt[q][0] = xt_fma(Ws, TD2[q], U[0]) * rD[q][0];
            if constexpr (GAPS) tt[q][0] = gap ? 0.0 : tt[q][0];
            gf[q] = xt_pow_half<D>(Ws * rD[q][0]);
        } else {
            double xx = 0.0, gg = 1.0;
            XT_UNROLL
            for (int d = 0; d < D; ++d) {
                xx = xt_fma(dmW[d] * dmW[d], rD[q][d], xx);
                tt[q][d] = xt_fma(Ws, TD2[q], U[d]) * rD[q][d];
                gg *= Ws * rD[q][d];
            }
            x[q] = xx * (-0.5 * rW);
            gf[q] = sqrt(gg);
        }
    }
    double p[2];
    int j[2], n[2];
    xt_exp_tab_x2(x[0], x[1], p[0], p[1], j[0], j[1], n[0], n[1]);
    double nz[2], nm[2][D], nu[2][K];
    int ne[2];
    XT_UNROLL
    for (int q = 0; q < 2; ++q) {
        int en = We + n[q];
        const double tj = xt_at<double>(lds, XT_F2_EXPB_OFF + j[q] * 8);
        double zn = (Wm * TT[q]) * (gf[q] * tj) * p[q];
        if constexpr (GAPS) {
            zn = gap ? Wm * TT[q] : zn;
            en = gap ? We : en;
        }
        if (!LAZY) {
            en += xt_frexp_exp(zn);
            zn = xt_frexp_mant(zn);
        }
        nz[q] = zn;
        ne[q] = en > XT_EMIN ? en : XT_EMIN;
        XT_UNROLL
        for (int d = 0; d < D; ++d) nm[q][d] = xt_fma(dmW[d], tt[q][K == 1 ? 0 : d], M[d]) * rW;
        XT_UNROLL
        for (int k = 0; k < K; ++k) nu[q][k] = l2[k] * tt[q][k];
        if constexpr (GAPS) nu[q][0] = gap ? xt_fma(U[0], rW, TD2[q]) : nu[q][0];
    }

    // ---- tangents (formulas: header of xt_grad.h), all on normalised quantities; first the primal factors they share (kept few:
    // with 7-8 directions x 16 VGPRs of tangent state the step must fit the rest into ~100 registers)
    double a0 = 0.0, a1 = 0.0, cm[D], cu[K], dn[D], Aq[2][K], rq[2][K];
    if (NP > 0) {
        a0 = w0 * rW;  // a0 = a1 = 0 for an all-zero group (rW = 1 then)
        a1 = w1 * rW;
        const double aa = a0 * a1;
        XT_UNROLL
        for (int d = 0; d < D; ++d) {
            cm[d] = aa * (s.m[0][d] - s.m[1][d]);
            dn[d] = dmW[d] * rW;  // c - m_bar
        }
        XT_UNROLL
        for (int k = 0; k < K; ++k) cu[k] = aa * (s.u[0][k] - s.u[1][k]);
        XT_UNROLL
        for (int q = 0; q < 2; ++q)
            XT_UNROLL
            for (int k = 0; k < K; ++k) {
                rq[q][k] = Ws * rD[q][k];  // 1 / den
                if constexpr (GAPS) rq[q][k] = gap ? 0.0 : rq[q][k];
                if (K == 1)
                    Aq[q][0] = -0.5 * rq[q][0] * xt_fma(-(dsqW * rW * rW), rq[q][0], (double)D);
                else
                    Aq[q][k] = -0.5 * rq[q][k] * xt_fma(-(dn[k] * dn[k]), rq[q][k], 1.0);
            }
    }
    // ---- the lane exchange: the oldest remaining digit comes into the registers, the new digit goes to lane bit XB (primal state
    // first: that frees the registers of the new state before the tangent passes)
    cx.template pair_exchange<XB>(nz[0], nz[1]);
    cx.template pair_exchange_i32<XB>(ne[0], ne[1]);
    XT_UNROLL
    for (int d = 0; d < D; ++d) cx.template pair_exchange<XB>(nm[0][d], nm[1][d]);
    XT_UNROLL
    for (int k = 0; k < K; ++k) cx.template pair_exchange<XB>(nu[0][k], nu[1][k]);
    XT_UNROLL
    for (int q = 0; q < 2; ++q) {
        s.z[q] = nz[q];
        s.e[q] = ne[q];
        XT_UNROLL
        for (int d = 0; d < D; ++d) s.m[q][d] = nm[q][d];
        XT_UNROLL
        for (int k = 0; k < K; ++k) s.u[q][k] = nu[q][k];
    }
    if (NP > 0) {
        XT_UNROLL
        for (int pp = 0; pp < NP; ++pp) {
            if (!(VAR & 1)) xt_sched_fence();  // one direction at a time: interleaved directions multiply the live temporaries
            const int tb = XT_R2_TAN0 + pp * XT_R2_TB * 8;
            double dl[K];
            XT_UNROLL
            for (int k = 0; k < K; ++k) dl[k] = xt_at<double>(lds, tb + k * 8);
            const double del = s.rz[pp][0] - s.rz[pp][1];
            // R, d m_bar, d u_bar = sum a_j (.)_j as the convex combinations they are.  The shorter x_1 + a0 (x_0 - x_1) rounds at ulp(x_1):
            // a member of negligible weight that carries a huge d log z (d log T = 1 / T along a tiny transition probability; its dm, du
            // inherit rounding of that size) then wipes out the dominant member's tangent
            const double R = xt_fma(a0, s.rz[pp][0], a1 * s.rz[pp][1]);
            double dmb[D], dub[K];
            XT_UNROLL
            for (int d = 0; d < D; ++d) dmb[d] = xt_fma(cm[d], del, xt_fma(a0, s.dm[pp][0][d], a1 * s.dm[pp][1][d]));
            XT_UNROLL
            for (int k = 0; k < K; ++k) dub[k] = xt_fma(cu[k], del, xt_fma(a0, s.du[pp][0][k], a1 * s.du[pp][1][k]));
            double hd[K];  // -1/2 d |c - m_bar|^2 = sum_d (c - m_bar)_d d m_bar_d (per dim when K == D)
            if (K == 1) {
                hd[0] = 0.0;
                XT_UNROLL
                for (int d = 0; d < D; ++d) hd[0] = xt_fma(dn[d], dmb[d], hd[0]);
            } else {
                XT_UNROLL
                for (int d = 0; d < D; ++d) hd[d] = dn[d] * dmb[d];
            }
            double trz[2], tdm[2][D], tdu[2][K];
            XT_UNROLL
            for (int q = 0; q < 2; ++q) {
                const double dlT = xt_at<double>(lds, tb + tab + io[q]);
                const double dd2 = xt_at<double>(lds, tb + XT_R2_TAB0 + 4 * 32 + io[q]);
                double rzn = R + dlT, dtt[K];
                XT_UNROLL
                for (int k = 0; k < K; ++k) {
                    const double ds2 = dd2 + dub[k], dden = dl[k] + ds2;
                    dtt[k] = rq[q][k] * xt_fma(-tt[q][k], dden, ds2);
                    rzn = xt_fma(Aq[q][k], dden, rzn);
                    rzn = xt_fma(rq[q][k], hd[k], rzn);  // - r/2 * d|c - m_bar|^2
                    tdu[q][k] = xt_fma(l2[k], dtt[k], dl[k] * tt[q][k]);
                    if constexpr (GAPS) tdu[q][k] = gap ? ds2 : tdu[q][k];
                }
                trz[q] = ZF ? rzn : (live ? rzn : 0.0);
                XT_UNROLL
                for (int d = 0; d < D; ++d) {
                    const int kk = K == 1 ? 0 : d;
                    tdm[q][d] = xt_fma(dn[d], dtt[kk], xt_fma(-tt[q][kk], dmb[d], dmb[d]));  // d m_bar (1 - tt) + (c - m_bar) d tt
                }
            }
            cx.template pair_exchange<XB>(trz[0], trz[1]);
            XT_UNROLL
            for (int d = 0; d < D; ++d) cx.template pair_exchange<XB>(tdm[0][d], tdm[1][d]);
            XT_UNROLL
            for (int k = 0; k < K; ++k) cx.template pair_exchange<XB>(tdu[0][k], tdu[1][k]);
            XT_UNROLL
            for (int q = 0; q < 2; ++q) {
                s.rz[pp][q] = trz[q];
                XT_UNROLL
                for (int d = 0; d < D; ++d) s.dm[pp][q][d] = tdm[q][d];
                XT_UNROLL
                for (int k = 0; k < K; ++k) s.du[pp][q][k] = tdu[q][k];
            }
        }
    }
}

// The same step in "g-form" with LOG-CARRIED weights: scalar variance (K == 1), ONE global localisation variance l2 > 0, likelihood only,
// zero-free and lazily re-normalised (xt_r2_step<.., ZF = true, LAZY = true> is what it replaces; FIRST as there).  Every per-child quantity
// is a function of the one ratio g_q = l2 / den_q in (0, 1]:
//     tt_q = 1 - g_q           =>  m_q = c - (c - m_bar) g_q                       (one fma per dimension)
//     u_q = l2 (1 - g_q)       =>  the members carry v = l2 + u:  v_q = 2 l2 - l2 g_q,  W den_q = Ws d2_q + V  (no l2 + d2 add)
//     den_q^(-D/2) = (g_q / l2)^(D/2),  -|c - m_bar|^2 / (2 den_q) = A g_q  with  A = -|c - m_bar|^2 / (2 l2)
//     weight_q = Wm g_q^(D/2) exp(A g_q + lnT'[prev][q]),  lnT' = ln T - D/2 ln l2   (table built per workgroup: no T multiply, no gf)
// RATIO FORM: none of 1 / W, g_q or c - m_bar is formed.  With Dq_q = Ws d2_q + V = W den_q, the shared reciprocal R = 1 / (Ws Dq0 Dq1)
// (xt_rcp3) gives h_q = R Dq[1 - q] = 1 / (Ws Dq_q) directly, and everything is written on the un-normalised e_d = Ws (c - m_bar)_d:
//     -2 A g_q = (sum_d e_d^2) h_q                                (|c - m_bar|^2 / den_q = (sum e_d^2 / Ws^2) (Ws / Dq_q); no -1 / (2 l2) constant)
//     k_q = (l2 Ws) h_q = l2 / Dq_q = g_q / Ws   =>   m_q = c - e_d k_q,   v_q = 2 l2 - (l2 Ws) k_q
//     y_q = Wm (Ws k_q)^(D/2);  D = 2:  y_q = (Wm Ws) k_q         (FIRST: Ws = 1, so h_q = R Dq[1 - q], k_q = l2 h_q, e_d = (c - m)_d)
// RESIDUAL FORM: the recursion is translation invariant - it only ever uses a position minus a member's mean.  The members of a g-form launch
// carry r = c_next - m (in s.m) instead of m, and the staged array holds the position deltas dc_t = c_{t+1} - c_t (xt_r2_body: stage).  The merge
// E_d = w0 r0_d + w1 r1_d IS e_d (no c_d Ws - M_d), the children are r_q[d] = dc_d + E_d k_q (m_q = c - e k_q, minus it from c_next), the
// merge-free first step and the read-out take r for c - m, and the warm-up (xt_r2_chain_g) never forms c - m.  No absolute coordinate is
// read on these paths; a delta is rounded once at ulp(|c|), as c - m was.
// A member's weight is y exp(-lambda / 2) (s.z = y, a lazily normalised double; lambda, a double next to the lane state; s.e is not used): the
// child's exponential is never taken, and the log part is carried in DOUBLED, NEGATED units so that -1/2 sum e_d^2 needs no multiply:
//     lambda_q = (sum_d e_d^2) h_q + LT2[prev][q] + base,   LT2 = -2 lnT'   (the table is built in these units),   y_q = Wm g_q^(D/2).
// The merge of the NEXT step needs only the ratio of its two members, ONE exponential E = exp(-|lambda1 - lambda0| / 2) (xt_exp_tab_half_x1:
// the 1/2 is in its constants; clamp at |d lambda| = 2.2e7, E = 0 beyond, where the magic-number reduction would leave its range - the same
// integer n as xt_exp_tab_x1 at 1.1e7) that scales the member with the LARGER lambda; the other keeps scale 1 and base = min(lambda0, lambda1)
// is exact.  The absolute magnitude is only needed at the read-out of the last position (x = -1/2 (|r|^2 / den + lambda): one fma).
// Lazy re-normalisation (every XT_F2_RENORM-th phase): Wm = frexp_mant(Ws), base -= 2 ln2 frexp_exp(Ws).  Range of the lazy mantissa:
// y = Wm g^(D/2) with g = l2 / den in [1e-16, 1] (well-scaled bounds: l2 >= 1e-12, den <= 1e4) and a merge at most doubles the sum
// (E <= 1): three un-normalised steps stay within [1e-72, 8]; the products of a step are then Ws Dq0 Dq1 = W^3 den^2 >= 1e-240 (<= 8^3 * 1e8),
// h_q = 1 / (W^2 den_q) <= 1 / (W_min den_min W_min) = 1e144 * 1e12, k_q = l2 h_q Ws <= 1 / W_min = 1e72 (g_q <= 1), e_d^2 <= 64 |c - m_bar|^2,
// sum e_d^2 h_q = |c - m_bar|^2 / den_q is the same number as before, and Wm Ws <= 64, >= 1e-144 (Wm = Ws between re-normalisations) - all
// far inside the fp64 range; the transition weight and l2^(-D/2) live in lambda.
// Re-centring (phase XT_R2_RC_H, once per F - 1 steps): lambda is rounded at ulp(|lambda|), so it must not grow with the accumulated
// log-likelihood.  The lanes of a track take the MINIMUM of their truncated bases (an integer atomic max of the negated integers on the
// track's LDS cell; LDS and cx.wave_sync() only): sh, an integer common to the track, in lambda units.  base -= sh (exact, or one rounding at
// the ulp of the small difference) and the lane's LDS accumulator += sh (integers: exact); the read-out adds -1/2 x the accumulator to the
// track's log-likelihood.  The reference has to be the SMALLEST base (the largest log-weight), not that of a fixed lane: a fixed lane's
// sequence may be hopeless (a still state on a moving track is at -600 per step), and shifting by its base leaves |lambda| in the thousands on
// the lanes that matter (measured in log units: 1e-12 on 33-position tracks at l2 = 1e-10).  In a re-normalisation phase y is in [0.5, 1), so the
// smallest base is -2 x the dominant group's log-weight to within 2 ln 2, and the lanes that matter end within a few units of 0; lanes far
// above are negligible at the read-out.  No execution mask and no branch: the step stays one basic block.  Between two re-centrings |lambda|
// grows by at most F - 1 steps' worth of 2 x log-weight (a few units per step on ordinary data; at small l2 the lazy mantissa takes
// D/2 ln(den / l2) per step out of the log-weight until the next re-normalisation: |lambda| < 300 at l2 = 1e-12, D = 3, ulp 5.7e-14, i.e. 2.8e-14
// in the log-likelihood, as before the doubling: lambda / 2 has the rounding error of lambda halved).
#ifndef XT_R2_RC_H
#define XT_R2_RC_H 0  // re-centring phase: a re-normalisation phase
#endif
#define XT_R2_RC_NONE (-2147483647 - 1)
// Which likelihood-only instances stage complete batches through stage_ld / stage_st (xt_r2_body).  D = 3 keeps the loop alone: with the second
// path its kernels spill ten more scalar registers and with them one more vector register (xt_ll_r2_kernel<6,3,1>: 28 -> 32 bytes of scratch).
#ifndef XT_R2_STAGE_FAST
#define XT_R2_STAGE_FAST(D) ((D) < 3)
#endif
// lambda of a member that carries no sequence (y = 0: the dead member of a lane before the first full step, lanes whose digits are still dummies
// at the end of a short bucket's chain): a quiet NaN (a constant the kernel already holds).  fmin passes it over, so it stays out of the
// read-out's minimum; the exponential's clamp (x > c ? x : c) turns the NaN argument into c, and 0 x exp(c / 2) is the member's zero term.
#define XT_R2_LAM_DEAD NAN
// What the staging of a gap-aware gradient launch leaves in LDS for an element it read as v: v itself (a missed row stays NaN).  tests/emul defines
// it to put a finite number in place of a NaN, to show that no step uses the coordinates of a missed row.
#ifndef XT_R2_GAP_STAGED
#define XT_R2_GAP_STAGED(v) (v)
#endif
#ifndef XT_R2_STAGE_GRP
#define XT_R2_STAGE_GRP 4  // rounds of the wave whose loads are in flight together when a chunk is staged (xt_r2_body: stage)
#endif
// The [prev][q] table byte offset of a lane's first output, (prev * 2 + qa) * 8 (xt_r2_step), is a per-lane constant of the phase: all F - 1 of
// them packed into one word, 5 bits per phase, built once per kernel.  The step extracts its field (the second output's offset is that ^ 8)
// instead of deriving both from the lane id with shifts, ands and bit insertions in every step.
#define XT_R2_IO_BITS 5
template <int F, int H, class Ctx>
XT_HD int xt_r2_pack_io(int lane)
{
    constexpr int NGB = F - 1;
    if constexpr (H >= NGB) {
        return 0;
    } else {
        constexpr int XB = xt_r2_gbit(F, H), PB = xt_r2_gbit(F, (H + NGB - 1) % NGB);
        const int prev = (lane >> PB) & 1;
        const int qa = Ctx::template pair_natural<XB>() ? 0 : (lane >> XB) & 1;
        return ((prev * 2 + qa) * 8) << (XT_R2_IO_BITS * H) | xt_r2_pack_io<F, H + 1, Ctx>(lane);
    }
}
// In-place barrier on the packed word: the compiler cannot hoist the 2 (F - 1) extracted offsets out of the step loop into registers of their
// own (as xt_opaque does for the lane id), and no copy of the word is made.
XT_HD void xt_r2_opaque_inplace(int& pk)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(pk));
#else
    (void)pk;
#endif
}
// 8 * tid, the byte offset of the thread's re-centring cells, formed where it is used: the shift is the barrier itself (no copy of the thread id as
// xt_opaque makes, and nothing for the compiler to keep in a register across the step loop).
template <class Ctx>
XT_HD int xt_r2_tid8(Ctx& cx)
{
#if defined(__HIP_DEVICE_COMPILE__)
    int o;
    asm volatile("v_lshlrev_b32 %0, 3, %1" : "=v"(o) : "v"(cx.tid()));
    return o;
#else
    return cx.tid() * 8;
#endif
}
// GAPS (missed detections): `gap` = position t of this lane's track is a missed frame.  The l2 -> infinity limit of the step
// above: g_q -> 0 in the update of the mean (m_q = m_bar, so r_q = r_bar + dc: k_q = 1 / Ws), l2 s2 / (l2 + s2) -> s2 (v_q = v_bar + d2_q =
// Dq_q / Ws), no Gaussian factor (y_q = Wm, no esq h_q in lambda).  1 / Ws = R Dq0 Dq1 comes out of the shared reciprocal.  lambda keeps the
// table's -2 lnT' = -2 lnT + D ln l2: every sequence of a track passes the same gaps, so the D/2 ln l2 per gap is a per-track constant that the
// read-out gives back together with the gap's share of log 2 pi (xt_r2_body).  Per-lane selects on top of the observed step: no branch.
template <int F, int D, int H, bool FIRST = false, bool GAPS = false, class Ctx>
XT_HD void xt_r2_step_g(Ctx& cx, char* lds, XtR2Lane<D, 1, 0>& s, double (&lam)[2], int& pk, int tab, const double* dc, bool gap = false)
{
    constexpr int NGB = F - 1;
    constexpr int XB = xt_r2_gbit(F, H);
    xt_r2_opaque_inplace(pk);
    int io0 = (int)(((unsigned int)pk >> (XT_R2_IO_BITS * H)) & ((1u << XT_R2_IO_BITS) - 1u));
    xt_r2_opaque_inplace(io0);  // the second offset from the extracted field (one xor), not from the word again (a shift and a three-input bit operation)
    const int io[2] = {io0, io0 ^ 8};
    double TD2[2], LT[2];
    XT_UNROLL
    for (int q = 0; q < 2; ++q) {
        TD2[q] = xt_at<double>(lds, XT_R2_TAB0 + 4 * 32 + io[q]);
        LT[q] = xt_at<double>(lds, tab + XT_R2_LNT_REL + io[q]);  // -2 lnT'
    }
    const double l2 = xt_at<double>(lds, 0), l22 = xt_at<double>(lds, XT_R2_GC_OFF + 8);

    // ---- merge (members carry v = l2 + u and r = c - m): the member with the larger lambda is scaled by exp(-|lambda1 - lambda0| / 2)
    double w0 = 1.0, w1 = 0.0, base = lam[0];
    if (!FIRST) {
        const double dl = lam[1] - lam[0];
        double p;
        int j, n;
        xt_exp_tab_half_x1(-fabs(dl), p, j, n);
        const double E = xt_ldexp(xt_at<double>(lds, XT_F2_EXPB_OFF + j * 8) * p, n);  // n <= 0
        const bool up = dl < 0.0;
        w0 = s.z[0] * (up ? E : 1.0);
        w1 = s.z[1] * (up ? 1.0 : E);
        base = up ? lam[1] : lam[0];
    }
    const double Ws = FIRST ? 1.0 : w0 + w1;
    double ed[D], esq = 0.0;  // Ws (c - m_bar)
    XT_UNROLL
    for (int d = 0; d < D; ++d) {
        ed[d] = FIRST ? s.m[0][d] : xt_fma(w1, s.m[1][d], w0 * s.m[0][d]);
        esq = xt_fma(ed[d], ed[d], esq);
    }
    const double V = FIRST ? s.u[0][0] : xt_fma(w1, s.u[1][0], w0 * s.u[0][0]);
    constexpr bool RN = !FIRST && (H % XT_F2_RENORM) == 0;
    const double Wm = FIRST ? s.z[0] : (RN ? xt_frexp_mant(Ws) : Ws);
    if (RN) base = xt_fma((double)xt_frexp_exp(Ws), -2.0 * XT_LN2, base);
    if (!FIRST && H == XT_R2_RC_H) {
        // re-centring: the integer shift is the smallest (truncated) base among the track's lanes - an atomic max of the negated integers on the
        // track's LDS cell, which every lane of the track reset one phase later in the previous pass (or at position 0)
        const int tid8 = xt_r2_tid8(cx);
        const int rc0 = xt_r2_rc0(D, 0, XtR2Geom<F>::TPW);  // g-form launches stage no per-peak errors (KS = 0)
        const int cell = rc0 + (tid8 & ~(xt_r2_gmask(F) * 8));
        cx.atomic_max_i32(&xt_at<int>(lds, cell), (int)fmin(fmax(-base, -1e9), 1e9));  // a NaN base (poisoned track) counts as lambda = +1e9
        cx.wave_sync();
        const int nsh = xt_at<int>(lds, cell);  // - min over the lanes
        base += (double)nsh;
        xt_at<unsigned int>(lds, rc0 + XT_R2_RC_ARR + tid8) -= (unsigned int)nsh;  // read back as int; wraps only on a poisoned track (1e9 per pass)
    }
    if (!FIRST && H == (XT_R2_RC_H + 1) % NGB) xt_at<int>(lds, xt_r2_rc0(D, 0, XtR2Geom<F>::TPW) + (xt_r2_tid8(cx) & ~(xt_r2_gmask(F) * 8))) = XT_R2_RC_NONE;

    // ---- the shared reciprocal, h_q and k_q
    const double Dq0 = xt_fma(Ws, TD2[0], V), Dq1 = xt_fma(Ws, TD2[1], V);
    const double R = xt_rcp3(Ws * (Dq0 * Dq1));
    const double h[2] = {R * Dq1, R * Dq0};
    const double l2W = FIRST ? l2 : l2 * Ws;
    const double WmW = FIRST ? Wm : Wm * Ws;
    double ny[2], nl[2], nr[2][D], nv[2];
    if constexpr (GAPS) {
        const double Dq[2] = {Dq0, Dq1};
        const double rW = FIRST ? 1.0 : R * (Dq0 * Dq1);  // 1 / Ws
        const double esqg = gap ? 0.0 : esq;
        XT_UNROLL
        for (int q = 0; q < 2; ++q) {
            const double ko = l2W * h[q];
            const double k = gap ? rW : ko;
            const double yo = D == 2 ? WmW * ko : Wm * xt_pow_half<D>(FIRST ? ko : Ws * ko);
            ny[q] = gap ? Wm : yo;
            nl[q] = xt_fma(esqg, h[q], LT[q]) + base;
            XT_UNROLL
            for (int d = 0; d < D; ++d) nr[q][d] = xt_fma(ed[d], k, dc[d]);
            const double vo = xt_fma(-l2W, ko, l22);
            nv[q] = gap ? Dq[q] * rW : vo;
        }
    } else {
        XT_UNROLL
        for (int q = 0; q < 2; ++q) {
            const double k = l2W * h[q];
            ny[q] = D == 2 ? WmW * k : Wm * xt_pow_half<D>(FIRST ? k : Ws * k);
            nl[q] = xt_fma(esq, h[q], LT[q]) + base;
            XT_UNROLL
            for (int d = 0; d < D; ++d) nr[q][d] = xt_fma(ed[d], k, dc[d]);
            nv[q] = xt_fma(-l2W, k, l22);
        }
    }
    cx.template pair_exchange<XB>(ny[0], ny[1]);
    cx.template pair_exchange<XB>(nl[0], nl[1]);
    XT_UNROLL
    for (int d = 0; d < D; ++d) cx.template pair_exchange<XB>(nr[0][d], nr[1][d]);
    cx.template pair_exchange<XB>(nv[0], nv[1]);
    XT_UNROLL
    for (int q = 0; q < 2; ++q) {
        s.z[q] = ny[q];
        lam[q] = nl[q];
        XT_UNROLL
        for (int d = 0; d < D; ++d) s.m[q][d] = nr[q][d];
        s.u[q][0] = nv[q];
    }
}

// Warm-up of a g-form launch: the chain of xt_r2_chain in the quantities the g-form step carries - (y, lambda, r = c_next - m, v = l2 + u) -
// with NO exponential, no frexp per position and no integer exponent.  One position of the lane's own state path, g = l2 / den, den = d2 + v:
//     y *= g^(D/2),   lambda += |r|^2 / den - 2 lnT'[prev][q],   v = 2 l2 - l2 g,   r_d = dc_d + r_d g      (dc: the staged position deltas)
// on the tables the steady step reads (the stay factor sets in at stay_from).  Range: g in [1e-16, 1] (well-scaled bounds), at most F - 2 = 5
// positions: y >= 1e-120 times the initial fraction.  The first full step and the merges after it form W^3-sized products, so the chain hands
// over a normalised mantissa: ONE frexp at its end, its exponent folded into lambda.  Lanes whose digits are still dummies (a bucket too
// short to fill the window) end at y = 0 with finite lambda, r, v; such a bucket goes from here straight to the read-out.
// GAPS: bit t of gm = position t of this lane's track is a missed frame - g = 1 in the mean, v = v + d2, no factor (xt_r2_step_g), per-lane selects.
template <int F, int D, bool GAPS = false, class Ctx, class GetPos>
XT_HD void xt_r2_chain_g(Ctx& cx, char* lds, XtR2Lane<D, 1, 0>& s, double (&lam)[2], int T, int stay_from, GetPos& getpos, unsigned int gm = 0u)
{
    constexpr int NGB = F - 1;
    const int lane = xt_opaque(cx.lane());
    const double l2 = xt_at<double>(lds, 0), l22 = xt_at<double>(lds, XT_R2_GC_OFF + 8);
    double y = s.z[0], la = lam[0], v = s.u[0][0];
    XT_UNROLL
    for (int t = 1; t < NGB; ++t) {
        if (t > T) break;  // wave-uniform (per bucket)
        const int prev = (lane >> xt_r2_gbit(F, t == 1 ? NGB - 1 : t - 2)) & 1;
        const int q = (lane >> xt_r2_gbit(F, t - 1)) & 1;
        const int io = (prev * 2 + q) * 8;  // [prev][q] byte offset
        const double LT = xt_at<double>(lds, XT_R2_LNT_OFF + (t >= stay_from ? 32 : 0) + io);
        const double d2 = xt_at<double>(lds, XT_R2_TAB0 + 4 * 32 + io);
        double dc[D], l2u[1];
        getpos(t, dc, l2u);
        const double rd = xt_rcp3(d2 + v);
        const double g = l2 * rd;
        double rsq = 0.0;
        XT_UNROLL
        for (int d = 0; d < D; ++d) rsq = xt_fma(s.m[0][d], s.m[0][d], rsq);
        if constexpr (GAPS) {
            const bool gap = (gm >> t) & 1u;
            y *= gap ? 1.0 : xt_pow_half<D>(g);
            la = xt_fma(gap ? 0.0 : rsq, rd, la + LT);
            v = gap ? d2 + v : xt_fma(-l2, g, l22);
            XT_UNROLL
            for (int d = 0; d < D; ++d) s.m[0][d] = xt_fma(s.m[0][d], gap ? 1.0 : g, dc[d]);
        } else {
            y *= xt_pow_half<D>(g);
            la = xt_fma(rsq, rd, la + LT);
            v = xt_fma(-l2, g, l22);
            XT_UNROLL
            for (int d = 0; d < D; ++d) s.m[0][d] = xt_fma(s.m[0][d], g, dc[d]);
        }
    }
    int dummy = 0;  // lane bits of digits that are still dummies (time < 0)
    XT_UNROLL
    for (int i = 0; i < NGB - 1; ++i)
        if (i >= T) dummy |= 1 << xt_r2_gbit(F, i);
    const bool live = (lane & dummy) == 0;
    s.z[0] = live ? xt_frexp_mant(y) : 0.0;
    const double lae = xt_fma((double)xt_frexp_exp(y), -2.0 * XT_LN2, la);
    lam[0] = live ? lae : XT_R2_LAM_DEAD;  // only a bucket that goes from here straight to the read-out has such lanes
    s.u[0][0] = v;
}

// all-reduce over the lanes of a track (the F - 1 group bits)
template <int F, class Ctx>
XT_HD double xt_r2_gsum(Ctx& cx, double v)
{
    constexpr int NGB = F - 1;
    v += cx.template xor_f64<xt_r2_gbit(F, 0)>(v);
    v += cx.template xor_f64<xt_r2_gbit(F, 1)>(v);
    v += cx.template xor_f64<xt_r2_gbit(F, 2)>(v);
    if (NGB > 3) v += cx.template xor_f64<xt_r2_gbit(F, NGB > 3 ? 3 : 0)>(v);
    if (NGB > 4) v += cx.template xor_f64<xt_r2_gbit(F, NGB > 4 ? 4 : 0)>(v);
    if (NGB > 5) v += cx.template xor_f64<xt_r2_gbit(F, NGB > 5 ? 5 : 0)>(v);
    return v;
}
template <int F, class Ctx>
XT_HD int xt_r2_gmax(Ctx& cx, int v)
{
    constexpr int NGB = F - 1;
    auto mx = [](int a, int b) XT_INL { return a > b ? a : b; };
    v = mx(v, cx.template xor_i32<xt_r2_gbit(F, 0)>(v));
    v = mx(v, cx.template xor_i32<xt_r2_gbit(F, 1)>(v));
    v = mx(v, cx.template xor_i32<xt_r2_gbit(F, 2)>(v));
    if (NGB > 3) v = mx(v, cx.template xor_i32<xt_r2_gbit(F, NGB > 3 ? 3 : 0)>(v));
    if (NGB > 4) v = mx(v, cx.template xor_i32<xt_r2_gbit(F, NGB > 4 ? 4 : 0)>(v));
    if (NGB > 5) v = mx(v, cx.template xor_i32<xt_r2_gbit(F, NGB > 5 ? 5 : 0)>(v));
    return v;
}

// Warm-up of the likelihood-only recursion of a well-scaled launch: positions 1 .. T (T = min(L - 2, F - 2)), before the window is full.
// No fusion happens there, so member 0 of a lane is ONE Kalman chain over positions 0 .. T along the state path of the lane's own group
// bits (time 0 in GB[F-2], time t in GB[t-1]) and member 1 (a dummy oldest digit) stays dead.  Every lane computes on its own - one child
// per position, no merge, no exchange, no zero-weight handling - what the merge / expand / exchange steps would leave in its registers;
// shared prefixes are recomputed by the lanes that share them (in the stepped form those lanes idle).  Hands over a normalised mantissa
// (the first full step, xt_r2_step<..., FIRST>, forms W^3-sized products).  A bucket too short to fill the window (T < F - 2) still has
// dummy digits in GB[T .. F-3] at the last position: lanes with one of them set end at zero weight, as the stepped form leaves them.
template <int F, int D, int K, int NP, class Ctx, class GetPos>
XT_HD void xt_r2_chain(Ctx& cx, char* lds, XtR2Lane<D, K, NP>& s, int T, int stay_from, GetPos& getpos)
{
    constexpr int NGB = F - 1;
    const int lane = xt_opaque(cx.lane());  // as in xt_r2_step: lane-derived constants stay out of the registers live across the step loop
    double z = s.z[0];
    int e = s.e[0];
    XT_UNROLL
    for (int t = 1; t < NGB; ++t) {
        if (t > T) break;  // wave-uniform (per bucket)
        const int prev = (lane >> xt_r2_gbit(F, t == 1 ? NGB - 1 : t - 2)) & 1;
        const int q = (lane >> xt_r2_gbit(F, t - 1)) & 1;
        const int io = (prev * 2 + q) * 8;  // [prev][q] byte offset
        const double TT = xt_at<double>(lds, XT_R2_TAB0 + (t >= stay_from ? 32 : 0) + io);
        const double d2 = xt_at<double>(lds, XT_R2_TAB0 + 4 * 32 + io);
        double c[D], l2[K];
        getpos(t, c, l2);
        double tt[K], r[K], dm[D], x = 0.0, gf;
        XT_UNROLL
        for (int k = 0; k < K; ++k) {
            const double a = d2 + s.u[0][k];
            r[k] = NP == 0 ? xt_rcp3(l2[k] + a) : xt_rcp(l2[k] + a);
            tt[k] = a * r[k];
        }
        XT_UNROLL
        for (int d = 0; d < D; ++d) dm[d] = c[d] - s.m[0][d];
        if (K == 1) {
            XT_UNROLL
            for (int d = 0; d < D; ++d) x = xt_fma(dm[d], dm[d], x);
            x *= -0.5 * r[0];
            gf = xt_pow_half<D>(r[0]);
        } else {
            double gg = 1.0;
            XT_UNROLL
            for (int d = 0; d < D; ++d) {
                x = xt_fma(-0.5 * dm[d] * dm[d], r[d], x);
                gg *= r[d];
            }
            gf = sqrt(gg);
        }
        double p;
        int j, n;
        xt_exp_tab_x1(x, p, j, n);
        z = (z * TT) * (gf * xt_at<double>(lds, XT_F2_EXPB_OFF + j * 8)) * p;
        e += n;
        XT_UNROLL
        for (int d = 0; d < D; ++d) s.m[0][d] = xt_fma(dm[d], tt[K == 1 ? 0 : d], s.m[0][d]);
        XT_UNROLL
        for (int k = 0; k < K; ++k) s.u[0][k] = l2[k] * tt[k];
    }
    int dummy = 0;  // lane bits of digits that are still dummies (time < 0)
    XT_UNROLL
    for (int i = 0; i < NGB - 1; ++i)
        if (i >= T) dummy |= 1 << xt_r2_gbit(F, i);
    const bool live = (lane & dummy) == 0;
    s.z[0] = live ? xt_frexp_mant(z) : 0.0;
    s.e[0] = live ? e + xt_frexp_exp(z) : XT_EMIN;
}

// NP == 0: log-likelihood only, per-block sums to a.partials (ga unused).  NP > 0: ga.gpartials[block][1 + NP] = {sum LL, sum dLL/dtheta_p}.
// GAPS: an all-NaN row is a missed frame, K == 1.  NP == 0: launches the host found fit for g-form steps (xt_ll_gap_reg2,
// xt_ll_geom.h; section 25), LDS of xt_r2_gap_block_bytes.  NP > 0: launches upgraded by xt_grad_gap_reg2 (xt_grad_geom.h; section 27), guarded
// or lazily normalised steps as a.well_scaled says, LDS of xt_r2_grad_gap_block_bytes.
template <int F, int D, int K, int NP, int VAR = 0, bool GAPS = false, class Ctx>
XT_HD void xt_r2_body(const XtKernelArgs& a, const XtGradArgs& ga, Ctx& cx)
{
    static_assert(!GAPS || K == 1, "the gap-aware instantiations have one scalar localisation error");
    constexpr bool GG = GAPS && NP == 0;  // the likelihood-only g-form gap path
    constexpr bool GN = GAPS && NP > 0;   // the gap-aware gradient path
    int lb, nb;
    const XtBucketDesc b = xt_bind_bucket(a, cx.block(), cx.nblocks(), lb, nb);
    typedef XtR2Geom<F> Gm;
    constexpr int NGB = Gm::NGB, TPW = Gm::TPW;
    constexpr int GMASK = xt_r2_gmask(F);
    const int lane = cx.lane();
    // likelihood only: the wave index as a scalar (batch, track and LDS base addresses then stay out of the vector registers: the kernel sits at
    // the 128-VGPR limit of four waves per SIMD)
    const int wib = NP == 0 ? cx.uniform(cx.wave_in_block()) : cx.wave_in_block();
    const int nwb = cx.waves_per_block();
    const int L = b.L;
    const int KS = a.locerr_mode ? a.KS : 0;
    double* smem = cx.smem();
    char* lds = (char*)smem;

    const int ntab = xt_tab_doubles(2, 2);
    for (int i = cx.tid(); i < ntab; i += cx.nthreads()) smem[i] = xt_blob_ptr(a)[i];
    if (NP > 0)
        for (int i = cx.tid(); i < NP * XT_R2_TB; i += cx.nthreads()) xt_at<double>(lds, XT_R2_TAN0 + i * 8) = ga.dblob[i];
    // "uniform" directions (ga.NU of them, tangent blocks after the NP full ones): d log of every weight factor of a step is the same for
    // all sequences (e.g. the bleaching probability pBL) - then rz stays equal over the sequences, dm = du = 0, and only the last
    // position's factor table tells the sequences apart: no per-step work at all (see the read-out below)
    const int NU = NP > 0 ? ga.NU : 0, NPT = NP + NU;
    for (int i = cx.tid(); i < NU * XT_R2_TB; i += cx.nthreads()) xt_at<double>(lds, XT_R2_TAN0 + (NP * XT_R2_TB + i) * 8) = ga.udblob[i];
    cx.sync();
    xt_f2_check_lds_base(lds);
    xt_f2_build_exp_table(cx, lds, XT_F2_EXPB_OFF, (const double*)(lds + XT_F2_T64_OFF));  // the 1024-entry table of xt_exp_tab_x2 from the blob's 64 entries
    // g-form steps (xt_r2_step_g): the launcher found one global localisation variance l2 >= 1e-12 in a well-scaled launch (well_scaled == 2)
    const bool gform = GG || (NP == 0 && K == 1 && a.well_scaled == 2 && a.locerr_mode == 0);
    if constexpr (NP == 0 && K == 1) {
        if (gform && cx.tid() < 10) {
            const int i = cx.tid();
            const double l2 = smem[0];
            if (i < 8)
                xt_at<double>(lds, XT_R2_LNT_OFF + i * 8) = -2.0 * (log(smem[XT_BLOB_HDR + i]) - 0.5 * D * log(l2));
            else
                xt_at<double>(lds, XT_R2_GC_OFF + (i - 8) * 8) = i == 8 ? (GAPS ? 0.5 * D * (XT_LOG2PI + log(l2)) : -0.5 / l2) : 2.0 * l2;  // GAPS: what the read-out gives back per missed row
        }
    }
    cx.sync();
    const double* hdr = smem;

    const int ts = xt_r2_slot<F>(lane);
    const bool leader = (lane & GMASK) == 0;
    const int tlast = L - 1;
    const int stay_from = a.min_len > 2 ? a.min_len : 2;
    const int vfin = (b.isBL ? 2 : 0) + (tlast >= stay_from ? 1 : 0);
    double l2g[K];
    XT_UNROLL
    for (int k = 0; k < K; ++k) l2g[k] = hdr[k];
    // g-form steps: the [prev][q] table offsets of this lane's outputs in all F - 1 phases (xt_r2_pack_io), kept across the step loop instead of
    // the lane id
    int pk = xt_r2_pack_io<F, 0, Ctx>(lane);
    const bool well_scaled = GG || a.well_scaled != 0;
    const bool chain = NP == 0 && well_scaled;  // warm-up as per-lane chains (xt_r2_chain)

    double* pos = (double*)(lds + xt_r2_pos0(NPT)) + wib * TPW * XT_F2_CHUNK * (D + KS);  // [TPW][CHUNK][D]
    double* sig = pos + TPW * XT_F2_CHUNK * D;                                           // [TPW][CHUNK][KS]
    // likelihood only: the byte address of this lane's staged positions as ONE opaque per-lane word (the compiler otherwise keeps the constant
    // base of the array apart from the per-lane part and adds it in every step)
    const int posb = NP == 0 ? xt_opaque(xt_r2_pos0(0) + (wib * TPW * XT_F2_CHUNK * (D + KS) + ts * XT_F2_CHUNK * D) * 8) : 0;
    // per (wave, track slot): NP == 0 {mantissa, exponent, count} of the running likelihood product; NP > 0 {sum LL, sum dLL_p}
    double* accp = (double*)(lds + xt_r2_acc0(NPT, D, KS, TPW)) + (wib * 8 + ts) * (NPT + 3);
    // NP == 0 reaches them by a byte address formed where it is used, as the re-centring cells below: nothing more is kept in registers
    // across the step loop
    auto accb = [&]() XT_INL { return xt_r2_acc0(0, D, KS, TPW) + (wib * 8 + xt_r2_slot<F>(xt_opaque(cx.lane()))) * 24; };
    // likelihood only: this lane's accumulated re-centring shift (xt_r2_step_g), and per (wave, slot) the sum over the finished tracks
    auto rcacc = [&]() XT_INL { return xt_r2_rc0(D, KS, TPW) + XT_R2_RC_ARR + xt_opaque(cx.tid()) * 8; };
    auto rcsum = [&]() XT_INL { return xt_r2_rc0(D, KS, TPW) + 2 * XT_R2_RC_ARR + (wib * 8 + xt_r2_slot<F>(xt_opaque(cx.lane()))) * 8; };
    if (leader) {
        if (NP == 0) {
            const int ab = accb();
            xt_at<double>(lds, ab) = 1.0;
            xt_at<double>(lds, ab + 8) = 0.0;
            xt_at<double>(lds, ab + 16) = 0.0;
            xt_at<double>(lds, rcsum()) = 0.0;
        } else {
            for (int i = 0; i < NPT + 1; ++i) accp[i] = 0.0;
        }
    }

    const int64_t nbatch = (b.N + TPW - 1) / TPW;
    const int64_t W0 = (int64_t)lb * nwb + wib, NW = (int64_t)nb * nwb;
    // likelihood only, scalar variance: the staging of complete batches below
    constexpr bool FAST = NP == 0 && K == 1 && XT_R2_STAGE_FAST(D);
    for (int64_t batch = W0; batch < nbatch; batch += NW) {
        const int64_t trk = batch * TPW + ts;
        const bool act = trk < b.N;

        // Staging of a chunk when every track of the batch exists (all but the last batch of a bucket; no per-peak errors): the batch's tracks
        // are contiguous, so the chunk is read at ONE wave-uniform base + a 32-bit per-lane byte offset (xt_gld), formed from the lane id where
        // it is used (nothing is kept across the step loop).  Loads (stage_ld: a position and the next one, for the delta, of up to
        // XT_R2_STAGE_GRP rounds of the wave, all issued before any is used) come before the writes to LDS (stage_st): one wait for memory
        // serves the chunk.
        // Lanes without an element read the base: no branch around the loads.
        constexpr int NE = TPW * XT_F2_CHUNK * D, NIT = (NE + 63) / 64, GRP = NIT < XT_R2_STAGE_GRP ? NIT : XT_R2_STAGE_GRP;
        // element i of the chunk: track slot t_, ok: its position exists, nx: so does the next; returns the byte offset from the base
        auto elem = [&](int p0, unsigned int i, unsigned int& t_, bool& ok, bool& nx) XT_INL {
            t_ = i / (XT_F2_CHUNK * D);
            const unsigned int r = i - t_ * (XT_F2_CHUNK * D), pp = (unsigned int)p0 + r / D;
            ok = (NE % 64 == 0 || i < NE) && pp < (unsigned int)L;
            nx = ok && pp + 1 < (unsigned int)L;
            return ok ? (t_ * (unsigned int)(L * D) + r) * 8u : 0u;
        };
        auto stage_ld = [&](int64_t bt, int p0, int k0, double* v, double* vn) XT_INL {
            const double* const base = b.tracks + xt_uniform64(cx, (bt * TPW * L + p0) * D);
            const unsigned int ln = (unsigned int)xt_opaque(cx.lane()) & 63u;
            XT_UNROLL
            for (int g = 0; g < GRP; ++g) {
                if (k0 + g >= NIT) continue;
                unsigned int t_;
                bool ok, nx;
                const unsigned int off = elem(p0, ln + 64u * (k0 + g), t_, ok, nx);
                v[g] = xt_gld(base, off);
                vn[g] = xt_gld(base, off + (nx ? D * 8u : 0u));
            }
        };
        auto stage_st = [&](int p0, int k0, const double* v, const double* vn) XT_INL {
            const unsigned int posw = xt_r2_pos0(0) + wib * TPW * XT_F2_CHUNK * D * 8, ln = (unsigned int)xt_opaque(cx.lane()) & 63u;
            XT_UNROLL
            for (int g = 0; g < GRP; ++g) {
                if (k0 + g >= NIT) continue;
                const unsigned int i = ln + 64u * (k0 + g);
                unsigned int t_;
                bool ok, nx;
                elem(p0, i, t_, ok, nx);
                if (ok) {
                    xt_at<double>(lds, (int)(posw + i * 8u)) = gform ? vn[g] - v[g] : v[g];  // g-form launches stage the deltas (see the loop below)
                    if (v[g] != v[g]) xt_at<int>(lds, XT_F2_NAN_OFF + (wib * 8 + (int)t_) * 4) = 1;
                }
            }
        };
        auto stage = [&](int p0) XT_INL {
            cx.wave_sync();  // the reads of the previous chunk are done
            if constexpr (GN) {
                // Missed frames of a gradient launch: absolute positions are staged as they are (a missed row stays NaN: its step never uses
                // it, xt_r2_step<.., GAPS>), so no stand-in row is needed - only the classification of section 25.  A row's coordinates may sit
                // in different lanes, so every element ORs its row into the track's "has a NaN" or "has a finite" mask (LDS atomics); then one
                // lane per slot forms missed = NaN & ~finite for the steps, counts the missed rows and poisons the track for a row with only
                // some NaN coordinates or a missed first / last row.  Complete and partial batches alike (the empty slots of the last batch
                // mirror the bucket's last track).
                const int gc0 = xt_r2_grad_gap0(NPT, D, TPW) + wib * 8 * 16;
                if (lane < 8) {
                    xt_at<uint32_t>(lds, gc0 + lane * 16) = 0u;
                    xt_at<uint32_t>(lds, gc0 + lane * 16 + 4) = 0u;
                }
                cx.wave_sync();
                for (int i = lane; i < TPW * XT_F2_CHUNK * D; i += 64) {
                    const int t_ = i / (XT_F2_CHUNK * D), r = i - t_ * (XT_F2_CHUNK * D);
                    const int64_t tk = batch * TPW + t_;
                    const int64_t tkc = tk < b.N ? tk : b.N - 1;
                    if (p0 + r / D < L) {
                        const double v = b.tracks[(tkc * L + p0) * D + r];
                        pos[i] = XT_R2_GAP_STAGED(v);
                        cx.atomic_or_u32(&xt_at<uint32_t>(lds, gc0 + t_ * 16 + (v != v ? 0 : 4)), 1u << (r / D));
                    }
                }
                cx.wave_sync();
                if (lane < TPW) {
                    const int cell = gc0 + lane * 16;
                    const int nrows = L - p0 < XT_F2_CHUNK ? L - p0 : XT_F2_CHUNK;
                    const unsigned int valid = 0xffffffffu >> (32 - nrows);
                    const unsigned int nanm = xt_at<uint32_t>(lds, cell) & valid, fin = xt_at<uint32_t>(lds, cell + 4) & valid;
                    const unsigned int gmm = nanm & ~fin;
                    // a row with only some NaN coordinates, a missed first or last row: the track is NaN
                    if ((nanm & fin) || (p0 == 0 && (gmm & 1u)) || (L - p0 <= XT_F2_CHUNK && ((gmm >> (nrows - 1)) & 1u)))
                        xt_at<int>(lds, XT_F2_NAN_OFF + (wib * 8 + lane) * 4) = 1;
                    xt_at<uint32_t>(lds, cell) = gmm;  // what the steps read
                    xt_at<int>(lds, cell + 12) += __builtin_popcount(gmm);
                }
                cx.wave_sync();
                return;
            }
            if constexpr (GG) {
                // Missed frames: a row is classified from ALL its coordinates (they may sit in different lanes, even rounds), so the chunk is
                // staged in two passes around two row masks per track (LDS atomics).  Pass 1 loads every element and its successor and ORs the
                // element's row into the NaN or the finite mask.  Pass 2 stages the deltas of the FILLED track: a missed row stands in as the last
                // observed row before it (found in the masks; before the chunk: the row index carried in the track's cell, read again from
                // memory), so the delta INTO a missed row is 0 and the one out of it reaches back to that row.  A NaN successor is a missed row
                // or poisons its track where it is staged itself.  Serves complete and partial batches (the empty slots of the last batch
                // mirror the bucket's last track); one wave-uniform base + 32-bit offsets.
                const int gc0 = xt_r2_gap0(D, TPW) + wib * 8 * 16;
                const unsigned int ln = (unsigned int)xt_opaque(cx.lane()) & 63u;
                if (ln < 8u) {
                    xt_at<uint32_t>(lds, gc0 + (int)ln * 16) = 0u;
                    xt_at<uint32_t>(lds, gc0 + (int)ln * 16 + 4) = 0u;
                }
                cx.wave_sync();
                const int64_t left = b.N - batch * TPW;
                const unsigned int tmax = left < TPW ? (unsigned int)left - 1u : (unsigned int)TPW - 1u;
                const double* const base = b.tracks + xt_uniform64(cx, batch * TPW * L * D);
                auto gelem = [&](unsigned int i, unsigned int& t_, unsigned int& row, unsigned int& pp, unsigned int& o0) XT_INL {
                    t_ = i / (XT_F2_CHUNK * D);
                    const unsigned int r = i - t_ * (XT_F2_CHUNK * D);
                    row = r / D;
                    pp = (unsigned int)p0 + row;
                    const unsigned int tc = t_ < tmax ? t_ : tmax;
                    o0 = (tc * (unsigned int)L * D + (r - row * D)) * 8u;  // the element's coordinate in row 0 of its track
                    return (NE % 64 == 0 || i < NE) && pp < (unsigned int)L;
                };
                double v[NIT], vn[NIT];
                XT_UNROLL
                for (int k = 0; k < NIT; ++k) {
                    unsigned int t_, row, pp, o0;
                    const bool ok = gelem(ln + 64u * k, t_, row, pp, o0);
                    const unsigned int off = ok ? o0 + pp * (D * 8u) : 0u;
                    v[k] = xt_gld(base, off);
                    vn[k] = xt_gld(base, off + (ok && pp + 1 < (unsigned int)L ? D * 8u : 0u));
                }
                XT_UNROLL
                for (int k = 0; k < NIT; ++k) {
                    unsigned int t_, row, pp, o0;
                    if (gelem(ln + 64u * k, t_, row, pp, o0)) cx.atomic_or_u32(&xt_at<uint32_t>(lds, gc0 + (int)t_ * 16 + (v[k] != v[k] ? 0 : 4)), 1u << row);
                }
                cx.wave_sync();
                XT_UNROLL
                for (int k = 0; k < NIT; ++k) {
                    const unsigned int i = ln + 64u * k;
                    unsigned int t_, row, pp, o0;
                    if (!gelem(i, t_, row, pp, o0)) continue;
                    const unsigned int gmm = xt_at<uint32_t>(lds, gc0 + (int)t_ * 16) & ~xt_at<uint32_t>(lds, gc0 + (int)t_ * 16 + 4);
                    const bool isgap = (gmm >> row) & 1u;
                    double cur = v[k];
                    if (isgap) {
                        const unsigned int x = ~gmm & (0xffffffffu >> (31u - row));  // observed rows of the chunk up to this one
                        const unsigned int src = x ? (unsigned int)p0 + 31u - (unsigned int)__builtin_clz(x) : (unsigned int)xt_at<int>(lds, gc0 + (int)t_ * 16 + 8);
                        cur = xt_gld(base, o0 + src * (D * 8u));
                    }
                    xt_at<double>(lds, xt_r2_pos0(0) + (wib * TPW * XT_F2_CHUNK * D + (int)i) * 8) = vn[k] != vn[k] ? 0.0 : vn[k] - cur;
                    // a row with only some NaN coordinates, a missed first or last row: the track is NaN
                    if ((v[k] != v[k] && !isgap) || (isgap && (pp == 0u || pp + 1u == (unsigned int)L))) xt_at<int>(lds, XT_F2_NAN_OFF + (wib * 8 + (int)t_) * 4) = 1;
                }
                cx.wave_sync();
                if (ln < (unsigned int)TPW) {
                    const int cell = gc0 + (int)ln * 16;
                    const int nrows = L - p0 < XT_F2_CHUNK ? L - p0 : XT_F2_CHUNK;
                    const unsigned int valid = 0xffffffffu >> (32 - nrows);
                    const unsigned int gmm = xt_at<uint32_t>(lds, cell) & ~xt_at<uint32_t>(lds, cell + 4) & valid, obs = ~gmm & valid;
                    xt_at<uint32_t>(lds, cell) = gmm;  // what the steps read
                    if (obs) xt_at<int>(lds, cell + 8) = p0 + 31 - __builtin_clz(obs);
                    xt_at<int>(lds, cell + 12) += __builtin_popcount(gmm);
                }
                cx.wave_sync();
                return;
            }
            if constexpr (FAST) {
                if (KS == 0 && (batch + 1) * TPW <= b.N) {
                    XT_UNROLL
                    for (int k0 = 0; k0 < NIT; k0 += GRP) {
                        double v[GRP], vn[GRP];
                        stage_ld(batch, p0, k0, v, vn);
                        stage_st(p0, k0, v, vn);
                    }
                    cx.wave_sync();
                    return;
                }
            }
            for (int i = lane; i < TPW * XT_F2_CHUNK * D; i += 64) {
                const int t_ = i / (XT_F2_CHUNK * D), r = i - t_ * (XT_F2_CHUNK * D);
                const int64_t tk = batch * TPW + t_;
                const int64_t tkc = tk < b.N ? tk : b.N - 1;
                const int pp = p0 + r / D;
                if (pp < L) {
                    const double* const src = b.tracks + (tkc * L + p0) * D + r;
                    const double v = src[0];
                    if constexpr (NP == 0 && K == 1) {
                        // g-form launches stage the position DELTAS c_{t+1} - c_t (0 at the last position): their steps never read an
                        // absolute coordinate.  The next position is in the cache line just read or the one after (a chunk's last delta
                        // reaches into the next chunk); both loads are issued before either is used, so the wave waits for memory once.
                        // The NaN flag is set from the raw position.
                        const double vn = src[pp + 1 < L ? D : 0];
                        pos[i] = gform ? vn - v : v;
                    } else {
                        pos[i] = v;
                    }
                    if (v != v) xt_at<int>(lds, XT_F2_NAN_OFF + (wib * 8 + t_) * 4) = 1;
                }
            }
            if (KS)
                for (int i = lane; i < TPW * XT_F2_CHUNK * KS; i += 64) {
                    const int t_ = i / (XT_F2_CHUNK * KS), r = i - t_ * (XT_F2_CHUNK * KS);
                    const int64_t tk = batch * TPW + t_;
                    const int64_t tkc = tk < b.N ? tk : b.N - 1;
                    const int pp = p0 + r / KS;
                    if (pp < L) {
                        const double v = b.sigma[(tkc * L + p0) * KS + r];
                        sig[i] = v;
                        if (v != v) xt_at<int>(lds, XT_F2_NAN_OFF + (wib * 8 + t_) * 4) = 1;
                    }
                }
            cx.wave_sync();
        };
        auto getpos = [&](int t, double* c, double* l2) XT_INL {
            const int r = t & (XT_F2_CHUNK - 1);
            XT_UNROLL
            for (int d = 0; d < D; ++d) c[d] = NP == 0 ? xt_at<double>(lds, posb + (r * D + d) * 8) : pos[(ts * XT_F2_CHUNK + r) * D + d];
            if (KS == 0) {
                XT_UNROLL
                for (int k = 0; k < K; ++k) l2[k] = xt_at<double>(lds, k * 8);  // broadcast read of the blob header (two fewer live VGPRs per k than a register copy)
            } else {
                XT_UNROLL
                for (int k = 0; k < K; ++k) {
                    double sg = sig[(ts * XT_F2_CHUNK + r) * KS + (KS == 1 ? 0 : k)];
                    if (a.locerr_mode == 2) {
                        sg = xt_fma(sg, hdr[3], hdr[4]);
                        sg = sg < 1e-6 ? 1e-6 : sg;
                    }
                    l2[k] = sg * sg;
                }
            }
        };

        XtR2Lane<D, K, NP> s;
        // g-form launches: -2 x the log part of the members' weights (xt_r2_step_g); member 1 is dead until the first full step gives it a value
        // (which reads lam[0] alone).  Otherwise only read by the old read-out of a launch without g-form steps, where lam[1] meets z[1] = 0
        double lam[2] = {0.0, 0.0};
        if constexpr (NP == 0 && K == 1) {
            if (gform) lam[1] = XT_R2_LAM_DEAD;
        }
        unsigned int gmk = 0u;       // GAPS: the missed rows of this lane's track in the staged chunk (bit = row of the chunk)
#define XT_R2_PHASE(H, ZF_, LAZY_)                                                                     \
    if (NGB > (H) && t <= tend2 && ph == (H)) {                                                        \
        double c[D], l2[K];                                                                            \
        getpos(t, c, l2);                                                                              \
        xt_r2_step<F, D, K, NP, ((H) < NGB ? (H) : 0), ZF_, LAZY_, VAR, false, GN>(cx, lds, s, XT_R2_TABSEL, c, l2, GN && ((gmk >> (t & (XT_F2_CHUNK - 1))) & 1u)); \
        ++t;                                                                                           \
        ph = (H) + 1 == NGB ? 0 : (H) + 1;                                                             \
    }
#define XT_R2_PHASE_G(H)                                                                               \
    if (NGB > (H) && t <= tend2 && ph == (H)) {                                                        \
        double c[D], l2[K];                                                                            \
        getpos(t, c, l2);                                                                              \
        xt_r2_step_g<F, D, ((H) < NGB ? (H) : 0), false, GAPS>(cx, lds, s, lam, pk, XT_R2_TABSEL, c, GAPS && ((gmk >> (t & (XT_F2_CHUNK - 1))) & 1u)); \
        ++t;                                                                                           \
        ph = (H) + 1 == NGB ? 0 : (H) + 1;                                                             \
    }
#define XT_R2_PHASES(ZF_, LAZY_) \
    XT_R2_PHASE(0, ZF_, LAZY_)   \
    XT_R2_PHASE(1, ZF_, LAZY_)   \
    XT_R2_PHASE(2, ZF_, LAZY_)   \
    XT_R2_PHASE(3, ZF_, LAZY_)   \
    XT_R2_PHASE(4, ZF_, LAZY_)   \
    XT_R2_PHASE(5, ZF_, LAZY_)
#define XT_R2_TABSEL tab
        auto run_steps = [&](int& t, int tend, int tab) XT_INL {
            int ph = (t - 1) % NGB;
            const int tend2 = tend;
            if (!well_scaled) {
                while (t <= tend2) { XT_R2_PHASES(false, false) }
                return;
            }
            // well-scaled: positions 1 .. F - 1 are done by the warm-up chain and the merge-free first step (every lane live from here on)
            if constexpr (NP == 0 && K == 1) {
                if (gform) {
                    while (t <= tend2) {
                        XT_R2_PHASE_G(0)
                        XT_R2_PHASE_G(1)
                        XT_R2_PHASE_G(2)
                        XT_R2_PHASE_G(3)
                        XT_R2_PHASE_G(4)
                        XT_R2_PHASE_G(5)
                    }
                    return;
                }
            }
            while (t <= tend2) { XT_R2_PHASES(true, true) }
        };
#undef XT_R2_TABSEL
#define XT_R2_TABSEL (XT_R2_TAB0 + (t >= stay_from ? 32 : 0))
        // gradient kernels: ONE variant of the unrolled loop per launch (guarded arithmetic: zero weights handled; LAZY only skips the
        // normalisation of the stored mantissas of well-scaled models) and the transition table picked per step - the three variants x
        // two tables of the likelihood-only loop would be 170 KB of code with 7 directions
        auto run_steps_g = [&](int& t, int tend) XT_INL {
            int ph = (t - 1) % NGB;
            const int tend2 = tend;
            if (well_scaled) {
                while (t <= tend2) { XT_R2_PHASES(false, true) }
            } else {
                while (t <= tend2) { XT_R2_PHASES(false, false) }
            }
        };
#undef XT_R2_TABSEL
#undef XT_R2_PHASES
#undef XT_R2_PHASE_G
#undef XT_R2_PHASE

        XtAcc tot;
        tot.clear();
        double gacc[NP ? NP : 1];  // sum over this lane's (Q, q) pairs of w * d log w, on the 2^fe scale
        double uacc[XT_R2_MAXU];   // the same for the uniform directions (d log w = the direction's constant + d log of the last factor)
        int fe = XT_EMIN;
        int t = 1;
        if (lane < 8) xt_at<int>(lds, XT_F2_NAN_OFF + (wib * 8 + lane) * 4) = 0;
        if constexpr (GN) {
            if (lane < 8) xt_at<int>(lds, xt_r2_grad_gap0(NPT, D, TPW) + (wib * 8 + lane) * 16 + 12) = 0;
        }
        if constexpr (GG) {
            if (lane < 8) {
                xt_at<int>(lds, xt_r2_gap0(D, TPW) + (wib * 8 + lane) * 16 + 8) = 0;
                xt_at<int>(lds, xt_r2_gap0(D, TPW) + (wib * 8 + lane) * 16 + 12) = 0;
            }
        }
        if (NP == 0) {
            xt_at<int>(lds, rcacc()) = 0;
            xt_at<int>(lds, rcacc() - XT_R2_RC_ARR) = XT_R2_RC_NONE;  // the lane's own cell: the track's leader resets the one in use
        }
        // ---- last position (+ leaving / bleaching factor): reduction over (member Q, new digit q), on the staged chunk that holds it (the last
        // one).  The likelihood-only scalar-variance kernels run it after the chunk loop, so that none of its results is carried around that
        // loop; g-form launches take the log-carried read-out there instead and never run this one.
        auto readout = [&]() XT_INL {
            double cl[D], l2l[K];
            getpos(tlast, cl, l2l);
            const int hp = (tlast - 2 + NGB) % NGB;  // group bit of the newest digit
            const int pbit = (F == 7 || hp < 2) ? hp : hp + 1;
            const int prev = (lane >> pbit) & 1;
            double wm[4], rr[4][K], dq[2][D], dsqQ[2];
            int we[4];
            if constexpr (NP == 0 && K == 1) {
                // the four 1 / den of the (Q, q) pairs from ONE reciprocal of their product (den in [1e-12, 1e4] on a well-scaled launch, and
                // any launch's variances are far from the fp64 range limits: xt_rcp)
                double dn[4];
                XT_UNROLL
                for (int i = 0; i < 4; ++i) dn[i] = xt_at<double>(lds, XT_R2_TAB0 + 4 * 32 + (prev * 2 + (i & 1)) * 8) + s.u[i >> 1][0] + l2l[0];
                const double p01 = dn[0] * dn[1], p23 = dn[2] * dn[3];
                const double R = xt_rcp3(p01 * p23);
                const double r01 = R * p23, r23 = R * p01;  // 1 / (dn0 dn1), 1 / (dn2 dn3)
                rr[0][0] = r01 * dn[1];
                rr[1][0] = r01 * dn[0];
                rr[2][0] = r23 * dn[3];
                rr[3][0] = r23 * dn[2];
            }
            XT_UNROLL
            for (int Q = 0; Q < 2; ++Q) {
                dsqQ[Q] = 0.0;
                XT_UNROLL
                for (int d = 0; d < D; ++d) {
                    dq[Q][d] = cl[d] - s.m[Q][d];
                    dsqQ[Q] = xt_fma(dq[Q][d], dq[Q][d], dsqQ[Q]);
                }
                double x[2], gf[2];
                XT_UNROLL
                for (int q = 0; q < 2; ++q) {
                    const double d2 = xt_at<double>(lds, XT_R2_TAB0 + 4 * 32 + (prev * 2 + q) * 8);
                    if (K == 1) {
                        double r;
                        if constexpr (NP == 0) {
                            r = rr[Q * 2 + q][0];
                        } else {
                            r = xt_rcp(d2 + s.u[Q][0] + l2l[0]);
                            rr[Q * 2 + q][0] = r;
                        }
                        if constexpr (NP == 0)
                            x[q] = -0.5 * xt_fma(dsqQ[Q], r, lam[Q]);  // lambda = 0 here: launches with g-form steps never take this read-out
                        else
                            x[q] = -0.5 * dsqQ[Q] * r;
                        gf[q] = xt_pow_half<D>(r);
                    } else {
                        double xx = 0.0, gg = 1.0;
                        XT_UNROLL
                        for (int d = 0; d < D; ++d) {
                            const double r = NP == 0 ? xt_rcp3(d2 + s.u[Q][d] + l2l[d]) : xt_rcp(d2 + s.u[Q][d] + l2l[d]);
                            rr[Q * 2 + q][d] = r;
                            xx = xt_fma(-0.5 * dq[Q][d] * dq[Q][d], r, xx);
                            gg *= r;
                        }
                        x[q] = xx;
                        gf[q] = sqrt(gg);
                    }
                }
                double p[2];
                int j[2], n[2];
                xt_exp_tab_x2(x[0], x[1], p[0], p[1], j[0], j[1], n[0], n[1]);
                XT_UNROLL
                for (int q = 0; q < 2; ++q) {
                    const double tf = xt_at<double>(lds, XT_R2_TAB0 + vfin * 32 + (prev * 2 + q) * 8);
                    wm[Q * 2 + q] = s.z[Q] * tf * gf[q] * xt_at<double>(lds, XT_F2_EXPB_OFF + j[q] * 8) * p[q];
                    we[Q * 2 + q] = s.e[Q] + n[q];
                    tot.add(wm[Q * 2 + q], we[Q * 2 + q]);
                }
            }
            fe = xt_r2_gmax<F>(cx, tot.m != 0.0 ? tot.e : XT_EMIN);
            if (NP > 0) {
                double ws[4];
                XT_UNROLL
                for (int i = 0; i < 4; ++i) ws[i] = wm[i] != 0.0 ? xt_ldexp(wm[i], we[i] - fe) : 0.0;
                XT_UNROLL
                for (int pp = 0; pp < NP; ++pp) {
                    const int tb = XT_R2_TAN0 + pp * XT_R2_TB * 8;
                    double dl[K];
                    XT_UNROLL
                    for (int k = 0; k < K; ++k) dl[k] = xt_at<double>(lds, tb + k * 8);
                    double acc = 0.0;
                    XT_UNROLL
                    for (int Q = 0; Q < 2; ++Q) {
                        XT_UNROLL
                        for (int q = 0; q < 2; ++q) {
                            const double dlT = xt_at<double>(lds, tb + XT_R2_TAB0 + vfin * 32 + (prev * 2 + q) * 8);
                            const double dd2 = xt_at<double>(lds, tb + XT_R2_TAB0 + 4 * 32 + (prev * 2 + q) * 8);
                            double rel = s.rz[pp][Q] + dlT;
                            if (K == 1) {
                                const double r = rr[Q * 2 + q][0];
                                const double dden = dd2 + s.du[pp][Q][0] + dl[0];
                                double ddsq = 0.0;
                                XT_UNROLL
                                for (int d = 0; d < D; ++d) ddsq = xt_fma(-2.0 * dq[Q][d], s.dm[pp][Q][d], ddsq);
                                rel -= 0.5 * r * (D * dden + ddsq - dsqQ[Q] * r * dden);
                            } else {
                                XT_UNROLL
                                for (int d = 0; d < D; ++d) {
                                    const double r = rr[Q * 2 + q][d];
                                    const double dden = dd2 + s.du[pp][Q][d] + dl[d];
                                    rel -= 0.5 * r * (dden - 2.0 * dq[Q][d] * s.dm[pp][Q][d] - dq[Q][d] * dq[Q][d] * r * dden);
                                }
                            }
                            acc = xt_fma(ws[Q * 2 + q], ws[Q * 2 + q] != 0.0 ? rel : 0.0, acc);
                        }
                    }
                    gacc[pp] = acc;
                }
                XT_UNROLL
                for (int u = 0; u < XT_R2_MAXU; ++u) {  // uniform directions: sum over the pairs of w * d log(last factor)
                    double acc = 0.0;
                    if (u < NU) {
                        const int tb = XT_R2_TAN0 + (NP + u) * XT_R2_TB * 8;
                        XT_UNROLL
                        for (int i = 0; i < 4; ++i) acc = xt_fma(ws[i], xt_at<double>(lds, tb + XT_R2_TAB0 + vfin * 32 + (prev * 2 + (i & 1)) * 8), acc);
                    }
                    uacc[u] = acc;
                }
            }
        };
        for (int p0 = 0; p0 < L; p0 += XT_F2_CHUNK) {
            stage(p0);
            if constexpr (GG) gmk = xt_at<uint32_t>(lds, xt_r2_gap0(D, TPW) + (wib * 8 + xt_r2_slot<F>(xt_opaque(cx.lane()))) * 16);
            if constexpr (GN) gmk = xt_at<uint32_t>(lds, xt_r2_grad_gap0(NPT, D, TPW) + (wib * 8 + ts) * 16);
            if (p0 == 0) {
                // ---- position 0: the initial state is the newest digit (group bit NGB - 1); dummy digits set -> zero weight
                constexpr int NBIT = xt_r2_gbit(F, NGB - 1);
                double c0[D], l20[K];
                getpos(0, c0, l20);
                const bool live0 = chain || (lane & (GMASK & ~(1 << NBIT))) == 0;  // the chain masks the dummy digits at its end
                const int s0 = (lane >> NBIT) & 1;
                s.z[0] = live0 ? hdr[8 + s0] : 0.0;
                s.e[0] = live0 ? 0 : XT_EMIN;
                s.z[1] = 0.0;
                s.e[1] = XT_EMIN;
                XT_UNROLL
                for (int q = 0; q < 2; ++q) {
                    XT_UNROLL
                    for (int d = 0; d < D; ++d) s.m[q][d] = c0[d];
                    XT_UNROLL
                    for (int k = 0; k < K; ++k) s.u[q][k] = l20[k];
                }
                if constexpr (NP == 0 && K == 1) {
                    // g-form launches: the members carry r = c_next - m (position 0: the staged delta that getpos just read), v = l2 + u and
                    // weights y exp(-lambda / 2), from here to the read-out of the last position
                    if (gform) s.u[0][0] = s.u[1][0] = 2.0 * l20[0];
                }
                XT_UNROLL
                for (int pp = 0; pp < NP; ++pp) {
                    const int tb = XT_R2_TAN0 + pp * XT_R2_TB * 8;
                    s.rz[pp][0] = live0 ? xt_at<double>(lds, tb + (8 + s0) * 8) : 0.0;
                    s.rz[pp][1] = 0.0;
                    XT_UNROLL
                    for (int q = 0; q < 2; ++q) {
                        XT_UNROLL
                        for (int d = 0; d < D; ++d) s.dm[pp][q][d] = 0.0;
                        XT_UNROLL
                        for (int k = 0; k < K; ++k) s.du[pp][q][k] = xt_at<double>(lds, tb + k * 8);
                    }
                }
                if constexpr (NP == 0) {
                    if (chain) {
                        // positions 1 .. F - 2 as per-lane chains, position F - 1 without the merge of the dead member: t = F after that
                        const int T = L - 2 < NGB - 1 ? L - 2 : NGB - 1;
                        bool chain_done = false;
                        if constexpr (K == 1) {
                            if (gform) {
                                xt_r2_chain_g<F, D, GAPS>(cx, lds, s, lam, T, stay_from, getpos, gmk);
                                s.e[0] = s.e[1] = 0;  // the read-out's integer exponents: all of the weight's scale is in lambda
                                chain_done = true;
                            }
                        }
                        if (!chain_done) xt_r2_chain<F>(cx, lds, s, T, stay_from, getpos);
                        if (L - 2 >= F - 1) {
                            double c[D], l2[K];
                            getpos(F - 1, c, l2);
                            bool first_done = false;
                            if constexpr (K == 1) {
                                if (gform) {
                                    xt_r2_step_g<F, D, NGB - 1, true, GAPS>(cx, lds, s, lam, pk, XT_R2_TAB0 + (F - 1 >= stay_from ? 32 : 0), c, GAPS && ((gmk >> (F - 1)) & 1u));
                                    first_done = true;
                                }
                            }
                            if (!first_done) xt_r2_step<F, D, K, NP, NGB - 1, true, true, VAR, true>(cx, lds, s, XT_R2_TAB0 + (F - 1 >= stay_from ? 32 : 0), c, l2);
                            t = F;
                        } else {
                            t = L - 1 > 1 ? L - 1 : 1;
                        }
                    }
                }
            }
            const int tend = (L - 2 < p0 + XT_F2_CHUNK - 1) ? L - 2 : p0 + XT_F2_CHUNK - 1;
            if (NP == 0) {
                run_steps(t, tend < stay_from - 1 ? tend : stay_from - 1, XT_R2_TAB0);
                run_steps(t, tend, XT_R2_TAB0 + 32);
            } else {
                run_steps_g(t, tend);
            }
            if constexpr (!(NP == 0 && K == 1)) {
                if (tlast >= p0 && tlast < p0 + XT_F2_CHUNK) readout();
            }
        }
        // reduce over the track's lanes (every lane ends with the same values)
        double lsum = 0.0;
        int ronsh = 0;  // the shift of the log-carried read-out
        bool ro_log = false;
        if constexpr (NP == 0 && K == 1) {
            if (gform) {
                ro_log = true;
                // ---- last position of a g-form launch, log-carried.  A member Q holds (y, lambda, r = c_last - m,
                // v = l2 + u); its term for the new digit q is y Tfin rho^(D/2) exp(-a / 2), a = |r|^2 rho + lambda, rho = 1 / (d2 + v).
                // ONE more re-centring instead of integer exponents: the track's smallest a (truncated and clamped as in xt_r2_step_g, through
                // the same LDS cell) is taken out of every a, so the track's largest term has an argument in (-1/2, 1/2) and the terms add up
                // as plain doubles (a negligible one underflows to 0); the shift goes back into the log-likelihood with the steps' shifts.
                const int hpl = (tlast - 2 + NGB) % NGB;  // group bit of the newest digit
                const int pbl = (F == 7 || hpl < 2) ? hpl : hpl + 1;
                const int iol = ((xt_opaque(cx.lane()) >> pbl) & 1) * 16;  // [prev][0] byte offset
                double d2l[2], tfl[2], dn[4], rho[4], aq[4], wq[4];  // wq: the terms' factors outside the exponential
                XT_UNROLL
                for (int q = 0; q < 2; ++q) {
                    d2l[q] = xt_at<double>(lds, XT_R2_TAB0 + 4 * 32 + iol + q * 8);
                    tfl[q] = xt_at<double>(lds, XT_R2_TAB0 + vfin * 32 + iol + q * 8);
                }
                XT_UNROLL
                for (int i = 0; i < 4; ++i) dn[i] = d2l[i & 1] + s.u[i >> 1][0];
                // the four rho from ONE reciprocal of the product of the dens (each in [1e-12, 1e4] on a well-scaled launch)
                const double p01 = dn[0] * dn[1], p23 = dn[2] * dn[3];
                const double R = xt_rcp3(p01 * p23);
                const double r01 = R * p23, r23 = R * p01;
                rho[0] = r01 * dn[1];
                rho[1] = r01 * dn[0];
                rho[2] = r23 * dn[3];
                rho[3] = r23 * dn[2];
                XT_UNROLL
                for (int Q = 0; Q < 2; ++Q) {
                    double rsq = 0.0;
                    XT_UNROLL
                    for (int d = 0; d < D; ++d) rsq = xt_fma(s.m[Q][d], s.m[Q][d], rsq);
                    aq[Q * 2] = xt_fma(rsq, rho[Q * 2], lam[Q]);
                    aq[Q * 2 + 1] = xt_fma(rsq, rho[Q * 2 + 1], lam[Q]);
                    wq[Q * 2] = (s.z[Q] * tfl[0]) * xt_pow_half<D>(rho[Q * 2]);
                    wq[Q * 2 + 1] = (s.z[Q] * tfl[1]) * xt_pow_half<D>(rho[Q * 2 + 1]);
                }
                const double amin = fmin(fmin(aq[0], aq[1]), fmin(aq[2], aq[3]));  // dead members stay out (XT_R2_LAM_DEAD)
                // the track's cell: a re-centring in the last step has left its shift there (reset one phase later); the next batch
                // starts from its own reset
                const int cell = xt_r2_rc0(D, 0, TPW) + (xt_r2_tid8(cx) & ~(GMASK * 8));
                xt_at<int>(lds, cell) = XT_R2_RC_NONE;
                cx.wave_sync();
                cx.atomic_max_i32(&xt_at<int>(lds, cell), (int)fmin(fmax(-amin, -1e9), 1e9));  // NaN (poisoned track): a = +1e9
                cx.wave_sync();
                const int nsh = xt_at<int>(lds, cell);  // - min over the track's lanes
                const double nsd = -(double)nsh;  // the argument below as a plain difference: the exponential's clamp stays the steps' constant
                double acc = 0.0;
                XT_UNROLL
                for (int i = 0; i < 4; ++i) {
                    double p;
                    int j, n;
                    xt_exp_tab_half_x1(nsd - aq[i], p, j, n);
                    const double E = xt_ldexp(xt_at<double>(lds, XT_F2_EXPB_OFF + j * 8) * p, n);
                    acc = xt_fma(wq[i], E, acc);
                }
                lsum = acc;
                ronsh = nsh;
                fe = 0;
            }
        }
        if (!ro_log) {
            if constexpr (NP == 0 && K == 1) readout();
            lsum = tot.m != 0.0 ? xt_ldexp(tot.m, tot.e - fe) : 0.0;
        }
        double sum = xt_r2_gsum<F>(cx, lsum);
        const bool poisoned = xt_at<int>(lds, XT_F2_NAN_OFF + (wib * 8 + ts) * 4) != 0;
        if (poisoned) sum = NAN;  // NaN input -> NaN likelihood, as in the reference
        if (NP == 0) {
            const int lz = xt_opaque(cx.lane());
            const int64_t trk = batch * TPW + xt_r2_slot<F>(lz);  // formed again: not held across the step loop
            if (trk < b.N && (lz & GMASK) == 0) {
                // the re-centring shifts of the steps (the lane's cell) and of the log-carried read-out (added as doubles: up to 1e9 on a last-row
                // outlier, which the 32-bit cell would not hold beside the steps' sum), in lambda units; 0 unless log-carried steps ran
                const double rcs0 = 0.5 * ((double)ronsh - (double)xt_at<int>(lds, rcacc()));
                double rcs = rcs0;
                // GAPS: + D/2 ln(2 pi l2) per missed row - its share of the bucket's ll_const and the D/2 ln l2 its steps left in lambda (xt_r2_step_g)
                if constexpr (GAPS) rcs = xt_fma((double)xt_at<int>(lds, xt_r2_gap0(D, TPW) + (wib * 8 + xt_r2_slot<F>(lz)) * 16 + 12), xt_at<double>(lds, XT_R2_GC_OFF), rcs);
                if (b.ll_out) b.ll_out[trk] = log(sum) + (double)fe * XT_LN2 + b.ll_const + rcs;
                xt_at<double>(lds, rcsum()) += rcs;
                const int ab = accb();
                const double pm = xt_at<double>(lds, ab) * xt_frexp_mant(sum);
                double acce = xt_at<double>(lds, ab + 8) + (double)(fe + xt_frexp_exp(sum) + xt_frexp_exp(pm));
                if (sum == 0.0) acce = -INFINITY;
                xt_at<double>(lds, ab) = xt_frexp_mant(pm);
                xt_at<double>(lds, ab + 8) = acce;
                xt_at<double>(lds, ab + 16) += 1.0;
            }
        } else {
            const double rs = 1.0 / sum;
            double gsum[NP ? NP : 1];
            XT_UNROLL
            for (int pp = 0; pp < NP; ++pp) gsum[pp] = xt_r2_gsum<F>(cx, gacc[pp]);
            double usum[XT_R2_MAXU];
            XT_UNROLL
            for (int u = 0; u < XT_R2_MAXU; ++u) usum[u] = u < NU ? xt_r2_gsum<F>(cx, uacc[u]) : 0.0;
            if (act && leader) {
                double ll = log(sum) + (double)fe * XT_LN2 + b.ll_const;
                // GAPS: + D/2 log 2 pi per missed row turns the bucket's ll_const (from L) into the track's (from its observed rows); model-independent
                if constexpr (GN) ll = xt_fma((double)xt_at<int>(lds, xt_r2_grad_gap0(NPT, D, TPW) + (wib * 8 + ts) * 16 + 12), 0.5 * D * XT_LOG2PI, ll);
                if (b.ll_out) b.ll_out[trk] = ll;
                accp[0] += ll;
                XT_UNROLL
                for (int pp = 0; pp < NP; ++pp) accp[1 + pp] += gsum[pp] * rs;
                double* const srow = b.scores_out ? b.scores_out + trk * ga.score_ld : nullptr;  // this track's row of the score matrix
                if (srow) {
                    XT_UNROLL
                    for (int pp = 0; pp < NP; ++pp) srow[ga.score_col0 + pp] = gsum[pp] * rs;
                }
                // uniform directions: d log of the initial fraction + one constant per step (without / with the stay-in-FOV factor)
                const int nsteps = L - 2 > 0 ? L - 2 : 0;
                const int n1 = nsteps >= stay_from ? nsteps - stay_from + 1 : 0, n0 = nsteps - n1;
                XT_UNROLL
                for (int u = 0; u < XT_R2_MAXU; ++u)
                    if (u < NU) {
                        const int tb = XT_R2_TAN0 + (NP + u) * XT_R2_TB * 8;
                        const double rzu = xt_at<double>(lds, tb + 8 * 8) + n0 * xt_at<double>(lds, tb + XT_R2_TAB0) + n1 * xt_at<double>(lds, tb + XT_R2_TAB0 + 32);
                        accp[1 + NP + u] += usum[u] * rs + rzu;
                        if (srow) srow[ga.score_ucol0 + u] = usum[u] * rs + rzu;
                    }
            }
        }
        cx.wave_sync();
    }

    // ---- per-slot sums -> block partials (fixed order)
    cx.sync();
    if (NP == 0) {
        if (leader) {
            const double* ac = &xt_at<double>(lds, accb());
            smem[wib * TPW + ts] = ac[2] > 0.0 ? log(ac[0]) + ac[1] * XT_LN2 + ac[2] * b.ll_const + xt_at<double>(lds, rcsum()) : 0.0;
        }
        cx.sync();
        if (cx.tid() == 0) {
            double sacc = 0.0;
            for (int i = 0; i < nwb * TPW; ++i) sacc += smem[i];
            a.partials[cx.block()] = sacc;
        }
    } else {
        const double* acc0 = (const double*)(lds + xt_r2_acc0(NPT, D, KS, TPW));
        for (int col = cx.tid(); col < NPT + 1; col += cx.nthreads()) {
            double sacc = 0.0;
            for (int w = 0; w < nwb; ++w)
                for (int i = 0; i < TPW; ++i) sacc += acc0[(w * 8 + i) * (NPT + 3) + col];
            ga.gpartials[(int64_t)cx.block() * (NPT + 1) + col] = sacc;
        }
    }
}
