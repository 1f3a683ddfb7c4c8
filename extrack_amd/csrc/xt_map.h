// Most-likely state path per track (windowed Viterbi decoding): the kernel body behind extrack_map_states, shared by the HIP kernels
// (extrack_map.hip) and by the CPU-thread emulator used in tests (tests/emul/emul_map.cpp).
//
// What it computes (nothing in the reference does; it sits beside predict_Bs, extrack/tracking.py:792-906; exact statement in
// DESIGN.md section 16): the recursion of xt_kernel.h (nb_substeps 1) with every sum over state sequences replaced
// by a selection -
//   * the group merge of a step keeps the member with the largest weight (lowest member on an exact tie) instead of moment-matching
//     the group, and records which one it kept: the back-pointer of (step, group);
//   * the last position is a max over (old entry Q, new state q) of the terms the likelihood sums; with isBL the state after the last
//     position is summed out (the T*Eend tables), as it is no position of the track;
//   * the states older than the window follow from the back-pointers, newest to oldest.
// For a track of at most frame_len + 1 positions nothing is ever merged and the path is the exact MAP sequence.
//
// GAPS (compile-time, default off: the instantiations without it are unchanged; the definition of xt_kernel.h and DESIGN.md section 18): a
// row whose coordinates are all NaN is a missed detection.  Its step selects and records its back-pointer as any other, the expand applies
// the transition / stay factor alone, the mean stays the selected member's and the stored u becomes d2 + u_selected; the state at the row
// is decoded like any other.  The score's constant counts the observed rows.
//
// Organisation: that of xt_track_body - one thread per group, the S^F live sequences of a track in LDS, staged positions, the bucket
// descriptor table.  Thread g is group g at every step (only the storage slots rotate), so the thread packs its own back-pointers, 2 bits
// each, into a register word and stores one 32-bit word per 16 steps: word w of group g at bp[w * NG + g], in LDS beside the state or in a
// per-(block, track slot) region of global memory.  After the track's last barrier one lane walks the back-pointers (serial, L steps)
// into an LDS row, which the track's threads write out as int8.
#pragma once
#include "xt_kernel.h"

struct XtMapOut {
    int8_t* states;  // [N][L]
    double* score;   // [N] or nullptr
};

struct XtMapArgs {
    const XtMapOut* out;  // [ndesc] outputs matching XtKernelArgs::desc, or nullptr: the single bucket of the two fields below
    int8_t* states;
    double* score;
    uint32_t* bp_ws;      // back-pointer words in global memory, [nblocks][TPB][bp_words][NG], or nullptr: they live in LDS
    int32_t bp_words;     // words per group: xt_map_bp_words(longest track of the launch, F)
    int32_t Lmax;         // longest track of the launch (sizes the LDS state row)
};

#define XT_MAP_BP_PER_WORD 16  // 2-bit back-pointers per 32-bit word (n_states <= 4)
#define XT_MAP_SCAN 16         // candidates per thread in the first level of the final argmax
XT_HD int xt_map_bp_words(int L, int F)
{
    const int n = L - 1 - F;  // merges that decide something: steps t = F .. L-2
    return n > 0 ? (n + XT_MAP_BP_PER_WORD - 1) / XT_MAP_BP_PER_WORD : 1;
}
XT_HD int xt_map_row_doubles(int Lmax) { return (Lmax + 7) / 8; }
XT_HD int xt_map_bp_doubles(int bp_words, int NG) { return (bp_words * NG + 1) / 2; }
// LDS footprint in doubles.  Layout: [tables][sequence state x TPB][staged positions x TPB][state rows x TPB][back-pointer words x TPB]
XT_HD size_t xt_map_lds_doubles(int S, int EP, int NG, int D, int K, int Lmax, int bp_words, bool bp_lds, int tpb)
{
    size_t per = (size_t)xt_region_doubles(EP, D, K) + xt_stage_doubles(D) + xt_map_row_doubles(Lmax);
    if (bp_lds) per += xt_map_bp_doubles(bp_words, NG);
    return (size_t)((xt_tab_doubles(S, S) + 1) & ~1) + per * tpb;
}

// Index of the bucket a block serves (the i of xt_bind_bucket).
XT_HD int xt_map_bucket_index(const XtKernelArgs& a, int block)
{
    int i = 0;
    for (int j = 0; j < a.ndesc - 1; ++j)
        if (block >= a.blk_end[j]) i = j + 1;
    return i;
}

// Reference index (digit c = (i / S^c) % S, c = 0 newest) of the sequence (fused-slot member Q, group g, new state q) at the last position:
// digit i of g is the state of position L - F + i, so the group's digits enter reversed.
XT_HD int xt_map_ref_index(const XtKernelArgs& a, int Q, int g, int q)
{
    const int S = a.S, F = a.F;
    int rev = 0;
    for (int i = 0; i <= F - 2; ++i) rev += ((g / a.pw[i]) % S) * a.pw[F - 2 - i];
    return Q * a.pw[F] + rev * S + q;
}

template <int G_, int D, int K, bool GAPS = false, class Ctx>
XT_HD void xt_map_body(const XtKernelArgs& a, const XtMapArgs& ma, Ctx& cx)
{
    static_assert(G_ >= 2 && G_ <= 4, "2-bit back-pointers");
    int lb, nb;
    const XtBucketDesc b = xt_bind_bucket(a, cx.block(), cx.nblocks(), lb, nb);
    XtMapOut o;
    if (a.desc == nullptr) {
        o.states = ma.states;
        o.score = ma.score;
    } else {
        o = ma.out[xt_map_bucket_index(a, cx.block())];
    }
    constexpr int G = G_;
    const int S = G, E = a.E, EP = a.EP, NG = a.NG, L = b.L, F = a.F;
    const int tid = cx.tid();
    double* smem = cx.smem();

    // ---- model tables -> LDS
    const int ntab = xt_tab_doubles(S, G);
    for (int i = tid; i < ntab; i += cx.nthreads()) smem[i] = xt_blob_ptr(a)[i];
    const double* hdr = smem;
    const double* TAB = smem + XT_BLOB_HDR;
    const double* T64 = TAB + XT_NTAB * S * G;

    const int slot = tid / NG;
    const int g = tid - slot * NG;
    const bool tvalid = slot < a.TPB;
    const int sl = tvalid ? slot : 0;
    const int rdoubles = xt_region_doubles(EP, D, K);
    double* reg = smem + ((ntab + 1) & ~1) + sl * rdoubles;
    double* zm = reg;
    double* mm = zm + EP;
    double* uu = mm + D * EP;
    int* ze = (int*)(uu + K * EP);
    int* red_e = ze + ((EP + 1) & ~1);  // [2] ints: spare (GAPS: missed detections of the track, counted where its rows are staged), NaN-input flag
    double* spos = smem + ((ntab + 1) & ~1) + a.TPB * rdoubles + sl * xt_stage_doubles(D);
    double* ssig = spos + XT_STAGE * D;
    double* rows0 = smem + ((ntab + 1) & ~1) + a.TPB * (rdoubles + xt_stage_doubles(D));
    int8_t* row = (int8_t*)(rows0 + sl * xt_map_row_doubles(ma.Lmax));
    uint32_t* bp = ma.bp_ws ? ma.bp_ws + ((size_t)cx.block() * a.TPB + sl) * ((size_t)ma.bp_words * NG)
                            : (uint32_t*)(rows0 + a.TPB * xt_map_row_doubles(ma.Lmax) + sl * xt_map_bp_doubles(ma.bp_words, NG));

    const int prev = g / a.prev_div;
    const double* T0 = TAB + (0 * S + prev) * G;
    const double* T1 = TAB + (1 * S + prev) * G;
    const double* TD2 = TAB + (4 * S + prev) * G;
    const int stay_from = a.min_len > 2 ? a.min_len : 2;

    const int64_t nbatch = (b.N + a.TPB - 1) / a.TPB;
    if (tvalid && g == 0) red_e[1] = 0;
    if (GAPS && tvalid && g == 0) red_e[0] = 0;
    cx.sync();
    double T0r[G], T1r[G], D2r[G];
    for (int q = 0; q < G; ++q) {
        T0r[q] = T0[q];
        T1r[q] = T1[q];
        D2r[q] = TD2[q];
    }

    for (int64_t batch = lb; batch < nbatch; batch += nb) {
        const int64_t trk = batch * a.TPB + slot;
        const bool act = tvalid && trk < b.N;
        const double* c = b.tracks + (act ? trk : 0) * (int64_t)L * D;
        const double* sg = b.sigma ? b.sigma + (act ? trk : 0) * (int64_t)L * a.KS : nullptr;

        auto stage = [&](int p0) {
            if constexpr (GAPS) {  // (discarded otherwise: the contexts of the plain body need no atomic_add_i32)
                // row by row (as xt_track_body): all coordinates NaN = a gap (counted; its error is copied but never looked at), some = a NaN input
                if (act) {
                    int ng = 0;
                    for (int r = g; r < XT_STAGE; r += NG)
                        if (p0 + r < L) {
                            int nn = 0;
                            for (int d = 0; d < D; ++d) {
                                const double v = c[(p0 + r) * D + d];
                                spos[r * D + d] = v;
                                nn += v != v ? 1 : 0;
                            }
                            const bool gap = nn == D;
                            if ((nn != 0 && !gap) || (gap && (p0 + r == 0 || p0 + r == L - 1))) red_e[1] = 1;
                            ng += gap ? 1 : 0;
                            if (sg)
                                for (int k = 0; k < a.KS; ++k) {
                                    const double v = sg[(p0 + r) * a.KS + k];
                                    ssig[r * a.KS + k] = v;
                                    if (!gap && v != v) red_e[1] = 1;
                                }
                        }
                    if (ng != 0) cx.atomic_add_i32(&red_e[0], ng);
                }
                cx.sync();
                return;
            }
            if (act) {
                for (int i = g; i < XT_STAGE * D; i += NG)
                    if (p0 + i / D < L) {
                        const double v = c[p0 * D + i];
                        spos[i] = v;
                        if (v != v) red_e[1] = 1;  // NaN input: states -1, score NaN
                    }
                if (sg)
                    for (int i = g; i < XT_STAGE * a.KS; i += NG)
                        if (p0 + i / a.KS < L) {
                            const double v = sg[p0 * a.KS + i];
                            ssig[i] = v;
                            if (v != v) red_e[1] = 1;
                        }
            }
            cx.sync();
        };
        auto load_l2 = [&](int pos, double* l2) {
            if (a.locerr_mode == 0) {
                for (int k = 0; k < K; ++k) l2[k] = hdr[k];
            } else {
                for (int k = 0; k < K; ++k) {
                    double s = ssig[(pos & (XT_STAGE - 1)) * a.KS + (a.KS == 1 ? 0 : k)];
                    if (a.locerr_mode == 2) {
                        s = xt_fma(s, hdr[3], hdr[4]);
                        s = s < 1e-6 ? 1e-6 : s;
                    }
                    l2[k] = s * s;
                }
            }
        };

        stage(0);
        // ---- position 0: one digit (initial state) in slot 0, everything else zero weight
        if (act) {
            double l20[K], c0[D];
            load_l2(0, l20);
            for (int d = 0; d < D; ++d) c0[d] = spos[d];
            for (int il = g; il < E; il += NG) {
                const bool live = il < S;
                const int i = xt_skew(il, a.skew);
                zm[i] = live ? hdr[8 + il] : 0.0;
                ze[i] = live ? 0 : XT_EMIN;
                for (int d = 0; d < D; ++d) mm[d * EP + i] = c0[d];
                for (int k = 0; k < K; ++k) uu[k * EP + i] = l20[k];
            }
        }
        cx.sync();

        // ---- positions 1 .. L-2: select inside the group, expand by the new state, integrate position t
        uint32_t bpacc = 0;
        for (int t = 1; t <= L - 2; ++t) {
            if ((t & (XT_STAGE - 1)) == 0) stage(t);
            const int ph = (t - 1) % a.P;
            if (act) {
                const int base = a.base_tab[ph * NG + g];
                const int32_t* off = a.off_tab + ph * G;
                double ct[D], l2t[K];
                for (int d = 0; d < D; ++d) ct[d] = spos[(t & (XT_STAGE - 1)) * D + d];
                const bool gap = GAPS && ct[0] != ct[0];  // staged rows are all-NaN or poison the track: the first coordinate decides
                if (!gap) load_l2(t, l2t);
                const bool stay = t >= stay_from;

                int emax = XT_EMIN;
                for (int q = 0; q < G; ++q) {
                    const int e = ze[xt_skew(base + off[q], a.skew)];
                    emax = e > emax ? e : emax;
                }
                // the member with the largest zm * 2^ze, the lowest one on an exact tie (warm-up: only member 0 can be live)
                int best = 0, bidx = xt_skew(base + off[0], a.skew);
                double ab = xt_ldexp(zm[bidx], ze[bidx] - emax);
                for (int q = 1; q < G; ++q) {
                    const int idx = xt_skew(base + off[q], a.skew);
                    const double aq = xt_ldexp(zm[idx], ze[idx] - emax);
                    if (aq > ab) {
                        ab = aq;
                        best = q;
                        bidx = idx;
                    }
                }
                double mb[D], ub[K];
                for (int d = 0; d < D; ++d) mb[d] = mm[d * EP + bidx];
                for (int k = 0; k < K; ++k) ub[k] = uu[k * EP + bidx];
                if (t >= F) {  // this merge decides the state of position t - F
                    const int kk = t - F;
                    bpacc |= (uint32_t)best << (2 * (kk & (XT_MAP_BP_PER_WORD - 1)));
                    if ((kk & (XT_MAP_BP_PER_WORD - 1)) == XT_MAP_BP_PER_WORD - 1 || t == L - 2) {
                        bp[(kk / XT_MAP_BP_PER_WORD) * NG + g] = bpacc;
                        bpacc = 0;
                    }
                }
                const double Wm = xt_frexp_mant(ab);
                const int We = ab > 0.0 ? emax + xt_frexp_exp(ab) : XT_EMIN;

                double dm[D], dsq = 0.0;
                for (int d = 0; d < D; ++d) {
                    dm[d] = ct[d] - mb[d];
                    dsq = xt_fma(dm[d], dm[d], dsq);
                }
                if (gap) {  // transition-only step (a branch: lanes of a neighbouring track may take the other side at the same t, this is the cheap one)
                    for (int q = 0; q < G; ++q) {
                        const int idx = xt_skew(base + off[q], a.skew);
                        zm[idx] = Wm * (stay ? T1r[q] : T0r[q]);
                        ze[idx] = We;
                        for (int d = 0; d < D; ++d) mm[d * EP + idx] = mb[d];
                        for (int k = 0; k < K; ++k) uu[k * EP + idx] = D2r[q] + ub[k];
                    }
                }
                for (int q = 0; q < (gap ? 0 : G); ++q) {
                    const int idx = xt_skew(base + off[q], a.skew);
                    const double d2 = D2r[q];
                    double quad, gf, tt[K];
                    if (K == 1) {
                        const double s2 = d2 + ub[0];
                        const double r = xt_rcp(l2t[0] + s2);
                        tt[0] = s2 * r;
                        quad = 0.5 * dsq * r;
                        gf = xt_pow_half<D>(r);
                    } else {
                        quad = 0.0;
                        gf = 1.0;
                        for (int d = 0; d < D; ++d) {
                            const double s2 = d2 + ub[d];
                            const double r = xt_rcp(l2t[d] + s2);
                            tt[d] = s2 * r;
                            quad = xt_fma(0.5 * dm[d] * dm[d], r, quad);
                            gf *= r;
                        }
                        gf = sqrt(gf);
                    }
                    double p;
                    int j, n;
                    xt_exp_tab(-quad, p, j, n);
                    const int en = We + n;
                    zm[idx] = (Wm * (stay ? T1r[q] : T0r[q])) * (gf * T64[j]) * p;  // Wm == 0 for an all-zero group, whose We is XT_EMIN
                    ze[idx] = en > XT_EMIN ? en : XT_EMIN;
                    for (int d = 0; d < D; ++d) mm[d * EP + idx] = xt_fma(dm[d], tt[K == 1 ? 0 : d], mb[d]);
                    for (int k = 0; k < K; ++k) uu[k * EP + idx] = l2t[k] * tt[k];
                }
            }
            cx.sync();
        }

        // ---- last position (+ leaving/bleaching term): max over (old entry Q, new state q), normalised as fm * 2^fe
        if (((L - 1) & (XT_STAGE - 1)) == 0) stage(L - 1);
        double fm = 0.0;
        int fe = XT_EMIN, fQ = 0, fq = 0;
        if (act) {
            const int tl = L - 1;
            const int ph = (tl - 1) % a.P;
            const int base = a.base_tab[ph * NG + g];
            const int32_t* off = a.off_tab + ph * G;
            const int vfin = (b.isBL ? 2 : 0) + (tl >= stay_from ? 1 : 0);
            const double* TF = TAB + (vfin * S + prev) * G;
            double cl[D], l2l[K];
            for (int d = 0; d < D; ++d) cl[d] = spos[(tl & (XT_STAGE - 1)) * D + d];
            load_l2(tl, l2l);
            for (int Q = 0; Q < G; ++Q) {
                const int idx = xt_skew(base + off[Q], a.skew);
                const double zq = zm[idx];
                if (!(zq != 0.0)) continue;
                const int eq = ze[idx];
                double dq[D], uq[K], dsq = 0.0;
                for (int d = 0; d < D; ++d) {
                    dq[d] = cl[d] - mm[d * EP + idx];
                    dsq = xt_fma(dq[d], dq[d], dsq);
                }
                for (int k = 0; k < K; ++k) uq[k] = uu[k * EP + idx];
                for (int q = 0; q < G; ++q) {
                    double quad, gf;
                    if (K == 1) {
                        const double r = xt_rcp(D2r[q] + uq[0] + l2l[0]);
                        quad = 0.5 * dsq * r;
                        gf = xt_pow_half<D>(r);
                    } else {
                        quad = 0.0;
                        gf = 1.0;
                        for (int d = 0; d < D; ++d) {
                            const double r = xt_rcp(D2r[q] + uq[d] + l2l[d]);
                            quad = xt_fma(0.5 * dq[d] * dq[d], r, quad);
                            gf *= r;
                        }
                        gf = sqrt(gf);
                    }
                    double p;
                    int j, n;
                    xt_exp_tab(-quad, p, j, n);
                    const double wm = zq * TF[q] * (gf * T64[j]) * p;
                    if (wm > 0.0) {
                        const double m1 = xt_frexp_mant(wm);
                        const int e1 = eq + n + xt_frexp_exp(wm);
                        if (e1 > fe || (e1 == fe && m1 > fm)) {  // (Q, q) ascending = reference index ascending inside a group: first wins a tie
                            fm = m1;
                            fe = e1;
                            fQ = Q;
                            fq = q;
                        }
                    }
                }
            }
        }
        cx.sync();  // all reads of the state are done: zm / ze / mm are reused as the per-group candidates
        int* cand = (int*)mm;   // [NG] fQ * G + fq of the candidate
        int* cgrp = cand + NG;  // [NG] its group
        if (act) {
            zm[g] = fm;
            ze[g] = fe;
            cand[g] = fQ * G + fq;
            cgrp[g] = g;
        }
        cx.sync();
        // argmax over the track's groups in two serial levels (XT_MAP_SCAN candidates per thread, then one lane over the winners): the
        // largest fm * 2^fe, on an exact tie the lowest reference index
        auto scan = [&](int i0, int i1, int stride, double& bm, int& be, int& bg, int& bc) {
            bm = 0.0;
            be = XT_EMIN;
            bg = 0;
            bc = 0;
            for (int i = i0; i < i1; i += stride) {
                const double m1 = zm[i];
                const int e1 = ze[i];
                if (!(m1 > 0.0)) continue;
                bool better = e1 > be || (e1 == be && m1 > bm);
                if (!better && e1 == be && m1 == bm)
                    better = xt_map_ref_index(a, cand[i] / G, cgrp[i], cand[i] % G) < xt_map_ref_index(a, bc / G, bg, bc % G);
                if (better) {
                    bm = m1;
                    be = e1;
                    bg = cgrp[i];
                    bc = cand[i];
                }
            }
        };
        if (NG > XT_MAP_SCAN) {
            double bm;
            int be, bg, bc;
            const bool lead = act && (g % XT_MAP_SCAN) == 0;
            if (lead) {  // reads and writes its own chunk only
                scan(g, g + XT_MAP_SCAN < NG ? g + XT_MAP_SCAN : NG, 1, bm, be, bg, bc);
                zm[g] = bm;
                ze[g] = be;
                cand[g] = bc;
                cgrp[g] = bg;
            }
            cx.sync();
        }
        if (act && g == 0) {
            const bool poisoned = red_e[1] != 0;
            double bm;
            int be, bg, bc;
            scan(0, NG, NG > XT_MAP_SCAN ? XT_MAP_SCAN : 1, bm, be, bg, bc);
            const bool ok = !poisoned && bm > 0.0;
            double llc = b.ll_const;
            if (GAPS) {  // b.ll_const counts every row of the bucket: give back the missed ones' share
                llc += (double)red_e[0] * (0.5 * D * XT_LOG2PI);
                // for the next batch: only this thread reads the two, and no row is staged before the barriers below (the plain body clears
                // its flag after them, where a wavefront of the track that is already staging the next batch can set it first)
                red_e[0] = 0;
                red_e[1] = 0;
            }
            if (o.score) o.score[trk] = poisoned ? NAN : (bm > 0.0 ? log(bm) + (double)be * XT_LN2 + llc : -INFINITY);
            if (!ok) {
                for (int i = 0; i < L; ++i) row[i] = -1;
            } else {
                // the window: new state, the group's digits (digit i = state of position L - F + i), the fused-slot member
                row[L - 1] = (int8_t)(bc % G);
                for (int i = 0; i <= F - 2; ++i)
                    if (L - F + i >= 0) row[L - F + i] = (int8_t)((bg / a.pw[i]) % S);
                if (L - 1 - F >= 0) row[L - 1 - F] = (int8_t)(bc / G);
                // older states: the merge of step t chose, for the group made of the states of positions t-F+1 .. t-1, the state of position t-F
                int gc = bg, last = bc / G;  // one dependent load per step: the state just decoded stays in a register
                for (int t = L - 2; t >= F; --t) {
                    gc = (gc % a.pw[F - 2]) * S + last;
                    const int kk = t - F;
                    last = (int)((bp[(kk / XT_MAP_BP_PER_WORD) * NG + gc] >> (2 * (kk & (XT_MAP_BP_PER_WORD - 1)))) & 3u);
                    row[kk] = (int8_t)last;
                }
            }
        }
        cx.sync();
        if (act)
            for (int i = g; i < L; i += NG) o.states[trk * L + i] = row[i];
        cx.sync();  // the row, the candidates and the back-pointer words are re-used by the next batch
        if (!GAPS && act && g == 0) red_e[1] = 0;
    }
}
