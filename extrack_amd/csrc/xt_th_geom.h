// Launch geometry of the threshold-fusion likelihood path (host only, no HIP calls, no context, no environment: the library and tests/emul
// compile the same functions; tests/test_th_geom_cpu.py).  Two calculations of the launcher in extrack_th.hip:
//  - xt_th_plan_geom: grid, LDS bytes and workspace layout of one plan-kernel launch;
//  - xt_th_apply_geom: which of the five apply variants runs, its tile, workgroup, LDS bytes and grid.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>

#include "xt_th.h"

// Tuning knobs of the context (extrack_create reads them from the environment once).
struct XtThKnobs {
    int force_tt = 0, force_threads = 0, force_single = 0, no_gen_single = 0;  // EXTRACK_TH_TT / _THREADS / _SINGLE / _NO_GEN_SINGLE
    int oversub = 2;                                                           // EXTRACK_TH_OVERSUB
    int stage_in_lds_mode = 0;                                                 // EXTRACK_TH_STAGE_LDS
    int plan_threads = 512, plan_threads_forced = 0;                           // EXTRACK_TH_PLAN_THREADS
    int no_direct = 0;                                                         // EXTRACK_TH_NO_DIRECT
};

struct XtThPlanGeom {
    int grid, ws_lds, wsP, wsE, stP, stE, plan_glb, plan_threads;
    int fits;           // 0: the plan tables do not fit the 160 KiB LDS of a CU
    int64_t ws_stride;  // doubles per workgroup
    size_t lds;         // bytes
    size_t ws_bytes;    // global workspace of the launch (0: the pilot-track state lives in LDS)
};

// learnP / learnE: live parent / expanded sequence counts of the previous plan (+ headroom), 0 = none yet; force_global: the learned LDS
// capacities overflowed in this evaluation
inline XtThPlanGeom xt_th_plan_geom(int S, int G, int capE, int D, int K, int F, int NS, int pcap, int nchunks, int n_cu, int learnP, int learnE,
                                    bool force_global, const XtThKnobs& kn)
{
    XtThPlanGeom g;
    int grid = (int)std::min<int64_t>(nchunks, (int64_t)n_cu * 2);
    // pilot-track state: in LDS when the sequence counts of the previous evaluation (+25 %) fit 64 KiB, else in a global
    // workspace sized for the full plan capacity
    size_t lds = (size_t)xt_th_plan_lds_doubles(S, G, capE, D, K) * sizeof(double);
    bool lds_mode = false;
    g.wsP = g.wsE = capE;
    if (learnE > 0 && !force_global) {
        // ODD per-pilot strides: the pair tests read the pilots' means / stds with lanes = pilot tracks, i.e. at a stride of wsP / wsE
        // doubles - an even stride put the 32 lanes on 16 ... 1 bank pairs (r02 PMC: 59 - 71 % of the plan kernel's LDS cycles were conflicts)
        const int wp = std::min(capE, std::max(S * G, learnP)) | 1, we = std::min(capE, std::max(S * G, learnE)) | 1;
        const size_t need = lds + (size_t)xt_th_ws_doubles(wp, we, D, K, F, NS, S, pcap) * sizeof(double);
        if (need <= 64 * 1024) {
            lds_mode = true;
            lds = need;
            g.wsP = wp;
            g.wsE = we;
        }
    }
    g.ws_lds = lds_mode ? 1 : 0;
    // more expanded sequences per step than the LDS holds plan arrays for (4 states x 3 substeps: 4^4 x 4^3 = 16 384 at the second position):
    // the per-step plan arrays move to the global workspace too
    g.plan_glb = (!lds_mode && capE > XT_TH_MAXCAP) ? 1 : 0;
    if (g.plan_glb) lds = (size_t)xt_th_plan_lds_doubles(S, G, capE, D, K, XT_TH_CMAT_WORDS, true) * sizeof(double);
    g.stP = g.stE = 0;
    if (lds_mode && kn.stage_in_lds_mode) {
        const size_t st = (size_t)pcap * ((size_t)g.wsP * D + (size_t)g.wsE * K) * sizeof(double);
        if (lds + st <= 80 * 1024) {
            g.stP = g.wsP;
            g.stE = g.wsE;
            lds += st;
        }
    }
    if (!lds_mode && learnE > 0 && !force_global) {
        // LDS copy of what the grouping reads (pilot means, stds), sized by the previous evaluation's sequence counts
        const int sp = std::min(capE, learnP) | 1, se = std::min(capE, learnE) | 1;
        const size_t st = (size_t)pcap * ((size_t)sp * D + (size_t)se * K) * sizeof(double);
        if (lds + st <= 120 * 1024) {
            g.stP = sp;
            g.stE = se;
            lds += st;
        }
    }
    g.ws_stride = xt_th_ws_doubles(g.wsP, g.wsE, D, K, F, NS, S, pcap) + (g.plan_glb ? xt_th_plan_glb_doubles(capE) : 0);
    g.ws_bytes = 0;
    if (!lds_mode) {
        // the compatibility bit matrix of a workgroup grows with capE^2 (32 MiB at 16 384): fewer workgroups in flight keep the workspace below ~24 GiB
        const size_t per_wg = (size_t)g.ws_stride * sizeof(double);
        grid = (int)std::max<size_t>(1, std::min<size_t>((size_t)grid, ((size_t)24 << 30) / per_wg));
        g.ws_bytes = (size_t)g.ws_stride * grid * sizeof(double);
    }
    g.grid = grid;
    g.lds = lds;
    g.fits = lds > 160 * 1024 ? 0 : 1;
    // workgroup size: a chunk's plan is a serial walk over its positions; with many live sequences (more than 64 expanded per
    // step at the previous evaluation) the grouping's pair tests dominate a step and are shared by all wavefronts
    g.plan_threads = kn.plan_threads_forced ? kn.plan_threads : (learnE > 64 + 64 / 4 + 2 ? 1024 : kn.plan_threads);
    return g;
}

struct XtThApplyGeom {
    int plan_cap;  // > 0: the whole plan of a chunk in LDS (entries), 0: one step at a time, -1: member lists read from global memory
    int TT, logTT, single_buf;
    int mode;      // 0: general (fewer than 64 tracks per tile), 1: wave-uniform, two state buffers, 2: wave-uniform, one state buffer,
                   // 3: general with one state buffer (more than 64 live sequences), 4: general + the per-sequence matrix of the last position
    int threads, blocks_per_cu, bpc, grid;
    int fits;      // 0: the live state sequences do not fit the 160 KiB LDS of a CU (only plan_cap, TT, single_buf and lds are set then)
    size_t lds;    // bytes
};

// A workgroup serves tiles of TT tracks of one chunk and keeps that chunk's plan in LDS when it is small enough (always, for the usual 2-3
// state models); TT = as many tracks as keep the tile within ~48 KiB of LDS.  KS: sigma dims of the buckets in per-peak error modes, else 0;
// maxG / sumE: largest group count of a step / largest sum of expanded sequences over the steps, over the launch's chunks.
inline XtThApplyGeom xt_th_apply_geom(int S, int G, int D, int K, int KS, int Lmax, int chunk, int nchunks, int nbuckets, int maxG, int sumE, bool want_seq,
                                      int n_cu, const XtThKnobs& kn)
{
    XtThApplyGeom g = {};
    g.plan_cap = (size_t)sumE * 6 + 2 * (size_t)Lmax <= 24 * 1024 ? std::max(sumE, 1) : 0;
    // a step whose member list alone would take more than 32 KiB of LDS (4 states x 3 substeps: 16 384 members at the second position): the
    // general variants read the lists from global memory instead, which leaves the LDS to the state of more tracks per tile
    if (g.plan_cap == 0 && (size_t)maxG * G * 6 > 32 * 1024 && !kn.no_direct) g.plan_cap = -1;
    auto lds_of = [&](int tt, bool single = false) {
        return (size_t)xt_th_apply_lds_doubles(S, G, maxG, tt, D, K, KS, Lmax, g.plan_cap, tt == 64, single) * 8;
    };
    // 64 tracks per tile (wave-uniform scalar path): two state buffers when two such workgroups fit a CU's LDS, one buffer
    // (merged sequences wait in registers) while at most XT_TH_GPW groups fall to a wavefront; else fewer tracks
    int TT = 64;
    int single_buf = 0;
    if (kn.force_tt > 0) TT = kn.force_tt;
    else if (chunk < 48 || lds_of(64) > 76 * 1024) {
        if (chunk >= 48 && maxG <= 16 * XT_TH_GPW && lds_of(64, true) <= 160 * 1024) {
            single_buf = 1;
        } else {
            // more live sequences than the wave-uniform variants hold: the largest tile whose single state buffer fits the
            // LDS and whose groups fit XT_TH_GPW per thread of a 1024-thread workgroup; else the two-buffer general variant
            TT = 0;
            if (chunk >= 48 && !kn.no_gen_single)
                for (int tt = 32; tt >= 8; tt >>= 1)
                    if (lds_of(tt, true) <= 150 * 1024 && maxG <= (1024 / tt) * XT_TH_GPW) {
                        TT = tt;
                        single_buf = 1;
                        break;
                    }
            if (!TT) {
                TT = 32;
                while (TT > 1 && (TT > chunk * 2 || lds_of(TT) > 48 * 1024)) TT >>= 1;
            }
        }
    }
    if (TT == 64 && kn.force_single && maxG <= 16 * XT_TH_GPW) single_buf = 1;
    if (want_seq) {  // extrack_sequence_matrix_th: only the general two-buffer variant writes the per-sequence matrix
        single_buf = 0;
        TT = 32;
        while (TT > 1 && (TT > chunk * 2 || lds_of(TT) > 48 * 1024)) TT >>= 1;
    }
    while (TT > 1 && lds_of(TT, single_buf) > 160 * 1024) TT >>= 1;
    if (TT != 64 && single_buf && maxG > (1024 / TT) * XT_TH_GPW) single_buf = 0;
    const bool uni = TT == 64;
    const size_t lds = lds_of(TT, single_buf);
    g.TT = TT;
    g.single_buf = single_buf;
    g.lds = lds;
    if (lds > 160 * 1024) return g;
    g.fits = 1;
    g.logTT = 0;
    while ((1 << g.logTT) < TT) ++g.logTT;
    int threads = (maxG * TT + 63) / 64 * 64;
    threads = threads > 256 ? 256 : threads;
    threads = threads < TT ? TT : threads;
    if (uni) threads = 64 * std::max(4, std::min(16, maxG));  // one wavefront per live parent sequence of the 64-track tile
    if (!uni && single_buf) threads = 1024;
    int force_threads = kn.force_threads;
    if (!uni && single_buf) force_threads = 0;
    if (uni && single_buf && force_threads > 0 && (force_threads / 64) * XT_TH_GPW < maxG) force_threads = 0;
    if (force_threads > 0 && force_threads % TT == 0) threads = force_threads;
    const int64_t tpc = (chunk + TT - 1) / TT;
    int blocks_per_cu = (int)std::min<size_t>(8, (160 * 1024) / lds);
    blocks_per_cu = std::max(1, std::min(blocks_per_cu, 2048 / threads));
    // several length buckets in one launch: chunks differ in cost by the ratio of their track lengths, so cut them finer
    const int64_t target = (int64_t)n_cu * blocks_per_cu * kn.oversub * (nbuckets > 1 ? 2 : 1);
    int64_t bpc = (target + nchunks - 1) / nchunks;
    bpc = std::max<int64_t>(1, std::min<int64_t>(bpc, tpc));
    g.bpc = (int32_t)bpc;
    g.grid = (int)(nchunks * bpc);
    g.threads = threads;
    g.blocks_per_cu = blocks_per_cu;
    g.mode = want_seq ? 4 : (uni ? (single_buf ? 2 : 1) : (single_buf ? 3 : 0));
    return g;
}
