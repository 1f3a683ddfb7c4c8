// Path choice and launch geometry of the pairwise state posteriors (extrack_predict_pairs*): host only, no HIP calls, no
// context, no environment - the library (extrack_pairs.hip), tests/emul/emul_pairs.cpp and tests/test_pairs_cpu.py compile the same function.
// A pair launch always runs the PAIRS instantiations of the fixed-window body (xt_kernel.h), two states included: xt_ll_pick (xt_ll_geom.h) is
// neither consulted nor changed.  The geometry is xt_geometry's rule - as many tracks as fit 256 threads and a 64 KiB budget, one track may
// take the CU's 160 KiB - with the pair accumulators (xt_pair_doubles) in place of the posterior accumulators (xt_pred_doubles).
#pragma once
#include <stddef.h>

#include "xt_grad_geom.h"
#include "xt_tables.h"

// why no kernel serves the call (all EXTRACK_E_UNSUPPORTED)
enum XtPairRefusal { XT_PAIR_FITS = 0, XT_PAIR_NO_SUBSTEPS, XT_PAIR_NO_STATES, XT_PAIR_NO_GROUPS, XT_PAIR_NO_LDS, XT_PAIR_NO_VARIANT };
static inline const char* xt_pair_refusal_text(int r)
{
    switch (r) {
    case XT_PAIR_NO_SUBSTEPS: return "pair posteriors: built for nb_substeps == 1";
    case XT_PAIR_NO_STATES: return "pair posteriors are built for 2, 3 and 4 states";
    case XT_PAIR_NO_GROUPS: return "pair posteriors: n_states^(frame_len - 1) groups per track do not fit a workgroup (lower frame_len)";
    case XT_PAIR_NO_LDS: return "pair posteriors: the sequence state and pair accumulators of one track exceed the LDS of a CU (lower frame_len)";
    default: return "pair posteriors: kernel variant not built";
    }
}

struct XtPairPick {
    int refusal = XT_PAIR_FITS;
    int tpb = 0, threads = 0;
    size_t lds = 0;
    bool wide = false;  // more than 256 threads: the 1024-thread instantiation
    int sel = 0;        // template selector: members per group = n_states
};

// the domain of xt_pair_kernel_ptr (extrack_pairs.hip)
static inline bool xt_pair_built(int G, int D, int K) { return G >= 2 && G <= 4 && xt_grad_dk_built(D, K); }

static inline size_t xt_pair_lds_bytes(const XtConfig& c, int D, int K, int tpb)
{
    size_t d = (size_t)((xt_tab_doubles(c.S, c.G) + 1) & ~1) + (size_t)tpb * xt_region_doubles(c.EP, D, K);
    d += (size_t)tpb * (xt_pair_doubles(c.S, c.F) + xt_stage_doubles(D));  // pair accumulators + staged positions
    return d * sizeof(double);
}

static inline XtPairPick xt_pair_pick(const XtConfig& c, int D, int K)
{
    XtPairPick p, none;
    if (c.NS != 1) return none.refusal = XT_PAIR_NO_SUBSTEPS, none;
    if (c.S < 2 || c.S > 4) return none.refusal = XT_PAIR_NO_STATES, none;
    if (c.NG > 1024) return none.refusal = XT_PAIR_NO_GROUPS, none;
    const size_t fixed = xt_pair_lds_bytes(c, D, K, 0);
    const size_t per_track = xt_pair_lds_bytes(c, D, K, 1) - fixed;
    const size_t budget = 64 * 1024;
    const int by_threads = c.NG >= 256 ? 1 : 256 / c.NG;
    const int by_lds = budget > fixed + per_track ? (int)((budget - fixed) / per_track) : 1;
    p.tpb = by_threads < by_lds ? by_threads : by_lds;
    if (p.tpb < 1) p.tpb = 1;
    p.threads = (p.tpb * c.NG + 63) / 64 * 64;
    p.lds = xt_pair_lds_bytes(c, D, K, p.tpb);
    if (p.threads > 1024) return none.refusal = XT_PAIR_NO_GROUPS, none;
    if (p.lds > 160 * 1024) return none.refusal = XT_PAIR_NO_LDS, none;
    p.wide = p.threads > 256;
    p.sel = c.G;
    if (!xt_pair_built(p.sel, D, K)) return none.refusal = XT_PAIR_NO_VARIANT, none;
    return p;
}
