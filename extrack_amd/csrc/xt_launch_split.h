// Grid split of one launch over its length buckets (host only, no HIP dependency: the library and tests/emul compile the same function).
//
// A bucket of N tracks of length L is served by blocks of `tracks_per_block` tracks each, nbatch = ceil(N / tracks_per_block) batches.
// It gets blocks in proportion to its work nbatch * (L - 1): ceil(target * w_i / sum w), at least 1 and at most nbatch.  A sum of ceilings
// can exceed `target` by up to nb - 1 blocks, so the split takes a hard upper bound `cap` (a scratch or partial-sum buffer sized for that
// many blocks):
//  - when the ceilings fit in cap, the split is exactly the proportional one above;
//  - otherwise the same rule is applied at the largest target t < target whose split fits in cap, and the cap - grid(t) blocks left are
//    given, in bucket order, to the buckets whose count is the next to rise above t.  The grid is then exactly cap and every bucket keeps
//    between 1 block and the count it had at the full target.
#pragma once
#include <math.h>
#include <stdint.h>

// Blocks of bucket i at target t (the proportional rule, before any cap).
inline int64_t xt_split_bucket_blocks(double t, double w, double wsum, int64_t nbatch)
{
    const int64_t n = (int64_t)ceil(t * w / wsum);
    return n < 1 ? 1 : (n > nbatch ? nbatch : n);
}

// Blocks per bucket in proportion to nbatch_i * (L_i - 1).  Fills blk_end[0 .. nb) with the inclusive prefix of the per-bucket counts and
// returns the grid (== blk_end[nb - 1] <= cap), or -1 when no split exists: nb < 1, cap < nb, tracks_per_block < 1, N_i < 1 or L_i < 2.
inline int64_t xt_split_blocks(double target, int64_t cap, int nb, const int64_t* N, const int32_t* L, int tracks_per_block, int32_t* blk_end)
{
    if (nb < 1 || cap < nb || tracks_per_block < 1) return -1;
    if (cap > INT32_MAX) cap = INT32_MAX;  // blk_end holds int32 block indices
    double wsum = 0.0;
    for (int i = 0; i < nb; ++i) {
        if (N[i] < 1 || L[i] < 2) return -1;
        wsum += (double)((N[i] + tracks_per_block - 1) / tracks_per_block) * (L[i] - 1);
    }
    auto nbatch = [&](int i) { return (N[i] + tracks_per_block - 1) / tracks_per_block; };
    auto blocks = [&](double t, int i) { return xt_split_bucket_blocks(t, (double)nbatch(i) * (L[i] - 1), wsum, nbatch(i)); };
    auto grid_at = [&](double t) {
        int64_t g = 0;
        for (int i = 0; i < nb; ++i) g += blocks(t, i);
        return g;
    };
    int64_t acc = 0;
    if (grid_at(target) <= cap) {
        for (int i = 0; i < nb; ++i) {
            acc += blocks(target, i);
            blk_end[i] = (int32_t)acc;
        }
        return acc;
    }
    // grid_at is non-decreasing in t (correctly rounded products and quotients are monotone), grid_at(0) == nb <= cap < grid_at(target):
    // bisect for the last t whose split fits
    double lo = 0.0, hi = target;
    for (int it = 0; it < 200; ++it) {
        const double mid = 0.5 * (lo + hi);
        if (mid <= lo || mid >= hi) break;
        (grid_at(mid) <= cap ? lo : hi) = mid;
    }
    int64_t rest = cap - grid_at(lo);
    for (int i = 0; i < nb; ++i) {
        int64_t n = blocks(lo, i);
        const int64_t more = blocks(hi, i) - n;
        const int64_t add = more < rest ? more : rest;
        n += add;
        rest -= add;
        acc += n;
        blk_end[i] = (int32_t)acc;
    }
    return acc;  // == cap: sum over i of blocks(hi, i) > cap
}
