"""The state-duration histogram kernel body with GAPS (extrack_amd/csrc/xt_hist.h) run on CPU threads
(tests/emul/emul_hist_gap.cpp) against the numpy restatement of the gap rule (tests/hist_gap_reference.py (b)), within the histogram
bound of tests/test_emul_hist_body.py: 1e-9 * max(1, N)."""
import os
import sys

import numpy as np
import pytest

import hist_gap_reference as HG
from oracle import oracle_np as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul"))


def _run(case, **kw):
    import run_emul_hist_gap as E
    ps = O.p_stay_table(case["ds"], case["S"], 1, case["cell_dims"])
    return E.run_hist(case["Cs"], case["LE"], case["ds"], case["Fs"], case["T"], case["pBL"], case["isBL"], ps, case["min_l"], case["K"],
                      slope_offset=case["slope_offset"], **kw)


def test_emulated_gap_body_on_the_shared_shapes():
    """L = 2; L = 3 with its only interior row missing (the streamed final step alone); L = 4; gaps at p = 1, at L - 2, at p + 1 of a pruned
    step; two adjacent gaps and every interior row missing, unpruned; 2 - 5 states, 1 - 3 dims, one error or one per dim, global / per-peak /
    affine errors with NaN at the gap rows; parent buffers in LDS and in global memory; one and two blocks."""
    worst = 0.0
    seen = set()
    for i, case in enumerate(HG.shared_cases()):
        ref = HG.reference_of(case)
        h = _run(case, nblocks=1 + i % 2, par_lds=i % 3 != 2)
        d = np.abs(h - ref).max()
        assert np.all(np.isfinite(ref)) and ref.sum() > 0
        assert d < 1e-9 * max(1.0, len(case["Cs"])), (case["name"], d)
        worst = max(worst, d)
        seen.add((case["name"].split()[0], case["S"]))
    assert len(seen) == 32  # every shape with every number of states
    print("cases", 32, "worst |d hist|", worst)


def test_emulated_gap_body_history_across_a_word_boundary():
    for i, case in enumerate(HG.word_boundary_cases()):
        h = _run(case, nblocks=1, par_lds=1 - i)
        ref = HG.reference_of(case)
        d = np.abs(h - ref).max()
        assert d < 1e-9 * len(case["Cs"]), (case["name"], d)


def _walk_case(layout):
    """Four 9-frame tracks for ONE block: gapped, gap-free, (to be poisoned), gapped.  Pruned, isolated gaps."""
    rng = np.random.default_rng(77)
    ds, Fs, T = HG.random_model(3, 77)
    N, L, D = 4, 9, 2
    mask = np.zeros((N, L), bool)
    mask[0, [1, 4, 7]] = True
    mask[3, [2, 5]] = True
    Cs = HG.tracks(N, L, D, ds, Fs, T, rng)
    Cs[mask] = np.nan
    LE, so, eff = HG.error_layout(layout, 2 if layout == "peak" else 1, N, L, mask, rng)
    return dict(name="walk " + layout, Cs=Cs, mask=mask, LE=LE, slope_offset=so, eff=eff, ds=ds, Fs=Fs, T=T, pBL=0.07, isBL=1, min_l=3, K=7,
                cell_dims=[1.0], S=3, D=D)


@pytest.mark.parametrize("layout", ("global", "peak", "affine"))
def test_one_block_walks_gapped_gap_free_poisoned_gapped(layout):
    """The per-track state of the block-stride loop (poison flag, gap flags read from the staged rows) does not leak from one track into the
    next: one block over the four tracks equals the restatement, equals the sum over four one-track launches, and a poisoned third track
    turns the block's histogram into NaN whichever rule it breaks."""
    case = _walk_case(layout)
    ref = HG.reference_of(case)
    h = _run(case, nblocks=1, par_lds=1)
    assert np.abs(h - ref).max() < 1e-9 * 4
    single = sum(_run(dict(case, Cs=case["Cs"][n:n + 1], LE=case["LE"][n:n + 1] if case["LE"].shape[0] > 1 else case["LE"]), nblocks=1, par_lds=0)
                 for n in range(4))
    assert np.abs(h - single).max() < 1e-12
    kinds = ["partial", "first", "last"] + (["error"] if layout != "global" else [])
    for what in kinds:
        Cs, LE = case["Cs"].copy(), case["LE"].copy()
        if what == "partial":
            Cs[2, 3, 1] = np.nan
        elif what == "first":
            Cs[2, 0] = np.nan
        elif what == "last":
            Cs[2, -1] = np.nan
        else:
            LE[2, 4] = np.nan  # a NaN error at an observed row
        bad = dict(case, Cs=Cs, LE=LE, eff=case["eff"] if what != "error" else np.where(np.isnan(LE), np.nan, case["eff"]))
        assert np.all(np.isnan(HG.reference_of(bad))), what
        assert np.all(np.isnan(_run(bad, nblocks=1, par_lds=1))), what
        two = _run(bad, nblocks=2, par_lds=1)  # block 0: tracks 0 and 2, block 1: tracks 1 and 3
        assert np.all(np.isnan(two)), what


def test_gap_free_data_gives_the_plain_body_up_to_the_order_of_the_atomic_additions_and_gaps_poison_the_plain_body():
    """On gap-free data the GAPS body performs the operations of the plain body, so every sequence gets the same weight bit for bit; what a
    histogram shows of that is limited by the fp64 atomic additions into a bin, whose order is free (two runs of the PLAIN body differ in the
    last bits too).  A bin is a sum of at most n = N * K * S non-negative weights; two summation orders differ by at most 2 (n - 1) 2^-53
    times the sum.  That bound is asserted - for GAPS against plain and, to show it is the atomics, for plain against plain."""
    for i, case in enumerate(HG.shared_cases()[2:14:2] + HG.word_boundary_cases()[:1]):
        rng = np.random.default_rng(i)
        N, L, D = case["Cs"].shape
        full = HG.tracks(N, L, D, case["ds"], case["Fs"], case["T"], rng)
        LE = case["LE"] if case["LE"].shape[1] == 1 else np.where(np.isnan(case["LE"]), 0.03, case["LE"])
        free = dict(case, Cs=full, LE=LE)
        a = _run(free, nblocks=2, par_lds=i % 2, gaps=True)
        b = _run(free, nblocks=2, par_lds=i % 2, gaps=False)
        b2 = _run(free, nblocks=2, par_lds=i % 2, gaps=False)
        bound = 2.0 * (N * max(case["K"], case["S"] ** 2) * case["S"] - 1) * 2.0 ** -53 * np.maximum(b, b2)
        assert np.all(np.isfinite(a)) and np.all(np.abs(a - b) <= bound) and np.all(np.abs(b2 - b) <= bound), (case["name"], np.abs(a - b).max())
        if case["mask"].any():
            assert np.all(np.isnan(_run(case, nblocks=1, par_lds=1, gaps=False))), case["name"]  # without the flag a NaN poisons its bucket
