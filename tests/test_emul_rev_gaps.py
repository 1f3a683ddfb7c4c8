"""CPU checks of the gap-aware reverse-mode gradient: ``xt_rev_body<.., GAPS = true>`` on CPU threads
(tests/emul/emul_rev_gap.cpp), with one and with two exchange buffers, all buckets of ``gap_reference.make_case`` in one emulated launch, against
Richardson differences of the reference built from the unchanged oracle (tests/grad_gap_reference.py; cases and stored arrays:
tests/rev_gap_reference.py) and against the gap instantiation of xt_gradr.h on the same inputs; the flag on gap-free data; the poison rules; the
per-peak error of a gap row.
Tolerances: LL as tests/test_hip_gaps.py (per track rtol 1e-13 / atol 1e-10, total 1e-12 relative); gradient by
``test_grad_edges_cpu.check_gradient`` with the reference's own condition asserted first; body against body by
``test_emul_grad_gaps.assert_bodies_agree`` (1e-9 |y| + 1e-12)."""
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul"))

import gap_reference as R
import grad_gap_reference as GR
import rev_gap_reference as RG
from oracle import oracle_np as O
from test_emul_grad_gaps import assert_bodies_agree, emulate as emulate_forward
from test_grad_edges_cpu import check_gradient

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def emulate(case, nbuf, dirs, gaps=True, buckets=None, sig=None, blocks=2):
    """(LL [sum N], sum LL, gradient) in upload order (short -> long); launched longest first."""
    import run_emul_rev_gap as E
    Ds, Tm, Fs = R.MODELS[case["S"]]
    ds = np.sqrt(2 * Ds * R.DT)
    bk = case["buckets"] if buckets is None else buckets
    sg = case["sig"] if sig is None else sig
    order = list(range(len(bk)))[::-1]
    ll, tot, g = E.run_rev_gap(nbuf, [bk[i] for i in order], case["le"] if case["le"] is not None else [0.0], ds, Fs, Tm, R.PBL,
                               O.p_stay_table(ds, case["S"], 1, R.CELL), case["F"], R.MIN_LEN, max(b.shape[1] for b in bk), [d[1] for d in dirs],
                               sigmas=None if sg is None else [sg[i] for i in order], slope_offset=case["slope_offset"], gaps=gaps,
                               blocks_per_bucket=[blocks] * len(bk))
    lls = [None] * len(bk)
    for j, i in enumerate(order):
        lls[i] = ll[j]
    return np.concatenate(lls), tot, g


def same_bits(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal([a[1]], [b[1]], equal_nan=True) and np.array_equal(a[2], b[2], equal_nan=True)


@pytest.mark.parametrize("S,D,layout,F", RG.CASES)
def test_emulated_rev_gap_body(S, D, layout, F):
    """The eight cases with one and with two exchange buffers: LL per track and in total, the gradient against the reference, and everything
    against the gap instantiation of xt_gradr.h (4 directions per pass)."""
    key = (S, D, layout, F)
    case = R.make_case(*key)
    assert any(m.any() for m in case["masks"])
    ref = GR.reference(case, key)
    RG.assert_golden_is_current(case, key, ref)  # what the GPU test reads
    assert np.all(np.isfinite(ref["ll"]))
    GR.assert_condition("%s sum" % (key,), ref["gfd"], ref["gest"])
    fwd = emulate_forward(case, 4, ref["dirs"])[:3]
    for nbuf in (1, 2):
        tag = "%s nbuf %d" % (key, nbuf)
        ll, tot, g = emulate(case, nbuf, ref["dirs"])
        np.testing.assert_allclose(ll, ref["ll"], rtol=1e-13, atol=1e-10, err_msg=tag + " LL")
        assert abs(tot - ref["ll"].sum()) <= 1e-12 * abs(ref["ll"].sum()), (tag, tot, ref["ll"].sum())
        check_gradient(tag + " sum", ref["dirs"], g, ref["gfd"], ref["gest"])
        assert_bodies_agree((ll, tot, g), fwd)


@pytest.mark.parametrize("nbuf", [1, 2])
def test_block_count_does_not_change_the_per_track_values(nbuf):
    """One block per bucket walks several batches and reuses its log region and its gap counter; the per-track LL has the bits of the two-block launch."""
    case = R.make_case(3, 2, "global1", 5)
    dirs = GR.directions(case)
    a, b = emulate(case, nbuf, dirs, blocks=1), emulate(case, nbuf, dirs, blocks=2)
    assert np.all(np.isfinite(a[0])) and np.array_equal(a[0], b[0])
    assert_bodies_agree(a, b)


@pytest.mark.parametrize("nbuf", [1, 2])
def test_flag_on_gap_free_data_is_the_plain_body(nbuf):
    """Gap-free data: the flag changes nothing - value and gradient bit for bit (the same operations in the same order).
    One exception, which is the plain body's: with L = 2 it resets the exponent of the track total without a barrier before the atomic maximum
    of the last position (see the note in xt_rev.h), so on CPU threads the scale 2^fe of log(sw) + fe ln 2 can differ from run to run: a
    power of two, which changes the rounding of that track's LL (a few ulp) and not a bit of the gradient.  The flag-on body resets behind a
    barrier.  Hence: gradient and the LL of every track with L >= 3 bit for bit; the L = 2 tracks to 4 ulp, the total to 1e-14 relative."""
    from extrack_amd import synth
    case = R.make_case(3, 2, "global1", 3)
    Ds, Tm, Fs = R.MODELS[3]
    full = [synth.brownian_tracks(len(b), b.shape[1], list(Ds), Tm.tolist(), list(Fs), dt=R.DT, dims=2, seed=3 + i) for i, b in enumerate(case["buckets"])]
    dirs = GR.directions(case)
    a = emulate(case, nbuf, dirs, gaps=True, buckets=full)
    b = emulate(case, nbuf, dirs, gaps=False, buckets=full)
    assert np.all(np.isfinite(a[0])) and np.all(np.isfinite(a[2]))
    n2 = len(case["buckets"][0])
    assert case["buckets"][0].shape[1] == 2 and case["buckets"][1].shape[1] == 3
    assert np.array_equal(a[0][n2:], b[0][n2:]) and np.array_equal(a[2], b[2])
    assert np.all(np.abs(a[0][:n2] - b[0][:n2]) <= 4 * np.spacing(np.abs(b[0][:n2]))) and abs(a[1] - b[1]) <= 1e-14 * abs(b[1])
    assert np.array_equal(emulate(case, nbuf, dirs, gaps=True, buckets=full)[0], a[0])  # the flag-on body gives the same bits every time


@pytest.mark.parametrize("nbuf", [1, 2])
def test_poison_rules(nbuf):
    """A row with some NaN coordinates, a NaN first row, a NaN last row and a NaN error at an observed row give their track a NaN LL and the
    launch a NaN total and gradient (reverse mode sums its adjoints across tracks); every other track keeps its bits."""
    case = R.make_case(2, 2, "peak", 3)
    dirs = GR.directions(case)
    clean = emulate(case, nbuf, dirs)
    assert np.all(np.isfinite(clean[0])) and np.isfinite(clean[1]) and np.all(np.isfinite(clean[2]))
    r0 = np.concatenate([[0], np.cumsum([len(b) for b in case["buckets"]])])
    obs = int(np.nonzero(~case["masks"][3][7])[0][1])  # an observed interior row of track 7 of the L = 14 bucket
    for what, (bi, n, t) in dict(partial=(3, 6, 5), first=(3, 9, 0), last=(4, 5, -1), error=(3, 7, obs)).items():
        dirty, sig = [b.copy() for b in case["buckets"]], [s.copy() for s in case["sig"]]
        if what == "partial":
            dirty[bi][n, t, 1] = np.nan
        elif what == "error":
            sig[bi][n, t, 0] = np.nan
        else:
            dirty[bi][n, t] = np.nan
        got = emulate(case, nbuf, dirs, buckets=dirty, sig=sig)
        bad = np.zeros(r0[-1], bool)
        bad[r0[bi] + n] = True
        assert np.all(np.isnan(got[0][bad])) and np.isnan(got[1]) and np.all(np.isnan(got[2])), what
        assert np.array_equal(got[0][~bad], clean[0][~bad]), what


@pytest.mark.parametrize("nbuf,layout", [(1, "affine"), (2, "affine"), (2, "peak")])
def test_error_of_a_gap_row_is_never_read(nbuf, layout):
    """Per-peak errors: NaN and 123.0 at the gap rows give the same bits (the affine layout: slope and offset directions included)."""
    case = R.make_case(3, 2, layout, 4)
    dirs = GR.directions(case)
    res = []
    for fill in (np.nan, 123.0):
        sig = [s.copy() for s in case["sig"]]
        for s, m in zip(sig, case["masks"]):
            s[m] = fill
        res.append(emulate(case, nbuf, dirs, sig=sig))
    assert np.all(np.isfinite(res[0][0])) and np.all(np.isfinite(res[0][2]))
    assert same_bits(res[0], res[1])
