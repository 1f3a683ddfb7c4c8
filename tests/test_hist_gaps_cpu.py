"""State-duration histograms with missed detections, CPU part: the two references of tests/hist_gap_reference.py
against each other and against the unchanged numpy oracle, and the host-side validation of ``P_segment_len`` / ``len_hist`` with
``gaps=True``.  No GPU."""
import numpy as np
import pytest

import hist_gap_reference as HG
from oracle import oracle_hist as OH

# (b) on gap-free data performs the oracle's operations except for the association of the child variance (d2 + l2 s2 / den instead of
# (d2 l2 + d2 s2 + l2 s2) / den): a few ulp per step on log-weights of magnitude up to a few hundred (ulp 5.7e-14), over <= 30 steps, on
# normalised weights <= 1 summed over N tracks: 1e-12 per track.  Measured: <= 7.1e-15 on a chunk of 7 tracks.
GAP_FREE_TOL = 1e-12
# (b) against the limit reference (a) at LAMBDA = 1e7: the bias of a finite error falls as 1 / LAMBDA^2 (~1e-14 relative at variances of
# 1e-3 .. 1e-1), the rest is rounding noise of log-weights shifted by ~17 D per gap.  Ten times the worst difference of a chunk's histogram
# measured on the case set below (8.7e-15; 5.2e-14 was measured on the larger set the feature was prepared with).
LIMIT_TOL = 8.7e-14


def _limit_cases():
    """(name, Cs, eff, ds, Fs, T, min_l, pBL, isBL, K).  Unpruned (K >= S^L) with runs of gaps and a track with every interior row missing;
    pruned with isolated gaps only; at most 4 gaps per track, L <= 30."""
    out = []
    # unpruned: 2 states L <= 9, 3 states L <= 7
    for S, L, D, per_peak, seed in ((2, 9, 2, False, 1), (2, 6, 1, True, 2), (3, 7, 2, True, 3), (3, 6, 1, False, 4), (2, 8, 2, True, 5)):
        rng = np.random.default_rng(300 + seed)
        ds, Fs, T = HG.random_model(S, 200 + seed)
        N = 6
        Cs = HG.tracks(N, L, D, ds, Fs, T, rng)
        mask = np.zeros((N, L), bool)
        mask[0, 1:3] = True                      # a run of two
        mask[1, 2:5] = True                      # a run of three
        mask[2, 1:1 + min(L - 2, 4)] = True      # every interior row (up to the 4 gaps a track may hold)
        mask[3, 1] = mask[3, L - 2] = True
        mask[4, L - 3:L - 1] = True              # a run that ends at L - 2
        if L - 2 > 4:
            mask[2, 5:] = False
        Cs[mask] = np.nan
        eff = rng.uniform(0.01, 0.05, (N, L, D if seed % 2 else 1)) if per_peak else np.array([[[0.025]]])
        out.append(("unpruned S=%d L=%d" % (S, L), Cs, eff, ds, Fs, T, 2 + seed % 2, 0.08, seed % 2, S ** L))
    # a short track whose interior rows are ALL missing
    for S, L, seed in ((2, 6, 6), (3, 5, 7)):
        rng = np.random.default_rng(300 + seed)
        ds, Fs, T = HG.random_model(S, 200 + seed)
        Cs = HG.tracks(4, L, 2, ds, Fs, T, rng)
        Cs[:, 1:-1] = np.nan
        out.append(("all interior S=%d L=%d" % (S, L), Cs, np.array([[[0.02]]]), ds, Fs, T, 3, 0.08, 1, S ** L))
    # pruned, isolated gaps
    for S, L, D, K, per_peak, seed in ((2, 30, 1, 30, False, 8), (2, 20, 2, 100, True, 9), (3, 12, 2, 60, False, 10), (3, 25, 1, 1000, True, 11),
                                       (2, 13, 2, 50, False, 12), (3, 17, 2, 200, True, 13)):
        rng = np.random.default_rng(300 + seed)
        ds, Fs, T = HG.random_model(S, 200 + seed)
        N = 8
        Cs = HG.tracks(N, L, D, ds, Fs, T, rng)
        mask = HG.isolated_mask(N, L, rng, share=0.3, max_gaps=4)
        mask[0] = False
        mask[0, 1] = mask[0, L - 2] = True
        Cs[mask] = np.nan
        eff = rng.uniform(0.01, 0.05, (N, L, 1)) if per_peak else np.array([[[0.02]]])
        out.append(("pruned S=%d L=%d K=%d" % (S, L, K), Cs, eff, ds, Fs, T, 3, 0.08, seed % 2, K))
    return out


def test_restatement_equals_the_oracle_on_gap_free_data():
    worst = 0.0
    for S, L, D, K, kd, seed in ((2, 2, 1, 5, 1, 0), (2, 12, 2, 20, 1, 1), (3, 9, 2, 40, 2, 2), (4, 7, 3, 1000, 1, 3), (2, 30, 1, 60, 1, 4), (3, 17, 3, 9, 3, 5)):
        rng = np.random.default_rng(seed)
        ds, Fs, T = HG.random_model(S, 10 + seed)
        N = 7
        Cs = HG.tracks(N, L, D, ds, Fs, T, rng)
        LE = rng.uniform(0.01, 0.05, (N, L, kd)) if seed % 2 else np.array([0.02, 0.03, 0.04][:kd])[None, None]
        ref = OH.p_segment_len(Cs, LE, ds, Fs, T, 3, 0.1, seed % 2, [1.0], 1, K)
        got = HG.p_segment_len_gaps(Cs, LE, ds, Fs, T, 3, 0.1, seed % 2, [1.0], K)
        d = np.abs(got - ref).max()
        print("gap-free S=%d L=%d K=%d: |d| %.2e" % (S, L, K, d))
        assert got.shape == ref.shape and d <= GAP_FREE_TOL * N, (S, L, d)
        worst = max(worst, d)
    print("worst", worst)


def test_restatement_is_the_limit_of_a_large_error_at_the_gap_rows():
    worst = 0.0
    for name, Cs, eff, ds, Fs, T, min_l, pBL, isBL, K in _limit_cases():
        assert Cs.shape[1] <= 30 and np.isnan(Cs[:, :, 0]).sum(1).max() <= 4
        a = HG.limit_reference(Cs, eff, ds, Fs, T, min_l, pBL, isBL, [1.0], K)
        b = HG.p_segment_len_gaps(Cs, eff, ds, Fs, T, min_l, pBL, isBL, [1.0], K)
        d = np.abs(a - b).max()
        print("%s: |(a) - (b)| %.2e  (sum %.3f)" % (name, d, b.sum()))
        assert np.all(np.isfinite(b)) and np.all(b >= 0)
        assert d <= LIMIT_TOL, (name, d)
        worst = max(worst, d)
    print("worst", worst)


def test_restatement_poisons_like_the_abi():
    rng = np.random.default_rng(3)
    ds, Fs, T = HG.random_model(2, 1)
    Cs = HG.tracks(5, 6, 2, ds, Fs, T, rng)
    LE = np.full((5, 6, 1), 0.02)
    ok = Cs.copy()
    ok[1, 2] = np.nan
    LE[1, 2] = np.nan  # the error of a gap row is never read
    assert np.all(np.isfinite(HG.p_segment_len_gaps(ok, LE, ds, Fs, T, 3, 0.1, 1, [1.0], 10)))
    for what in ("partial", "first", "last", "error"):
        bad, le = ok.copy(), LE.copy()
        if what == "partial":
            bad[3, 2, 1] = np.nan
        elif what == "first":
            bad[3, 0] = np.nan
        elif what == "last":
            bad[3, -1] = np.nan
        else:
            le[3, 4] = np.nan
        assert np.all(np.isnan(HG.p_segment_len_gaps(bad, le, ds, Fs, T, 3, 0.1, 1, [1.0], 10))), what


# ---- host validation: raised before any device call -------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    from extrack_amd import _lib

    def boom(*a, **k):
        raise AssertionError("a device context was opened")
    monkeypatch.setattr(_lib, "Context", boom)


def _params():
    from extrack_amd.lmfit_compat import Parameters
    p = Parameters()
    for k, v in dict(D0=1e-3, D1=0.25, LocErr=0.02, F0=0.6, F1=0.4, p01=0.1, p10=0.12, pBL=0.1).items():
        p.add(k, value=v)
    return p


def test_gap_rules_are_checked_on_the_host(no_device):
    from extrack_amd import histograms as H
    rng = np.random.default_rng(0)
    ds, Fs, T = HG.random_model(2, 0)
    Cs = HG.tracks(6, 7, 2, ds, Fs, T, rng)
    LE = np.array([[[0.02]]])
    for what, (n, t, d), msg in (("first", (2, 0, slice(None)), "first and last"), ("last", (4, 6, slice(None)), "first and last"),
                                 ("partial", (3, 2, 1), "finite or NaN in all")):
        bad = Cs.copy()
        bad[n, t, d] = np.nan
        with pytest.raises(ValueError, match=r"gaps=True: bucket 0 \(length 7\), track %d: .*%s" % (n, msg)):
            H.P_segment_len(bad, LE, ds, Fs, T, gaps=True)
        with pytest.raises(ValueError, match=r"gaps=True: bucket 1 \(length 7\), track %d: .*%s" % (n, msg)):
            H.len_hist({"5": Cs[:, :5], "7": bad}, _params(), 0.02, cell_dims=[1.0], gaps=True)
    with pytest.raises(NotImplementedError):
        H.P_segment_len(Cs, LE, ds, Fs, T, nb_substeps=2, gaps=True)
    with pytest.raises(NotImplementedError):
        H.len_hist({"7": Cs}, _params(), 0.02, cell_dims=[1.0], nb_substeps=2, gaps=True)
    with pytest.raises(NotImplementedError, match="comm must be None"):
        H.len_hist({"7": Cs}, _params(), 0.02, cell_dims=[1.0], gaps=True, comm=object())


def test_the_new_symbol_is_declared_exported_and_bound():
    import os
    from extrack_amd import _lib
    assert "extrack_segment_len_hist_gaps" in _lib.EXPORTS
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "extrack_hip.h")).read()
    assert "int extrack_segment_len_hist_gaps(extrack_ctx* ctx, const extrack_model* model, int32_t bucket_id, int32_t max_nb_states, double* hist);" in hdr
