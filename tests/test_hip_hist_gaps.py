"""GPU tests of the state-duration histograms with missed detections (extrack_segment_len_hist_gaps, csrc/xt_hist.h with GAPS;
``P_segment_len(gaps=True)`` / ``len_hist(gaps=True)``) against the numpy restatement of the gap rule
(tests/hist_gap_reference.py (b)) within the histogram bound of tests/test_hip_hist.py, 1e-9 * max(1, N).  Two implementations are compared
on pruned data with ISOLATED gaps only and on runs of gaps only unpruned: inside a run distinct histories tie exactly and, with pruning,
rounding decides their order (tests/hist_gap_reference.py); pruned runs of gaps are checked through what is well defined."""
import numpy as np
import pytest

import hist_gap_reference as HG

pytestmark = pytest.mark.gpu


def _params(vals):
    from extrack_amd.lmfit_compat import Parameters
    p = Parameters()
    for k, v in vals.items():
        p.add(k, value=v)
    return p


def _hist(case, gaps=True):
    """One bucket through ``P_segment_len``; the affine error map, which ``P_segment_len`` has no argument for, through the calls
    ``len_hist`` makes for it."""
    from extrack_amd import histograms as H
    from extrack_amd.engine import TrackSet
    c = case
    if c["slope_offset"] is None:
        return H.P_segment_len(c["Cs"], c["LE"], c["ds"], c["Fs"], c["T"], c["min_l"], c["pBL"], c["isBL"], c["cell_dims"], 1, c["K"], gaps=gaps)[2]
    L = c["Cs"].shape[1]
    ts = TrackSet([c["Cs"]], [c["LE"]], min_len=max(c["min_l"], 1), max_len=L + 1 if c["isBL"] else L, gaps=gaps)
    try:
        model = ts.make_model(None, c["ds"], c["Fs"], c["T"], c["pBL"], c["cell_dims"], 1, 2, slope_offset=c["slope_offset"])
        model.c.min_len = int(c["min_l"])
        return ts.ctx.segment_len_hist(model, 0, c["K"], gaps=True) if gaps else ts.ctx.segment_len_hist(model, 0, c["K"])
    finally:
        ts.close()


# ---- 1. the shapes of the emulation ------------------------------------------------------------------------------------------------------
def test_shared_shapes_against_the_restatement(monkeypatch):
    """tests/test_emul_hist_gaps.py's 32 buckets + the two whose histories cross a 64-bit word; parent buffers in LDS and in global memory."""
    worst = 0.0
    for i, case in enumerate(HG.shared_cases() + HG.word_boundary_cases()):
        assert len(case["Cs"]) <= 50
        ref = HG.reference_of(case)
        monkeypatch.setenv("EXTRACK_HIST_PAR_LDS", "0" if i % 3 == 2 else "1")
        h = _hist(case)
        d = np.abs(h - ref).max()
        print("%-45s |d| %.2e" % (case["name"], d))
        assert h.shape == ref.shape and d < 1e-9 * max(1.0, len(case["Cs"])), (case["name"], d)
        worst = max(worst, d)
    print("worst |d hist|", worst)


# ---- 2. more tracks than workgroups: the block-stride loop -------------------------------------------------------------------------------
def test_bucket_larger_than_the_grid_and_shard_additivity():
    """5000 x 6, 2 states, 12 sequences kept (pruned: isolated gaps only), about a fifth of the interior rows missing and a gap-free track
    in every ten: every workgroup walks from gapped to gap-free tracks and back."""
    from extrack_amd import _lib, engine
    rng = np.random.default_rng(12)
    ds, Fs, T = HG.random_model(2, 12)
    N, L, K = 5000, 6, 12
    Cs = HG.tracks(N, L, 2, ds, Fs, T, rng)
    mask = HG.isolated_mask(N, L, rng, share=0.35)
    mask[::10] = False
    Cs[mask] = np.nan
    LE = np.array([[[0.02]]])
    case = dict(Cs=Cs, LE=LE, eff=LE, slope_offset=None, ds=ds, Fs=Fs, T=T, min_l=3, pBL=0.07, isBL=1, cell_dims=[1.0], K=K, S=2, D=2)
    c = _lib.Context(0)
    try:
        c.upload_bucket(Cs)
        h = c.segment_len_hist(_lib.ModelHandle(ds, Fs, T, engine.p_stay_table(ds, 2, 1, [1.0]), 0.07, 1, 2, 3, L + 1, locerr=[0.02]), 0, K, gaps=True)
        assert c.last_launch_info()["blocks"] < N  # fewer workgroups than tracks
    finally:
        c.close()
    sl = dict(case, Cs=Cs[1230:1270])
    d = np.abs(_hist(sl) - HG.reference_of(sl)).max()
    assert d < 1e-9 * 40, d
    ref = sum(HG.reference_of(dict(case, Cs=Cs[a:a + 500])) for a in range(0, N, 500))
    d_full = np.abs(h - ref).max()
    parts = _hist(dict(case, Cs=Cs[:N // 2])) + _hist(dict(case, Cs=Cs[N // 2:]))
    d_add = np.abs(parts - h).max()
    print("slice |d| %.2e, all 5000 |d| %.2e, two shards |d| %.2e" % (d, d_full, d_add))
    assert d_full < 1e-9 * N and d_add < 1e-9 * max(1.0, h.max())


# ---- 3. len_hist end to end --------------------------------------------------------------------------------------------------------------
VALS3 = dict(D0=1e-4, D1=0.04, D2=0.25, LocErr=0.02, F0=0.3, F1=0.33, F2=0.37, p01=0.071, p02=0.033, p10=0.052, p12=0.047, p20=0.029, p21=0.068,
             pBL=0.1)


def test_len_hist_on_an_insert_gaps_data_set(capsys):
    """Tracks as a gap-closing tracker writes them (positions + frame numbers, missed frames absent) -> ``insert_gaps`` -> buckets of frame
    span 4 / 9 / 17; 3 states, asymmetric rates, isolated missed frames; against (b) driven bucket by bucket."""
    from extrack_amd import gaps, histograms as H, synth
    Tm = np.array([[0.9, 0.07, 0.03], [0.05, 0.9, 0.05], [0.03, 0.07, 0.9]])
    rng = np.random.default_rng(31)
    closed, frames = {}, {}
    for i, (L, N) in enumerate(((4, 60), (9, 50), (17, 40))):
        tr = synth.brownian_tracks(N, L, [0.0, 0.04, 0.25], Tm, [0.3, 0.3, 0.4], seed=70 + i)
        miss = HG.isolated_mask(N, L, rng)
        for n in range(N):
            keep = ~miss[n]
            key = str(int(keep.sum()))
            closed.setdefault(key, []).append(tr[n, keep])
            frames.setdefault(key, []).append(np.nonzero(keep)[0] + 100 + n)
    closed = {k: np.array(v) for k, v in closed.items()}
    frames = {k: np.array(v) for k, v in frames.items()}
    tracks, _, _, _ = gaps.insert_gaps(closed, frames)
    assert sorted(int(k) for k in tracks) == [4, 9, 17] and sum(len(v) for v in tracks.values()) == 150
    assert all(np.isnan(v).any() for v in tracks.values())
    for K in (500, 30):
        h = H.len_hist(tracks, _params(VALS3), 0.02, cell_dims=[1.0, None], nb_states=3, max_nb_states=K, gaps=True)
        capsys.readouterr()
        ref = HG.len_hist_gaps(VALS3, tracks, 0.02, [1.0, None], max_nb_states=K)
        d = np.abs(h - ref).max()
        print("len_hist(gaps=True) max_nb_states %d: |d| %.2e" % (K, d))
        assert h.shape == ref.shape == (17, 3) and d < 1e-9 * 150, (K, d)
    # without the flag the same dict poisons every bucket that holds a missed frame
    plain = H.len_hist(tracks, _params(VALS3), 0.02, cell_dims=[1.0, None], nb_states=3, max_nb_states=30)
    capsys.readouterr()
    assert np.all(np.isnan(plain[:3]))


# ---- 4. gap-free data: the new entry point against the plain one -------------------------------------------------------------------------
def test_gap_free_data_against_the_plain_entry_point():
    """The same operations on the same data; the histograms differ by the order of the fp64 atomic additions into a bin (as two runs of
    the plain entry point do)."""
    worst = 0.0
    for i, case in enumerate(HG.shared_cases()[2:16] + HG.word_boundary_cases()):
        rng = np.random.default_rng(i)
        N, L, D = case["Cs"].shape
        full = HG.tracks(N, L, D, case["ds"], case["Fs"], case["T"], rng)
        LE = case["LE"] if case["LE"].shape[1] == 1 else np.where(np.isnan(case["LE"]), 0.03, case["LE"])
        free = dict(case, Cs=full, LE=LE)
        a, b = _hist(free, gaps=True), _hist(free, gaps=False)
        d = np.abs(a - b).max()
        assert np.all(np.isfinite(b)) and d < 1e-9 * max(1.0, N), (case["name"], d)
        worst = max(worst, d)
    print("gap-free: worst |gaps entry - plain entry| %.2e" % worst)


# ---- 5. pruned runs of gaps: what is well defined ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", (2, 3))
def test_pruned_runs_of_gaps(S, capsys):
    """One 300-frame track with 250 frames missed (hundreds of transition-only steps in a row, histories of 5 / 10 words) beside a bucket of
    30 x 12 with a quarter of the interior rows missing, 50 sequences kept.  The order of the exact ties inside the runs is rounding's, so
    only the shape, finite non-negative values, the empty last row (no segment as long as the longest track) and the total are asserted."""
    from extrack_amd import histograms as H, synth
    from gap_reference import MODELS
    Ds, Tm, Fs = MODELS[S]
    long = synth.brownian_tracks(1, 300, list(Ds), Tm.tolist(), list(Fs), dims=1, seed=8)
    miss = np.zeros(300, bool)
    miss[np.random.default_rng(8).permutation(np.arange(1, 299))[:250]] = True
    long[0, miss] = np.nan
    short = synth.drop_positions(synth.brownian_tracks(30, 12, list(Ds), Tm.tolist(), list(Fs), dims=1, seed=9), 0.25, seed=4)
    vals = dict(LocErr=0.02, pBL=0.1)
    for s in range(S):
        vals["D%d" % s], vals["F%d" % s] = float(Ds[s]), float(Fs[s])
        for t in range(S):
            if s != t:
                vals["p%d%d" % (s, t)] = float(Tm[s, t])
    h = H.len_hist({"12": short, "300": long}, _params(vals), 0.02, cell_dims=[1.0], nb_states=S, max_nb_states=50, gaps=True)
    capsys.readouterr()
    assert h.shape == (300, S) and np.all(np.isfinite(h)) and np.all(h >= 0)
    assert h[-1].sum() == 0.0 and 0 < h.sum() < 30 * 12 + 300


# ---- 6. poison and refusals through the ABI ----------------------------------------------------------------------------------------------
def test_poison_and_refusals_through_the_abi():
    from extrack_amd import _lib, engine
    rng = np.random.default_rng(5)
    ds, Fs, T = HG.random_model(2, 5)
    Cs = HG.tracks(12, 8, 2, ds, Fs, T, rng)
    Cs[3, 2] = Cs[3, 5] = Cs[7, 6] = np.nan
    sig = np.full((12, 8, 1), 0.02)
    sig[np.isnan(Cs[:, :, 0])] = np.nan  # the errors of gap rows are never read
    ps = engine.p_stay_table(ds, 2, 1, [1.0])

    def model(mode=0, nb_substeps=1, max_len=9, S=2, ds=ds, Fs=Fs, T=T, ps=ps):
        return _lib.ModelHandle(ds, Fs, T, ps, 0.07, nb_substeps, 2, 3, max_len, locerr=[0.02], locerr_mode=mode)
    c = _lib.Context(0)
    try:
        def hist(tr, sg, **kw):
            c.clear_buckets()
            c.upload_bucket(tr, sg)
            return c.segment_len_hist(model(mode=0 if sg is None else 1), 0, 10, **kw)
        ref = HG.p_segment_len_gaps(Cs, np.array([[[0.02]]]), ds, Fs, T, 3, 0.07, 1, [1.0], 10)
        for sg in (None, sig):
            assert np.abs(hist(Cs, sg, gaps=True) - ref).max() < 1e-9 * 12
            assert np.all(np.isnan(hist(Cs, sg)))  # without the flag a NaN row still poisons its bucket
        for what in ("partial", "first", "last", "error"):
            bad, sg = Cs.copy(), sig.copy()
            if what == "partial":
                bad[5, 3, 1] = np.nan
            elif what == "first":
                bad[5, 0] = np.nan
            elif what == "last":
                bad[5, -1] = np.nan
            else:
                sg[5, 4] = np.nan
            assert np.all(np.isnan(hist(bad, sg, gaps=True))), what
        assert np.abs(hist(Cs, sig, gaps=True) - ref).max() < 1e-9 * 12  # ... and the context serves the clean bucket again
        for kw in (dict(gaps=True), dict()):  # the refusals of the plain entry point, with its codes
            with pytest.raises(_lib.ExtrackError) as e:
                c.segment_len_hist(model(nb_substeps=2, ps=engine.p_stay_table(ds, 2, 2, [1.0])), 0, 10, **kw)
            assert e.value.code == _lib.E_INVALID
            c.clear_buckets()
            c.upload_bucket(HG.tracks(2, 2100, 2, *HG.random_model(3, 1), rng))  # 2100 frames x 2 bits > 4096
            d3, F3, T3 = HG.random_model(3, 1)
            with pytest.raises(_lib.ExtrackError) as e:
                c.segment_len_hist(model(max_len=2101, ds=d3, Fs=F3, T=T3, ps=engine.p_stay_table(d3, 3, 1, [1.0])), 0, 20, **kw)
            assert e.value.code == _lib.E_UNSUPPORTED
            c.clear_buckets()
            c.upload_bucket(Cs, sig)
    finally:
        c.close()
