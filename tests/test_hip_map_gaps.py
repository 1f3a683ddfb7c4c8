"""GPU tests of the most-likely state path with missed detections (extrack_map_states_gaps, csrc/xt_map.h with GAPS;
``predict_states(gaps=True)``), through the C ABI and ``predict_states``, against the numpy restatement of the gap rule
(tests/map_gap_reference.py) under its path comparison rule: every score within 1e-10 (the tolerance of tests/test_hip_map.py), the
returned path's own density (prior + dense gap-aware logdens) within 2e-10 of the returned score, states equal wherever the
restatement's margin is >= 1e-6, and at most 4 of a case's 64 tracks - each with a run of two or more gap rows - left out.
Inputs: ``gap_reference.make_case`` at seed 0."""
import numpy as np
import pytest

import gap_reference as G
import map_gap_reference as MG

pytestmark = pytest.mark.gpu
SCORE_TOL = 1e-10


@pytest.fixture(scope="module")
def ctx():
    from extrack_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _model(S, F, min_len, max_len, le=None, mode=0, slope_offset=None, nb_substeps=1, models=G.MODELS):
    from extrack_amd import _lib, engine
    Ds, Tm, Fs = models[S]
    ds = np.sqrt(2 * Ds * G.DT)
    so = slope_offset or (0.0, 0.0)
    return _lib.ModelHandle(ds, Fs, Tm, engine.p_stay_table(ds, S, nb_substeps, G.CELL), G.PBL, nb_substeps, F, min_len, max_len, locerr=le,
                            locerr_mode=mode, slope=so[0], offset=so[1])


def _case_model(case):
    mode = 0 if case["sig"] is None else (2 if case["slope_offset"] is not None else 1)
    return _model(case["S"], case["F"], G.MIN_LEN, max(b.shape[1] for b in case["buckets"]), le=case["le"], mode=mode,
                  slope_offset=case["slope_offset"])


def _upload(ctx, case, buckets=None, sigmas=None):
    ctx.clear_buckets()
    sg = case["sig"] if sigmas is None else sigmas
    for i, b in enumerate(case["buckets"] if buckets is None else buckets):
        ctx.upload_bucket(b, None if sg is None else sg[i])


def _reference(case):
    Ds, Tm, Fs = G.MODELS[case["S"]]
    ds = np.sqrt(2 * Ds * G.DT)
    Lmax = max(b.shape[1] for b in case["buckets"])
    refs, models = [], []
    for b, eff in zip(case["buckets"], case["eff"]):
        isBL = int(b.shape[1] != Lmax)
        refs.append(MG.map_path(b, eff, ds, Fs, Tm, G.PBL, isBL, G.CELL, case["F"], G.MIN_LEN))
        models.append((ds, Fs, Tm, G.PBL, isBL, G.CELL, G.MIN_LEN))
    return refs, models


def _check_case(ctx, case, what, only=None):
    refs, models = _reference(case)
    model = _case_model(case)
    left = []
    for i, (b, eff) in enumerate(zip(case["buckets"], case["eff"])):
        if only is not None and i != only:
            left.append(np.zeros(len(b), bool))
            continue
        st, sc = ctx.map_states(model, i, scores=True, gaps=True)
        left.append(MG.compare_paths(st, sc, refs[i], b, eff, models[i], SCORE_TOL, "%s bucket %d" % (what, i)))
    MG.check_exclusions(left, case["masks"], what=what)


# ---- 1. the shared cases through the C ABI ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", G.LAYOUTS)
@pytest.mark.parametrize("D", (1, 2, 3))
@pytest.mark.parametrize("S", (2, 3, 4))
def test_gap_paths_against_restatement(ctx, S, D, layout):
    """L = 2, 3 (its only interior row missing), frame_len + 1, 14 (gaps at t = 1, L - 2, a run longer than the window, every interior row),
    40 (gaps across the staging boundary); min_len 3, the longest bucket isBL = 0; frame_len 3 and 5."""
    for F in (3, 5):
        case = G.make_case(S, D, layout, F)
        _upload(ctx, case)
        _check_case(ctx, case, "S=%d D=%d %s F=%d" % (S, D, layout, F))


# ---- 2. gap-free buckets: the same bits as extrack_map_states -----------------------------------------------------------------------
@pytest.mark.parametrize("S,D,layout,F", [(3, 2, "global1", 6), (2, 2, "globalD", 6), (4, 3, "peak", 4), (2, 1, "affine", 5)])
def test_gap_free_buckets_are_bit_identical_to_the_plain_entry_point(ctx, S, D, layout, F):
    from extrack_amd import synth
    case = G.make_case(S, D, layout, F)
    Ds, Tm, Fs = G.MODELS[S]
    full = [synth.brownian_tracks(len(b), b.shape[1], list(Ds), Tm.tolist(), list(Fs), dt=G.DT, dims=D, seed=3 + i) for i, b in enumerate(case["buckets"])]
    sig = None if case["sig"] is None else [np.where(np.isnan(s) | (s > 1), 0.03, s) for s in case["sig"]]
    _upload(ctx, case, full, sig)
    model = _case_model(case)
    for i in range(len(full)):
        s0, c0 = ctx.map_states(model, i, scores=True)
        s1, c1 = ctx.map_states(model, i, scores=True, gaps=True)
        assert np.array_equal(s0, s1) and np.array_equal(c0, c1) and not np.any(s0 < 0) and np.all(np.isfinite(c0))


# ---- 3. the poison rules through the ABI --------------------------------------------------------------------------------------------
def test_poison_rules_through_the_abi(ctx):
    case = G.make_case(2, 2, "peak", 4)
    model = _case_model(case)
    _upload(ctx, case)
    clean = [ctx.map_states(model, i, scores=True, gaps=True) for i in range(5)]
    dirty = [b.copy() for b in case["buckets"]]
    sig = [s.copy() for s in case["sig"]]
    dirty[3][6, 5, 1] = np.nan   # a row with one NaN coordinate
    dirty[3][9, 0] = np.nan      # NaN first row
    dirty[4][5, -1] = np.nan     # NaN last row
    obs = np.nonzero(~case["masks"][3][12])[0]
    sig[3][12, obs[1], 1] = np.nan  # NaN error at an observed row
    for s, m in zip(sig, case["masks"]):
        s[m] = np.nan               # ... and at every gap row: never read
    _upload(ctx, case, dirty, sig)
    bad = {3: [6, 9, 12], 4: [5]}
    for i in range(5):
        st, sc = ctx.map_states(model, i, scores=True, gaps=True)
        keep = np.ones(len(dirty[i]), bool)
        keep[bad.get(i, [])] = False
        assert np.all(st[~keep] == -1) and np.all(np.isnan(sc[~keep]))
        assert np.array_equal(st[keep], clean[i][0][keep]) and np.array_equal(sc[keep], clean[i][1][keep])
        assert not np.any(clean[i][0] < 0) and np.all(np.isfinite(clean[i][1]))
        # without the flag the same arrays behave as before: every track with a NaN row is -1 / NaN
        pst, psc = ctx.map_states(model, i, scores=True)
        nan = np.isnan(dirty[i]).any(axis=(1, 2)) | np.isnan(sig[i]).any(axis=(1, 2))
        assert np.array_equal(np.isnan(psc), nan) and np.array_equal((pst == -1).all(axis=1), nan)


# ---- 4. back-pointer words in global scratch ----------------------------------------------------------------------------------------
def test_global_back_pointers_on_the_longest_bucket(ctx, monkeypatch):
    case = G.make_case(3, 2, "peak", 3)
    _upload(ctx, case)
    model = _case_model(case)
    monkeypatch.setenv("EXTRACK_MAP_BP", "lds")
    lds = ctx.map_states(model, 4, scores=True, gaps=True)
    monkeypatch.setenv("EXTRACK_MAP_BP", "global")
    glb = ctx.map_states(model, 4, scores=True, gaps=True)
    assert np.array_equal(lds[0], glb[0]) and np.array_equal(lds[1], glb[1])
    _check_case(ctx, case, "global back-pointers", only=4)


# ---- 5. one large bucket: many blocks, many batches ---------------------------------------------------------------------------------
@pytest.mark.parametrize("S,F", [(3, 4), (4, 3)])
def test_large_bucket(ctx, S, F):
    """3000 x 14, two dimensions, 25 % of the interior rows missing.  Rules (a) - (c); the restatement leaves out 4 of 3000 tracks on each
    model, inside the TIE_SHARE of tests/map_reference.py.  (Two-state data is not used here: at frame_len 5 it leaves out 54 of 3000.)"""
    from extrack_amd import synth
    Ds, Tm, Fs = G.MODELS[S]
    ds = np.sqrt(2 * Ds * G.DT)
    tr = synth.drop_positions(synth.brownian_tracks(3000, 14, list(Ds), Tm.tolist(), list(Fs), LocErr=0.02, dt=G.DT, dims=2, seed=11), 0.25, seed=3)
    eff = np.array([[[0.02]]])
    ref = MG.map_path(tr, eff, ds, Fs, Tm, G.PBL, 0, G.CELL, F, G.MIN_LEN)
    ctx.clear_buckets()
    ctx.upload_bucket(tr)
    st, sc = ctx.map_states(_model(S, F, G.MIN_LEN, 14, le=[0.02]), 0, scores=True, gaps=True)
    left = MG.compare_paths(st, sc, ref, tr, eff, (ds, Fs, Tm, G.PBL, 0, G.CELL, G.MIN_LEN), SCORE_TOL, "3000 x 14, S=%d F=%d" % (S, F))
    assert left.sum() <= MG.TIE_SHARE * len(left), "%d of %d tracks are near-ties" % (left.sum(), len(left))


# ---- 6. a long run of transition-only steps -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,F", [(2, 4), (3, 3)])
def test_long_run_of_missing_rows(ctx, S, F):
    """One 300-position track with 250 rows missing: hundreds of transition-only steps in a row carry the weights' exponents and fill 18
    back-pointer words."""
    from extrack_amd import synth
    Ds, Tm, Fs = G.MODELS[S]
    ds = np.sqrt(2 * Ds * G.DT)
    tr = synth.brownian_tracks(1, 300, list(Ds), Tm.tolist(), list(Fs), dt=G.DT, dims=1, seed=8)
    miss = np.zeros(300, bool)
    miss[np.random.default_rng(8).permutation(np.arange(1, 299))[:250]] = True
    tr[0, miss] = np.nan
    eff = np.array([[[0.02]]])
    ref = MG.map_path(tr, eff, ds, Fs, Tm, G.PBL, 0, G.CELL, F, 3)
    ctx.clear_buckets()
    ctx.upload_bucket(tr)
    st, sc = ctx.map_states(_model(S, F, 3, 300, le=[0.02]), 0, scores=True, gaps=True)
    assert np.isfinite(sc[0])
    MG.compare_paths(st, sc, ref, tr, eff, (ds, Fs, Tm, G.PBL, 0, G.CELL, 3), SCORE_TOL, "300 positions, 250 missing, S=%d" % S)


# ---- 7. refusals decided on the host ------------------------------------------------------------------------------------------------
def test_host_decided_refusals(ctx):
    from extrack_amd import _lib
    case = G.make_case(2, 2, "global1", 4)
    _upload(ctx, case)
    model = _case_model(case)
    ctx.map_states(model, 1, gaps=True)
    info = ctx.last_launch_info()

    def refused(call):
        with pytest.raises(_lib.ExtrackError) as e:
            call()
        assert e.value.code == _lib.E_UNSUPPORTED and ctx.last_launch_info() == info  # nothing was launched to find that out
    refused(lambda: ctx.map_states(_model(2, 4, G.MIN_LEN, 40, le=[0.02], nb_substeps=2), 0, gaps=True))
    five = {5: (np.linspace(0.001, 0.3, 5), np.full((5, 5), 0.05) + np.eye(5) * 0.75, np.full(5, 0.2))}
    refused(lambda: ctx.map_states(_model(5, 3, G.MIN_LEN, 40, le=[0.02], models=five), 0, gaps=True))
    refused(lambda: ctx.map_states(_model(2, 12, G.MIN_LEN, 40, le=[0.02]), 0, gaps=True))  # 2048 groups per track
    refused(lambda: ctx.map_states(_model(4, 7, G.MIN_LEN, 40, le=[0.02]), 0, gaps=True))   # 4096
    ctx.set_bucket_dt(1, np.full(case["buckets"][1].shape[:2], G.DT))
    refused(lambda: ctx.map_states(model, 1, gaps=True))
    ctx.map_states(model, 0, gaps=True)  # a bucket without time steps is still served
    ctx.set_bucket_dt(1, None)
    assert not np.any(ctx.map_states(model, 1, gaps=True) < 0)


# ---- 8. predict_states end to end on gap-closed tracks ------------------------------------------------------------------------------
def _params(S):
    from extrack_amd.lmfit_compat import Parameters
    Ds, Tm, Fs = G.MODELS[S]
    p = Parameters()
    for s in range(S):
        p.add("D%d" % s, value=Ds[s])
        p.add("F%d" % s, value=Fs[s])
        for t in range(S):
            if s != t:
                p.add("p%d%d" % (s, t), value=Tm[s, t])
    p.add("LocErr", value=0.02)
    p.add("pBL", value=G.PBL)
    return p


def test_predict_states_on_an_insert_gaps_data_set():
    """Tracks as a gap-closing tracker writes them - positions and frame numbers, missed frames absent - through ``insert_gaps`` and
    ``predict_states(gaps=True, return_scores=True)``: keys are frame spans, min / max length and isBL come from them."""
    from extrack_amd import gaps, synth, tracking
    S, F = 2, 4
    Ds, Tm, Fs = G.MODELS[S]
    rng = np.random.default_rng(21)
    closed, frames = {}, {}
    for i, (L, N) in enumerate(((6, 40), (11, 70))):
        tr = synth.brownian_tracks(N, L, list(Ds), Tm.tolist(), list(Fs), LocErr=0.02, dt=G.DT, dims=2, seed=60 + i)
        fr = np.sort(np.argsort(rng.random((N, L + 5)), axis=1)[:, :L], axis=1) + 100  # L of L + 5 consecutive frames
        closed[str(L)], frames[str(L)] = tr, fr
    tracks, _, _, origin = gaps.insert_gaps(closed, frames)
    assert any(np.isnan(v).any() for v in tracks.values()) and len(tracks) > 2
    p = _params(S)
    only = tracking.predict_states(tracks, G.DT, p, cell_dims=G.CELL, frame_len=F, gaps=True)
    st, sc = tracking.predict_states(tracks, G.DT, p, cell_dims=G.CELL, frame_len=F, gaps=True, return_scores=True)
    assert set(st) == set(sc) == set(only) == set(tracks)
    le, Dv, Fv, Tv, pBL, _ = tracking._extract_arrays(p, G.DT, 1, 1)
    ds = np.sqrt(2 * Dv * G.DT)
    lens = sorted(int(k) for k in tracks)
    n_out = 0
    for k, b in tracks.items():
        assert st[k].dtype == np.int8 and st[k].shape == b.shape[:2] and np.array_equal(only[k], st[k]) and sc[k].shape == (len(b),)
        isBL, min_len = int(int(k) != lens[-1]), max(lens[0], 2)
        ref = MG.map_path(b, le[None, None], ds, Fv, Tv, pBL, isBL, G.CELL, F, min_len)
        left = MG.compare_paths(st[k], sc[k], ref, b, le[None, None], (ds, Fv, Tv, pBL, isBL, G.CELL, min_len), SCORE_TOL, "span %s" % k)
        assert np.all(MG.has_gap_run(np.isnan(b).all(axis=2))[left])
        n_out += int(left.sum())
    assert n_out <= MG.TIE_SHARE * 110 + MG.MAX_TIES_PER_CASE
    # without the flag the same arrays poison every track with a missed frame
    plain = tracking.predict_states(tracks, G.DT, p, cell_dims=G.CELL, frame_len=F)
    for k, b in tracks.items():
        assert np.array_equal((plain[k] == -1).all(axis=1), np.isnan(b).any(axis=(1, 2)))


# ---- 9. the other entry points are untouched ----------------------------------------------------------------------------------------
def test_plain_entry_points_give_the_same_bits_around_a_gap_call(ctx):
    case = G.make_case(3, 2, "global1", 4)
    _upload(ctx, case)
    model = _case_model(case)
    before = [ctx.map_states(model, i, scores=True) for i in range(5)]
    ll0 = ctx.loglik(model, per_track=True)
    a = [ctx.map_states(model, i, scores=True, gaps=True) for i in range(5)]
    assert ctx.last_kernel_ms() > 0.0
    b = [ctx.map_states(model, i, scores=True, gaps=True) for i in range(5)]
    after = [ctx.map_states(model, i, scores=True) for i in range(5)]
    ll1 = ctx.loglik(model, per_track=True)
    for x, y in list(zip(before, after)) + list(zip(a, b)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1], equal_nan=True)
    assert np.array_equal(ll0[1], ll1[1], equal_nan=True) and (ll0[0] == ll1[0] or (np.isnan(ll0[0]) and np.isnan(ll1[0])))
