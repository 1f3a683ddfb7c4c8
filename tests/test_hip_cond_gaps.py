"""GPU tests of the fixed-state position refinement with missed detections (extrack_refine_fixed_states_gaps, csrc/xt_cond.h with GAPS;
``refine_along_states(gaps=True)``), through the C ABI and the Python function, against the dense oracle of tests/cond_gap_reference.py with
the tolerances of tests/cond_reference.py: mu 1e-12 absolute, sigma 1e-12 relative, logdens 1e-10.  Inputs: ``gap_reference.make_case`` at
seed 0; state paths: the reference decoder's (tests/map_gap_reference.py) and random ones."""
import numpy as np
import pytest

import cond_gap_reference as CG
import gap_reference as G
import map_gap_reference as MG

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from extrack_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _ds(S):
    return np.sqrt(2 * G.MODELS[S][0] * G.DT)


def _model(S, F, min_len, max_len, le=None, mode=0, slope_offset=None, nb_substeps=1):
    from extrack_amd import _lib, engine
    Ds, Tm, Fs = G.MODELS[S]
    so = slope_offset or (0.0, 0.0)
    return _lib.ModelHandle(_ds(S), Fs, Tm, engine.p_stay_table(_ds(S), S, nb_substeps, G.CELL), G.PBL, nb_substeps, F, min_len, max_len, locerr=le,
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


def _oracle(case, b, st, i, sigma=None):
    sg = sigma if sigma is not None else (None if case["sig"] is None else case["sig"][i])
    return CG.refine(b, st, _ds(case["S"]), le=case["le"], sigma=sg, slope_offset=case["slope_offset"])


def _tab_bytes(S):
    return 8 * ((S * S + 1) & ~1)


# ---- 1. the shared cases through the C ABI ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", G.LAYOUTS)
@pytest.mark.parametrize("D", (1, 2, 3))
@pytest.mark.parametrize("S", (2, 3, 4))
def test_gap_buckets_match_dense_oracle(ctx, S, D, layout):
    case = G.make_case(S, D, layout, 3)
    Ds, Tm, Fs = G.MODELS[S]
    _upload(ctx, case)
    model = _case_model(case)
    rng = np.random.default_rng(17)
    Lmax = max(b.shape[1] for b in case["buckets"])
    for i, (b, eff) in enumerate(zip(case["buckets"], case["eff"])):
        decoded, _, _ = MG.map_path(b, eff, _ds(S), Fs, Tm, G.PBL, int(b.shape[1] != Lmax), G.CELL, 3, G.MIN_LEN)
        for what, st in (("decoded", decoded), ("random", rng.integers(0, S, b.shape[:2]).astype(np.int8))):
            got = ctx.refine_fixed_states(model, i, st, logdens=True, gaps=True)
            info = ctx.last_launch_info()
            assert info["lds_bytes"] > _tab_bytes(S) and info["threads"] == info["tracks_per_block"] == 64, info  # rows in LDS
            CG.compare(got, _oracle(case, b, st, i), "S=%d D=%d %s bucket %d %s paths" % (S, D, layout, i, what))
            assert np.all(np.isfinite(got[2])) and ctx.last_kernel_ms() > 0.0
            mu, sg = ctx.refine_fixed_states(model, i, st, gaps=True)  # without the log density: the same bits
            assert np.array_equal(mu, got[0]) and np.array_equal(sg, got[1])


# ---- 2. the global placement, at the shortest track length that takes it ----------------------------------------------------------------
def _lds_bytes(S, L, D, K):
    """xt_cond_lds_doubles of csrc/xt_cond.h for 64 tracks in LDS, in bytes."""
    row = (L * (D + K)) | 1
    srow = 4 * (((L + 3) // 4) | 1)
    return 8 * (((S * S + 1) & ~1) + 64 * row + (64 * srow + 7) // 8)


@pytest.mark.parametrize("layout", ("globalD", "peak"))
def test_global_placement_at_the_shortest_length_that_takes_it(ctx, layout):
    """4 states, 3 dimensions, 3 error channels: 64 rows of 6 L + 1 doubles and their states pass the 160 KiB of a CU at L = 53.  70 tracks
    (a partial second block), 25 % of the interior rows missing and the structured masks of the 14-position bucket; a NaN error at every
    gap row of the per-peak layout.  L - 1 still runs in LDS."""
    from extrack_amd import synth
    S, D = 4, 3
    L = next(l for l in range(2, 400) if _lds_bytes(S, l, D, D) > 160 * 1024)
    assert L == 53
    Ds, Tm, Fs = G.MODELS[S]
    rng = np.random.default_rng(41)
    for length, placement in ((L, "global"), (L - 1, "lds")):
        b = synth.drop_positions(synth.brownian_tracks(70, length, list(Ds), Tm.tolist(), list(Fs), LocErr=0.02, dt=G.DT, dims=D, seed=length), 0.25, seed=5)
        b[0, 1:-1] = np.nan
        b[1, 1] = b[1, -2] = np.nan
        m = np.isnan(b).all(axis=2)
        sg = None
        if layout == "peak":
            sg = rng.uniform(0.01, 0.05, b.shape)
            sg[m] = np.nan
        le = None if layout == "peak" else [0.02, 0.03, 0.05]
        st = rng.integers(0, S, b.shape[:2]).astype(np.int8)
        ctx.clear_buckets()
        ctx.upload_bucket(b, sg)
        model = _model(S, 3, G.MIN_LEN, length, le=le, mode=0 if sg is None else 1)
        got = ctx.refine_fixed_states(model, 0, st, logdens=True, gaps=True)
        info = ctx.last_launch_info()
        if placement == "global":
            assert info["lds_bytes"] == _tab_bytes(S), info
        else:
            assert 64 * 1024 < info["lds_bytes"] <= 160 * 1024, info
        CG.compare(got, CG.refine(b, st, _ds(S), le=le, sigma=sg), "%s placement, L=%d, %s" % (placement, length, layout))


# ---- 3. gap-free data: the same bits as extrack_refine_fixed_states ---------------------------------------------------------------------
@pytest.mark.parametrize("S,D,layout", [(2, 1, "global1"), (3, 2, "peak"), (4, 3, "affine"), (2, 3, "globalD")])
def test_gap_free_data_are_bit_identical_to_the_plain_entry_point(ctx, S, D, layout):
    from extrack_amd import synth
    case = G.make_case(S, D, layout, 3)
    Ds, Tm, Fs = G.MODELS[S]
    rng = np.random.default_rng(23)
    full = [synth.brownian_tracks(len(b), b.shape[1], list(Ds), Tm.tolist(), list(Fs), dt=G.DT, dims=D, seed=3 + i) for i, b in enumerate(case["buckets"])]
    full.append(synth.brownian_tracks(70, 60, list(Ds), Tm.tolist(), list(Fs), dt=G.DT, dims=D, seed=9))  # D = 3 with 3 channels: the global placement
    sig = None if case["sig"] is None else [np.where(np.isnan(s) | (s > 1), 0.03, s) for s in case["sig"]]
    if sig is not None:
        sig.append(rng.uniform(0.01, 0.05, (70, 60, sig[0].shape[2])))
    _upload(ctx, case, full, sig)
    model = _model(S, 3, G.MIN_LEN, 60, le=case["le"], mode=0 if sig is None else (2 if case["slope_offset"] else 1), slope_offset=case["slope_offset"])
    for i, b in enumerate(full):
        st = rng.integers(0, S, b.shape[:2]).astype(np.int8)
        a = ctx.refine_fixed_states(model, i, st, logdens=True, gaps=True)
        p = ctx.refine_fixed_states(model, i, st, logdens=True)
        assert all(np.array_equal(x, y) for x, y in zip(a, p)) and np.all(np.isfinite(a[2]))


# ---- 4. the poison rules ----------------------------------------------------------------------------------------------------------------
def test_poison_rules_through_the_abi(ctx):
    case = G.make_case(2, 2, "peak", 3)
    b, sg, m = case["buckets"][3].copy(), case["sig"][3].copy(), case["masks"][3]
    st = np.random.default_rng(29).integers(0, 2, b.shape[:2]).astype(np.int8)
    model = _case_model(case)
    ctx.clear_buckets()
    ctx.upload_bucket(b, sg)
    clean = ctx.refine_fixed_states(model, 0, st, logdens=True, gaps=True)
    assert np.all(np.isfinite(clean[2]))
    gaprow = np.nonzero(m[3])[0][0]
    st2 = st.copy()
    st2[3, gaprow] = -1      # negative state at a gap row
    st2[20, 4] = -1          # ... and at any row
    b[6, 5, 1] = np.nan      # a row with one NaN coordinate
    b[9, 0] = np.nan         # NaN first row
    b[11, -1] = np.nan       # NaN last row
    obs = np.nonzero(~m[12])[0]
    sg[12, obs[1], 0] = np.nan  # NaN error at an observed row
    sg[m] = np.nan              # ... and at every gap row: never read
    ctx.clear_buckets()
    ctx.upload_bucket(b, sg)
    got = ctx.refine_fixed_states(model, 0, st2, logdens=True, gaps=True)
    bad = np.zeros(len(b), bool)
    bad[[3, 20, 6, 9, 11, 12]] = True
    for g, c in zip(got, clean):
        assert np.all(np.isnan(g[bad])) and np.array_equal(g[~bad], c[~bad])
    # without the flag the same arrays behave as before: every track with a NaN anywhere is NaN
    plain = ctx.refine_fixed_states(model, 0, st, logdens=True)
    nan = np.isnan(b).any(axis=(1, 2)) | np.isnan(sg).any(axis=(1, 2))
    assert np.array_equal(np.isnan(plain[2]), nan) and np.array_equal(np.isnan(plain[0]).all(axis=(1, 2)), nan)


# ---- 5. refine_along_states -------------------------------------------------------------------------------------------------------------
def _params(S, so=None):
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
    if so is not None:
        p.add("slope_LocErr", value=so[0])
        p.add("offset_LocErr", value=so[1])
    p.add("pBL", value=G.PBL)
    return p


@pytest.mark.parametrize("layout", ("global1", "affine"))
def test_refine_along_states_with_gaps(layout):
    """``states=None`` decodes with gaps first and gives the bits of handing over ``predict_states(gaps=True)``; both match the dense oracle
    along those paths; without the flag every track with a missed frame is NaN."""
    from extrack_amd import refined_localization as RL, tracking
    S, F = 3, 4
    case = G.make_case(S, 2, layout, F)
    tracks = {str(b.shape[1]): b for b in case["buckets"]}
    sig = None if case["sig"] is None else {str(s.shape[1]): s for s in case["sig"]}
    tracks["8"] = np.empty((0, 8, 2))
    if sig is not None:
        sig["8"] = np.empty((0, 8, 1))
    p = _params(S, case["slope_offset"])
    st = tracking.predict_states(tracks, G.DT, p, cell_dims=G.CELL, frame_len=F, input_LocErr=sig, gaps=True)
    a = RL.refine_along_states(tracks, G.DT, p, frame_len=F, cell_dims=G.CELL, input_LocErr=sig, return_logdensity=True, gaps=True)
    b = RL.refine_along_states(tracks, G.DT, p, states=st, frame_len=F, cell_dims=G.CELL, input_LocErr=sig, return_logdensity=True, gaps=True)
    plain = RL.refine_along_states(tracks, G.DT, p, frame_len=F, cell_dims=G.CELL, input_LocErr=sig, return_logdensity=True)
    for k, Cs in tracks.items():
        assert all(np.array_equal(x[k], y[k]) for x, y in zip(a, b))
        assert a[0][k].shape == Cs.shape and a[1][k].shape == Cs.shape[:2] and a[2][k].shape == (len(Cs),)
        if len(Cs) == 0:
            continue
        ref = CG.refine(Cs, st[k], _ds(S), le=None if sig is not None else [0.02], sigma=None if sig is None else sig[k],
                        slope_offset=case["slope_offset"])
        CG.compare((a[0][k], a[1][k][:, :, None], a[2][k]), ref, "refine_along_states %s L=%s" % (layout, k))
        assert np.all(np.isfinite(a[2][k])) and not np.any(st[k] < 0)
        assert np.array_equal(np.isnan(plain[2][k]), np.isnan(Cs).any(axis=(1, 2)))


# ---- 6. what the posterior of a missed position looks like ------------------------------------------------------------------------------
def test_interpolated_posterior_of_a_single_missed_position(ctx):
    """One dimension, 9 positions, the middle row missing, one state along the whole track (state 0 for even tracks, 1 for odd ones).
    With A the filtered variance left of the gap, C the variance of what the right side knows about the position after one step q, the
    gap's posterior variance minus its left neighbour's is q (C - A) / (A + C + q); the track is symmetric about the gap (same error,
    same step variance everywhere), so C - A = q > 0, and likewise on the right: sigma at the gap exceeds both observed neighbours'.
    mu[4] = f[3] + J (mu[5] - f[3]) and mu[3] = f[3] + J' (mu[4] - f[3]) with 0 < J, J' < 1: mu at the gap lies between theirs."""
    from extrack_amd import synth
    S = 2
    Ds, Tm, Fs = G.MODELS[S]
    b = synth.brownian_tracks(40, 9, list(Ds), Tm.tolist(), list(Fs), LocErr=0.02, dt=G.DT, dims=1, seed=2)
    b[:, 4] = np.nan
    st = np.repeat((np.arange(40) % 2).astype(np.int8)[:, None], 9, axis=1)
    ctx.clear_buckets()
    ctx.upload_bucket(b)
    mu, sg, ld = ctx.refine_fixed_states(_model(S, 3, G.MIN_LEN, 9, le=[0.02]), 0, st, logdens=True, gaps=True)
    CG.compare((mu, sg, ld), CG.refine(b, st, _ds(S), le=[0.02]), "single gap")
    assert np.all(sg[:, 4, 0] > sg[:, 3, 0]) and np.all(sg[:, 4, 0] > sg[:, 5, 0])
    lo, hi = np.minimum(mu[:, 3, 0], mu[:, 5, 0]), np.maximum(mu[:, 3, 0], mu[:, 5, 0])
    assert np.all((mu[:, 4, 0] >= lo) & (mu[:, 4, 0] <= hi))


# ---- 7. refusals decided on the host; the plain entry point is untouched ----------------------------------------------------------------
def test_refusals_and_the_plain_entry_point_around_a_gap_call(ctx):
    from extrack_amd import _lib
    case = G.make_case(2, 2, "global1", 3)
    _upload(ctx, case)
    model = _case_model(case)
    st = [np.random.default_rng(i).integers(0, 2, b.shape[:2]).astype(np.int8) for i, b in enumerate(case["buckets"])]
    before = ctx.refine_fixed_states(model, 3, st[3], logdens=True)
    ll0 = ctx.loglik(model, per_track=True, gaps=True)
    a = ctx.refine_fixed_states(model, 3, st[3], logdens=True, gaps=True)
    info = ctx.last_launch_info()

    def refused(call, code):
        with pytest.raises(_lib.ExtrackError) as e:
            call()
        assert e.value.code == code and ctx.last_launch_info() == info  # nothing was launched to find that out
    refused(lambda: ctx.refine_fixed_states(_model(2, 3, G.MIN_LEN, 40, le=[0.02], nb_substeps=2), 3, st[3], gaps=True), _lib.E_UNSUPPORTED)
    three = st[3].copy()
    three[5, 2] = 2
    refused(lambda: ctx.refine_fixed_states(model, 3, three, gaps=True), _lib.E_INVALID)  # a state >= n_states
    ctx.set_bucket_dt(3, np.full(case["buckets"][3].shape[:2], G.DT))
    refused(lambda: ctx.refine_fixed_states(model, 3, st[3], gaps=True), _lib.E_UNSUPPORTED)
    ctx.set_bucket_dt(3, None)
    b = ctx.refine_fixed_states(model, 3, st[3], logdens=True, gaps=True)
    after = ctx.refine_fixed_states(model, 3, st[3], logdens=True)
    ll1 = ctx.loglik(model, per_track=True, gaps=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(before, after))
    assert ll0[0] == ll1[0] and np.array_equal(ll0[1], ll1[1])
