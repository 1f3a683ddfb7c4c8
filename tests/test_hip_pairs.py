"""GPU tests of the pairwise state posteriors (extrack_predict_pairs / extrack_predict_pairs_gaps; csrc/xt_kernel.h PAIRS,
csrc/extrack_pairs.hip), through the C ABI, against the reference built from the oracle's pieces (tests/pair_reference.py).  Buckets: those of
gap_reference.make_case with and without their gap rows - L = 2 (one pair, tail only), 3, frame_len + 1 (no pair inside the loop), 14 (loop and
tail, gap runs longer than the window, N = 37: a ragged last batch), 40 (across the staging boundary) - plus L = frame_len + 2 (exactly one
pair inside the loop).  Tolerances: pairs and their first marginal at the project's posterior tolerance (tests/test_hip_parity.py,
tests/test_hip_gaps.py) 1e-9 absolute; counts against the sum of the pairs over t at 1e-12 * L.

Largest errors seen on one MI355X (all cases below): see DESIGN.md section 29."""
import ctypes as C

import numpy as np
import pytest

import gap_reference as R
import pair_reference as PR

pytestmark = pytest.mark.gpu

TOL_PRED = 1e-9
# S = 2, 3, 4 at frame_len 2 (S threads per track write S^2 values), 3 and 6; 4 states at frame_len 6: 1024 threads per track; the four error
# layouts; D = 1, 2, 3
_CASES = [(2, 2, "global1", 2), (3, 1, "global1", 2), (4, 2, "peak", 2), (2, 1, "affine", 3), (3, 3, "globalD", 3), (4, 2, "affine", 3),
          (2, 3, "peak", 6), (3, 2, "global1", 6), (4, 2, "global1", 6)]


@pytest.fixture(scope="module")
def ctx():
    from extrack_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _model(S, F, min_len, max_len, le=None, mode=0, slope_offset=None, nb_substeps=1):
    from extrack_amd import _lib, engine
    Ds, Tm, Fs = R.MODELS[S] if S in R.MODELS else (np.linspace(0.001, 0.3, S), np.full((S, S), 0.05) + np.eye(S) * (1 - 0.05 * S), np.full(S, 1.0 / S))
    ds = np.sqrt(2 * Ds * R.DT)
    so = slope_offset or (0.0, 0.0)
    return _lib.ModelHandle(ds, Fs, Tm, engine.p_stay_table(ds, S, nb_substeps, R.CELL), R.PBL, nb_substeps, F, min_len, max_len, locerr=le,
                            locerr_mode=mode, slope=so[0], offset=so[1])


def _case_model(case):
    mode = 0 if case["sig"] is None else (2 if case["slope_offset"] is not None else 1)
    return _model(case["S"], case["F"], R.MIN_LEN, max(b.shape[1] for b in case["buckets"]), le=case["le"], mode=mode,
                  slope_offset=case["slope_offset"])


def _upload(ctx, buckets, sigmas):
    ctx.clear_buckets()
    for i, b in enumerate(buckets):
        ctx.upload_bucket(b, None if sigmas is None else sigmas[i])


@pytest.mark.parametrize("S,D,layout,F", _CASES)
def test_pairs_against_reference(ctx, S, D, layout, F):
    case = PR.make_case(S, D, layout, F)
    model = _case_model(case)
    worst = {}
    for gaps in (True, False):
        buckets = case["buckets"] if gaps else PR.plain_buckets(case)
        _upload(ctx, buckets, case["sig"] if gaps else PR.plain_sigmas(case))
        ref = PR.case_reference(case, gaps=gaps)
        e_pair = e_marg = e_cnt = 0.0
        for i, (b, (_, r)) in enumerate(zip(buckets, ref)):
            L = b.shape[1]
            assert np.all(np.isfinite(r))
            pairs, counts = ctx.predict_pairs(model, i, pairs=True, counts=True, gaps=gaps)
            if i == 0:
                info = ctx.last_launch_info()
                assert ctx.last_ll_path() == ("gaps" if gaps else "general") and ctx.last_kernel_ms() > 0.0
                assert info["threads"] == (1024 if (S, F) == (4, 6) else info["threads"]) and info["threads"] >= min(S ** (F - 1), 64)
            assert pairs.shape == (len(b), L - 1, S, S) and counts.shape == (len(b), S, S)
            e_pair = max(e_pair, np.abs(pairs - r).max())
            e_marg = max(e_marg, np.abs(pairs.sum(axis=3) - ctx.predict(model, i, gaps=gaps)[:, :-1]).max())
            e_cnt = max(e_cnt, np.abs(counts - pairs.sum(axis=1)).max() / L)
            only = ctx.predict_pairs(model, i, pairs=False, counts=True, gaps=gaps)
            # the same kernel with one pointer null.  Bit for bit where the sums have a fixed order: a track's groups are one aligned
            # power-of-two lane range (2 states; 4 states up to 64 groups).  Else (3 states, several wavefronts per track) the LDS atomics
            # arrive in any order: a pair is a ratio of two sums of at most S^F non-negative terms, 2 * S^F * eps, and a count adds L - 1
            if S != 3 and S ** (F - 1) <= 64:
                assert np.array_equal(only, counts), "counts-only call, bucket %d" % i
            else:
                assert np.abs(only - counts).max() <= 2 * S ** F * np.finfo(float).eps * (L - 1), "counts-only call, bucket %d" % i
            if not gaps:  # gap-free data through the _gaps entry
                e_pair = max(e_pair, np.abs(ctx.predict_pairs(model, i, gaps=True) - pairs).max())
        print("S=%d D=%d %s F=%d gaps=%d: max |pairs - ref| %.2e, first marginal %.2e, counts / L %.2e" % (S, D, layout, F, gaps, e_pair, e_marg, e_cnt))
        worst[gaps] = (e_pair, e_marg, e_cnt)
    for gaps, (e_pair, e_marg, e_cnt) in worst.items():
        assert e_pair <= TOL_PRED and e_marg <= TOL_PRED and e_cnt <= 1e-12, (gaps, e_pair, e_marg, e_cnt)


def test_block_serves_several_batches(ctx, monkeypatch):
    """20 000 tracks on a grid of at most 16 blocks: every block walks many batches, the last one ragged."""
    from extrack_amd import synth
    monkeypatch.setenv("EXTRACK_PAIRS_MAX_BLOCKS", "16")
    S, F, L, N = 2, 4, 9, 20000
    Ds, Tm, Fs = R.MODELS[S]
    tr = synth.brownian_tracks(N, L, list(Ds), Tm.tolist(), list(Fs), LocErr=0.02, dt=R.DT, dims=2, seed=77)
    _upload(ctx, [tr], None)
    model = _model(S, F, R.MIN_LEN, L, le=[0.02])
    pairs, counts = ctx.predict_pairs(model, 0, pairs=True, counts=True)
    info = ctx.last_launch_info()
    assert info["blocks"] <= 16 and info["blocks"] * info["tracks_per_block"] * 4 <= N, info
    _, ref = PR.windowed(tr, np.array([[[0.02]]]), np.sqrt(2 * Ds * R.DT), Fs, Tm, R.PBL, 0, R.CELL, F, R.MIN_LEN)
    assert np.abs(pairs - ref).max() <= TOL_PRED and np.abs(counts - pairs.sum(axis=1)).max() <= 1e-12 * L


def test_loglik_is_untouched_by_a_pair_call(ctx):
    case = PR.make_case(3, 2, "global1", 3)
    _upload(ctx, case["buckets"], None)
    model = _case_model(case)
    t0, l0 = ctx.loglik(model, per_track=True, gaps=True)
    for i in range(len(case["buckets"])):
        ctx.predict_pairs(model, i, pairs=True, counts=True, gaps=True)
    t1, l1 = ctx.loglik(model, per_track=True, gaps=True)
    assert t0 == t1 and np.array_equal(l0, l1) and np.all(np.isfinite(l0))
    plain = PR.plain_buckets(case)
    _upload(ctx, plain, None)
    t0, l0 = ctx.loglik(model, per_track=True)
    ctx.predict_pairs(model, 4, counts=True)
    t1, l1 = ctx.loglik(model, per_track=True)
    assert t0 == t1 and np.array_equal(l0, l1)


def test_nan_track_is_nan_everywhere(ctx):
    case = PR.make_case(2, 2, "global1", 3)
    dirty = [b.copy() for b in case["buckets"]]
    dirty[4][6, 5, 1] = np.nan  # L = 14: a row with one NaN coordinate
    model = _case_model(case)
    _upload(ctx, dirty, None)
    pairs, counts = ctx.predict_pairs(model, 4, pairs=True, counts=True, gaps=True)
    ref = PR.case_reference(case, gaps=True)[4][1]
    keep = np.arange(len(dirty[4])) != 6
    assert np.all(np.isnan(pairs[6])) and np.all(np.isnan(counts[6])) and np.abs(pairs[keep] - ref[keep]).max() <= TOL_PRED
    assert np.all(np.isnan(ctx.predict(model, 4, gaps=True)[6]))


def test_refusals_launch_nothing():
    """Every refusal is decided on the host: its code comes back and the context has still launched nothing."""
    from extrack_amd import _lib
    from extrack_amd import synth
    c = _lib.Context(0)
    try:
        Ds, Tm, Fs = R.MODELS[2]
        tr = synth.brownian_tracks(8, 6, list(Ds), Tm.tolist(), list(Fs), LocErr=0.02, dt=R.DT, dims=3, seed=3)
        c.upload_bucket(tr, None)
        c.upload_bucket(tr[:, :5].copy(), None)
        c.set_bucket_dt(1, np.full((8, 5), R.DT))
        lib = c._lib

        def code(model, gaps, bucket=0, pairs=True, counts=True):
            out = np.empty((8, 5, 16))
            cnt = np.empty((8, 16))
            fn = lib.extrack_predict_pairs_gaps if gaps else lib.extrack_predict_pairs
            return fn(c._h, C.byref(model.c), bucket, out.ctypes.data_as(C.c_void_p) if pairs else None, cnt.ctypes.data_as(C.c_void_p) if counts else None)

        ok = _model(2, 3, 3, 6, le=[0.02])
        for gaps in (False, True):
            assert code(ok, gaps, pairs=False, counts=False) == _lib.E_INVALID  # both outputs NULL
            assert code(ok, gaps, bucket=7) == _lib.E_INVALID
            assert code(_model(2, 3, 3, 6, le=[0.02], nb_substeps=2), gaps) == (_lib.E_UNSUPPORTED if gaps else _lib.E_INVALID)
            assert code(_model(5, 3, 3, 6, le=[0.02]), gaps) == _lib.E_UNSUPPORTED      # five states
            assert code(_model(2, 12, 3, 6, le=[0.02]), gaps) == _lib.E_UNSUPPORTED     # 2048 groups per track
            assert code(_model(4, 6, 3, 6, le=[0.02, 0.02, 0.02]), gaps) == _lib.E_UNSUPPORTED  # 1024 groups fit, the state of D = K = 3 does not
            assert code(ok, gaps, bucket=1) == _lib.E_UNSUPPORTED                       # per-track time steps
            assert b"" != lib.extrack_last_error(c._h)
        assert all(v == 0 for k, v in c.last_launch_info().items() if k != "compute_units")
        assert c.last_ll_path() == "none"
        with pytest.raises(_lib.ExtrackError):  # nothing was launched to find all that out
            c.last_kernel_ms()
        assert code(ok, False) == 0 and c.last_kernel_ms() > 0.0
    finally:
        c.close()


def test_predict_transitions_end_to_end():
    from extrack_amd import synth, tracking
    from extrack_amd.lmfit_compat import Parameters
    p = Parameters()
    vals = dict(D0=1e-3, D1=0.05, D2=0.3, LocErr=0.02, F0=0.3, F1=0.3, F2=0.4, p01=0.08, p02=0.04, p10=0.06, p12=0.05, p20=0.03, p21=0.07, pBL=0.1)
    for k, v in vals.items():
        p.add(k, value=v)
    le, Ds, Fs, Tm, pBL, _ = tracking._extract_arrays(p, R.DT, 1, 1)
    ds = np.sqrt(2 * Ds * R.DT)
    tracks = {str(L): synth.brownian_tracks(N, L, list(Ds), Tm.tolist(), list(Fs), LocErr=0.02, dt=R.DT, dims=2, seed=40 + L) for L, N in ((5, 33), (12, 41))}
    tracks["8"] = np.empty((0, 8, 2))
    pairs, counts = tracking.predict_transitions(tracks, R.DT, p, cell_dims=R.CELL, nb_states=3, frame_len=4, output="both")
    only_p = tracking.predict_transitions(tracks, R.DT, p, cell_dims=R.CELL, nb_states=3, frame_len=4)
    only_c = tracking.predict_transitions(tracks, R.DT, p, cell_dims=R.CELL, nb_states=3, frame_len=4, output="counts")
    preds = tracking.predict_Bs(tracks, R.DT, p, cell_dims=R.CELL, nb_states=3, frame_len=4, fusion="window")
    assert set(pairs) == set(counts) == set(only_p) == set(only_c) == {"5", "8", "12"}
    assert pairs["8"].shape == (0, 7, 3, 3) and counts["8"].shape == (0, 3, 3)
    for k, isBL in (("5", 1), ("12", 0)):
        _, ref = PR.windowed(tracks[k], le[None, None], ds, Fs, Tm, pBL, isBL, R.CELL, 4, 5)
        assert np.abs(pairs[k] - ref).max() <= TOL_PRED
        assert np.abs(pairs[k].sum(axis=3) - preds[k][:, :-1]).max() <= TOL_PRED
        reorder = 2 * 3 ** 4 * np.finfo(float).eps  # three states: the order of the atomic sums is not fixed (see test_pairs_against_reference)
        assert np.abs(only_c[k] - counts[k]).max() <= reorder * (int(k) - 1) and np.abs(only_p[k] - pairs[k]).max() <= reorder
    # rows in input order
    rev = tracking.predict_transitions({k: v[::-1].copy() for k, v in tracks.items()}, R.DT, p, cell_dims=R.CELL, nb_states=3, frame_len=4)
    assert all(np.abs(rev[k] - pairs[k][::-1]).max() <= 2 * 3 ** 4 * np.finfo(float).eps for k in ("5", "12"))
    # with missed detections
    g = {k: v.copy() for k, v in tracks.items()}
    g["12"][3, 4:7] = np.nan
    gp = tracking.predict_transitions(g, R.DT, p, cell_dims=R.CELL, nb_states=3, frame_len=4, gaps=True)
    _, gref = PR.windowed_gaps(g["12"], le[None, None], ds, Fs, Tm, pBL, 0, R.CELL, 4, 5)
    assert np.abs(gp["12"] - gref).max() <= TOL_PRED and np.all(np.isfinite(gp["12"]))
    Cm, Pm = tracking.transition_matrix(counts)
    assert Cm.shape == (3, 3) and np.allclose(Pm.sum(axis=1), 1.0) and abs(Cm.sum() - (33 * 4 + 41 * 11)) <= 1e-9
