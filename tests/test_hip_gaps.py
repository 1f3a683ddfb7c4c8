"""GPU tests of the gap-aware likelihood and posteriors (extrack_loglik_gaps / extrack_predict_gaps) against the
reference built from the unchanged oracle (tests/gap_reference.py).  Tolerances are those of tests/test_hip_parity.py: totals 1e-12 relative,
per-track LL rtol 1e-13 / atol 1e-10, posteriors TOL_PRED."""
import numpy as np
import pytest

import gap_reference as R
from oracle import oracle_np as O

pytestmark = pytest.mark.gpu

TOL_PRED = 1e-9


@pytest.fixture(scope="module")
def ctx():
    from extrack_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _model(S, F, min_len, max_len, le=None, mode=0, slope_offset=None, nb_substeps=1):
    from extrack_amd import _lib, engine
    Ds, Tm, Fs = R.MODELS[S]
    ds = np.sqrt(2 * Ds * R.DT)
    so = slope_offset or (0.0, 0.0)
    return _lib.ModelHandle(ds, Fs, Tm, engine.p_stay_table(ds, S, nb_substeps, R.CELL), R.PBL, nb_substeps, F, min_len, max_len, locerr=le,
                            locerr_mode=mode, slope=so[0], offset=so[1])


def _case_model(case):
    mode = 0 if case["sig"] is None else (2 if case["slope_offset"] is not None else 1)
    return _model(case["S"], case["F"], R.MIN_LEN, max(b.shape[1] for b in case["buckets"]), le=case["le"], mode=mode,
                  slope_offset=case["slope_offset"])


def _upload(ctx, case, buckets=None):
    ctx.clear_buckets()
    for i, b in enumerate(case["buckets"] if buckets is None else buckets):
        ctx.upload_bucket(b, None if case["sig"] is None else case["sig"][i])


def _split(flat, buckets):
    o = np.concatenate([[0], np.cumsum([len(b) for b in buckets])])
    return [flat[o[i]:o[i + 1]] for i in range(len(buckets))]


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("D", (1, 2, 3))
@pytest.mark.parametrize("S", (2, 3, 4))
def test_gaps_against_reference(ctx, S, D, layout):
    """Every bucket of the case in ONE likelihood call (descriptor table), min_len 3, the longest bucket isBL = 0; at frame_len 3 (L = 14 runs
    the fused steady state with gaps at t = 1, L - 2, a run longer than the window, every interior row) and frame_len 5 (L = 40: gaps across
    the staging boundary)."""
    for F in (3, 5):
        case = R.make_case(S, D, layout, F)
        _upload(ctx, case)
        model = _case_model(case)
        tot, flat = ctx.loglik(model, per_track=True, gaps=True)
        ref = R.case_reference(case, False)
        worst = 0.0
        for i, (g, r) in enumerate(zip(_split(flat, case["buckets"]), ref)):
            assert np.all(np.isfinite(r))
            worst = max(worst, np.abs(g - r).max())
            np.testing.assert_allclose(g, r, rtol=1e-13, atol=1e-10, err_msg="F=%d LL bucket %d" % (F, i))
        rt = sum(r.sum() for r in ref)
        print("S=%d D=%d %s F=%d: worst |dLL| %.2e, total rel. %.2e" % (S, D, layout, F, worst, abs(tot - rt) / abs(rt)))
        assert abs(tot - rt) <= 1e-12 * abs(rt), (F, tot, rt)
        refp = R.case_reference(case, True)
        for i, r in enumerate(refp):
            g = ctx.predict(model, i, gaps=True)
            np.testing.assert_allclose(g, r, rtol=0, atol=TOL_PRED, err_msg="F=%d posteriors bucket %d" % (F, i))


@pytest.mark.parametrize("S,D,layout,F", [(3, 2, "global1", 6), (2, 2, "global1", 6), (4, 3, "peak", 4), (2, 1, "affine", 5)])
def test_gap_free_data_agree_with_the_plain_entry_points(ctx, S, D, layout, F):
    from extrack_amd import synth
    case = R.make_case(S, D, layout, F)
    Ds, Tm, Fs = R.MODELS[S]
    full = [synth.brownian_tracks(len(b), b.shape[1], list(Ds), Tm.tolist(), list(Fs), dt=R.DT, dims=D, seed=3 + i) for i, b in enumerate(case["buckets"])]
    if case["sig"] is not None:
        case["sig"] = [np.where(np.isnan(s) | (s > 1), 0.03, s) for s in case["sig"]]
    _upload(ctx, case, full)
    model = _case_model(case)
    t0, l0 = ctx.loglik(model, per_track=True)
    t1, l1 = ctx.loglik(model, per_track=True, gaps=True)
    assert abs(t0 - t1) <= 1e-12 * abs(t0), (t0, t1)
    np.testing.assert_allclose(l1, l0, rtol=1e-13, atol=1e-10)
    for i in range(len(full)):
        np.testing.assert_allclose(ctx.predict(model, i, gaps=True), ctx.predict(model, i), rtol=0, atol=TOL_PRED)


def test_poison_rules_through_the_abi(ctx):
    case = R.make_case(2, 2, "global1", 4)
    dirty = [b.copy() for b in case["buckets"]]
    dirty[3][6, 5, 1] = np.nan   # a row with one NaN coordinate
    dirty[3][9, 0] = np.nan      # NaN first row
    dirty[4][5, -1] = np.nan     # NaN last row
    model = _case_model(case)
    _upload(ctx, case)
    _, clean = ctx.loglik(model, per_track=True, gaps=True)
    _upload(ctx, case, dirty)
    tot, got = ctx.loglik(model, per_track=True, gaps=True)
    clean, got = _split(clean, dirty), _split(got, dirty)
    bad = {3: [6, 9], 4: [5]}
    assert np.isnan(tot)
    for i in range(len(dirty)):
        keep = np.ones(len(dirty[i]), bool)
        keep[bad.get(i, [])] = False
        assert np.all(np.isnan(got[i][~keep])) and np.array_equal(got[i][keep], clean[i][keep]) and np.all(np.isfinite(clean[i]))
    p3, p4 = ctx.predict(model, 3, gaps=True), ctx.predict(model, 4, gaps=True)
    assert np.all(np.isnan(p3[[6, 9]])) and np.all(np.isnan(p4[5])) and np.all(np.isfinite(np.delete(p3, [6, 9], axis=0)))
    # without the flag the same arrays behave as before: every track with a NaN anywhere is NaN, the others are not
    _, plain = ctx.loglik(model, per_track=True)
    for d, p in zip(dirty, _split(plain, dirty)):
        assert np.array_equal(np.isnan(p), np.isnan(d).any(axis=(1, 2)))
    pp = ctx.predict(model, 3)
    assert np.array_equal(np.isnan(pp).all(axis=(1, 2)), np.isnan(dirty[3]).any(axis=(1, 2)))


@pytest.mark.parametrize("S,F", [(2, 4), (3, 3)])
def test_long_run_of_missing_rows(ctx, S, F):
    """One 300-position track with 250 rows missing: hundreds of transition-only steps in a row carry the weights' exponents.
    One dimension: the reference adds and removes 250 * D * log(sqrt(2 pi) 1e7) = 4250 D to a log-likelihood of ~20, in ~1200 operations of
    half an ulp (4.5e-13 D) each - its own rounding noise, measured by moving its error between 1e6 and 1e8 (bias <= 5e-12 throughout), is
    +-3e-11 for D = 1 and +-8e-11 for D = 2, which would leave the tolerance of 1e-10 no room."""
    from extrack_amd import synth
    Ds, Tm, Fs = R.MODELS[S]
    tr = synth.brownian_tracks(1, 300, list(Ds), Tm.tolist(), list(Fs), dt=R.DT, dims=1, seed=8)
    miss = np.zeros(300, bool)
    miss[np.random.default_rng(8).permutation(np.arange(1, 299))[:250]] = True
    tr[0, miss] = np.nan
    ctx.clear_buckets()
    ctx.upload_bucket(tr)
    model = _model(S, F, 3, 300, le=[0.02])
    tot, ll = ctx.loglik(model, per_track=True, gaps=True)
    ref, refp = R.loglik_and_preds(tr, np.array([[[0.02]]]), np.sqrt(2 * Ds * R.DT), Fs, Tm, R.PBL, 0, R.CELL, F, 3, do_preds=True)
    print("S=%d: LL %.12f reference %.12f" % (S, ll[0], ref[0]))
    assert np.isfinite(ll[0]) and tot == ll[0]
    np.testing.assert_allclose(ll, ref, rtol=1e-13, atol=1e-10)
    np.testing.assert_allclose(ctx.predict(model, 0, gaps=True), refp, rtol=0, atol=TOL_PRED)


def test_host_decided_refusals(ctx):
    from extrack_amd import _lib
    case = R.make_case(2, 2, "global1", 4)
    _upload(ctx, case)
    model = _case_model(case)
    ctx.loglik(model, gaps=True)
    info = ctx.last_launch_info()
    two = _model(2, 4, R.MIN_LEN, 40, le=[0.02], nb_substeps=2)
    for call in (lambda: ctx.loglik(two, gaps=True), lambda: ctx.predict(two, 0, gaps=True)):
        with pytest.raises(_lib.ExtrackError) as e:
            call()
        assert e.value.code == _lib.E_UNSUPPORTED and ctx.last_launch_info() == info
    ctx.set_bucket_dt(1, np.full(case["buckets"][1].shape[:2], R.DT))
    for call in (lambda: ctx.loglik(model, gaps=True), lambda: ctx.predict(model, 1, gaps=True)):
        with pytest.raises(_lib.ExtrackError) as e:
            call()
        assert e.value.code == _lib.E_UNSUPPORTED and ctx.last_launch_info() == info
    ctx.predict(model, 0, gaps=True)  # a bucket without time steps is still served
    ctx.set_bucket_dt(1, None)
    assert np.isfinite(ctx.loglik(model, gaps=True))


def test_fit_recovers_the_diffusion_coefficient():
    """3000 tracks x 12 positions, 25 % of the interior positions missed: marginalising them ends at the truth (D1 = 0.25), deleting the rows and
    treating the rest as consecutive frames inflates D1 (the likelihood profile of the oracle peaks at 0.25-0.275 against 0.325-0.375)."""
    from extrack_amd import synth, tracking as T
    from extrack_amd.lmfit_compat import Parameters
    vals = dict(D0=1e-3, D1=0.25, LocErr=0.02, F0=0.6, F1=0.4, p01=0.1, p10=0.1, pBL=0.1)
    Tm = O.extract_params(vals, 0.02, 1, 1)[3]
    tr = synth.brownian_tracks(3000, 12, [1e-3, 0.25], Tm, [0.6, 0.4], seed=5)
    mask = np.random.default_rng(11).random((3000, 12)) < 0.25
    mask[:, 0] = mask[:, -1] = False
    gapped = tr.copy()
    gapped[mask] = np.nan

    def start():
        p = Parameters()
        for k, v in vals.items():
            p.add(k, value=0.4 if k == "D1" else v, min=0.0 if k == "D1" else -np.inf, max=3.0 if k == "D1" else np.inf, vary=k == "D1")
        return p
    fit = T.param_fitting({"12": gapped}, 0.02, params=start(), nb_states=2, frame_len=6, verbose=0, cell_dims=[1], gaps=True)
    d1 = fit.params["D1"].value
    ref = R.objective(dict(vals, D1=d1), {"12": gapped}, 0.02, (1,), 6)
    print("gaps=True: D1 %.4f, objective %.9f, reference %.9f (%s)" % (d1, fit.residual[0], ref, fit.gradient_why))
    assert fit.gradient_path == "fd" and "gap" in fit.gradient_why
    assert 0.22 <= d1 <= 0.29, d1
    assert abs(fit.residual[0] - ref) <= 1e-9 * abs(ref), (fit.residual[0], ref)
    comp = {}
    for row, m in zip(tr, mask):
        comp.setdefault(str(int((~m).sum())), []).append(row[~m])
    comp = {k: np.array(v) for k, v in comp.items()}
    fit2 = T.param_fitting(comp, 0.02, params=start(), nb_states=2, frame_len=6, verbose=0, cell_dims=[1])
    print("compressed: D1 %.4f" % fit2.params["D1"].value)
    assert fit2.params["D1"].value > 0.31, fit2.params["D1"].value
