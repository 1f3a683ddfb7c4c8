"""GPU tests of missed detections on the register-resident 2-state kernel: extrack_loglik_gaps runs two-state likelihood
launches with one global scalar error on the gap-aware instantiation of xt_reg2.h (extrack_last_ll_path: "gaps_reg2"); everything else keeps
the general gap body ("gaps").  Frame_len 5, 6, 7 in a default context; frame_len 4 in a context created under EXTRACK_GAP_REG2_F=all (a default
context keeps frame_len 4 on the general gap body: tests/test_hip_parity.py pins that launch's geometry).  Reference: tests/gap_reference.py
(the unchanged oracle with error 1e7 at the missed rows).  Tolerances as tests/test_hip_gaps.py: per-track LL rtol 1e-13 / atol 1e-10, totals 1e-12 relative, posteriors 1e-9."""
import os

import numpy as np
import pytest

import gap_reference as R
from oracle import oracle_np as O

pytestmark = pytest.mark.gpu

Ds2, TM, FS = R.MODELS[2]
DS = np.sqrt(2 * Ds2 * R.DT)
LE = 0.02


@pytest.fixture(scope="module")
def ctx():
    from extrack_amd import _lib
    c = _lib.Context(0)
    yield c
    c.close()


def _context_under(name, value):
    """A context created with the environment variable set (the knobs bind when the context is created)."""
    from extrack_amd import _lib
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        return _lib.Context(0)
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


@pytest.fixture(scope="module")
def lds_ctx():
    """EXTRACK_LL_PATH=lds: the parent's path, the general gap body."""
    c = _context_under("EXTRACK_LL_PATH", "lds")
    yield c
    c.close()


@pytest.fixture(scope="module")
def all_ctx():
    """EXTRACK_GAP_REG2_F=all: frame_len 4 is upgraded too."""
    c = _context_under("EXTRACK_GAP_REG2_F", "all")
    yield c
    c.close()


def _model(F, min_len, max_len, S=2, le=(LE,)):
    from extrack_amd import _lib, engine
    Ds, Tm, Fs = R.MODELS[S]
    ds = np.sqrt(2 * Ds * R.DT)
    return _lib.ModelHandle(ds, Fs, Tm, engine.p_stay_table(ds, S, 1, R.CELL), R.PBL, 1, F, min_len, max_len, locerr=list(le))


def _walk(rng, N, L, D):
    return np.cumsum(rng.normal(0, 0.08, (N, L, D)), 1)


def _masks(rng, N, L, F):
    """[N, L] missed rows (N >= 8): 25 % at random; the first tracks carry the named patterns."""
    m = rng.random((N, L)) < 0.25
    if L == 3:
        m[:, 1] = np.arange(N) % 2 == 0  # the only interior row
    if L >= 4:
        m[:5] = False
        m[0, 1] = True               # the first step (warm-up chain)
        m[1, L - 2] = True           # the last step before the read-out
        m[2, 1:-1] = True            # every interior row
        m[4, 1] = m[4, L - 2] = True  # (track 3: gap-free neighbour)
    if L >= F + 1:
        m[5] = False
        m[5, F - 1] = True           # the merge-free first step
    if L >= F + 2:
        m[6] = False
        m[6, F] = True               # the first merged step
    if L >= F + 6:
        m[7] = False
        m[7, 3:3 + F + 2] = True     # a run longer than the window
    if L >= 34:
        m[3, 30:34] = True           # a run across the staging boundary; a gap as the first row of the second chunk
    m[:, 0] = m[:, -1] = False
    return m


def _buckets(F, D, seed, lengths=None):
    """Buckets short -> long: L = 2, 3, F - 1 .. F + 2, 14, 34, 40, 66, each with 2 tracks-per-wave + 1 (>= 9) tracks: complete and partial batches."""
    rng = np.random.default_rng(seed)
    N = max(2 * (64 >> (F - 1)) + 1, 9)
    out = []
    for L in sorted(set(lengths or (2, 3, F - 1, F, F + 1, F + 2, 14, 34, 40, 66))):
        Cs = _walk(rng, N, L, D)
        Cs[_masks(rng, N, L, F)] = np.nan
        out.append(Cs)
    return out


def _reference(buckets, F, min_len, S=2, le=((LE,),), preds=False):
    Ds, Tm, Fs = R.MODELS[S]
    Lmax = max(b.shape[1] for b in buckets)
    res = [R.loglik_and_preds(b, np.array([le]), np.sqrt(2 * Ds * R.DT), Fs, Tm, R.PBL, int(b.shape[1] != Lmax), R.CELL, F, min_len, do_preds=preds)
           for b in buckets]
    return [r[1] if preds else r[0] for r in res]


def _loglik(ctx, model, buckets, sig=None):
    ctx.clear_buckets()
    for i, b in enumerate(buckets):
        ctx.upload_bucket(b, None if sig is None else sig[i])
    tot, flat = ctx.loglik(model, per_track=True, gaps=True)
    o = np.concatenate([[0], np.cumsum([len(b) for b in buckets])])
    return tot, [flat[o[i]:o[i + 1]] for i in range(len(buckets))]


def _compare(tot, got, ref, what):
    worst = 0.0
    for i, (g, r) in enumerate(zip(got, ref)):
        ok = np.isfinite(r)
        assert np.array_equal(np.isnan(g), ~ok), (what, i)
        worst = max(worst, np.abs(g[ok] - r[ok]).max())
        np.testing.assert_allclose(g[ok], r[ok], rtol=1e-13, atol=1e-10, err_msg="%s bucket %d" % (what, i))
    rt = sum(r.sum() for r in ref)
    print("%s: worst |dLL| %.2e, total rel. %.2e" % (what, worst, abs(tot - rt) / abs(rt) if np.isfinite(rt) else np.nan))
    if np.isfinite(rt):
        assert abs(tot - rt) <= 1e-12 * abs(rt), (what, tot, rt)


@pytest.mark.parametrize("F", [4, 5, 6, 7])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_upgraded_launch_against_reference(ctx, all_ctx, F, D):
    """All ten buckets in ONE call (descriptor table); min_len 3, the longest bucket isBL = 0, the others 1.  The launch is upgraded, its geometry
    is that of xt_ll_gap_reg2 (256 threads, 4 waves x 64 >> (F - 1) tracks, LDS = the plain kernel's + 512 bytes of gap cells), and a second call
    gives the same bits."""
    ctx = all_ctx if F == 4 else ctx
    buckets = _buckets(F, D, 100 * F + D)
    model = _model(F, 3, 66)
    tot, got = _loglik(ctx, model, buckets)
    assert ctx.last_ll_path() == "gaps_reg2"
    tpw = 64 >> (F - 1)
    info = ctx.last_launch_info()
    assert (info["threads"], info["tracks_per_block"], info["lds_bytes"]) == (256, 4 * tpw, 14848 + 1024 * tpw * D), info
    _compare(tot, got, _reference(buckets, F, 3), "F=%d D=%d" % (F, D))
    tot2, flat2 = ctx.loglik(model, per_track=True, gaps=True)
    assert tot2 == tot and np.array_equal(flat2, np.concatenate(got))


def test_stay_factor_sets_in_inside_a_run_of_gaps(ctx, all_ctx):
    """min_len 9, larger than the window: the switch to the stay-in-field-of-view table falls into the missed rows 3 .. F + 4 of track 7."""
    for F, D in ((6, 2), (4, 3), (7, 1)):
        buckets = _buckets(F, D, 7 * F + D, lengths=(F + 2, 14, 40))
        c = all_ctx if F == 4 else ctx
        tot, got = _loglik(c, _model(F, 9, 40), buckets)
        assert c.last_ll_path() == "gaps_reg2"
        _compare(tot, got, _reference(buckets, F, 9), "min_len 9, F=%d D=%d" % (F, D))


@pytest.mark.parametrize("F", [4, 6])
def test_long_run_of_missing_rows(ctx, all_ctx, F):
    """One 300-position track with 250 rows missed, one dimension (the reference's own rounding noise: tests/test_hip_gaps.py)."""
    rng = np.random.default_rng(8 + F)
    Cs = _walk(rng, 2, 300, 1)
    miss = np.zeros(300, bool)
    miss[rng.permutation(np.arange(1, 299))[:250]] = True
    Cs[0, miss] = np.nan
    ctx = all_ctx if F == 4 else ctx
    tot, got = _loglik(ctx, _model(F, 3, 300), [Cs])
    assert ctx.last_ll_path() == "gaps_reg2"
    _compare(tot, got, _reference([Cs], F, 3), "300 x 1, 250 missed, F=%d" % F)


def test_frame_len_4_is_upgraded_on_request_only(ctx, all_ctx):
    """A default context keeps frame_len 4 on the general gap body (values as before); the requested set upgrades 4 and still 5 .. 7."""
    buckets = _buckets(4, 2, 17, lengths=(3, 6, 14, 40))
    model = _model(4, 3, 40)
    tot, got = _loglik(ctx, model, buckets)
    assert ctx.last_ll_path() == "gaps"
    _compare(tot, got, _reference(buckets, 4, 3), "frame_len 4, default context")
    tot1, got1 = _loglik(all_ctx, model, buckets)
    assert all_ctx.last_ll_path() == "gaps_reg2"
    np.testing.assert_allclose(np.concatenate(got1), np.concatenate(got), rtol=1e-13, atol=1e-10)
    for F in (5, 6, 7):
        _loglik(all_ctx, _model(F, 3, 40), buckets)
        assert all_ctx.last_ll_path() == "gaps_reg2"


def test_what_keeps_the_general_gap_body(ctx, lds_ctx):
    """Per-peak errors, one error per dimension, three states, posteriors and a context created under EXTRACK_LL_PATH=lds: path "gaps", values as
    before (against the reference); extrack_predict_gaps on the upgrading context stays on "gaps" and the likelihood after it is upgraded again."""
    F, D = 5, 2
    buckets = _buckets(F, D, 3, lengths=(3, F + 1, 14, 40))
    Lmax = 40
    rng = np.random.default_rng(5)
    # per-peak errors (locerr_mode 1)
    from extrack_amd import _lib, engine
    sig = [rng.uniform(0.01, 0.05, b.shape[:2] + (1,)) for b in buckets]
    for s, b in zip(sig, buckets):
        s[np.isnan(b[:, :, 0])] = np.nan
    peak = _lib.ModelHandle(DS, FS, TM, engine.p_stay_table(DS, 2, 1, R.CELL), R.PBL, 1, F, 3, Lmax, locerr=None, locerr_mode=1)
    tot, got = _loglik(ctx, peak, buckets, sig)
    assert ctx.last_ll_path() == "gaps"
    ref = [R.loglik_and_preds(b, s, DS, FS, TM, R.PBL, int(b.shape[1] != Lmax), R.CELL, F, 3)[0] for b, s in zip(buckets, sig)]
    _compare(tot, got, ref, "per-peak errors")
    # one error per dimension
    tot, got = _loglik(ctx, _model(F, 3, Lmax, le=(0.02, 0.03)), buckets)
    assert ctx.last_ll_path() == "gaps"
    _compare(tot, got, _reference(buckets, F, 3, le=((0.02, 0.03),)), "one error per dimension")
    # three states
    tot, got = _loglik(ctx, _model(F, 3, Lmax, S=3), buckets)
    assert ctx.last_ll_path() == "gaps"
    _compare(tot, got, _reference(buckets, F, 3, S=3), "three states")
    # two states, one global error: upgraded; posteriors of the same context are not, and do not change what the next likelihood runs
    model = _model(F, 3, Lmax)
    tot, got = _loglik(ctx, model, buckets)
    assert ctx.last_ll_path() == "gaps_reg2"
    pr = ctx.predict(model, 2, gaps=True)
    assert ctx.last_ll_path() == "gaps"
    np.testing.assert_allclose(pr, _reference(buckets, F, 3, preds=True)[2], rtol=0, atol=1e-9)
    tot2, flat2 = ctx.loglik(model, per_track=True, gaps=True)
    assert ctx.last_ll_path() == "gaps_reg2" and tot2 == tot and np.array_equal(flat2, np.concatenate(got))
    # the switch: EXTRACK_LL_PATH=lds
    tot3, got3 = _loglik(lds_ctx, model, buckets)
    assert lds_ctx.last_ll_path() == "gaps"
    _compare(tot3, got3, _reference(buckets, F, 3), "EXTRACK_LL_PATH=lds")


def test_upgraded_path_against_the_general_gap_body(ctx, lds_ctx):
    """The same data through both kernels: one bucket of 20 000 x 12 with 25 % of the interior rows missed (frame_len 6), and one of 70 000 x 9 at
    frame_len 7, large enough that - by last_launch_info - every wave of the upgraded launch walks at least two batches."""
    from extrack_amd import synth
    for F, N, L, D in ((6, 20000, 12, 2), (7, 70000, 9, 1)):
        tr = synth.drop_positions(synth.brownian_tracks(N, L, list(Ds2), TM.tolist(), list(FS), LocErr=LE, dt=R.DT, dims=D, seed=F), 0.25, seed=F)
        model = _model(F, 3, L)
        t1, (l1,) = _loglik(ctx, model, [tr])
        assert ctx.last_ll_path() == "gaps_reg2"
        info = ctx.last_launch_info()
        if F == 7:
            assert N >= 2 * info["blocks"] * info["tracks_per_block"], info  # a block's four waves take tracks_per_block tracks per round
        t0, (l0,) = _loglik(lds_ctx, model, [tr])
        assert lds_ctx.last_ll_path() == "gaps"
        assert np.all(np.isfinite(l0))
        print("F=%d %d x %d: max |dLL| %.2e, total rel. %.2e" % (F, N, L, np.abs(l1 - l0).max(), abs(t1 - t0) / abs(t0)))
        np.testing.assert_allclose(l1, l0, rtol=1e-13, atol=1e-10)
        assert abs(t1 - t0) <= 1e-12 * abs(t0), (t1, t0)


def test_poison_rules_through_the_abi(ctx):
    F = 6
    buckets = _buckets(F, 2, 11, lengths=(F + 1, 14, 40))
    model = _model(F, 3, 40)
    _, clean = _loglik(ctx, model, buckets)
    dirty = [b.copy() for b in buckets]
    dirty[1][8, 5] = [np.nan, 0.3]   # a row with one NaN coordinate
    dirty[2][8, 33] = [0.1, np.nan]  # ... in the second staging chunk
    dirty[1][3, 0] = np.nan          # NaN first row
    dirty[2][5, -1] = np.nan         # NaN last row
    tot, got = _loglik(ctx, model, dirty)
    assert ctx.last_ll_path() == "gaps_reg2" and np.isnan(tot)
    bad = {1: [3, 8], 2: [5, 8]}
    for i in range(len(dirty)):
        keep = np.ones(len(dirty[i]), bool)
        keep[bad.get(i, [])] = False
        assert np.all(np.isnan(got[i][~keep])) and np.array_equal(got[i][keep], clean[i][keep]) and np.all(np.isfinite(clean[i]))


def test_fit_on_the_upgraded_path():
    """param_fitting(gaps=True) on the 3000 x 12 dataset of tests/test_hip_gaps.py (25 % of the interior rows missed): ends inside the same D1
    interval, its objective within 1e-9 relative of the reference; the launch of that dataset is an upgraded one."""
    from extrack_amd import _lib, synth, tracking as T
    from extrack_amd.lmfit_compat import Parameters
    vals = dict(D0=1e-3, D1=0.25, LocErr=0.02, F0=0.6, F1=0.4, p01=0.1, p10=0.1, pBL=0.1)
    Tm = O.extract_params(vals, 0.02, 1, 1)[3]
    tr = synth.brownian_tracks(3000, 12, [1e-3, 0.25], Tm, [0.6, 0.4], seed=5)
    mask = np.random.default_rng(11).random((3000, 12)) < 0.25
    mask[:, 0] = mask[:, -1] = False
    gapped = tr.copy()
    gapped[mask] = np.nan
    p = Parameters()
    for k, v in vals.items():
        p.add(k, value=0.4 if k == "D1" else v, min=0.0 if k == "D1" else -np.inf, max=3.0 if k == "D1" else np.inf, vary=k == "D1")
    fit = T.param_fitting({"12": gapped}, 0.02, params=p, nb_states=2, frame_len=6, verbose=0, cell_dims=[1], gaps=True)
    d1 = fit.params["D1"].value
    ref = R.objective(dict(vals, D1=d1), {"12": gapped}, 0.02, (1,), 6)
    print("gaps=True: D1 %.4f, objective %.9f, reference %.9f (%s)" % (d1, fit.residual[0], ref, fit.gradient_why))
    assert fit.gradient_path == "fd" and "gap" in fit.gradient_why
    assert 0.22 <= d1 <= 0.29, d1
    assert abs(fit.residual[0] - ref) <= 1e-9 * abs(ref), (fit.residual[0], ref)
    LocErr, ds, Fs, TrMat, pBL = O.extract_params(dict(vals, D1=d1), 0.02, 1, 1)
    from extrack_amd import engine
    c = _lib.Context(0)
    try:
        c.upload_bucket(gapped, None)
        m = _lib.ModelHandle(ds, Fs, TrMat, engine.p_stay_table(ds, 2, 1, [1.0]), pBL, 1, 6, 12, 12, locerr=[0.02])
        tot = c.loglik(m, gaps=True)
        assert c.last_ll_path() == "gaps_reg2" and abs(-tot - ref) <= 1e-9 * abs(ref), (c.last_ll_path(), tot, ref)
    finally:
        c.close()
