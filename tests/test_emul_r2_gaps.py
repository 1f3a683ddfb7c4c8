"""The gap-aware likelihood-only instantiation of the register-resident 2-state body (extrack_amd/csrc/xt_reg2.h: xt_r2_body<.., GAPS>, DESIGN.md
section 25) on CPU threads (tests/emul/emul_r2_gap.cpp) under the product's own decisions - xt_ll_pick(gaps), xt_launch_scaling,
xt_ll_gap_reg2 - against the reference built from the unchanged oracle (tests/gap_reference.py, error 1e7 at the missed rows).  Every launch
asserts that it was upgraded (path 7, XT_LL_GAPS_REG2) and ran g-form steps (scaling 2).  Tolerances: per-track LL rtol 1e-13 / atol 1e-10,
totals 1e-12 relative (tests/test_hip_gaps.py)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import gap_reference as R
from oracle import oracle_np as O

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

GAPS_REG2, REG2, GAPS = 7, 1, 5
F_DEFAULT, F_ALL = 0xe0, 0xf0  # frame lengths a context upgrades (bit F): by default 5, 6, 7; frame_len 4 on request (EXTRACK_GAP_REG2_F)
DS_, TM, FS = R.MODELS[2]
DS = np.sqrt(2 * DS_ * R.DT)
LE = 0.02
HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul")
CSRC = os.path.join(HERE, "..", "..", "extrack_amd", "csrc")
_lib = None


def gap_lib():
    """tests/emul/emul_r2_gap.cpp -> tests/emul/libxt_emul_r2_gap.so (rebuilt when a source it includes is newer)."""
    global _lib
    if _lib is None:
        so, src = os.path.join(HERE, "libxt_emul_r2_gap.so"), os.path.join(HERE, "emul_r2_gap.cpp")
        deps = [src, os.path.join(HERE, "emul_ctx.h")] + [os.path.join(CSRC, h) for h in ("xt_kernel.h", "xt_math.h", "xt_tables.h", "xt_fast2.h", "xt_grad.h", "xt_reg2.h", "xt_ll_geom.h")]
        if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-pthread", "-shared", src, "-o", so])
        _lib = C.CDLL(so)
    return _lib


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def emul(Cs, F, isBL, min_len, nblocks=2, gaps=True, ll_reg2=1, le=LE, ds=DS, fmask=None):
    """(rc, per-track LL, total, info = [path, scaling, tracks per block, LDS bytes]) of one emulated launch.  fmask: the context's frame
    lengths; None: the default where it upgrades F, the requested set at frame_len 4."""
    fmask = (F_DEFAULT if (F_DEFAULT >> F) & 1 else F_ALL) if fmask is None else fmask
    Cs = np.ascontiguousarray(Cs, float)
    N, L, D = Cs.shape
    ps = np.ascontiguousarray(O.p_stay_table(ds, 2, 1, R.CELL), float)
    ll, tot, info = np.zeros(N), C.c_double(0), (C.c_int * 4)()
    dsc, Fsc, Tc = [np.ascontiguousarray(x, float) for x in (ds, FS, TM)]
    rc = gap_lib().xt_emul_r2_gap_run(_dp(Cs), C.c_longlong(N), L, D, F, int(isBL), int(min_len), C.c_double(le), C.c_double(R.PBL), _dp(dsc),
                                      _dp(Fsc), _dp(Tc), _dp(ps), nblocks, int(gaps), ll_reg2, int(fmask), _dp(ll), C.byref(tot), info)
    return rc, ll, tot.value, list(info)


def reference(Cs, F, isBL, min_len, le=LE, ds=DS):
    return R.loglik_and_preds(Cs, np.array([[[le]]]), ds, FS, TM, R.PBL, isBL, R.CELL, F, min_len)[0]


def served(Cs, F, isBL, min_len, **kw):
    """Per-track LL of a launch that must have been upgraded and have run g-form steps, checked against the reference."""
    rc, ll, tot, info = emul(Cs, F, isBL, min_len, **kw)
    assert rc == 0 and info[0] == GAPS_REG2 and info[1] == 2, (rc, info)
    ref = reference(Cs, F, isBL, min_len)
    ok = np.isfinite(ref)
    assert np.array_equal(np.isnan(ll), ~ok), (np.isnan(ll), ok)
    err = np.abs(ll[ok] - ref[ok]).max() if ok.any() else 0.0
    print("F=%d shape=%s min_len=%d isBL=%d: max |dLL| %.3e" % (F, Cs.shape, min_len, isBL, err))
    np.testing.assert_allclose(ll[ok], ref[ok], rtol=1e-13, atol=1e-10, err_msg="F=%d shape=%s min_len=%d isBL=%d" % (F, Cs.shape, min_len, isBL))
    if ok.all():
        assert abs(tot - ref.sum()) <= 1e-12 * abs(ref.sum()), (tot, ref.sum())
    return ll


def walk(rng, N, L, D):
    return np.cumsum(rng.normal(0, 0.08, (N, L, D)), 1)


def masks(rng, N, L, F):
    """[N, L] missed rows: 25 % at random, with the special tracks of the issue's list in the first rows (N >= 8)."""
    m = rng.random((N, L)) < 0.25
    if L == 3:
        m[:, 1] = np.arange(N) % 2 == 0  # the only interior row
    if L >= 4:
        m[0] = False
        m[0, 1] = True               # the first step (warm-up chain)
        m[1] = False
        m[1, L - 2] = True           # the last step before the read-out
        m[2] = False
        m[2, 1:-1] = True            # every interior row
        m[3] = False                 # gap-free neighbour
        m[4] = False
        m[4, 1] = m[4, L - 2] = True
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


@pytest.mark.parametrize("F", [4, 5, 6, 7])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_short_buckets_and_the_window(F, D):
    """L = 2, 3 (the only interior row missed on every other track), F - 1, F, F + 1, F + 2: gaps in the warm-up chain, at the merge-free first
    step and at the first merged step; isBL 0 / 1; min_len 3 and F + 1.  N = 2 tracks-per-wave + 1 in two blocks: complete and partial batches."""
    rng = np.random.default_rng(F * 10 + D)
    N = max(2 * (64 >> (F - 1)) + 1, 9)
    for L in sorted({2, 3, F - 1, F, F + 1, F + 2}):
        Cs = walk(rng, N, L, D)
        Cs[masks(rng, N, L, F)] = np.nan
        for isBL, min_len in ((0, 3), (1, 3), (1, F + 1)):
            served(Cs, F, isBL, min_len)


@pytest.mark.parametrize("F", [4, 5, 6, 7])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_steady_state_and_staging_chunks(F, D):
    """L = 14 (gaps at t = 1 and t = L - 2, a run longer than the window, every interior row), L = 34 and 40 with rows 30..33 missed (a run across
    the staging boundary, a gap as the first row of the second chunk), L = 66 (a third chunk); min_len 3 and 9 - larger than the window, so the stay
    factor sets in inside the run of gaps of rows 3 .. F + 4."""
    rng = np.random.default_rng(F * 100 + D)
    N = max(2 * (64 >> (F - 1)) + 1, 9)
    for L, isBL in ((14, 0), (14, 1), (34, 1), (40, 0), (66, 1)):
        Cs = walk(rng, N, L, D)
        m = masks(rng, N, L, F)
        if L == 66:
            m[5, 60:65] = True
            m[6, 31:34] = m[6, 63:65] = True
        Cs[m] = np.nan
        for min_len in (3, 9):
            served(Cs, F, isBL, min_len)


@pytest.mark.parametrize("F", [4, 6, 7])
def test_long_run_of_missing_rows(F):
    """One 300-position track with 250 rows missed, one dimension (the reference's own rounding noise, tests/test_hip_gaps.py), beside a gap-free and
    a lightly gapped one: ten staging chunks, hundreds of transition-only steps."""
    rng = np.random.default_rng(8 + F)
    Cs = walk(rng, 3, 300, 1)
    miss = np.zeros(300, bool)
    miss[rng.permutation(np.arange(1, 299))[:250]] = True
    Cs[0, miss] = np.nan
    Cs[2, rng.random(300) < 0.25] = np.nan
    Cs[2, 0] = Cs[2, -1] = 0.1
    served(Cs, F, 0, 3, nblocks=1)


@pytest.mark.parametrize("F,D", [(4, 2), (5, 3), (6, 2), (7, 1)])
def test_block_stride_resets_the_gap_state(F, D):
    """Fewer blocks than batches: one block, nine batches and a partial one for its four waves.  Consecutive tracks alternate gapped, gap-free
    and poisoned (a row with one NaN coordinate where there are two, a NaN first row, a NaN last row), so every slot of a wave sees all three kinds in turn: the
    track's mask, count and last observed row must not leak into the next track of the slot.  Poisoned tracks are NaN, alone."""
    rng = np.random.default_rng(F * 7 + D)
    tpw = 64 >> (F - 1)
    N, L = 9 * 4 * tpw + tpw // 2 + 1, 38
    Cs = walk(rng, N, L, D)
    m = rng.random((N, L)) < 0.3
    m[:, 0] = m[:, -1] = False
    kind = (np.arange(N) + np.arange(N) // tpw) % 3  # shifts by one per batch
    m[kind == 1] = False
    Cs[m] = np.nan
    bad = np.flatnonzero(kind == 2)
    for j, i in enumerate(bad):
        Cs[i] = walk(rng, 1, L, D)[0]
        if j % 3 == 0 and D > 1:
            Cs[i, 5 + j % 28, 1] = np.nan
        elif j % 3 == 1:
            Cs[i, 0] = np.nan
        else:
            Cs[i, -1] = np.nan
    ll = served(Cs, F, 1, 3, nblocks=1)
    assert np.array_equal(np.isnan(ll), kind == 2)


@pytest.mark.parametrize("F", [4, 5, 6, 7])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_gap_free_data_match_the_plain_body(F, D):
    """Gap-free data through the GAPS body against the plain body (and the plain oracle): same tolerance, bit-identity not asserted."""
    rng = np.random.default_rng(F + 31 * D)
    N = 2 * (64 >> (F - 1)) + 1
    for L in (F + 1, 14, 40):
        Cs = walk(rng, N, L, D)
        rc0, plain, tot0, info0 = emul(Cs, F, 1, 3, gaps=False)
        assert rc0 == 0 and info0[:2] == [REG2, 2], info0
        ll = served(Cs, F, 1, 3)
        np.testing.assert_allclose(ll, plain, rtol=1e-13, atol=1e-10)
        ref = O.proba_cs(Cs, np.array([[[LE]]]), DS, FS, TM, R.PBL, 1, R.CELL, 1, F, 3)
        np.testing.assert_allclose(ll, ref, rtol=1e-13, atol=1e-10)


@pytest.mark.parametrize("F", [4, 6, 7])
def test_poison_rules(F):
    """A row with only some NaN coordinates (in the warm-up, in a steady step, in the second chunk), a NaN first row and a NaN last row give NaN for
    that track alone; the others equal the clean launch bit for bit."""
    rng = np.random.default_rng(F)
    N, L = 11, 37
    Cs = walk(rng, N, L, 2)
    m = rng.random((N, L)) < 0.25
    m[:, 0] = m[:, -1] = False
    Cs[m] = np.nan
    clean = served(Cs, F, 1, 3, nblocks=1)
    dirty = Cs.copy()
    dirty[1, 2, 0] = np.nan
    dirty[3, F + 3, 1] = np.nan
    dirty[4, 33, 0] = np.nan
    dirty[6, 0] = np.nan
    dirty[9, -1] = np.nan
    for i, t, d in ((1, 2, 1), (3, F + 3, 0), (4, 33, 1)):
        dirty[i, t, d] = 0.3  # make sure the row is partly finite whatever the random mask said
    got = served(dirty, F, 1, 3, nblocks=1)
    bad = [1, 3, 4, 6, 9]
    keep = np.ones(N, bool)
    keep[bad] = False
    assert np.all(np.isnan(got[bad])) and np.array_equal(got[keep], clean[keep]) and np.all(np.isfinite(clean))


def test_what_is_not_upgraded_is_reported_not_run():
    """Frame_len 4 in a default context, EXTRACK_LL_PATH=lds (ll_reg2 = 0), a localisation error below the g-form's bound (scaling 1) and a group beyond the gap-extended range
    keep the general gap body: the emulated launcher reports path 5 and runs nothing."""
    rng = np.random.default_rng(0)
    Cs = walk(rng, 5, 12, 2)
    rc, _, _, info = emul(Cs, 4, 1, 3, fmask=F_DEFAULT)
    assert rc == 1 and info[:2] == [GAPS, 2]
    for F in (5, 6, 7):
        assert emul(Cs, F, 1, 3, fmask=F_DEFAULT)[3][0] == GAPS_REG2 and emul(Cs, F, 1, 3, fmask=1 << 4)[3][0] == GAPS
    rc, _, _, info = emul(Cs, 6, 1, 3, ll_reg2=0)
    assert rc == 1 and info[0] == GAPS
    rc, _, _, info = emul(Cs, 6, 1, 3, le=1e-7)
    assert rc == 1 and info[:2] == [GAPS, 1]
    big = np.array([30.0, 60.0])  # d2max = 3600: (L - 2) d2max = 36 000 > 1e4 at L = 12, 7200 at L = 4
    rc, _, _, info = emul(Cs, 6, 1, 3, ds=big)
    assert rc == 1 and info[:2] == [GAPS, 2]
    rc, _, _, info = emul(Cs[:, :4], 6, 1, 3, ds=big)
    assert rc == 0 and info[:2] == [GAPS_REG2, 2]
