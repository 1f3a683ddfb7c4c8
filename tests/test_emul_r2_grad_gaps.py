"""The gap-aware GRADIENT instantiation of the register-resident 2-state body (extrack_amd/csrc/xt_reg2.h: xt_r2_body<.., NP > 0, .., GAPS>, DESIGN.md
section 27) on CPU threads (tests/emul/emul_r2_grad_gap.cpp) under the product's own decisions - xt_grad_pick(gaps), xt_grad_gap_reg2,
xt_grad_gap_reg2_lazy, the uniform / full split and the pass sizes of xt_grad_run_reg2.  Every launch asserts that it was upgraded (path 5,
XT_GRAD_GAPS_REG2) and which variant ran (lazily normalised or guarded).
Reference: ``grad_gap_reference.reference`` (Richardson differences of the unchanged oracle) on the four cases of tests/r2_grad_gap_cases.py, stored in
tests/golden/r2_grad_gap_reference.npz (checked here to be current).  Metrics, unchanged: ``test_emul_grad_gaps.check_against_reference`` (LL per
track rtol 1e-13 / atol 1e-10, totals 1e-12, |g - fd| <= 1e-6 |fd| + est after ``assert_condition``) and ``assert_bodies_agree`` (1e-9 relative +
1e-12) against the emulated gap body of xt_gradr.h (tests/emul/emul_grad_gap.cpp), the kernel these launches ran on before."""
import shutil

import numpy as np
import pytest

import gap_reference as R
import grad_gap_reference as GR
import r2_grad_gap_cases as RC
from test_emul_grad_gaps import assert_bodies_agree, check_against_reference
from test_emul_grad_gaps import emulate as emulate_general
from test_emul_r2_gaps import masks, walk

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


def tpw(F):
    return 64 >> (F - 1)


def served(case, dirs, lazy=True, passes=None, **kw):
    """(LL, sum LL, gradient, scores) of a launch that must have been upgraded, with the register-resident geometry and the expected variant."""
    ll, tot, g, sc, info = RC.emulate(case, dirs, guarded=not lazy, **kw)
    F = case["F"]
    assert info[0] == RC.GAPS_REG2 and info[1] == int(lazy) and info[2:4] == [4 * tpw(F), 256], info
    assert passes is None or info[4] == passes, info
    return ll, tot, g, sc


def short_dirs(case):
    """Five of the case's directions: one diffusion variance, one transition, one fraction, the localisation error and the uniform pBL."""
    dirs = GR.directions(case)
    names = [d[0] for d in dirs]
    pick = [names.index(n) for n in (names[1], [n for n in names if n.startswith("T")][1], [n for n in names if n.startswith("F")][0], "le0", "pBL")]
    return [dirs[i] for i in pick]


@pytest.mark.parametrize("D,F", RC.CASES)
def test_cases_against_reference_and_the_general_gap_body(D, F):
    """The four cases, five buckets in one launch, 10 directions: two passes of full directions (5 + 4) with the uniform pBL riding on the first; the lazy
    and the guarded variant against the reference and against the emulated xt_gradr.h gap body."""
    case = RC.make(D, F)
    assert [b.shape[1] for b in case["buckets"]] == [2, 3, F + 1, 14, 40] and any(m.any() for m in case["masks"])
    ref = GR.reference(case, RC.key(D, F))
    RC.assert_golden_is_current(case, RC.key(D, F), ref)  # what the GPU test reads
    assert [d[0] for d in ref["dirs"]][-2:] == ["le0", "pBL"] and len(ref["dirs"]) == 10
    general = emulate_general(case, 4, ref["dirs"])
    for lazy in (True, False):
        got = served(case, ref["dirs"], lazy=lazy, passes=2)
        check_against_reference("D %d F %d %s" % (D, F, "lazy" if lazy else "guarded"), case, ref, *got)
        assert_bodies_agree(got, general)


@pytest.mark.parametrize("F", [4, 5, 6, 7])
def test_edge_shapes_against_the_general_gap_body(F):
    """The likelihood's edge shapes (test_emul_r2_gaps.walk / masks): L = F - 1 .. F + 2, 34, 66 with a gap at t = 1 and at L - 2, a run longer than the
    window, every interior row missed, rows 30..33 (a run across the 32-row staging chunk, a gap as the first row of the second chunk), a third chunk;
    N = 1, tpw - 1, tpw, tpw + 1 and 2 tpw + 1 tracks (empty slots, complete and partial batches)."""
    D = RC.DIMS[F]
    rng = np.random.default_rng(270 + F)
    t = tpw(F)
    for L, Ns in ((F - 1, (9,)), (F, (9,)), (F + 1, (9,)), (F + 2, (1, t + 1, 9)), (34, (t, max(2 * t + 1, 9))), (66, (max(t - 1, 1), 9))):
        for N in Ns:
            Cs = walk(rng, max(N, 9), L, D)
            m = masks(rng, max(N, 9), L, F)
            if L == 66:
                m[5, 60:65] = True
                m[6, 31:34] = m[6, 63:65] = True
            Cs[m] = np.nan
            case = RC.simple_case([Cs[:N]], D, F)
            dirs = short_dirs(case)
            general = emulate_general(case, 4, dirs)
            for lazy in (True, False):
                got = served(case, dirs, lazy=lazy, passes=1)
                assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[3]))
                assert_bodies_agree(got, general)


@pytest.mark.parametrize("F", [4, 5, 6, 7])
def test_block_stride_resets_the_gap_state(F):
    """One block walking ten batches (nine complete and a partial one for its four waves): consecutive tracks alternate gapped, gap-free and poisoned (a row
    with one NaN coordinate where there are two, a NaN first row, a NaN last row), so every slot of a wave sees all three kinds in turn - mask, count and
    NaN flag of a track must not leak into the next track of the slot.  Poisoned tracks are NaN in LL and scores, alone."""
    D = RC.DIMS[F]
    rng = np.random.default_rng(F * 7 + D)
    t = tpw(F)
    N, L = 9 * 4 * t + t // 2 + 1, 38
    Cs = walk(rng, N, L, D)
    m = rng.random((N, L)) < 0.3
    m[:, 0] = m[:, -1] = False
    kind = (np.arange(N) + np.arange(N) // t) % 3  # shifts by one per batch
    m[kind == 1] = False
    Cs[m] = np.nan
    for j, i in enumerate(np.flatnonzero(kind == 2)):
        Cs[i] = walk(rng, 1, L, D)[0]
        if j % 3 == 0 and D > 1:
            Cs[i, 5 + j % 28, 1] = np.nan
        elif j % 3 == 1:
            Cs[i, 0] = np.nan
        else:
            Cs[i, -1] = np.nan
    case = RC.simple_case([Cs], D, F)
    dirs = short_dirs(case)
    ll, _, _, sc = served(case, dirs, blocks=1)
    bad = kind == 2
    assert np.array_equal(np.isnan(ll), bad) and np.array_equal(np.isnan(sc).all(axis=1), bad) and np.array_equal(np.isnan(sc).any(axis=1), bad)
    general = emulate_general(case, 4, dirs)
    assert_bodies_agree((ll[~bad], sc[~bad]), (general[0][~bad], general[3][~bad]))


@pytest.mark.parametrize("F", [4, 5, 6, 7])
def test_flag_on_gap_free_data_is_the_plain_body(F):
    """Gap-free data: the flag changes nothing - LL, sums and scores bit for bit (every select passes the observed value, the count of missed rows is 0),
    in the lazy and (frame_len 4, 5) in the guarded variant."""
    from extrack_amd import synth
    D = RC.DIMS[F]
    case = RC.make(D, F)
    Ds, Tm, Fs = R.MODELS[2]
    full = [synth.brownian_tracks(len(b), b.shape[1], list(Ds), Tm.tolist(), list(Fs), dt=R.DT, dims=D, seed=3 + i) for i, b in enumerate(case["buckets"])]
    dirs = GR.directions(case)
    for lazy in ((True, False) if F <= 5 else (True,)):  # the guarded variant at the two cheaper frame lengths
        a = served(case, dirs, lazy=lazy, buckets=full)
        b = RC.emulate(case, dirs, gaps=False, buckets=full, guarded=not lazy)
        assert b[4][0] == RC.REG2 and b[4][1] == int(lazy), b[4]
        assert np.all(np.isfinite(a[0])) and np.all(np.isfinite(a[3]))
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


@pytest.mark.parametrize("F", [4, 6, 7])
def test_poison_rules(F):
    """A row with only some NaN coordinates (in the first steps, in a steady step, in the second chunk), a NaN first row and a NaN last row give their track
    a NaN LL and NaN scores; every other track equals the clean launch bit for bit.  One dimension (frame_len 4) has no partly-NaN row."""
    D = RC.DIMS[F]
    rng = np.random.default_rng(F)
    N, L = 11, 37
    Cs = walk(rng, N, L, D)
    m = rng.random((N, L)) < 0.25
    m[:, 0] = m[:, -1] = False
    Cs[m] = np.nan
    case = RC.simple_case([Cs], D, F)
    dirs = short_dirs(case)
    clean = served(case, dirs, blocks=1)
    dirty = Cs.copy()
    bad = [6, 9]
    dirty[6, 0] = np.nan
    dirty[9, -1] = np.nan
    if D > 1:
        for i, t_, d in ((1, 2, 1), (3, F + 3, 0), (4, 33, 1)):
            dirty[i, t_] = 0.3
            dirty[i, t_, d] = np.nan
        bad += [1, 3, 4]
    got = served(case, dirs, blocks=1, buckets=[dirty])
    keep = np.ones(N, bool)
    keep[bad] = False
    assert np.all(np.isfinite(clean[0])) and np.all(np.isfinite(clean[3]))
    assert np.all(np.isnan(got[0][bad])) and np.all(np.isnan(got[3][bad]))
    assert np.array_equal(got[0][keep], clean[0][keep]) and np.array_equal(got[3][keep], clean[3][keep])


@pytest.mark.parametrize("F", [4, 5, 6, 7])
def test_coordinate_of_a_missed_row_is_never_used(F):
    """NaN or 123.0 as the coordinates of the missed rows in the staged array (the rows are classified from the NaN input; the emulated staging then leaves
    123.0 in LDS where the product leaves the NaN): the same bits in LL, sums and scores; both variants at frame_len 4, 5."""
    D = RC.DIMS[F]
    case = RC.make(D, F)
    dirs = GR.directions(case)
    for lazy in ((True, False) if F <= 5 else (True,)):  # the guarded variant at the two cheaper frame lengths
        a = served(case, dirs, lazy=lazy)
        assert np.all(np.isfinite(a[0])) and np.all(np.isfinite(a[3]))
        again = served(case, dirs, lazy=lazy, fill=123.0)
        assert np.array_equal(a[0], again[0]) and a[1] == again[1] and np.array_equal(a[2], again[2]) and np.array_equal(a[3], again[3])


@pytest.mark.parametrize("F", [4, 5])
def test_directions_per_pass(F):
    """One direction and eight full directions each run in ONE pass (NP = 1, NP = 8); nine full directions with at most 3 and at most 8 per pass (three
    passes of 3, two of 5 + 4) give the same sums to 1e-12 and every pass count is what xt_grad_run_reg2 computes."""
    D = RC.DIMS[F]
    case = RC.make(D, F)
    dirs = GR.directions(case)
    full = [d for d in dirs if d[0] != "pBL"]
    assert len(full) == 9
    one = served(case, full[:1], passes=1)
    eight = served(case, full[:8], passes=1)
    a = served(case, dirs, passes=2, maxnp=8)
    b = served(case, dirs, passes=3, maxnp=3)
    assert np.all(np.abs(a[2] - b[2]) <= 1e-12 * np.abs(a[2])) and abs(a[1] - b[1]) <= 1e-12 * abs(a[1])
    assert np.all(np.abs(a[3] - b[3]) <= 1e-12 * np.abs(a[3]) + 1e-15)
    assert abs(one[2][0] - a[2][0]) <= 1e-12 * abs(a[2][0]) and np.all(np.abs(eight[2] - a[2][:8]) <= 1e-12 * np.abs(a[2][:8]))
    assert np.array_equal(one[0], a[0]) and np.array_equal(eight[0], a[0])  # the primal recursion does not depend on the directions


def test_lds_block_of_the_gap_gradient_launch():
    """One size function for kernel, launcher and emulator: 512 bytes (16 per wave and slot) after everything xt_r2_block_bytes(NP + NU, D, 0, tpw) counts,
    within the 64 KiB a launch gets without asking."""
    L = RC.lib(6)
    for F in (4, 5, 6, 7):
        for D in (1, 2, 3):
            for NPT in (1, 5, 8, 12):
                g, p = L.xt_emul_r2gg_block_bytes(NPT, D, tpw(F), 1), L.xt_emul_r2gg_block_bytes(NPT, D, tpw(F), 0)
                assert g == p + 512 and g <= 64 * 1024 and g % 8 == 0, (F, D, NPT, g, p)


def test_what_is_not_upgraded_is_reported_not_run():
    """Frame_len 4 in a default context and EXTRACK_GRAD_PATH=gradr | lds keep the general gap kernels: the emulated launcher reports their path and runs
    nothing.  A model beyond the gap-extended range is upgraded all the same, on the guarded variant."""
    case4 = RC.make(1, 4)
    dirs = GR.directions(case4)
    assert RC.emulate(case4, dirs, fmask=RC.F_DEFAULT)[4][0] == RC.GRADR and RC.emulate(case4, dirs, fmask=RC.F_ALL)[4][0] == RC.GAPS_REG2
    case6 = RC.make(2, 6)
    dirs = GR.directions(case6)
    assert RC.emulate(case6, dirs, grad_reg2=2)[4][0] == RC.GRADR and RC.emulate(case6, dirs, grad_reg2=0)[4][0] == RC.LDS
    assert RC.emulate(case6, dirs, fmask=1 << 4)[4][0] == RC.GRADR
    big = np.array([30.0, 60.0])  # d2max = 3600: (Lmax - 2) d2max = 136 800 > 1e4 - well scaled without gaps (2 l2 + d2max <= 1e4), guarded with them
    info = RC.emulate(case6, dirs, ds=big)[4]
    assert info[:2] == [RC.GAPS_REG2, 0], info
    tiny = RC.emulate(case6, dirs, le=1e-7, ds=np.array([1e-8, 0.1]))[4]  # l2 + d2min = 1e-14 + 1e-16 < 1e-12: not well scaled at all
    assert tiny[:2] == [RC.GAPS_REG2, 0], tiny
