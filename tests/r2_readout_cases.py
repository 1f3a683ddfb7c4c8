"""Inputs shared by tests/test_emul_r2_readout.py (CPU threads) and tests/test_hip_r2_readout.py (GPU): the shapes at which the log-carried
read-out of the last position (extrack_amd/csrc/xt_reg2.h) can go wrong.  Not a test module.

Model and localisation error are those of tests/test_emul_r2_gform.py.  N = 2 (64 >> (F - 1)) 4 + 1 tracks unless a case says otherwise: two
workgroups of four waves and a partial batch."""
import numpy as np

DS, FS, TM = np.array([0.004, 0.1]), np.array([.35, .65]), np.array([[.92, .08], [.15, .85]])
LE = 0.02
TOL_LL = 1e-10
FS_ALL, DS_ALL = (4, 6, 7), (1, 2, 3)
SMALL_L2 = [(6, 3, 1e-5), (7, 3, 2e-6), (4, 2, 1e-5)]  # the (F, D, le) triples of test_logcarry_small_l2
OUTLIER_L = (8, 12, 33)
# Outlier cases.  The bound is not invented but taken from the parent commit, by this rule: run the parent commit's library (EXTRACK_HIP_LIB)
# on exactly these inputs, take its largest |LL - oracle| / |LL|, allow 4 x that (for the different rounding order of a plain sum), but not
# less than 4 ulp of |LL|.  Measured on MI355X, parent: 0.562 on the track shifted by 520, in every one of the 18 cases (its read-out's
# exponential clamps at -1.1e7 where the argument is -2.5e7; LL = -1.1e7 instead of -2.5e7), and 5.94e-16 (3.00 ulp) on the tracks shifted by
# 20.  The rule is applied per population, which is never wider than applying it to the pool: the tracks shifted by 20 get
# max(4 x 5.94e-16 |LL|, 4 ulp) = 2.4e-15 |LL|; the track shifted by 520 gets 4 x 0.562 |LL|, which is no check of accuracy (the parent is
# wrong there) - it must be finite, and its error is printed.  This build: at most 4.00 ulp (7.9e-16 relative) over all tracks on MI355X; in
# the emulation 4 ulp on the tracks shifted by 20 and 3 ulp on the 520 one.
PARENT_REL_520 = 0.562
PARENT_REL_20 = 5.94e-16
SHIFTED_520 = 3


def n_default(F):
    return 2 * (64 >> (F - 1)) * 4 + 1


def walk(rng, N, L, D):
    return np.cumsum(rng.normal(0, 0.08, (N, L, D)), 1)


def lengths(F):
    """3, F, F + 1: read-out straight after the chain or after the merge-free first step (3: no step at all); F + 2 .. 2 F: the last position
    on every exchange phase; 32, 33, 34: last row of the first staging chunk, first and second row of the second; 65."""
    return sorted({3, F, F + 1} | set(range(F + 2, 2 * F + 1)) | {32, 33, 34, 65})


def length_cases(F, D):
    rng = np.random.default_rng(3000 + F * 10 + D)
    return [("L=%d" % L, walk(rng, n_default(F), L, D)) for L in lengths(F)]


def outlier_cases(F, D, last_only):
    """The last position (last_only) or every position from L - 2 on shifted by 20, one track's by 520."""
    rng = np.random.default_rng(4000 + F * 10 + D + (0 if last_only else 100))
    out = []
    for L in OUTLIER_L:
        Cs = walk(rng, n_default(F), L, D)
        sh = np.full(len(Cs), 20.0)
        sh[SHIFTED_520] = 520.0
        Cs[:, (L - 1 if last_only else L - 2):] += sh[:, None, None]
        out.append(("L=%d" % L, Cs))
    return out


def small_l2_cases(F, D):
    rng = np.random.default_rng(5000 + F * 10 + D)
    return [("L=%d" % L, walk(rng, n_default(F), L, D)) for L in (F + 2, 33)]


def single_track_cases(F, D):
    rng = np.random.default_rng(6000 + F * 10 + D)
    tpw = 64 >> (F - 1)
    return [("N=%d L=%d" % (N, L), walk(rng, N, L, D)) for N in (1, tpw + 1) for L in (3, F + 3, 33)]


def nan_case(F, D, L):
    """Track 1 (the second slot of the first wave where a wave holds several tracks) has one NaN coordinate in its last row, track 5 one in a
    steady step."""
    rng = np.random.default_rng(7000 + F * 10 + D + L)
    Cs = walk(rng, n_default(F), L, D)
    Cs[1, L - 1, D - 1] = np.nan
    Cs[5, min(F + 1, L - 2), 0] = np.nan
    bad = np.zeros(len(Cs), bool)
    bad[[1, 5]] = True
    return Cs, bad


def gap_cases(F, D):
    """25 % of the interior rows missed, at L = F + 2, 12, 33; track 0 gap-free, track 1 with row L - 2 missed alone, track 2 with row L - 2
    missed on top of its random rows."""
    rng = np.random.default_rng(8000 + F * 10 + D)
    out = []
    for L in sorted({F + 2, 12, 33}):
        Cs = walk(rng, max(n_default(F), 9), L, D)
        m = rng.random(Cs.shape[:2]) < 0.25
        m[0] = m[1] = False
        m[1, L - 2] = m[2, L - 2] = True
        m[:, 0] = m[:, -1] = False
        Cs[m] = np.nan
        out.append(("L=%d" % L, Cs))
    return out


def check_outlier(ll, ref, what):
    """Finite, and within the parent-derived bound of the oracle (see above); returns the largest error in ulp of |LL|."""
    assert np.all(np.isfinite(ref)), what
    assert np.all(np.isfinite(ll)), (what, ll)
    err, ulp = np.abs(ll - ref), np.spacing(np.abs(ref))
    is520 = np.arange(len(ll)) == SHIFTED_520
    print("%s: |LL| %.5g .. %.5g; tracks shifted by 20: max %.2f ulp (%.3e relative); by 520: %.2f ulp (%.3e relative)"
          % (what, np.abs(ref).min(), np.abs(ref).max(), (err / ulp)[~is520].max(), (err / np.abs(ref))[~is520].max(), (err / ulp)[is520].max(),
             (err / np.abs(ref))[is520].max()))
    assert np.abs(ref).min() > 1e4  # every track is beyond the range of the absolute tolerance
    bound = np.where(is520, np.maximum(4 * PARENT_REL_520 * np.abs(ref), 4 * ulp), np.maximum(4 * PARENT_REL_20 * np.abs(ref), 4 * ulp))
    assert np.all(err <= bound), (what, (err / ulp).max())
    return (err / ulp).max()
