"""CPU check of the per-track score store: the epilogues of the three forward-mode gradient bodies (xt_reg2.h, xt_gradr.h, xt_grad.h) run
on CPU threads through the bucket-descriptor table (tests/emul/emul_scores.cpp), three buckets launched longest first whose rows are in
upload order - against Richardson central differences of the oracle's per-track log-likelihood (1e-6, the project's gradient tolerance,
per track), against the gradient of the same run, and against the run without a score pointer (bit-identical sums)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul"))

from test_hip_scores import _CELL, _DT, _LE, _MINLEN, _MODELS, _PBL, _dirs, _pool, assert_scores_match  # helpers only (no GPU)


@pytest.mark.parametrize("family,S", [(2, 2), (4, 2), (3, 3), (0, 2), (1, 3)])
def test_emulated_score_store(family, S):
    import run_emul_scores as R
    from oracle import oracle_np as O
    F, shapes = 4, ((2, 4), (3, 5), (9, 14))  # (L, N) in upload order; launched longest first
    Lmax = max(L for L, _ in shapes)
    parts = [_pool(S, L, N, F, int(L != Lmax)) for L, N in shapes]
    row0 = np.concatenate([[0], np.cumsum([N for _, N in shapes])])[:-1]
    order = [2, 1, 0]
    Ds, Tm, Fs = _MODELS[S]
    ds = np.sqrt(2 * Ds * _DT)
    dirs = _dirs(S)
    args = (family, [parts[i][0] for i in order], [row0[i] for i in order], _LE, ds, Fs, Tm, _PBL, O.p_stay_table(ds, S, 1, _CELL), 1, F, _MINLEN, Lmax,
            [d[1] for d in dirs])
    ll, g, sc = R.run_scores(*args)
    fd = np.concatenate([p[1] for p in parts])
    assert sc.shape == fd.shape and np.all(np.isfinite(sc))
    assert_scores_match(sc, fd, "emulated family %d:" % family)
    N = len(sc)
    assert np.all(np.abs(sc.sum(0) - g) <= 4 * N * np.finfo(float).eps * np.abs(sc).sum(0))
    ref = sum(O.proba_cs(p[0], _LE[None, None], ds, Fs, Tm, _PBL, int(L != Lmax), _CELL, 1, F, _MINLEN).sum() for p, (L, _) in zip(parts, shapes))
    assert abs(ll - ref) <= 1e-12 * abs(ref)
    ll0, g0, sc0 = R.run_scores(*args, with_scores=False)
    assert ll0 == ll and np.array_equal(g0, g) and np.all(np.isnan(sc0))  # a null score pointer: same sums, nothing stored
