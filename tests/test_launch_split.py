"""The grid split of a multi-bucket launch (csrc/xt_launch_split.h), compiled for the host through tests/emul, and the global-state body
(csrc/xt_big.h) served several buckets by that split on CPU threads with a guarded scratch.

Every launch gives bucket i ceil(target * nbatch_i * (L_i - 1) / wsum) blocks, at least 1 and at most nbatch_i.  A sum of ceilings can exceed
the target by up to nb - 1 blocks; the global-state kernel's scratch holds `max_blocks` blocks and nothing more, so an unbounded split wrote
whole wavefront regions past its end.  The regression cases below are datasets where the plain formula overshoots its bound (the first
assertion of each keeps the case meaningful); xt_split_blocks must stay within it."""
import math
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emul"))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

N_CU = 256  # MI355X compute units
NW_BIG = 4  # wavefronts per block of the global-state kernel (extrack_ll.hip: xt_launch_group)


def _E():
    import run_emul as E
    return E


def old_split(target, Ns, Ls, tpb):
    """The proportional split as the launchers computed it before the cap (same float operations, same order)."""
    nbatch = [(int(n) + tpb - 1) // tpb for n in Ns]
    wsum = 0.0
    for nbt, L in zip(nbatch, Ls):
        wsum += float(nbt) * (L - 1)
    out = []
    for nbt, L in zip(nbatch, Ls):
        n = math.ceil(target * (float(nbt) * (L - 1)) / wsum)
        out.append(min(max(n, 1), nbt))
    return np.array(out, np.int64), np.array(nbatch, np.int64)


def big_ws_doubles(E, D, K):
    """csrc/xt_big.h xt_big_ws_doubles: one wavefront's region."""
    return E * 64 * (1 + D + K) + (E * 64 + 1) // 2


def big_max_blocks(S, F, D, K=1, budget_mb=32 * 1024, n_cu=N_CU):
    """Blocks of the global-state kernel's scratch budget (xt_launch_group: budget / (ws_stride x 8 B x NW), at most 8 per CU)."""
    per_block = big_ws_doubles(S ** F, D, K) * 8 * NW_BIG
    return min(max(1, (budget_mb << 20) // per_block), n_cu * 8)


# (name, S, F, D, budget MiB, tracks per bucket, lengths, blocks of the budget)
REGRESSION = [
    ("5_states_frame_len_6", 5, 6, 2, 32 * 1024, (30000, 30000, 30000), (7, 8, 10), 238),
    ("2_states_frame_len_12", 2, 12, 2, 32 * 1024, (1000000, 1000000), (20, 31), 910),
    ("forced_big_16MiB", 2, 6, 2, 16, (3000, 4100, 5200), (9, 14, 23), 28),
    ("advice_2x1e6_frame_len_12", 2, 12, 2, 32 * 1024, (1000000, 1000000), (15, 30), 910),
]


@pytest.mark.parametrize("name,S,F,D,budget,Ns,Ls,cap", REGRESSION, ids=[r[0] for r in REGRESSION])
def test_regression_split_stays_within_the_scratch_budget(name, S, F, D, budget, Ns, Ls, cap):
    """Global-state launches (256 tracks per block) whose budget binds: the launcher's target is then the budget's block count itself."""
    E = _E()
    assert big_max_blocks(S, F, D, budget_mb=budget) == cap
    target = float(max(len(Ns), cap))
    old, _ = old_split(target, Ns, Ls, 256)
    assert old.sum() > cap, (name, old)  # the plain formula overshoots here
    g, blocks = E.split_blocks(target, cap, Ns, Ls, 256)
    assert 0 < g <= cap and blocks.sum() == g, (name, g, blocks)
    assert np.all(blocks >= 1) and np.all(blocks <= old)


def test_split_property_random():
    """20 000 seeded configurations: every invariant of xt_split_blocks, and the plain formula wherever its ceilings fit."""
    E = _E()
    rng = np.random.default_rng(20261016)
    n_fit = n_trim = n_at_nb = n_tight = 0
    for case in range(20000):
        nb = int(rng.integers(1, 65))
        Ns = np.maximum(1, np.exp(rng.uniform(0.0, math.log(1e7), nb)).astype(np.int64))
        Ls = rng.integers(2, 4097, nb)
        tpb = int(rng.choice([1, 3, 64, 256]))
        target = float(math.exp(rng.uniform(0.0, math.log(1e5))))
        old, nbatch = old_split(target, Ns, Ls, tpb)
        mode = case % 4
        if mode == 0:
            cap = nb
        elif mode == 1:
            cap = max(nb, int(old.sum()) - 1)
        else:
            cap = int(rng.integers(nb, 100001))
        g, blocks = E.split_blocks(target, cap, Ns.tolist(), Ls.tolist(), tpb)
        ctx = (case, nb, tpb, target, cap)
        assert g >= nb and g <= cap, ctx
        assert len(blocks) == nb and blocks.sum() == g, ctx
        assert np.all(blocks >= 1) and np.all(blocks <= nbatch), ctx  # blk_end strictly increasing, last == grid
        if old.sum() <= cap:
            assert np.array_equal(blocks, old), ctx
            n_fit += 1
        else:
            assert g == cap and np.all(blocks <= old), ctx  # trimmed to exactly the bound, no bucket grows
            n_trim += 1
        n_at_nb += cap == nb
        n_tight += mode == 1 and old.sum() > nb
    assert n_fit > 3000 and n_trim > 3000 and n_at_nb > 4000 and n_tight > 4000, (n_fit, n_trim, n_at_nb, n_tight)


def test_split_error_paths():
    E = _E()
    assert E.split_blocks(100.0, 2, [10, 10, 10], [5, 6, 7], 1)[0] < 0  # cap < nb
    assert E.split_blocks(100.0, 50, [10, 10], [5, 1], 1)[0] < 0  # L < 2
    assert E.split_blocks(100.0, 50, [10, 0], [5, 6], 1)[0] < 0  # N < 1
    assert E.split_blocks(100.0, 50, [10, -3], [5, 6], 64)[0] < 0
    assert E.split_blocks(100.0, 50, [], [], 64)[0] < 0  # no bucket
    assert E.split_blocks(100.0, 50, [10], [5], 0)[0] < 0  # no track per block


@pytest.mark.parametrize("target", [2048.0, 2048.5, 16384.0, 1953.25, 124999.0, 125000.0, 200000.0])
def test_single_bucket_gets_ceil_target(target):
    """The headline geometry - one bucket of 1e6 x 30, 8 tracks per block of the 2-state kernel, partial-sum slots n_cu x 64 + 64 -
    gets min(nbatch, ceil(target)) blocks, as before the cap."""
    E = _E()
    nbatch = 1000000 // 8
    g, blocks = E.split_blocks(target, N_CU * 8 * 8 + 64, [1000000], [30], 8)
    assert g == min(nbatch, math.ceil(target), N_CU * 8 * 8 + 64) and blocks.tolist() == [g]


def _model(S, seed):
    rng = np.random.default_rng(seed)
    Ds = np.sort(rng.uniform(0.01, 0.3, S))
    Ds[0] = 0.001
    T = np.full((S, S), 0.05) + rng.uniform(0, 0.03, (S, S))
    T[np.arange(S), np.arange(S)] = 0
    T[np.arange(S), np.arange(S)] = 1 - T.sum(1)
    Fs = rng.dirichlet(np.ones(S) * 3)
    return Ds, T, Fs


# (S, F, tracks per bucket, lengths, cap, posteriors)
BIG_CASES = [
    (2, 4, (300, 260, 410), (5, 9, 13), 4, False),
    (3, 3, (200, 350, 280, 420), (4, 7, 10, 12), 5, False),
    (3, 5, (150, 300, 260, 330, 210), (6, 7, 9, 11, 15), 6, False),
    (2, 6, (260, 300, 200), (8, 11, 16), 4, True),
]


@pytest.mark.parametrize("S,F,Ns,Ls,cap,preds", BIG_CASES)
def test_emulated_big_multi_bucket_stays_in_its_scratch(S, F, Ns, Ls, cap, preds):
    """One emulated global-state launch over several buckets, grid from xt_split_blocks(cap, cap), scratch of exactly cap blocks and a
    sentinel tail: the tail is intact, the grid within the bound, per-track LL 1e-10 of the oracle (posteriors 1e-9) for every bucket."""
    from extrack_amd import synth
    from oracle import oracle_np as O
    E = _E()
    Ds, T, Fs = _model(S, S * 10 + F)
    buckets = [synth.brownian_tracks(n, L, Ds, T, Fs, seed=100 * F + L, dims=2) for n, L in zip(Ns, Ls)]
    ds, cell, pBL, min_len, max_len = np.sqrt(2 * Ds * 0.02), [1.0], 0.1, 3, max(Ls)
    le = np.array([[[0.02]]])
    ps = O.p_stay_table(ds, S, 1, cell)
    E.lib()
    tpb = 128  # tests/emul: 2 wavefronts per block
    old, _ = old_split(float(cap), Ns, Ls, tpb)
    assert old.sum() > cap  # the proportional split overshoots the scratch
    outs, prs, tot, info = E.run_big_multi(buckets, 0.02, ds, Fs, T, pBL, ps, 1, F, min_len, max_len, float(cap), cap, preds=preds)
    assert info["tracks_per_block"] == tpb
    assert info["guard_intact"] == 1 and info["grid"] <= cap, info
    total = 0.0
    for b, ll, pr in zip(buckets, outs, prs or [None] * len(buckets)):
        isBL = int(b.shape[1] != max_len)
        ref = O.proba_cs(b, le, ds, Fs, T, pBL, isBL, cell, 1, F, min_len)
        assert np.abs(ll - ref).max() < 1e-10, (b.shape, np.abs(ll - ref).max())
        total += ref.sum()
        if preds:
            refp = O.p_cs_inter_bound_stats(b, le, ds, Fs, T, pBL, isBL, cell, 1, F, 1, min_len)[1]
            assert np.abs(pr - refp).max() < 1e-9
    assert abs(tot - total) < 1e-12 * abs(total)


def test_emulated_guard_detects_a_grid_over_the_bound():
    """The detector itself: explicit block counts that sum to cap + 1 (what the uncapped split launched) break the guard.  The emulated
    scratch is allocated for the larger grid, so the overrun lands in memory the test owns."""
    from extrack_amd import synth
    from oracle import oracle_np as O
    E = _E()
    S, F, Ns, Ls, cap = 2, 4, (300, 260, 410), (5, 9, 13), 4
    Ds, T, Fs = _model(S, S * 10 + F)
    buckets = [synth.brownian_tracks(n, L, Ds, T, Fs, seed=100 * F + L, dims=2) for n, L in zip(Ns, Ls)]
    ds = np.sqrt(2 * Ds * 0.02)
    ps = O.p_stay_table(ds, S, 1, [1.0])
    blocks = [1, 2, 2]  # every wavefront of the last block has a batch of tracks
    assert sum(blocks) == cap + 1
    outs, _, _, info = E.run_big_multi(buckets, 0.02, ds, Fs, T, 0.1, ps, 1, F, 3, max(Ls), float(cap), cap, blocks_per_bucket=blocks)
    assert info["grid"] == cap + 1 and info["guard_intact"] == 0, info
    ok, _, _, info = E.run_big_multi(buckets, 0.02, ds, Fs, T, 0.1, ps, 1, F, 3, max(Ls), float(cap), cap, blocks_per_bucket=[1, 1, 2])
    assert info["grid"] == cap and info["guard_intact"] == 1, info
    for a, b in zip(outs, ok):
        assert np.abs(a - b).max() < 1e-12
