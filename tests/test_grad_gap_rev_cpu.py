"""The third decision of a gapped gradient launch group (csrc/xt_grad_geom.h: xt_grad_gap_rev), compiled for the host through
tests/emul/emul_rev_gap.cpp and applied, as in the launcher, to the result of xt_grad_gap_reg2: gapped data go where their gap-free twin would go.
Upgraded to the gap-aware reverse-mode kernels (path 6, "gaps_rev") exactly when gaps is set, the call is not a scores evaluation, the pick so far is
gradr or lds (or gaps_reg2 under grad_rev == 2), and xt_grad_pick of the same group with gaps = scores = false returns reverse mode; the upgraded
pick has that twin's geometry.  Everything else comes back unchanged.  No GPU."""
import itertools
import os
import shutil
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul"))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

# models named for the GPU test (tests/test_hip_rev_gaps.py): one exchange buffer / two exchange buffers per track, found with the pure function
NBUF1_MODEL = dict(S=4, F=4, D=2, K=1)  # gap_reference.make_case(4, 2, "global1", 4)
NBUF2_MODEL = dict(S=3, F=5, D=2, K=1)  # gap_reference.make_case(3, 2, "global1", 5)


def decide(**kw):
    import run_emul_rev_gap as E
    r = E.decide(**kw)
    assert r is not None, kw
    return r


def upgraded(r):
    """The rule's outcome, with its consistency: an upgraded pick is the twin's geometry under the new path, anything else the pick before it."""
    import run_emul_rev_gap as E
    p0, p1, p2, tw = r
    if p2["path"] == "gaps_rev":
        assert tw["path"] == "rev" and p2["refusal"] == 0 and all(p2[k] == tw[k] for k in E.GEOMETRY), r
        return True
    assert p2 == p1, r
    return False


def test_upgrade_rule_over_the_grid():
    """S x frame_len x (D, K) x locerr_mode x n_dir x gaps x scores x grad_reg2 x grad_rev: upgraded exactly under the rule as the issue states it,
    restated here from the picks around it."""
    import run_emul_rev_gap as E
    n_up = n_keep = 0
    for S, F, (D, K), mode, n_dir, gaps, scores, reg2, rev in itertools.product(
            (2, 3, 4), (3, 4, 5, 6, 7), ((1, 1), (2, 1), (2, 2), (3, 3)), (0, 1, 2), (0, 5), (0, 1), (0, 1), (0, 1, 2), (0, 1, 2)):
        if mode and K != 1 and K != D:
            continue
        r = E.decide(S=S, F=F, D=D, K=K, locerr_mode=mode, n_dir=n_dir, gaps=gaps, scores=scores, grad_reg2=reg2, grad_rev=rev)
        if r is None:
            continue
        p0, p1, p2, tw = r
        rule = bool(gaps and not scores and (p1["path"] in ("gradr", "lds") or (p1["path"] == "gaps_reg2" and rev == 2)) and tw["path"] == "rev")
        assert upgraded(r) == rule, (S, F, D, K, mode, n_dir, gaps, scores, reg2, rev, r)
        if p1["path"] == "none":
            assert p2["path"] == "none"
        n_up += rule
        n_keep += not rule
    assert n_up > 100 and n_keep > 1000, (n_up, n_keep)


@pytest.mark.parametrize("S,F", [(3, 3), (3, 4), (3, 5), (3, 6), (4, 3), (4, 4), (4, 5)])
def test_three_and_four_states_are_upgraded(S, F):
    for (D, K), mode in itertools.product(((1, 1), (2, 1), (2, 2), (3, 1), (3, 3)), (0, 1, 2)):
        if mode == 2 and K != 1:
            continue
        r = decide(S=S, F=F, D=D, K=K, locerr_mode=mode, n_dir=13)
        assert r[0]["path"] == "gradr" and r[1] == r[0] and upgraded(r), (S, F, D, K, mode, r)
        assert r[2]["threads"] <= 256 and r[2]["lds"] <= 160 * 1024 and r[2]["nbuf"] in (1, 2)


def test_scores_calls_are_never_upgraded():
    for kw in (dict(S=3, F=5), dict(S=4, F=4), dict(S=2, F=3), dict(S=2, F=6, locerr_mode=1), dict(S=3, F=5, grad_rev=2)):
        r = decide(scores=1, **kw)
        assert not upgraded(r) and r[2]["path"] in ("gradr", "lds"), (kw, r)
        assert upgraded(decide(scores=0, **kw)), kw


def test_forward_mode_requests_keep_their_kernels():
    """grad_reg2 = 0 (EXTRACK_GRAD_PATH=lds) and 2 (=gradr) with the grad_rev = 0 those settings come with, and with the default grad_rev;
    grad_rev = 0 alone (EXTRACK_GRAD_PATH=reg2)."""
    for S, F in ((3, 5), (4, 4), (2, 3)):
        for reg2, rev in ((0, 0), (2, 0), (0, 1), (2, 1), (1, 0)):
            r = decide(S=S, F=F, grad_reg2=reg2, grad_rev=rev)
            assert not upgraded(r), (S, F, reg2, rev, r)
            assert r[2]["path"] == ("lds" if reg2 == 0 else "gradr")


@pytest.mark.parametrize("F", [4, 5, 6, 7])
def test_two_states_with_one_scalar_error_need_grad_rev_2(F):
    import run_emul_rev_gap as E
    for D in (1, 2, 3):
        for fmask in (0xe0, 0xf0):
            r = decide(S=2, F=F, D=D, K=1, n_dir=7, fmask=fmask)
            assert r[3]["path"] == "reg2" and not upgraded(r), (F, D, r)
            assert r[2]["path"] == ("gaps_reg2" if (fmask >> F) & 1 else "gradr")
            r = decide(S=2, F=F, D=D, K=1, n_dir=7, fmask=fmask, grad_rev=2)
            assert r[3]["path"] == "rev" and upgraded(r), (F, D, r)
    # per-peak errors (with or without the affine map) and frame_len 3 go to reverse mode as they do gap-free
    for kw in (dict(F=F, locerr_mode=1), dict(F=F, locerr_mode=2), dict(F=F, D=3, K=3, locerr_mode=1), dict(F=3)):
        r = decide(S=2, n_dir=7, **kw)
        assert r[3]["path"] == "rev" and upgraded(r), (kw, r)
    assert E.PATHS.index("gaps_rev") == 6 and E.PATHS[:6] == ("none", "rev", "reg2", "gradr", "lds", "gaps_reg2")


def test_log_budget():
    """Fewer log regions than max(n_cu / 2, nbuckets) blocks: the forward-mode kernels, from both sides of either bound."""
    g = decide(S=3, F=5, Lmax=40)[2]  # a budget of mb MiB pays for (mb << 20) / (tpb * log_stride * 8) log regions
    assert g["path"] == "gaps_rev" and g["log_stride"] == 38 * ((1 + 2 + 1) * 81 + 41)
    for mb, n_cu, nbk in ((16384, 256, 1), (64, 256, 1), (4, 256, 1), (1, 256, 1), (1, 8, 1), (1, 8, 3), (1, 8, 64), (2, 8, 64), (16384, 256, 64)):
        r = decide(S=3, F=5, Lmax=40, rev_log_mb=mb, n_cu=n_cu, nbuckets=nbk)
        mbk = (mb << 20) // (g["tpb"] * g["log_stride"] * 8)
        enough = mbk >= max(n_cu // 2, nbk)
        assert upgraded(r) == enough, (mb, n_cu, nbk, mbk, r)
        if enough:
            assert r[2]["max_blocks"] == mbk
        else:
            assert r[2]["path"] == "gradr"
    # exactly at the bound
    mbk1 = (1 << 20) // (g["tpb"] * g["log_stride"] * 8)
    assert mbk1 >= 2
    assert upgraded(decide(S=3, F=5, Lmax=40, rev_log_mb=1, n_cu=2 * mbk1, nbuckets=mbk1))
    assert not upgraded(decide(S=3, F=5, Lmax=40, rev_log_mb=1, n_cu=2 * mbk1 + 2, nbuckets=1))
    assert not upgraded(decide(S=3, F=5, Lmax=40, rev_log_mb=1, n_cu=2, nbuckets=mbk1 + 1))


def test_a_refused_group_stays_refused():
    """4 states at frame_len 6 fit no gap-aware forward-mode kernel (tests/test_hip_grad_gaps.py: test_host_decided_refusals); whatever the knobs."""
    for rev, reg2 in itertools.product((0, 1, 2), (0, 1, 2)):
        r = decide(S=4, F=6, grad_rev=rev, grad_reg2=reg2)
        assert r[0]["path"] == "none" and r[0]["refusal"] != 0 and r[2] == r[0], (rev, reg2, r)


def test_gap_free_picks_pass_through():
    for kw in (dict(S=3, F=5), dict(S=2, F=6), dict(S=2, F=3), dict(S=4, F=4, grad_rev=2)):
        r = decide(gaps=0, **kw)
        assert r[2] == r[0] and r[2]["path"] != "gaps_rev", (kw, r)


def test_geometry_is_the_plain_twins_and_both_buffer_counts_occur():
    r1, r2 = decide(n_dir=9, **NBUF1_MODEL), decide(n_dir=13, **NBUF2_MODEL)
    assert upgraded(r1) and upgraded(r2)
    assert r1[2]["nbuf"] == 1 and r1[3]["nbuf"] == 1, r1
    assert r2[2]["nbuf"] == 2 and r2[3]["nbuf"] == 2, r2
    # what the launcher sizes the log regions by
    assert r1[2]["tpb"] == 4 and r1[2]["threads"] == 256 and r2[2]["tpb"] == 3 and r2[2]["threads"] == 256
    assert r1[2]["log_stride"] == 28 * ((1 + 2 + 1) * 64 + 32) and r2[2]["log_stride"] == 28 * ((1 + 2 + 1) * 81 + 41)
