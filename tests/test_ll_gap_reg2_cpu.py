"""The second decision of a gapped likelihood launch group (csrc/xt_ll_geom.h: xt_ll_gap_reg2), compiled for the host
through tests/emul/emul_r2_gap.cpp: after xt_ll_pick said "general gap body" (path 5) and the group's scaling is known, a two-state launch is
upgraded to the gap-aware register-resident kernel (path 7) exactly when it is a likelihood launch (with or without per-track output), S = 2,
nb_substeps = 1, frame_len 4..7 and in the context's set (default 5, 6, 7; frame_len 4 on request), ll_reg2 == 1, one global scalar error
(KS == 0, K == 1) and scaling == 2 with (Lmax - 2) d2max <= 1e4.
Everything else comes back as the unchanged pick.  Pure integer / double arithmetic, no GPU."""
import ctypes as C
import itertools
import shutil

import pytest

from test_emul_r2_gaps import gap_lib

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

GAPS, GAPS_REG2 = 5, 7
FIELDS = ("path", "refusal", "tpb", "threads", "lds", "wide", "sel", "ws_stride", "max_blocks")


F_DEFAULT, F_ALL = 0xe0, 0xf0


def decide(S=2, NS=1, F=6, D=2, K=1, KS=0, preds=0, per_track=0, ll_reg2=1, scaling=2, Lmax=30, gaps=1, d2max=0.01, fmask=-1):
    """(pick of xt_ll_pick, pick after xt_ll_gap_reg2) as dicts, or None where xt_build_config refuses the model."""
    out = (C.c_longlong * 18)()
    inp = (C.c_longlong * 13)(S, NS, F, D, K, KS, preds, per_track, ll_reg2, scaling, Lmax, gaps, fmask)  # fmask < 0: the function's default
    rc = gap_lib().xt_emul_ll_gap_reg2(inp, C.c_double(d2max), out)
    if rc != 0:
        return None
    o = list(out)
    return dict(zip(FIELDS, o[:9])), dict(zip(FIELDS, o[9:]))


def test_upgrade_rule_over_the_grid():
    """S x nb_substeps x frame_len x D x (K, KS) x posteriors x per-track x ll_reg2 x scaling x frame-length set: upgraded exactly under the rule, with the
    register-resident geometry; anything else is the pick of xt_ll_pick, field by field."""
    n_up = n_keep = 0
    for S, NS, F, D, (K, KS), preds, per_track, ll_reg2, scaling, fmask in itertools.product(
            (2, 3), (1, 2), (3, 4, 5, 6, 7, 8), (1, 2, 3), ((1, 0), (0, 0), (1, 1), (0, 1)), (0, 1), (0, 1), (0, 1), (0, 1, 2), (-1, F_ALL, 0xffff)):
        K = K or D  # K = 0 above: one error per dimension
        KS = KS and K  # per-peak errors: sigma dims = K
        r = decide(S=S, NS=NS, F=F, D=D, K=K, KS=KS, preds=preds, per_track=per_track, ll_reg2=ll_reg2, scaling=scaling, fmask=fmask)
        if r is None or r[0]["path"] != GAPS:
            continue  # refused by xt_build_config / xt_ll_pick: nothing to upgrade (checked below: such a pick comes back unchanged too)
        p0, p1 = r
        rule = S == 2 and NS == 1 and (5 if fmask < 0 else 4) <= F <= 7 and not preds and ll_reg2 == 1 and K == 1 and KS == 0 and scaling == 2
        if rule:
            n_up += 1
            tpw = 64 >> (F - 1)
            lds = gap_lib().xt_emul_r2_gap_block_bytes(D, tpw)
            assert p1 == dict(path=GAPS_REG2, refusal=0, tpb=4 * tpw, threads=256, lds=lds, wide=0, sel=F, ws_stride=0, max_blocks=0), (S, NS, F, D, K, KS, p1)
            assert lds == gap_lib().xt_emul_r2_block_bytes(D, tpw) + 512 and lds <= 64 * 1024
        else:
            n_keep += 1
            assert p1 == p0, (S, NS, F, D, K, KS, preds, per_track, ll_reg2, scaling, p0, p1)
    assert n_up == (3 + 4 + 4) * (2 + 1 + 1) * 2 and n_keep > 1000, (n_up, n_keep)  # D = 1: "one error per dimension" is the scalar error


def test_gap_extended_range_bound():
    """(Lmax - 2) d2max <= 1e4: pairs just inside and just outside, at both ends (a long group of small steps, a short group of large ones); a NaN
    d2max (no model tables) and Lmax = 2 (no interior row)."""
    for Lmax, inside, outside in ((102, 100.0, 100.0000001), (1002, 10.0, 10.00000001), (3, 1e4, 1.0000001e4), (12, 1000.0, 1000.000001)):
        assert decide(Lmax=Lmax, d2max=inside)[1]["path"] == GAPS_REG2, (Lmax, inside)
        p0, p1 = decide(Lmax=Lmax, d2max=outside)
        assert p1 == p0 and p0["path"] == GAPS, (Lmax, outside)
    assert decide(Lmax=10002, d2max=1.0)[1]["path"] == GAPS_REG2 and decide(Lmax=10003, d2max=1.0)[1]["path"] == GAPS
    assert decide(Lmax=2, d2max=1e300)[1]["path"] == GAPS_REG2
    assert decide(Lmax=30, d2max=float("nan"))[1]["path"] == GAPS


def test_a_pick_that_is_not_the_general_gap_body_is_left_alone():
    """Gap-free launches (register-resident, LDS-resident, general ...) and refusals pass through whatever the other inputs say."""
    assert decide(F=4)[1]["path"] == GAPS and decide(F=4, fmask=F_DEFAULT)[1]["path"] == GAPS and decide(F=4, fmask=F_ALL)[1]["path"] == GAPS_REG2
    assert decide(F=6, fmask=1 << 4)[1]["path"] == GAPS and decide(F=6, fmask=0)[1]["path"] == GAPS
    for kw in (dict(gaps=0), dict(gaps=0, ll_reg2=0), dict(gaps=0, S=3), dict(gaps=0, preds=1), dict(gaps=1, S=4, F=7), dict(gaps=1, S=2, F=12)):
        r = decide(**kw)
        assert r is not None and r[0] == r[1] and r[1]["path"] != GAPS_REG2, (kw, r)
