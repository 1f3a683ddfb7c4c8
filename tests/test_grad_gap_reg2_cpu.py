"""The second decision of a gapped gradient / scores launch group (csrc/xt_grad_geom.h: xt_grad_gap_reg2), compiled for the host
through tests/emul/emul_r2_grad_gap.cpp: after xt_grad_pick said "registers + LDS exchange" (path 3, xt_gradr.h), a two-state launch is upgraded to the
gap-aware register-resident kernels (path 5) exactly when gaps is set, S = 2, nb_substeps = 1, frame_len is in the context's set (default 5, 6, 7;
frame_len 4 on request), grad_reg2 == 1, one global scalar error (locerr_mode 0, K == 1), n_dir > 0 and the kernel is built.  Everything else comes
back as the unchanged pick.  The range of the model never refuses the upgrade: it only picks the variant (xt_grad_gap_reg2_lazy).  No GPU."""
import ctypes as C
import itertools
import shutil

import pytest

import r2_grad_gap_cases as RC

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

FIELDS = ("path", "refusal", "tpb", "threads", "lds", "tpw", "maxnp")


def decide(S=2, NS=1, F=6, D=2, K=1, locerr_mode=0, n_dir=7, Lmax=30, gaps=1, grad_reg2=1, maxnp=8, fmask=RC.F_DEFAULT):
    """(pick of xt_grad_pick, pick after xt_grad_gap_reg2) as dicts, or None where xt_build_config refuses the model."""
    out = (C.c_longlong * 14)()
    inp = (C.c_longlong * 12)(S, NS, F, D, K, locerr_mode, n_dir, Lmax, gaps, grad_reg2, maxnp, fmask)
    if RC.lib(6).xt_emul_grad_gap_reg2(inp, out) != 0:
        return None
    o = list(out)
    return dict(zip(FIELDS, o[:7])), dict(zip(FIELDS, o[7:]))


def test_upgrade_rule_over_the_grid():
    """S x nb_substeps x frame_len x D x K x locerr_mode x n_dir x gaps x grad_reg2 x frame-length set: upgraded exactly under the rule, with the
    register-resident geometry (4 waves x 64 >> (F - 1) tracks, 256 threads, maxnp); anything else is the pick of xt_grad_pick, field by field."""
    n_up = n_keep = 0
    for S, NS, F, D, K1, mode, n_dir, gaps, reg2, fmask in itertools.product(
            (2, 3), (1, 2), (3, 4, 5, 6, 7, 8), (1, 2, 3), (1, 0), (0, 1), (0, 1, 7, 10), (0, 1), (0, 1, 2), (RC.F_DEFAULT, RC.F_ALL, 0xffff, 0)):
        K = 1 if K1 else D  # D = 1: "one error per dimension" is the scalar error (counted twice below)
        r = decide(S=S, NS=NS, F=F, D=D, K=K, locerr_mode=mode, n_dir=n_dir, gaps=gaps, grad_reg2=reg2, maxnp=5, fmask=fmask)
        if r is None:
            continue
        p0, p1 = r
        rule = (gaps and p0["path"] == RC.GRADR and S == 2 and NS == 1 and 4 <= F <= 7 and (fmask >> F) & 1 and reg2 == 1 and mode == 0 and K == 1 and n_dir > 0)
        if rule:
            n_up += 1
            tpw = 64 >> (F - 1)
            assert p1 == dict(path=RC.GAPS_REG2, refusal=0, tpb=4 * tpw, threads=256, lds=0, tpw=tpw, maxnp=5), (S, NS, F, D, K, p1)
        else:
            n_keep += 1
            assert p1 == p0, (S, NS, F, D, K, mode, n_dir, gaps, reg2, fmask, p0, p1)
        if not gaps:
            assert p1["path"] != RC.GAPS_REG2
    # frame lengths in the three non-empty sets (3 + 4 + 4) x (D, K) with K = 1 (3 + the second D = 1) x positive n_dir (3)
    assert n_up == (3 + 4 + 4) * (3 + 1) * 3 and n_keep > 1000, (n_up, n_keep)


def test_every_condition_from_both_sides():
    base = decide()
    assert base[0]["path"] == RC.GRADR and base[1]["path"] == RC.GAPS_REG2
    for kw in (dict(gaps=0), dict(S=3), dict(NS=2, F=6), dict(F=8), dict(F=3), dict(grad_reg2=0), dict(grad_reg2=2), dict(locerr_mode=1), dict(locerr_mode=2),
               dict(K=2), dict(D=3, K=3), dict(n_dir=0), dict(fmask=0), dict(fmask=1 << 5)):
        r = decide(**kw)
        assert r is not None and r[1] == r[0] and r[1]["path"] != RC.GAPS_REG2, (kw, r)
    for kw in (dict(D=1), dict(D=3), dict(F=5), dict(F=7), dict(n_dir=1), dict(n_dir=20), dict(maxnp=3), dict(Lmax=2), dict(Lmax=100000), dict(fmask=1 << 6)):
        assert decide(**kw)[1]["path"] == RC.GAPS_REG2, kw
    assert decide(maxnp=3)[1]["maxnp"] == 3


def test_frame_len_4_needs_the_full_mask():
    """A default context keeps frame_len 4 on xt_gradr.h (the geometry tests/test_hip_grad.py records); EXTRACK_GAP_REG2_F=all upgrades it."""
    p0, p1 = decide(F=4, fmask=RC.F_DEFAULT)
    assert p1 == p0 and p0["path"] == RC.GRADR
    p0, p1 = decide(F=4, fmask=RC.F_ALL)
    assert p0["path"] == RC.GRADR and p1["path"] == RC.GAPS_REG2 and p1["tpb"] == 32 and p1["tpw"] == 8


def test_other_picks_are_returned_untouched():
    """Gap-free picks (register-resident, reverse mode), the LDS-resident pick of a gapped launch (EXTRACK_GRAD_PATH=lds; more than 256 groups) and a
    refusal pass through whatever the other inputs say."""
    for kw, path in ((dict(gaps=0), RC.REG2), (dict(gaps=0, S=3, F=5), 1), (dict(grad_reg2=0), RC.LDS), (dict(F=10), RC.LDS), (dict(S=4, F=6), 0)):
        r = decide(fmask=0xffff, **kw)
        assert r is not None and r[0]["path"] == path and r[1] == r[0], (kw, r)


def test_lazy_variant_bound():
    """(Lmax - 2) d2max <= 1e4 on top of a well-scaled model: pairs just inside and just outside, a NaN d2max, Lmax = 2 (no interior row)."""
    lazy = RC.lib(6).xt_emul_grad_gap_reg2_lazy
    for Lmax, inside, outside in ((102, 100.0, 100.0000001), (1002, 10.0, 10.00000001), (3, 1e4, 1.0000001e4), (12, 1000.0, 1000.000001)):
        assert lazy(1, Lmax, C.c_double(inside)) == 1 and lazy(1, Lmax, C.c_double(outside)) == 0, Lmax
        assert lazy(0, Lmax, C.c_double(inside)) == 0
    assert lazy(1, 2, C.c_double(1e300)) == 1 and lazy(1, 30, C.c_double(float("nan"))) == 0
