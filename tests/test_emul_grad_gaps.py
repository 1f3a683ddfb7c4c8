"""CPU checks of the gap-aware gradient: the two forward-mode bodies (xt_gradr.h, xt_grad.h) with their GAPS flag on CPU
threads (tests/emul/emul_grad_gap.cpp), all buckets of ``gap_reference.make_case`` in one emulated launch with per-track scores, against
Richardson differences of the reference built from the unchanged oracle (tests/grad_gap_reference.py); the flag on gap-free data; the poison
rules; the per-peak error of a gap row; and the host-side refusals of the Python layer.
Tolerances: LL as tests/test_hip_gaps.py (per track rtol 1e-13 / atol 1e-10, total 1e-12 relative); gradient and scores by
``test_grad_edges_cpu.check_gradient`` with the reference's own condition asserted first."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "emul"))

import gap_reference as R
import grad_gap_reference as GR
from oracle import oracle_np as O
from test_grad_edges_cpu import check_gradient

# directions per pass of xt_gradr.h for the cases of grad_gap_reference.CASES (both bodies run in every case)
CASES = [c + (npc,) for c, npc in zip(GR.CASES, (4, 3, 4, 3, 4))]

def emulate(case, body, dirs, gaps=True, buckets=None, sig=None):
    """(LL [sum N], sum LL, gradient, scores [sum N, n_dir]) in upload order (short -> long); launched longest first."""
    import run_emul_grad_gap as E
    Ds, Tm, Fs = R.MODELS[case["S"]]
    ds = np.sqrt(2 * Ds * R.DT)
    bk = case["buckets"] if buckets is None else buckets
    sg = case["sig"] if sig is None else sig
    order = list(range(len(bk)))[::-1]
    ll, tot, g, sc = E.run_grad_gap(body, [bk[i] for i in order], case["le"] if case["le"] is not None else [0.0], ds, Fs, Tm, R.PBL,
                                    O.p_stay_table(ds, case["S"], 1, R.CELL), case["F"], R.MIN_LEN, max(b.shape[1] for b in bk), [d[1] for d in dirs],
                                    sigmas=None if sg is None else [sg[i] for i in order], slope_offset=case["slope_offset"], gaps=gaps)
    r0 = np.concatenate([[0], np.cumsum([len(bk[i]) for i in order])])
    lls, scs = [None] * len(bk), [None] * len(bk)
    for j, i in enumerate(order):
        lls[i], scs[i] = ll[j], sc[r0[j]:r0[j + 1]]
    return np.concatenate(lls), tot, g, np.concatenate(scs)


def check_against_reference(tag, case, ref, ll, tot, g, sc):
    """LL, sum-gradient and per-track scores of one evaluation against the reference (scores: where ``grad_gap_reference.score_mask`` keeps them)."""
    dirs = ref["dirs"]
    assert np.all(np.isfinite(ref["ll"]))
    np.testing.assert_allclose(ll, ref["ll"], rtol=1e-13, atol=1e-10, err_msg=tag + " LL")
    assert abs(tot - ref["ll"].sum()) <= 1e-12 * abs(ref["ll"].sum()), (tag, tot, ref["ll"].sum())
    GR.assert_condition(tag + " sum", ref["gfd"], ref["gest"])
    check_gradient(tag + " sum", dirs, g, ref["gfd"], ref["gest"])
    keep = GR.score_mask(tag, case, ref)
    names = [("%s track %d" % (d[0], n),) for n in range(len(keep)) for d in dirs]
    k = keep.ravel()
    GR.assert_condition(tag + " scores", ref["fd"].ravel()[k], ref["est"].ravel()[k])
    check_gradient(tag + " scores", [n for n, kk in zip(names, k) if kk], sc.ravel()[k], ref["fd"].ravel()[k], ref["est"].ravel()[k])


def assert_bodies_agree(a, b):
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        assert np.all(np.abs(x - y) <= 1e-9 * np.abs(y) + 1e-12), float(np.abs(x - y).max())


@pytest.mark.parametrize("S,D,layout,F,npc", CASES)
def test_emulated_gap_gradient_bodies(S, D, layout, F, npc):
    case = R.make_case(S, D, layout, F)
    assert any(m.any() for m in case["masks"])
    ref = GR.reference(case, (S, D, layout, F))
    GR.assert_golden_is_current(case, (S, D, layout, F), ref)  # what the GPU test reads
    res = {}
    for body in (npc, 0):
        res[body] = emulate(case, body, ref["dirs"])
        check_against_reference("body %d" % body, case, ref, *res[body])
    assert_bodies_agree(res[npc], res[0])


@pytest.mark.parametrize("body", [4, 0])
def test_flag_on_gap_free_data_is_the_plain_body(body):
    """Gap-free data: the flag changes nothing - value, gradient and scores bit for bit (the same operations in the same order)."""
    from extrack_amd import synth
    case = R.make_case(3, 2, "global1", 3)
    Ds, Tm, Fs = R.MODELS[3]
    full = [synth.brownian_tracks(len(b), b.shape[1], list(Ds), Tm.tolist(), list(Fs), dt=R.DT, dims=2, seed=3 + i) for i, b in enumerate(case["buckets"])]
    dirs = GR.directions(case)
    a = emulate(case, body, dirs, gaps=True, buckets=full)
    b = emulate(case, body, dirs, gaps=False, buckets=full)
    assert np.all(np.isfinite(a[0])) and np.all(np.isfinite(a[3]))
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


@pytest.mark.parametrize("body", [3, 0])
def test_poison_rules(body):
    """A row with some NaN coordinates, a NaN first row and a NaN last row give their track a NaN LL and NaN scores and leave the other tracks
    alone: bit for bit in xt_gradr.h, to the tolerance of the body comparison in xt_grad.h."""
    case = R.make_case(2, 2, "global1", 3)
    dirs = GR.directions(case)
    clean = emulate(case, body, dirs)
    dirty = [b.copy() for b in case["buckets"]]
    dirty[3][6, 5, 1] = np.nan   # partial row
    dirty[3][9, 0] = np.nan      # first row
    dirty[4][5, -1] = np.nan     # last row
    got = emulate(case, body, dirs, buckets=dirty)
    r0 = np.concatenate([[0], np.cumsum([len(b) for b in dirty])])
    bad = np.zeros(r0[-1], bool)
    bad[[r0[3] + 6, r0[3] + 9, r0[4] + 5]] = True
    assert np.all(np.isfinite(clean[0])) and np.all(np.isfinite(clean[3]))
    assert np.all(np.isnan(got[0][bad])) and np.all(np.isnan(got[3][bad]))
    if body:
        assert np.array_equal(got[0][~bad], clean[0][~bad]) and np.array_equal(got[3][~bad], clean[3][~bad])
    else:
        assert_bodies_agree((got[0][~bad], got[3][~bad]), (clean[0][~bad], clean[3][~bad]))


@pytest.mark.parametrize("body", [4, 0])
def test_error_of_a_gap_row_is_never_read(body):
    """Per-peak errors: NaN or 123.0 at the gap rows give the same bits (the affine layout: slope and offset directions included)."""
    case = R.make_case(2, 2, "affine", 3)
    dirs = GR.directions(case)
    assert [d[0] for d in dirs][-2:] == ["slope", "offset"] and all(np.isnan(s[m]).all() for s, m in zip(case["sig"], case["masks"]))
    a = emulate(case, body, dirs)
    sig = [s.copy() for s in case["sig"]]
    for s, m in zip(sig, case["masks"]):
        s[m] = 123.0
    b = emulate(case, body, dirs, sig=sig)
    assert np.all(np.isfinite(a[0])) and np.all(np.isfinite(a[3]))
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


# ---- host logic (no device)

def _params():
    from extrack_amd.lmfit_compat import Parameters
    p = Parameters()
    for k, v in dict(D0=1e-3, D1=0.25, LocErr=0.02, F0=0.6, p01=0.1, p10=0.1, pBL=0.1).items():
        p.add(k, value=v, min=1e-6, max=1.0)
    p.add("F1", expr="1 - F0")
    return p


def _tracks():
    from extrack_amd import synth
    tr = synth.brownian_tracks(6, 8, [0.001, 0.25], [[0.9, 0.1], [0.1, 0.9]], [0.6, 0.4], seed=1)
    tr[0, 3] = np.nan
    return {"8": tr}


def test_pinned_refusals_still_raise_and_name_the_new_path():
    from extrack_amd import tracking
    with pytest.raises(NotImplementedError, match="forward"):
        tracking.param_fitting(_tracks(), 0.02, params=_params(), nb_states=2, gaps=True, gradient="analytic")
    with pytest.raises(NotImplementedError, match="parameter_uncertainties"):
        tracking.param_fitting(_tracks(), 0.02, params=_params(), nb_states=2, gaps=True, uncertainties=True)


def test_forward_gradient_without_gaps_is_a_value_error():
    from extrack_amd import tracking
    with pytest.raises(ValueError, match="forward"):
        tracking.param_fitting(_tracks(), 0.02, params=_params(), nb_states=2, gradient="forward")


def test_gap_uncertainties_refuse_comm():
    from extrack_amd import uncertainty
    with pytest.raises(NotImplementedError, match="gap"):
        uncertainty.parameter_uncertainties(_tracks(), 0.02, _params(), gaps=True, comm=object())


def test_gap_gradient_refuses_threshold_fusion_and_comm():
    from extrack_amd import gradient

    class TS:
        gaps, has_dt, has_sigma, n_tracks = True, False, False, 1
    for kw in (dict(threshold_fusion=(0.2, 120, 2000)), dict(comm=object())):
        with pytest.raises(NotImplementedError, match="gap"):
            gradient.objective_and_gradient(_params(), TS(), 0.02, [1], 2, 1, 6, **kw)
