"""The path choice and launch geometry of the fixed-window likelihood path (csrc/xt_ll_geom.h: xt_ll_pick), compiled for the host through
tests/emul: which kernel family serves a launch group of extrack_loglik* / extrack_predict* / extrack_sequence_matrix - register-resident
2-state, LDS-resident 2-state, entry-parallel, general, gap-aware general, global-state - or which refusal, and the geometry the launcher
(csrc/extrack_ll.hip) forwards to the kernels.  Pure integer arithmetic.

tests/golden/ll_geom_parent.json holds, for a grid of inputs, every output field of the same decision as the launcher carried it inline
before it became a function (recorded by a stand-alone program around those lines, unchanged, with the domains of the kernel-address
lookups in place of the lookups, n_cu = 256), and beside every gapped row what the separate arithmetic of the former xt_gaps_check said
(0 passes, 1 nb_substeps, 2 states, 3 xt_build_config, 6 does not fit a workgroup, 7 variant not built).  The grid (S 2-6, nb_substeps 1-3,
every frame_len xt_build_config accepts and 16 for two states, the five (D, K) pairs, KS 0 / 1 / D, likelihood / posteriors / sequence matrix
/ likelihood and posteriors with gaps, both EXTRACK_LL_PATH values, EXTRACK_FORCE_BIG 0 / 1, budgets of 16 and 32768 MiB, 1 / 3 / 64 buckets)
is thinned to one row per branch signature; the counts below are recomputed from the file and none may be zero.  The invariants are
independent of the recording: they are checked on a seeded sample of 20 000 points over the same axes."""
import json
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emul"))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "ll_geom_parent.json")
KIB = 1024
NONE, REG2, FAST2, ENTRY, GENERAL, GAPS, BIG = range(7)
PATHS = ("none", "reg2", "fast2", "entry", "general", "gaps", "big")
# Every refusal of the function is reached on the grid.  Two of them never leave the library: "posteriors: frame_len > 15" needs frame_len 16,
# which xt_build_config refuses first, and "posteriors are built for n_states <= 6" is reached by posteriors with gaps at 5 and 6 states (or
# nb_substeps > 1) only, which xt_gaps_check / extrack_predict refuse with their own messages first - without gaps, posteriors with more
# than 6 members per group go to the global-state kernel and every legal (D, K) is built.  Both guards are kept, as the launcher had them.
REFUSALS = {1: "gaps with big", 2: "sequence matrix with big", 3: "posteriors, frame_len > 15", 4: "scratch budget", 5: "posteriors not built",
            6: "variant not built"}
_cache = {}


def _cases():
    """(recording, [(inputs, recorded outputs, recorded asides, outputs of xt_ll_pick)]): computed once, shared by the tests."""
    if not _cache:
        import run_emul as E
        d = json.load(open(GOLDEN))
        n_in, n_out = len(d["in"]), len(d["out"])
        rows = []
        for r in sorted(d["rows"]):  # by model: the emulator keeps the digit tables of the last one
            inp, want = dict(zip(d["in"], r[:n_in])), dict(zip(d["out"], r[n_in:n_in + n_out]))
            rows.append((inp, want, dict(zip(d["aside"], r[n_in + n_out:])), dict(zip(d["out"], E.ll_pick(r[:n_in], d["n_cu"])))))
        _cache["d"], _cache["rows"] = d, rows
    return _cache["d"], _cache["rows"]


def _point(d, **kw):
    """xt_ll_pick at one point (defaults: nb_substeps 1, D 2, K 1, one global error, likelihood, default context, one bucket)."""
    import run_emul as E
    v = dict(NS=1, D=2, K=1, KS=0, preds=0, seq=0, gaps=0, ll_reg2=1, force_big=0, budget_mb=32768, nbuckets=1)
    v.update(kw)
    return dict(zip(d["out"], E.ll_pick([v[k] for k in d["in"]], d["n_cu"])))


def test_pick_equals_the_recorded_inline_decision():
    """Every output field of every recorded case, and the refusal messages character for character."""
    import run_emul as E
    d, rows = _cases()
    assert len(rows) >= 300
    for inp, want, _, got in rows:
        assert got == want, (inp, want, got)
    assert [E.ll_refusal_text(r) for r in range(1, len(d["refusal_text"]))] == d["refusal_text"][1:]


def test_recorded_grid_covers_every_branch():
    d, rows = _cases()
    n = {}

    def count(key, cond):
        n[key] = n.get(key, 0) + (1 if cond else 0)

    for inp, out, aside, _ in rows:
        for path in range(1, 7):
            count("path " + PATHS[path], out["path"] == path)
        for r, name in REFUSALS.items():
            count("refusal: " + name, out["path"] == NONE and out["refusal"] == r)
        count("wide", out["wide"] == 1 and out["path"] in (GENERAL, GAPS))
        count("not wide", out["wide"] == 0 and out["path"] in (GENERAL, GAPS))
        count("big for threads", aside["why_big"] in range(1, 8) and aside["why_big"] & 1)
        count("big for LDS", aside["why_big"] in range(1, 8) and aside["why_big"] & 2)
        count("big for LDS alone", aside["why_big"] == 2)
        count("big for posteriors with more than 6 members per group", aside["why_big"] in range(1, 8) and aside["why_big"] & 4)
        count("big for those posteriors alone", aside["why_big"] == 4)
        count("big because forced", aside["why_big"] == 8 and out["path"] == BIG)
        count("budget binds against n_cu * 8", out["path"] == BIG and aside["budget_binds"] == 1 and out["max_blocks"] < d["n_cu"] * 8)
        count("n_cu * 8 binds", out["path"] == BIG and aside["budget_binds"] == 0 and out["max_blocks"] == d["n_cu"] * 8)
        count("ll_reg2 1", out["path"] == REG2 and inp["ll_reg2"] == 1)
        count("ll_reg2 0", out["path"] == FAST2 and inp["ll_reg2"] == 0)
    print(n)
    assert all(v > 0 for v in n.values()), {k: v for k, v in n.items() if v == 0}


def test_named_points_of_the_design_document():
    """DESIGN section 23."""
    d, _ = _cases()
    assert _point(d, S=2, F=6)["path"] == REG2
    assert _point(d, S=2, F=6, ll_reg2=0)["path"] == FAST2
    assert _point(d, S=2, F=12)["path"] == BIG
    assert _point(d, S=2, NS=2, F=4)["path"] == ENTRY
    # 4 states at frame_len 6 with gaps: 1024 groups per track, 4096 sequences x (1 + D + K) doubles fit the LDS of a CU - served, one track per
    # 1024-thread workgroup (the gap-aware GRADIENT refuses this model: tests/test_grad_geom_cpu.py)
    g = _point(d, S=4, F=6, gaps=1)
    assert (g["path"], g["tpb"], g["threads"], g["wide"], g["sel"]) == (GAPS, 1, 1024, 1, 4), g
    assert 128 * KIB < g["lds"] <= 160 * KIB, g


def test_pick_invariants():
    import run_emul as E
    d, _ = _cases()
    rng = np.random.default_rng(20261019)
    pick = lambda *v: int(v[rng.integers(len(v))])
    n_path = [0] * 7
    points = []
    for _ in range(20000):
        S, NS = pick(2, 3, 4, 5, 6), pick(1, 2, 3)
        F = NS + 1 + pick(*range(14))
        while S ** F > 1 << 20 or F > 15:
            F -= 1
        if F <= NS:
            continue
        D, K = ((1, 1), (2, 1), (2, 2), (3, 1), (3, 3))[rng.integers(5)]
        preds, seq, gaps = ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1))[rng.integers(5)]
        points.append([S, NS, F, D, K, pick(0, 1, D), preds, seq, gaps, pick(0, 1), pick(0, 1), pick(16, 32768), pick(1, 3, 64)])
    for inp in sorted(points):  # by model: the emulator keeps the digit tables of the last one
        g = dict(zip(d["out"], E.ll_pick(inp, 256)))
        v = dict(zip(d["in"], inp))
        ctx = (v, g)
        n_path[g["path"]] += 1
        assert (g["path"] == NONE) == (g["refusal"] != 0), ctx
        if g["path"] == NONE:
            continue
        assert g["threads"] % 64 == 0 and g["threads"] > 0 and g["tpb"] >= 1 and g["wide"] == (g["threads"] > 256), ctx
        if g["path"] != BIG:
            assert g["threads"] <= 1024 and 0 < g["lds"] <= 160 * KIB, ctx
        if v["gaps"]:
            assert g["path"] == GAPS, ctx
        if v["seq"]:
            assert g["path"] == GENERAL, ctx
        if v["preds"]:
            assert g["path"] in (GENERAL, GAPS, BIG), ctx
        if g["path"] == BIG:
            assert g["threads"] == 256 and g["tpb"] == 256 and 1 <= g["max_blocks"] <= 256 * 8 and g["max_blocks"] >= v["nbuckets"] and g["ws_stride"] > 0, ctx
    assert all(c >= 10 for c in n_path), n_path  # the sample reaches every outcome (the 2-state fast paths are 1 point in 1000 of these axes)


def test_pick_with_gaps_refuses_exactly_where_the_former_check_did():
    """The one place the duplicate of the selection rules is kept: the former xt_gaps_check (its host-decided refusals and its own geometry
    and lookup), recorded beside every gapped row of the golden file.  The launcher asked the gap lookup for the runtime-G entry at nb_substeps
    > 1 where the check asked for G = n_states^nb_substeps; they agreed because the check had refused nb_substeps != 1 before: so they do here."""
    _, rows = _cases()
    n = {}
    for inp, _, aside, got in rows:
        check = aside["gaps_check"]
        if inp["gaps"]:
            assert (got["path"] == NONE) == (check != 0), (inp, got, check)
            n[check] = n.get(check, 0) + 1
        else:
            assert check == -1
    print(n)
    assert n[0] > 20 and n[1] > 20 and n[2] > 20 and n[6] > 20, n
