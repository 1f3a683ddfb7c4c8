"""The path choice and launch geometry of the gradient path (csrc/xt_grad_geom.h: xt_grad_pick), compiled for the host through tests/emul:
which kernel family serves a launch group - reverse mode, register-resident 2-state, register + LDS exchange, LDS-resident - or which
refusal, and the geometry the launcher (csrc/extrack_grad.hip) forwards to the kernels.  Pure integer arithmetic.

tests/golden/grad_geom_parent.json holds, for a grid of inputs, every output field of the same decision as the launcher carried it inline
before it became a function (recorded by a stand-alone program around those lines, unchanged, with the domains of the kernel-address
tables in place of the lookups, n_cu = 256), and what the separate arithmetic of the former xt_grad_gaps_check said of every gapped point.
The grid (S 2-5, nb_substeps 1-2, every frame_len xt_build_config accepts, the five (D, K) pairs, both error modes, 12 direction counts, 4
lengths, gaps x scores, every EXTRACK_GRAD_PATH / EXTRACK_GRADR_NPC value, two log budgets, plus forced EXTRACK_GRAD_PJ / EXTRACK_R2_MAXNP)
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

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "grad_geom_parent.json")
KIB = 1024
NONE, REV, REG2, GRADR, LDS = range(5)
# The refusals the grid reaches.  The other three messages of the launcher ("> 1024 groups per track", "sequence state does not fit", "more than
# 16 directions per pass") are shadowed on the whole grid, for the inline code as for the function: a model with more than 1024 groups, or whose
# pass exceeds 160 KiB, already fails the one-direction test that precedes them, and the pass size is capped at 16 before it is used.
REFUSALS = {1: "one direction does not fit", 4: "variant not built"}
_cache = {}


def _cases():
    """(recording, [(inputs, knobs, recorded outputs, recorded check, outputs of xt_grad_pick)]): computed once, shared by the tests."""
    if not _cache:
        import run_emul as E
        d = json.load(open(GOLDEN))
        n_in, n_out = len(d["in"]), len(d["out"])
        rows = []
        for r in sorted(d["rows"]):  # by model: the emulator keeps the digit tables of the last one
            inp, want = dict(zip(d["in"], r[:n_in])), dict(zip(d["out"], r[n_in:n_in + n_out]))
            kn = dict(zip(d["knob_fields"], d["knobs"][inp["knob"]]))
            got = dict(zip(d["out"], E.grad_pick(r[:n_in - 1], d["n_cu"], d["knobs"][inp["knob"]])))
            rows.append((inp, kn, want, r[n_in + n_out], got))
        _cache["d"], _cache["rows"] = d, rows
    return _cache["d"], _cache["rows"]


def _point(d, **kw):
    """xt_grad_pick at one point (defaults: D 2, K 1, one global error, 30 positions, one bucket, no knob set)."""
    import run_emul as E
    v = dict(NS=1, D=2, K=1, locerr_mode=0, Lmax=30, nbuckets=1, gaps=0, scores=0)
    v.update(kw)
    return dict(zip(d["out"], E.grad_pick([v[k] for k in d["in"][:-1]], d["n_cu"], [1, 1, 0, 16384, 8, 16, 0, 8])))


def test_pick_equals_the_recorded_inline_decision():
    """Every output field of every recorded case."""
    _, rows = _cases()
    assert len(rows) >= 300
    for inp, kn, want, _, got in rows:
        assert got == want, (inp, kn, want, got)


def test_recorded_grid_covers_every_branch():
    d, rows = _cases()
    n = {}

    def count(key, cond):
        n[key] = n.get(key, 0) + (1 if cond else 0)

    by_input = {tuple(r[:len(d["in"])]): r for r in d["rows"]}
    for inp, kn, out, _, _ in rows:
        for path, name in enumerate(("none", "rev", "reg2", "gradr", "lds")):
            # gapped data never go to rev or reg2, scores never to rev: those outcomes are counted where they can occur
            if not (inp["gaps"] and path in (REV, REG2)):
                count("%s, gaps %d" % (name, inp["gaps"]), out["path"] == path)
            if not (inp["scores"] and path == REV) and not (inp["gaps"] and path == REG2):
                count("%s, scores %d" % (name, inp["scores"]), out["path"] == path)
        for nbuf in (1, 2):
            count("rev, %d exchange buffers" % nbuf, out["path"] == REV and out["nbuf"] == nbuf)
        if kn["rev_log_mb"] == 1 and out["path"] != REV:  # the same point with the full budget is in the file and goes to rev
            twin = by_input.get(tuple([inp[k] for k in d["in"][:-1]] + [inp["knob"] + 1]))
            count("rev dropped for the log budget", twin is not None and d["knobs"][inp["knob"] + 1][3] == 16384 and twin[len(d["in"])] == REV)
        for npc in (3, 4):
            count("gradr, NPC %d" % npc, out["path"] == GRADR and out["NPC"] == npc)
        for t in (0, 1):
            count("lds, tan_lds %d" % t, out["path"] == LDS and out["tan_lds0"] == t)
        for pj in (1, 2, 4, 8):
            count("lds, PJ %d" % pj, out["path"] == LDS and out["PJ0"] == pj)
        count("lds, more than 256 threads", out["path"] == LDS and out["threads0"] > 256)
        count("lds, shorter last pass", out["path"] == LDS and out["rem"] > 0)
        for r, name in REFUSALS.items():
            count("refusal: " + name, out["path"] == NONE and out["refusal"] == r)
        count("knob lds_pj", kn["lds_pj"] != 0)
        count("knob r2_maxnp", out["path"] == REG2 and out["maxnp"] != 8)
    print(n)
    assert all(v > 0 for v in n.values()), {k: v for k, v in n.items() if v == 0}


def test_named_points_of_the_design_document():
    """DESIGN section 21."""
    d, _ = _cases()
    assert _point(d, S=4, F=6, n_dir=3, gaps=1)["path"] == NONE
    g = _point(d, S=2, F=10, n_dir=3, gaps=1)
    assert (g["path"], g["tpb0"], g["threads0"], g["npass_dir"]) == (LDS, 1, 512, 1), g
    assert _point(d, S=2, F=6, n_dir=7)["path"] == REG2
    assert _point(d, S=3, F=6, n_dir=13)["path"] == REV


def test_pick_invariants():
    import run_emul as E
    d, _ = _cases()
    rng = np.random.default_rng(20261018)
    pick = lambda *v: int(v[rng.integers(len(v))])
    n_path = [0] * 5
    points = []
    for _ in range(20000):
        S, NS = pick(2, 3, 4, 5), pick(1, 2)
        F = NS + 1 + pick(*range(14))
        while S ** F > 1 << 20 or F > 15:
            F -= 1
        D, K = ((1, 1), (2, 1), (2, 2), (3, 1), (3, 3))[rng.integers(5)]
        n_dir = pick(1, 2, 3, 4, 5, 7, 8, 9, 13, 16, 17, 32)
        knobs = d["knobs"][rng.integers(len(d["knobs"]))]
        points.append(([S, NS, F, D, K, pick(0, 1), n_dir, pick(3, 30, 400, 20000), pick(1, 2, 64), pick(0, 1), pick(0, 1)], knobs))
    for inp, knobs in sorted(points):  # by model: the emulator keeps the digit tables of the last one
        n_dir = inp[6]
        g = dict(zip(d["out"], E.grad_pick(inp, 256, knobs)))
        ctx = (inp, knobs, g)
        n_path[g["path"]] += 1
        gaps, scores = inp[9], inp[10]
        assert (g["path"] == NONE) == (g["refusal"] != 0), ctx
        assert not (gaps and g["path"] in (REV, REG2)) and not (scores and g["path"] == REV), ctx
        if g["path"] in (REV, GRADR):
            assert 64 <= g["threads"] <= 256 and 0 < g["lds"] <= 160 * KIB and g["tpb"] >= 1, ctx
        if g["path"] == REV:
            assert g["nbuf"] in (1, 2) and g["max_blocks"] >= 128 and g["log_stride"] > 0, ctx
        if g["path"] == REG2:
            assert g["threads"] == 256 and g["tpb"] == 4 * g["tpw"] and 1 <= g["maxnp"] <= 8, ctx  # passes of <= maxnp <= 8 directions cover any n_dir
        if g["path"] == GRADR:
            assert g["NPC"] in (3, 4) and 1 <= g["per"] <= g["NPC"] and -(-n_dir // g["per"]) * g["per"] >= n_dir, ctx
        if g["path"] == LDS:
            npd, rem = g["npass_dir"], g["rem"]
            assert 1 <= npd <= 16 and rem == (n_dir % npd if n_dir > npd else 0), ctx
            for i in range(2 if rem else 1):
                assert g["threads%d" % i] % 64 == 0 and g["threads%d" % i] <= 1024 and 0 < g["lds%d" % i] <= 160 * KIB, ctx
                assert g["PJ%d" % i] in (1, 2, 4, 8) and g["tpb%d" % i] >= 1, ctx
    assert all(v >= 50 for v in n_path), n_path  # the sample reaches every outcome


def test_pick_with_gaps_refuses_exactly_where_the_former_check_did():
    """The one place the duplicate of the selection rules is kept: the arithmetic of the former xt_grad_gaps_check, recorded beside every
    gapped row of the golden file."""
    _, rows = _cases()
    n = [0, 0]
    for inp, kn, want, check, got in rows:
        if inp["gaps"]:
            assert (got["path"] == NONE) == (check == 1), (inp, kn, got, check)
            n[check] += 1
        else:
            assert check == -1
    assert min(n) > 20, n
