"""The launch geometry of the threshold-fusion likelihood path (csrc/xt_th_geom.h), compiled for the host through tests/emul: which apply
variant runs, tile, workgroup, LDS bytes and grid of the plan and the apply launch - pure integer arithmetic the launcher (csrc/extrack_th.hip)
only forwards to the kernels.

tests/golden/th_geom_parent.json holds, for a grid of inputs, every output field of the same two calculations as the launcher carried them
inline before they became functions (recorded by a stand-alone program around those lines, unchanged).  The grid covers every branch; the
counts below are recomputed from the file and none may be zero.  The invariants are independent of the recording: they are checked on a
seeded sample of 20 000 points per function over the same axes."""
import json
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emul"))

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "th_geom_parent.json")
XT_TH_GPW = 4  # csrc/xt_th.h: merge groups per wavefront of the single-buffer apply variants
KIB = 1024
_cache = {}


def _cases():
    """(recording, [(inputs, knobs, recorded outputs, outputs of xt_th_geom.h)] per function): computed once, shared by the tests."""
    if not _cache:
        import run_emul as E
        d = json.load(open(GOLDEN))
        _cache["d"] = d
        for which in ("plan", "apply"):
            n_in = len(d[which + "_in"])
            rows = []
            for r in d[which]:
                inp, want = dict(zip(d[which + "_in"], r[:n_in])), dict(zip(d[which + "_out"], r[n_in:]))
                kn = dict(zip(d["knob_fields"], d["knobs"][inp["knob"]]))
                got = dict(zip(d[which + "_out"], E.th_geom(which, r[:n_in - 1], d["knobs"][inp["knob"]])))
                rows.append((inp, kn, want, got))
            _cache[which] = rows
    return _cache["d"], _cache["plan"], _cache["apply"]


def _sample(which, n=20000):
    """Seeded points of the axes the recording was drawn from -> (inputs, knobs, outputs of xt_th_geom.h)."""
    import run_emul as E
    d, _, _ = _cases()
    rng = np.random.default_rng(20261018)
    pick = lambda *v: int(v[rng.integers(len(v))])
    for _ in range(n):
        S, NS = pick(2, 3, 4), pick(1, 2, 3)
        D, K = ((1, 1), (2, 1), (2, 2), (3, 3), (3, 1))[rng.integers(5)]
        chunk, nchunks, knob = pick(1, 3, 30, 47, 48, 64, 2000), pick(1, 5, 300, 5000), pick(0, *range(len(d["knobs"])))
        if which == "plan":
            capE = pick(128, 1024, 8192, 16384)
            while capE < S ** (NS + 1):
                capE *= 2
            v = [S, S ** NS, capE, D, K, NS + 1 + pick(0, 1, 2, 3, 4), NS, min(chunk, 30), nchunks, 256, pick(0, 8, 40, 83, 3000), pick(0, 8, 40, 83, 3000),
                 pick(0, 0, 0, 1), knob]
        else:
            maxG = pick(1, 2, 7, 12, 16, 64, 65, 128, 700, 4096, 16384)
            v = [S, S ** NS, D, K, pick(0, 1, D), pick(3, 10, 60, 400), chunk, nchunks, pick(1, 1, 3), maxG, max(1, maxG * pick(1, 3, 20) - pick(0, maxG // 3)),
                 pick(0, 0, 0, 0, 0, 1), 256, knob]
        yield (dict(zip(d[which + "_in"], v)), dict(zip(d["knob_fields"], d["knobs"][knob])),
               dict(zip(d[which + "_out"], E.th_geom(which, v[:-1], d["knobs"][knob]))))


def test_geometry_equals_the_recorded_inline_calculation():
    """Every output field of every recorded case, plan and apply."""
    _, plan, apply = _cases()
    assert len(plan) >= 100 and len(apply) >= 100
    for rows in (plan, apply):
        for inp, kn, want, got in rows:
            assert got == want, (inp, kn, want, got)


def test_recorded_grid_covers_every_branch():
    _, plan, apply = _cases()
    n = {}

    def count(key, cond):
        n[key] = n.get(key, 0) + (1 if cond else 0)

    for inp, kn, out, _ in apply:
        for mode in range(5):
            count("apply mode %d" % mode, out["fits"] and out["mode"] == mode)
        count("plan_cap > 0", out["plan_cap"] > 0)
        count("plan_cap == 0", out["plan_cap"] == 0)
        count("plan_cap == -1", out["plan_cap"] == -1)
        count("chunk < 48", inp["chunk"] < 48)
        # the tile only exceeds 160 KiB of LDS before the halving loop when it was forced
        count("TT halved", kn["force_tt"] > 0 and not inp["want_seq"] and out["TT"] < kn["force_tt"])
        for k in ("force_tt", "force_threads", "force_single", "no_gen_single", "no_direct"):
            count("knob " + k, kn[k] != 0)
        count("forced threads taken", kn["force_threads"] > 0 and out["fits"] and out["threads"] == kn["force_threads"])
        count("nbuckets > 1", inp["nbuckets"] > 1)
        count("apply does not fit", not out["fits"])
    for inp, kn, out, _ in plan:
        count("plan lds_mode on", out["ws_lds"] == 1)
        count("plan lds_mode off", out["ws_lds"] == 0)
        count("plan_glb", out["plan_glb"] == 1)
        count("staging in lds mode", out["ws_lds"] == 1 and out["stP"] > 0)
        count("staging in global mode", out["ws_lds"] == 0 and out["stP"] > 0)
        count("force_global", inp["force_global"] != 0)
        count("24 GiB grid cap", not out["ws_lds"] and out["grid"] < min(inp["nchunks"], 2 * inp["n_cu"]))
        count("plan_threads 512", out["plan_threads"] == 512)
        count("plan_threads 1024", out["plan_threads"] == 1024)
        count("plan_threads forced", kn["plan_threads_forced"] != 0)
        count("plan does not fit", not out["fits"])
    print(n)
    assert all(v > 0 for v in n.values()), {k: v for k, v in n.items() if v == 0}


def test_apply_geometry_invariants():
    n_fit = 0
    for inp, kn, g in _sample("apply"):
        n_fit += g["fits"]
        if not g["fits"]:
            assert g["lds"] > 160 * KIB
            continue
        ctx = (inp, kn, g)
        TT, threads = g["TT"], g["threads"]
        assert g["lds"] <= 160 * KIB, ctx
        assert TT >= 1 and TT & (TT - 1) == 0 and 1 << g["logTT"] == TT, ctx
        assert threads % 64 == 0 and TT <= threads <= 1024 and threads % TT == 0, ctx
        assert 1 <= g["bpc"] <= (inp["chunk"] + TT - 1) // TT, ctx
        assert g["grid"] == inp["nchunks"] * g["bpc"], ctx
        assert 1 <= g["blocks_per_cu"] <= 8, ctx
        assert g["mode"] == (4 if inp["want_seq"] else (2 if g["single_buf"] else 1) if TT == 64 else (3 if g["single_buf"] else 0)), ctx
        if g["mode"] == 2:
            assert inp["maxG"] <= (threads // 64) * XT_TH_GPW, ctx
        if g["mode"] == 3:
            assert threads == 1024 and inp["maxG"] <= (1024 // TT) * XT_TH_GPW, ctx
        if g["mode"] == 4:
            assert g["single_buf"] == 0 and TT <= 32, ctx
    assert n_fit > 10000


def test_plan_geometry_invariants():
    n_fit = 0
    for inp, kn, g in _sample("plan"):
        n_fit += g["fits"]
        if not g["fits"]:
            assert g["lds"] > 160 * KIB
            continue
        ctx = (inp, kn, g)
        assert g["lds"] <= 160 * KIB, ctx
        assert 1 <= g["grid"] <= min(inp["nchunks"], 2 * inp["n_cu"]), ctx
        staging = inp["pcap"] * (g["stP"] * inp["D"] + g["stE"] * inp["K"]) * 8
        if g["ws_lds"]:
            assert g["lds"] - staging <= 64 * KIB and g["lds"] <= 80 * KIB, ctx
            assert g["wsP"] % 2 == 1 and g["wsE"] % 2 == 1, ctx
            assert g["ws_bytes"] == 0 and not g["plan_glb"], ctx  # the pilot-track state lives in LDS: no global workspace is sized
        else:
            assert g["ws_bytes"] == g["ws_stride"] * g["grid"] * 8, ctx
            assert g["ws_bytes"] <= 24 << 30 or g["grid"] == 1, ctx
            assert g["wsP"] == g["wsE"] == inp["capE"], ctx
        assert g["plan_threads"] in (kn["plan_threads"], 1024), ctx
    assert n_fit > 10000
