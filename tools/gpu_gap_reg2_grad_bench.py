#!/usr/bin/env python3
"""Device time of the two-state likelihood + gradient with missed detections on the register-resident kernels beside the gap
instantiation of xt_gradr.h, same data, same build, same process.  Datasets: 1e6 tracks x 30 at frame_len 6 (the headline shape) and 1e5 x 30 at
frame_len 4, 5 and 7; two dimensions, D = [0, 0.25], LocErr 0.02, p01 = p10 = 0.1; the 7 free parameters of the two-state model as directions.
Contexts are created under EXTRACK_GAP_REG2_F=all (frame_len 4 is upgraded on request only).  Rows per dataset:

    a  plain gradient entry, gap-free data               (xt_grad_r2_kernel)
    b  gap entry, the same gap-free data                 (xt_grad_r2_gap_kernel)
    c  gap entry, 25 % of the interior rows missed
    d  c in a context created under EXTRACK_GRAD_PATH=gradr (xt_gradr.h, GAPS: the path before section 27)

The four contexts live side by side; 25 untimed launches each, then 20 rounds of a, b, c, d in turn, extrack_last_grad_ms of each - median, min, max -
and the family extrack_last_grad_path reports.  `c_faster_than_d` compares the medians against the spread of the two rows (max - min of each, added).
Then the gradient="forward" fit of 3000 x 12 and of 1e5 x 30 (D1 free) on both paths: objective calls and wall time.  One JSON line per dataset / fit.

    python tools/gpu_gap_reg2_grad_bench.py [--scale 1.0] [--out profiles/reg2_grad_gaps_bench.json]
"""
import argparse
import contextlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM, TIMED = 25, 20
DS, TM, FS, LE = [0.0, 0.25], [[0.9, 0.1], [0.1, 0.9]], [0.6, 0.4], 0.02


@contextlib.contextmanager
def grad_path(value):
    """EXTRACK_GRAD_PATH (None: unset) and EXTRACK_GAP_REG2_F=all while a context is created (the knobs bind there)."""
    old = {k: os.environ.get(k) for k in ("EXTRACK_GRAD_PATH", "EXTRACK_GAP_REG2_F")}
    os.environ["EXTRACK_GAP_REG2_F"] = "all"
    if value is None:
        os.environ.pop("EXTRACK_GRAD_PATH", None)
    else:
        os.environ["EXTRACK_GRAD_PATH"] = value
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run(n, L, F):
    from extrack_amd import engine, gradient, synth, tracking as T
    full = synth.brownian_tracks(n, L, DS, TM, FS, LocErr=LE, seed=2)
    gapped = synth.drop_positions(full, 0.25, seed=3)
    p = T.generate_params(nb_states=2, LocErr_type=1, estimated_Ds=[0.001, 0.25], estimated_LocErr=[LE], estimated_Fs=[0.6], estimated_transition_rates=0.1)
    names = gradient.free_names(p)
    res = {"tracks": n, "len": L, "dims": full.shape[2], "frame_len": F, "directions": len(names), "warmup": WARM, "timed": TIMED,
           "missed_fraction": float(np.isnan(gapped[:, :, 0]).mean())}
    sets = {}
    try:
        for name, data, gaps, env in (("a", full, False, None), ("b", full, True, None), ("c", gapped, True, None), ("d", gapped, True, "gradr")):
            with grad_path(env):
                sets[name] = engine.TrackSet([data], None, device=0, gaps=gaps)
        call = {k: (lambda ts=ts: gradient.objective_and_gradient(p, ts, LE, [1], 2, 1, F, names=names)) for k, ts in sets.items()}
        for k in "abcd":
            for _ in range(WARM):
                call[k]()
        ms, val = {k: [] for k in "abcd"}, {}
        for _ in range(TIMED):
            for k in "abcd":
                val[k] = call[k]()
                ms[k].append(sets[k].ctx.last_grad_ms())
        for k in "abcd":
            res[k] = {"median": float(np.median(ms[k])), "min": float(np.min(ms[k])), "max": float(np.max(ms[k])), "path": sets[k].ctx.last_grad_path(),
                      "launch": sets[k].ctx.last_launch_info()}
    finally:
        for ts in sets.values():
            ts.close()
    res["objective"] = {k: float(v[0]) for k, v in val.items()}
    res["c_vs_d_rel_diff"] = {"objective": abs(val["c"][0] - val["d"][0]) / abs(val["d"][0]),
                              "gradient": float(np.max(np.abs(val["c"][1] - val["d"][1]) / np.maximum(np.abs(val["d"][1]), 1e-300)))}
    spread = (res["c"]["max"] - res["c"]["min"]) + (res["d"]["max"] - res["d"]["min"])
    res["d_over_c"] = res["d"]["median"] / res["c"]["median"]
    res["c_faster_than_d"] = bool(res["d"]["median"] - res["c"]["median"] > spread)
    res["b_over_a"] = res["b"]["median"] / res["a"]["median"]
    res["c_over_a"] = res["c"]["median"] / res["a"]["median"]
    print(json.dumps(res), flush=True)
    return res


def fit(n, L, seed):
    """The gradient="forward" fit (25 % missed, D1 free, frame_len 6) on both paths: objective calls and wall time."""
    from extrack_amd import synth, tracking as T
    from extrack_amd.lmfit_compat import Parameters
    from oracle import oracle_np as O
    vals = dict(D0=1e-3, D1=0.25, LocErr=0.02, F0=0.6, F1=0.4, p01=0.1, p10=0.1, pBL=0.1)
    Tm = O.extract_params(vals, 0.02, 1, 1)[3]
    tr = synth.brownian_tracks(n, L, [1e-3, 0.25], Tm, [0.6, 0.4], seed=seed)
    mask = np.random.default_rng(11).random((n, L)) < 0.25
    mask[:, 0] = mask[:, -1] = False
    tr[mask] = np.nan
    res = {"fit": "%d x %d, 25 %% missed, D1 free, frame_len 6, gradient='forward'" % (n, L)}
    for label, env in (("gaps_reg2", None), ("gradr", "gradr")):
        p = Parameters()
        for k, v in vals.items():
            p.add(k, value=0.4 if k == "D1" else v, min=0.0 if k == "D1" else -np.inf, max=3.0 if k == "D1" else np.inf, vary=k == "D1")
        kw = dict(params=p, nb_states=2, frame_len=6, verbose=0, cell_dims=[1], gaps=True, gradient="forward")
        with grad_path(env):
            T.param_fitting({str(L): tr}, 0.02, **kw)  # warm: library, context
            t0 = time.perf_counter()
            f = T.param_fitting({str(L): tr}, 0.02, **kw)
            res[label] = {"wall_s": time.perf_counter() - t0, "calls": int(f.nfev), "D1": float(f.params["D1"].value), "objective": float(f.residual[0]),
                          "why": f.gradient_why}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the track counts (rehearsals)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    s = a.scale
    out = [run(int(1000000 * s), 30, 6), run(int(100000 * s), 30, 4), run(int(100000 * s), 30, 5), run(int(100000 * s), 30, 7),
           fit(3000, 12, 5), fit(int(100000 * s), 30, 6)]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
