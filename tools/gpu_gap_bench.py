#!/usr/bin/env python3
"""Kernel time of the gap-aware likelihood (extrack_loglik_gaps) beside extrack_loglik on the same data, same build, same process
(DESIGN.md section 18).  1e6 tracks x 30 positions at frame_len 6, for 3 states (where extrack_loglik itself runs the general body) and
2 states (where it runs the register-resident kernel and the gap entry point the general body).  Per dataset: WARM untimed evaluations of
every version, then ROUNDS rounds of [extrack_loglik, extrack_loglik_gaps, extrack_loglik again] on gap-free data followed by
extrack_loglik_gaps on the same tracks with 25 % of the interior rows missing - versions alternated, device events
(extrack_last_kernel_ms).  The two extrack_loglik series of a round give the spread of repeated runs the difference is read against.
Writes gap_bench.json into the output directory and prints one JSON line per dataset.

    python tools/gpu_gap_bench.py [--scale 1.0] [--out profiles]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM, ROUNDS, DT, CELL, F = 3, 9, 0.02, [1.0], 6


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def run(name, n, L, Ds, Tm, Fs, vals, S):
    from extrack_amd import synth, tracking
    from extrack_amd.lmfit_compat import Parameters
    Cs = synth.brownian_tracks(n, L, Ds, Tm, Fs, seed=2)
    p = Parameters()
    for k, v in vals.items():
        p.add(k, value=v)
    full = tracking.TrackSet([Cs])
    holes = tracking.TrackSet([synth.drop_positions(Cs, 0.25, seed=3)], gaps=True)
    try:
        model = tracking._objective_model(p, full, DT, CELL, None, S, 1, F, 1)
        series = {"loglik_a": [], "loglik_gaps_gapfree": [], "loglik_b": [], "loglik_gaps_25pct": []}
        calls = [("loglik_a", lambda: full.ctx.loglik(model), full), ("loglik_gaps_gapfree", lambda: full.ctx.loglik(model, gaps=True), full),
                 ("loglik_b", lambda: full.ctx.loglik(model), full), ("loglik_gaps_25pct", lambda: holes.ctx.loglik(model, gaps=True), holes)]
        values, launch = {}, {}
        for r in range(WARM + ROUNDS):
            for key, call, ts in calls:
                values[key] = call()
                if r >= WARM:
                    series[key].append(ts.ctx.last_kernel_ms())
                launch[key] = ts.ctx.last_launch_info()
    finally:
        full.close()
        holes.close()
    res = {"dataset": name, "tracks": n, "len": L, "states": S, "frame_len": F, "warmup": WARM, "rounds": ROUNDS,
           "kernel_ms": {k: stats(v) for k, v in series.items()}, "values": values, "launch": launch}
    a, b, g = (res["kernel_ms"][k]["median"] for k in ("loglik_a", "loglik_b", "loglik_gaps_gapfree"))
    res["spread_of_repeated_loglik_pct"] = 100.0 * abs(a - b) / min(a, b)
    res["gaps_over_loglik_gapfree"] = g / (0.5 * (a + b))
    res["gaps_25pct_over_loglik_gapfree"] = res["kernel_ms"]["loglik_gaps_25pct"]["median"] / (0.5 * (a + b))
    res["total_ll_rel_diff_gapfree"] = abs(values["loglik_gaps_gapfree"] - values["loglik_a"]) / abs(values["loglik_a"])
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the track counts (rehearsals)")
    ap.add_argument("--out", default=None, help="output directory (gap_bench.json)")
    a = ap.parse_args()
    n = int(1000000 * a.scale)
    out = [run("3 states", n, 30, [0.0, 0.05, 0.3], [[0.9, 0.06, 0.04], [0.05, 0.9, 0.05], [0.03, 0.07, 0.9]], [0.3, 0.3, 0.4],
               dict(D0=1e-4, D1=0.05, D2=0.3, LocErr=0.02, F0=0.3, F1=0.3, F2=0.4, p01=0.08, p02=0.04, p10=0.06, p12=0.05, p20=0.03, p21=0.07,
                    pBL=0.1), 3),
           run("2 states", n, 30, [0.0, 0.25], [[0.9, 0.1], [0.1, 0.9]], [0.6, 0.4],
               dict(D0=1e-4, D1=0.25, LocErr=0.02, F0=0.6, F1=0.4, p01=0.1, p10=0.1, pBL=0.1), 2)]
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "gap_bench.json"), "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
