#!/usr/bin/env python3
"""Kernel time of the state-path decoder (extrack_map_states) beside extrack_predict and extrack_loglik on the same data, same build, same
process.  Two datasets: the headline shape (1e6 tracks x 30, 2 states, frame_len 6) and the predict shape of
bench.py's configs[4] (5e5 x 60, 4 states, frame_len 5).  Per entry point: 25 untimed launches, then the median extrack_last_kernel_ms of
20; plus the wall time of predict_states (upload, launch, N x L bytes back).  Prints one JSON line per dataset.

    python tools/gpu_map_bench.py [--scale 1.0] [--out profiles/map_bench.json] [--map-only]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM, TIMED, DT, CELL = 25, 20, 0.02, [1.0]


def median_kernel_ms(call, ctx):
    for _ in range(WARM):
        call()
    ms = []
    for _ in range(TIMED):
        call()
        ms.append(ctx.last_kernel_ms())
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def run(name, n, L, Ds, Tm, Fs, vals, S, F, map_only=False):
    from extrack_amd import synth, tracking
    from extrack_amd.lmfit_compat import Parameters
    Cs = synth.brownian_tracks(n, L, Ds, Tm, Fs, seed=2)
    p = Parameters()
    for k, v in vals.items():
        p.add(k, value=v)
    ts = tracking.TrackSet([Cs])
    res = {"dataset": name, "tracks": n, "len": L, "states": S, "frame_len": F, "warmup": WARM, "timed": TIMED}
    try:
        model = tracking._objective_model(p, ts, DT, CELL, None, S, 1, F, 1)
        for what, call in (("map_states", lambda: ts.ctx.map_states(model, 0, scores=True)), ("predict", lambda: ts.ctx.predict(model, 0)),
                           ("loglik", lambda: ts.loglik(model)))[:1 if map_only else 3]:
            med, lo, hi = median_kernel_ms(call, ts.ctx)
            res[what + "_kernel_ms"] = {"median": med, "min": lo, "max": hi}
            if what == "map_states":
                res["map_states_launch"] = ts.ctx.last_launch_info()
    finally:
        ts.close()
    t0 = time.perf_counter()
    tracking.predict_states({str(L): Cs}, DT, p, cell_dims=CELL, frame_len=F)
    res["predict_states_wall_s"] = time.perf_counter() - t0
    if not map_only:
        res["map_over_predict"] = res["map_states_kernel_ms"]["median"] / res["predict_kernel_ms"]["median"]
        res["map_over_loglik"] = res["map_states_kernel_ms"]["median"] / res["loglik_kernel_ms"]["median"]
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the track counts (rehearsals)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--map-only", action="store_true", help="time extrack_map_states alone (A/B of build variants: EXTRACK_HIP_LIB)")
    a = ap.parse_args()
    out = [run("c2", int(1000000 * a.scale), 30, [0.0, 0.25], [[0.9, 0.1], [0.1, 0.9]], [0.6, 0.4],
               dict(D0=1e-4, D1=0.25, LocErr=0.02, F0=0.6, F1=0.4, p01=0.1, p10=0.1, pBL=0.1), 2, 6, a.map_only)]
    Tm = np.full((4, 4), 0.05 / 3)
    Tm[np.arange(4), np.arange(4)] = 0.95
    vals = dict(D0=1e-4, D1=0.02, D2=0.1, D3=0.5, LocErr=0.02, F0=.25, F1=.25, F2=.25, F3=.25, pBL=0.1)
    for i in range(4):
        for j in range(4):
            if i != j:
                vals["p%d%d" % (i, j)] = 0.05 / 3
    out.append(run("c5_predict", int(500000 * a.scale), 60, [0.0, 0.02, 0.1, 0.5], Tm, [0.25] * 4, vals, 4, 5, a.map_only))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
