#!/usr/bin/env python3
"""Kernel time of the gap-aware state-path decoder and fixed-state smoother (extrack_map_states_gaps, extrack_refine_fixed_states_gaps)
beside their plain twins on the same data, same build, same process.  The headline shape of
tools/gpu_map_bench.py: 1e6 tracks x 30, 2 states, frame_len 6; once gap-free (plain and gap-aware entry points) and once with 25 % of the
interior rows missing (gap-aware only: the plain ones would poison every such track).  Per entry point: 25 untimed launches, then the
median extrack_last_kernel_ms of 20.  The smoother runs along the paths the decoder returned.  Prints one JSON line per dataset.

    python tools/gpu_map_gap_bench.py [--scale 1.0] [--out profiles/map_gap_bench.json]
"""
import argparse
import json
import os
import sys

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
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def run(name, Cs, p, S, F, plain):
    from extrack_amd import tracking
    n, L, _ = Cs.shape
    res = {"dataset": name, "tracks": n, "len": L, "states": S, "frame_len": F, "warmup": WARM, "timed": TIMED,
           "missing_rows": float(np.isnan(Cs).all(axis=2).mean())}
    ts = tracking.TrackSet([Cs], gaps=True)
    try:
        model = tracking._objective_model(p, ts, DT, CELL, None, S, 1, F, 1)
        st = ts.ctx.map_states(model, 0, gaps=True)
        res["tracks_without_path"] = int((st < 0).any(axis=1).sum())
        calls = [("map_states_gaps", lambda: ts.ctx.map_states(model, 0, scores=True, gaps=True)),
                 ("refine_fixed_states_gaps", lambda: ts.ctx.refine_fixed_states(model, 0, st, logdens=True, gaps=True))]
        if plain:
            calls += [("map_states", lambda: ts.ctx.map_states(model, 0, scores=True)),
                      ("refine_fixed_states", lambda: ts.ctx.refine_fixed_states(model, 0, st, logdens=True))]
        for what, call in calls:
            res[what + "_kernel_ms"] = median_kernel_ms(call, ts.ctx)
            res[what + "_launch"] = ts.ctx.last_launch_info()
        if plain:
            res["map_gaps_over_plain"] = res["map_states_gaps_kernel_ms"]["median"] / res["map_states_kernel_ms"]["median"]
            res["refine_gaps_over_plain"] = res["refine_fixed_states_gaps_kernel_ms"]["median"] / res["refine_fixed_states_kernel_ms"]["median"]
    finally:
        ts.close()
    print(json.dumps(res), flush=True)
    return res


def main():
    from extrack_amd import synth
    from extrack_amd.lmfit_compat import Parameters
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the track count (rehearsals)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = int(1000000 * a.scale)
    p = Parameters()
    for k, v in dict(D0=1e-4, D1=0.25, LocErr=0.02, F0=0.6, F1=0.4, p01=0.1, p10=0.1, pBL=0.1).items():
        p.add(k, value=v)
    Cs = synth.brownian_tracks(n, 30, [0.0, 0.25], [[0.9, 0.1], [0.1, 0.9]], [0.6, 0.4], seed=2)
    out = [run("c2 gap-free", Cs, p, 2, 6, True), run("c2 25% gaps", synth.drop_positions(Cs, 0.25, seed=3), p, 2, 6, False)]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
