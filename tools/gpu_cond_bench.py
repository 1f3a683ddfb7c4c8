#!/usr/bin/env python3
"""Kernel time of the fixed-state position refinement (extrack_refine_fixed_states) beside extrack_map_states and extrack_refine_positions
on the same data, same build, same process.  Two datasets, as tools/gpu_map_bench.py: 1e6 tracks x 30, 2 states
(frame_len 6) and 5e5 x 60, 4 states (frame_len 5); the paths are those extrack_map_states decodes.  Per placement of the smoother's rows
(the library's own choice, then EXTRACK_COND_WS=global): 25 untimed launches, then the median extrack_last_kernel_ms of 20, the bandwidth
that implies for the bytes the call has to move (positions and states in; means, stds and one density per track out) and the median
wall time of the same calls, host copies included.  extrack_map_states: the same 25 / 20.  extrack_refine_positions (hundreds of ms per
launch): 2 untimed, 5 timed, on the first 50 000 tracks for the 4-state dataset.  Prints one JSON line per dataset.

    python tools/gpu_cond_bench.py [--scale 1.0] [--out profiles/cond_bench.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM, TIMED, DT, CELL = 25, 20, 0.02, [1.0]
HBM_TBS = 6.3  # achievable HBM bandwidth quoted in VERDICT.md


def timed(call, ctx, warm=WARM, n=TIMED):
    for _ in range(warm):
        call()
    ms, wall = [], []
    for _ in range(n):
        t0 = time.perf_counter()
        call()
        wall.append(time.perf_counter() - t0)
        ms.append(ctx.last_kernel_ms())
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}, float(np.median(wall))


def run(name, n, L, Ds, Tm, Fs, vals, S, F, n_refine):
    from extrack_amd import synth, tracking
    from extrack_amd.lmfit_compat import Parameters
    Cs = synth.brownian_tracks(n, L, Ds, Tm, Fs, seed=2)
    D = Cs.shape[2]
    p = Parameters()
    for k, v in vals.items():
        p.add(k, value=v)
    nbytes = n * L * D * 8 + n * L + n * L * D * 8 + n * L * 8 + n * 8
    res = {"dataset": name, "tracks": n, "len": L, "dims": D, "states": S, "frame_len": F, "warmup": WARM, "timed": TIMED, "bytes_moved": nbytes,
           "bound_ms_at_%.1f_TBs" % HBM_TBS: nbytes / (HBM_TBS * 1e12) * 1e3}
    ts = tracking.TrackSet([Cs])
    try:
        model = tracking._objective_model(p, ts, DT, CELL, None, S, 1, F, 1)
        st = ts.ctx.map_states(model, 0)
        res["tracks_without_path"] = int((st < 0).any(axis=1).sum())
        for where in ("default", "global"):
            if where == "global":
                os.environ["EXTRACK_COND_WS"] = "global"
            try:
                k_ms, wall = timed(lambda: ts.ctx.refine_fixed_states(model, 0, st, logdens=True), ts.ctx)
            finally:
                os.environ.pop("EXTRACK_COND_WS", None)
            res["cond_" + where] = {"kernel_ms": k_ms, "wall_s": wall, "launch": ts.ctx.last_launch_info(),
                                    "implied_TBs": nbytes / (k_ms["median"] * 1e-3) / 1e12,
                                    "fraction_of_%.1f_TBs" % HBM_TBS: nbytes / (k_ms["median"] * 1e-3) / 1e12 / HBM_TBS}
        k_ms, wall = timed(lambda: ts.ctx.map_states(model, 0, scores=True), ts.ctx)
        res["map_states"] = {"kernel_ms": k_ms, "wall_s": wall}
    finally:
        ts.close()
    ts = tracking.TrackSet([Cs[:n_refine]])
    try:
        model = tracking._objective_model(p, ts, DT, CELL, None, S, 1, F, 1)
        k_ms, wall = timed(lambda: ts.ctx.refine_positions(model, 0, 0.1, 1000), ts.ctx, warm=2, n=5)
        res["refine_positions"] = {"tracks": int(min(n, n_refine)), "warmup": 2, "timed": 5, "kernel_ms": k_ms, "wall_s": wall}
    except Exception as e:  # outside what the mixture path is built for: reported, not fatal
        res["refine_positions"] = {"tracks": int(min(n, n_refine)), "error": str(e)}
    finally:
        ts.close()
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the track counts (rehearsals)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n2, n5 = int(1000000 * a.scale), int(500000 * a.scale)
    out = [run("c2", n2, 30, [0.0, 0.25], [[0.9, 0.1], [0.1, 0.9]], [0.6, 0.4],
               dict(D0=1e-4, D1=0.25, LocErr=0.02, F0=0.6, F1=0.4, p01=0.1, p10=0.1, pBL=0.1), 2, 6, n2)]
    Tm = np.full((4, 4), 0.05 / 3)
    Tm[np.arange(4), np.arange(4)] = 0.95
    vals = dict(D0=1e-4, D1=0.02, D2=0.1, D3=0.5, LocErr=0.02, F0=.25, F1=.25, F2=.25, F3=.25, pBL=0.1)
    for i in range(4):
        for j in range(4):
            if i != j:
                vals["p%d%d" % (i, j)] = 0.05 / 3
    out.append(run("c5_predict", n5, 60, [0.0, 0.02, 0.1, 0.5], Tm, [0.25] * 4, vals, 4, 5, min(n5, 50000)))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
