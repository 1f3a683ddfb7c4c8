#!/usr/bin/env python3
"""Kernel time of the gap-aware state-duration histogram (extrack_segment_len_hist_gaps) beside the plain entry point on the same box, same
build, same process.  The shape of section 10's measurements: 1e5 tracks x 30, 2 states, max_nb_states 500 and 120;
the tracks gap-free through both entry points, and with 25 % of the interior rows missing through the gap-aware one (the plain one would
return NaN).  Per call: 3 untimed launches, then the median extrack_last_kernel_ms of 7.  Prints one JSON line per max_nb_states.

    python tools/gpu_hist_gap_bench.py [--scale 1.0] [--out profiles/hist_gap_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM, TIMED, DT, CELL = 3, 7, 0.02, [1.0]


def median_kernel_ms(call, ctx):
    for _ in range(WARM):
        call()
    ms = []
    for _ in range(TIMED):
        call()
        ms.append(ctx.last_kernel_ms())
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def main():
    from extrack_amd import _lib, engine, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the track count (rehearsals)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, L = int(100000 * a.scale), 30
    Ds, Tm, Fs = [0.0, 0.25], [[0.9, 0.1], [0.1, 0.9]], [0.6, 0.4]
    full = synth.brownian_tracks(n, L, Ds, Tm, Fs, seed=2)
    gapped = synth.drop_positions(full, 0.25, seed=3)
    ds = np.sqrt(2 * np.array([1e-4, 0.25]) * DT)
    model = _lib.ModelHandle(ds, Fs, np.array(Tm), engine.p_stay_table(ds, 2, 1, CELL), 0.1, 1, 2, 3, L + 1, locerr=[0.02])
    ctx = _lib.Context(0)
    out = []
    try:
        ctx.upload_bucket(full)
        ctx.upload_bucket(gapped)
        for K in (500, 120):
            res = {"tracks": n, "len": L, "states": 2, "max_nb_states": K, "warmup": WARM, "timed": TIMED,
                   "missing_rows": float(np.isnan(gapped).all(axis=2).mean())}
            for what, call in (("plain_gap_free", lambda: ctx.segment_len_hist(model, 0, K)),
                               ("gaps_gap_free", lambda: ctx.segment_len_hist(model, 0, K, gaps=True)),
                               ("gaps_25pct_missing", lambda: ctx.segment_len_hist(model, 1, K, gaps=True))):
                res[what + "_kernel_ms"] = median_kernel_ms(call, ctx)
                res[what + "_launch"] = ctx.last_launch_info()
            h = ctx.segment_len_hist(model, 1, K, gaps=True)
            res["gapped_hist_finite"] = bool(np.all(np.isfinite(h)))
            res["gaps_over_plain"] = res["gaps_25pct_missing_kernel_ms"]["median"] / res["plain_gap_free_kernel_ms"]["median"]
            print(json.dumps(res), flush=True)
            out.append(res)
    finally:
        ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
