#!/usr/bin/env python3
"""Kernel time of the two-state likelihood with missed detections on the register-resident kernel beside the general gap
body, same data, same build, same process.  Datasets: 1e6 tracks x 30, 2 states, frame_len 6 (the headline shape) and 1e5 x 30 at frame_len 4
and 7; D = [0, 0.25], LocErr 0.02, p01 = p10 = 0.1.  Contexts are created under EXTRACK_GAP_REG2_F=all (frame_len 4 is upgraded on request
only).  Rows per dataset:

    a  extrack_loglik, gap-free data                    (xt_ll_r2_kernel: the plain kernel)
    b  extrack_loglik_gaps, the same gap-free data      (gap-aware register-resident kernel)
    c  extrack_loglik_gaps, 25 % of the interior rows missed
    d  c in a context created under EXTRACK_LL_PATH=lds (the general gap body: the path before section 25)

Per row: 25 untimed launches, then extrack_last_kernel_ms of 20 - median, min, max - and the kernel family extrack_last_ll_path reports.
`c_faster_than_d` compares the medians against the spread of the two rows (max - min of each, added).  Then the 3000 x 12 fit of
tests/test_hip_gaps.py on both paths: objective calls and wall time.  Prints one JSON line per dataset and one for the fit.

    python tools/gpu_gap_reg2_bench.py [--scale 1.0] [--out profiles/reg2_gaps_bench.json]
"""
import argparse
import contextlib
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM, TIMED, DT, CELL = 25, 20, 0.02, [1.0]
DS, TM, FS, LE, PBL = [0.0, 0.25], [[0.9, 0.1], [0.1, 0.9]], [0.6, 0.4], 0.02, 0.1


@contextlib.contextmanager
def ll_path(value):
    """EXTRACK_LL_PATH (None: unset) and EXTRACK_GAP_REG2_F=all while a context is created (the knobs bind there): frame_len 4 is upgraded on
    request only, and is measured like the others."""
    old = {k: os.environ.get(k) for k in ("EXTRACK_LL_PATH", "EXTRACK_GAP_REG2_F")}
    os.environ["EXTRACK_GAP_REG2_F"] = "all"
    if value is None:
        os.environ.pop("EXTRACK_LL_PATH", None)
    else:
        os.environ["EXTRACK_LL_PATH"] = value
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def timed(ctx, call):
    for _ in range(WARM):
        call()
    ms = []
    for _ in range(TIMED):
        call()
        ms.append(ctx.last_kernel_ms())
    return {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms)), "path": ctx.last_ll_path(),
            "launch": ctx.last_launch_info()}


def run(n, L, F):
    from extrack_amd import _lib, engine, synth
    full = synth.brownian_tracks(n, L, DS, TM, FS, LocErr=LE, dt=DT, seed=2)
    gapped = synth.drop_positions(full, 0.25, seed=3)
    ds = np.sqrt(2 * np.array(DS) * DT)
    model = _lib.ModelHandle(ds, FS, TM, engine.p_stay_table(ds, 2, 1, CELL), PBL, 1, F, L, L, locerr=[LE])
    res = {"tracks": n, "len": L, "dims": full.shape[2], "frame_len": F, "warmup": WARM, "timed": TIMED,
           "missed_fraction": float(np.isnan(gapped[:, :, 0]).mean())}
    totals = {}
    for label, env in (("reg2", None), ("lds", "lds")):
        with ll_path(env):
            ctx = _lib.Context(0)
        try:
            rows = (("a", full, False), ("b", full, True), ("c", gapped, True)) if label == "reg2" else (("d", gapped, True),)
            for name, data, gaps in rows:
                ctx.clear_buckets()
                ctx.upload_bucket(data, None)
                res[name] = timed(ctx, lambda: ctx.loglik(model, gaps=gaps))
                totals[name] = ctx.loglik(model, gaps=gaps)
        finally:
            ctx.close()
    res["total_ll"] = totals
    res["c_vs_d_rel_diff"] = abs(totals["c"] - totals["d"]) / abs(totals["d"])
    spread = (res["c"]["max"] - res["c"]["min"]) + (res["d"]["max"] - res["d"]["min"])
    res["d_over_c"] = res["d"]["median"] / res["c"]["median"]
    res["c_faster_than_d"] = bool(res["d"]["median"] - res["c"]["median"] > spread)
    res["b_over_a"] = res["b"]["median"] / res["a"]["median"]
    res["c_over_a"] = res["c"]["median"] / res["a"]["median"]
    print(json.dumps(res), flush=True)
    return res


def fit():
    """The fit of tests/test_hip_gaps.py (3000 x 12, 25 % missed, D1 free) on both paths: objective calls and wall time."""
    from extrack_amd import synth, tracking as T
    from extrack_amd.lmfit_compat import Parameters
    from oracle import oracle_np as O
    vals = dict(D0=1e-3, D1=0.25, LocErr=0.02, F0=0.6, F1=0.4, p01=0.1, p10=0.1, pBL=0.1)
    Tm = O.extract_params(vals, 0.02, 1, 1)[3]
    tr = synth.brownian_tracks(3000, 12, [1e-3, 0.25], Tm, [0.6, 0.4], seed=5)
    mask = np.random.default_rng(11).random((3000, 12)) < 0.25
    mask[:, 0] = mask[:, -1] = False
    tr[mask] = np.nan
    res = {"fit": "3000 x 12, 25 % missed, D1 free, frame_len 6"}
    for label, env in (("reg2", None), ("lds", "lds")):
        p = Parameters()
        for k, v in vals.items():
            p.add(k, value=0.4 if k == "D1" else v, min=0.0 if k == "D1" else -np.inf, max=3.0 if k == "D1" else np.inf, vary=k == "D1")
        with ll_path(env):
            T.param_fitting({"12": tr}, 0.02, params=p, nb_states=2, frame_len=6, verbose=0, cell_dims=[1], gaps=True)  # warm: library, context
            t0 = time.perf_counter()
            f = T.param_fitting({"12": tr}, 0.02, params=p, nb_states=2, frame_len=6, verbose=0, cell_dims=[1], gaps=True)
            res[label] = {"wall_s": time.perf_counter() - t0, "calls": int(f.nfev), "D1": float(f.params["D1"].value), "objective": float(f.residual[0])}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the track counts (rehearsals)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = [run(int(1000000 * a.scale), 30, 6), run(int(100000 * a.scale), 30, 4), run(int(100000 * a.scale), 30, 7), fit()]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
