#!/usr/bin/env python3
"""Kernel time of the pairwise state posteriors (extrack_predict_pairs: pairs + counts, and counts alone) beside extrack_predict and
extrack_loglik on the same data, same build, same process.  Two datasets: the headline shape (1e6 tracks x 30, 2 states,
frame_len 6) and the predict shape of bench.py's configs[4] (5e5 x 60, 4 states, frame_len 5).  Per entry point: 25 untimed launches, then the
median extrack_last_kernel_ms of 20.  Prints one JSON line per dataset.

    python tools/gpu_pairs_bench.py [--scale 1.0] [--out profiles/pairs_bench.json] [--base-only]

--base-only times extrack_predict and extrack_loglik alone: run it against a build of the parent commit (EXTRACK_HIP_LIB=...) on the same box
to see that the existing kernels did not move.

    python tools/gpu_pairs_bench.py --soft-counts [--out ...]

--soft-counts: on 400 synthetic tracks per row (the models of DESIGN.md section 16's table, frame_len 6 and 4), how far the row-normalised soft
transition-count matrix lies from the generating per-step matrix and from the hard count along predict_states (largest absolute entry)."""
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


def run(name, n, L, Ds, Tm, Fs, vals, S, F, base_only=False):
    from extrack_amd import synth, tracking
    from extrack_amd.lmfit_compat import Parameters
    Cs = synth.brownian_tracks(n, L, Ds, Tm, Fs, seed=2)
    p = Parameters()
    for k, v in vals.items():
        p.add(k, value=v)
    ts = tracking.TrackSet([Cs])
    res = {"dataset": name, "tracks": n, "len": L, "states": S, "frame_len": F, "warmup": WARM, "timed": TIMED, "base_only": bool(base_only)}
    try:
        model = tracking._objective_model(p, ts, DT, CELL, None, S, 1, F, 1)
        calls = [("predict", lambda: ts.ctx.predict(model, 0)), ("loglik", lambda: ts.loglik(model))]
        if not base_only:
            # the host arrays are made once: N * (L-1) * S^2 doubles per call would be paged in again 45 times
            import ctypes as C
            pr, ct = np.empty((n, L - 1, S, S)), np.empty((n, S, S))
            fn, h, vp = ts.ctx._lib.extrack_predict_pairs, ts.ctx._h, C.c_void_p

            def pairs_call(with_pairs):
                ts.ctx._check(fn(h, C.byref(model.c), 0, pr.ctypes.data_as(vp) if with_pairs else None, ct.ctypes.data_as(vp)))

            calls = [("pairs", lambda: pairs_call(True)), ("counts_only", lambda: pairs_call(False))] + calls
        for what, call in calls:
            res[what + "_kernel_ms"] = median_kernel_ms(call, ts.ctx)
            res[what + "_launch"] = ts.ctx.last_launch_info()
    finally:
        ts.close()
    if not base_only:
        res["pairs_over_predict"] = res["pairs_kernel_ms"]["median"] / res["predict_kernel_ms"]["median"]
        res["counts_only_over_predict"] = res["counts_only_kernel_ms"]["median"] / res["predict_kernel_ms"]["median"]
    print(json.dumps(res), flush=True)
    return res


def soft_counts():
    """The models and tracks of DESIGN.md section 16's table (tests/test_map_cpu.py): 2 states (D 0.0005 / 0.25, 10 % switches per step), 12
    positions; 3 states (0.0005 / 0.04 / 0.25, 10 % to each other state), 9 positions; 400 tracks, LocErr 0.02, seed 3."""
    from extrack_amd import synth, tracking
    from extrack_amd.lmfit_compat import Parameters
    out = []
    for S, L, Ds, Tm, Fs in ((2, 12, [0.0005, 0.25], np.array([[0.9, 0.1], [0.1, 0.9]]), [0.5, 0.5]),
                             (3, 9, [0.0005, 0.04, 0.25], np.array([[0.8, 0.1, 0.1], [0.1, 0.8, 0.1], [0.1, 0.1, 0.8]]), [1 / 3, 1 / 3, 1 / 3])):
        tr = {str(L): synth.brownian_tracks(400, L, Ds, Tm.tolist(), Fs, LocErr=0.02, dt=DT, dims=2, seed=3)}
        p = Parameters()
        for s in range(S):
            p.add("D%d" % s, value=Ds[s])
            p.add("F%d" % s, value=Fs[s])
            for t in range(S):
                if s != t:
                    p.add("p%d%d" % (s, t), value=float(-np.log(1 - Tm[s, t])))  # extract_params maps a rate k to 1 - exp(-k)
        p.add("LocErr", value=0.02)
        p.add("pBL", value=0.1)
        for F in (6, 4):
            cnt = tracking.predict_transitions(tr, DT, p, cell_dims=CELL, nb_states=S, frame_len=F, output="counts")
            C, P = tracking.transition_matrix(cnt)
            st = tracking.predict_states(tr, DT, p, cell_dims=CELL, nb_states=S, frame_len=F)[str(L)]
            H = np.zeros((S, S))
            np.add.at(H, (st[:, :-1].ravel(), st[:, 1:].ravel()), 1.0)
            Hn = H / H.sum(axis=1, keepdims=True)
            r = {"states": S, "frame_len": F, "tracks": 400, "len": L, "soft_counts": C.tolist(), "soft_matrix": P.tolist(), "hard_counts": H.tolist(),
                 "hard_matrix": Hn.tolist(), "generating": Tm.tolist(), "max_abs_soft_minus_generating": float(np.abs(P - Tm).max()),
                 "max_abs_soft_minus_hard": float(np.abs(P - Hn).max()), "max_abs_hard_minus_generating": float(np.abs(Hn - Tm).max())}
            print(json.dumps(r), flush=True)
            out.append(r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the track counts (rehearsals)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--base-only", action="store_true", help="time extrack_predict and extrack_loglik alone (a build of the parent: EXTRACK_HIP_LIB)")
    ap.add_argument("--soft-counts", action="store_true", help="soft against hard and generating transition matrices on 400 synthetic tracks")
    a = ap.parse_args()
    if a.soft_counts:
        out = soft_counts()
    else:
        out = [run("c2", int(1000000 * a.scale), 30, [0.0, 0.25], [[0.9, 0.1], [0.1, 0.9]], [0.6, 0.4],
                   dict(D0=1e-4, D1=0.25, LocErr=0.02, F0=0.6, F1=0.4, p01=0.1, p10=0.1, pBL=0.1), 2, 6, a.base_only)]
        Tm = np.full((4, 4), 0.05 / 3)
        Tm[np.arange(4), np.arange(4)] = 0.95
        vals = dict(D0=1e-4, D1=0.02, D2=0.1, D3=0.5, LocErr=0.02, F0=.25, F1=.25, F2=.25, F3=.25, pBL=0.1)
        for i in range(4):
            for j in range(4):
                if i != j:
                    vals["p%d%d" % (i, j)] = 0.05 / 3
        out.append(run("c5_predict", int(500000 * a.scale), 60, [0.0, 0.02, 0.1, 0.5], Tm, [0.25] * 4, vals, 4, 5, a.base_only))
    if a.out:
        mode = "r+" if os.path.exists(a.out) else "w"
        prev = []
        if mode == "r+":
            with open(a.out) as f:
                prev = json.load(f)
        with open(a.out, "w") as f:
            json.dump(prev + out, f, indent=1)


if __name__ == "__main__":
    main()
