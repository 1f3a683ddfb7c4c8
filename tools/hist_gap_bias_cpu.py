#!/usr/bin/env python3
"""What missed detections do to the state-duration histogram, on the CPU: synthetic 2-state tracks at the true
parameters, (1) complete, through the numpy oracle; (2) with 25 % of the interior rows missed, through the numpy restatement of the gap rule
(tests/hist_gap_reference.py (b)); (3) the same tracks with the missed rows deleted - dwell times that span a gap get shorter and the tracks
fall into shorter length buckets - through the oracle.  Prints, per state, the histogram mass (expected number of segments per track) and
the mean segment length in frames.

    python tools/hist_gap_bias_cpu.py [--tracks 2000] [--len 12] [--max-nb-states 200]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def summary(h, n):
    k = np.arange(1, h.shape[0] + 1)[:, None]
    return {"segments_per_track": (h.sum(0) / n).round(4).tolist(), "mean_len_frames": ((k * h).sum(0) / h.sum(0)).round(4).tolist(),
            "share_len_1": (h[0] / h.sum(0)).round(4).tolist()}


def main():
    import hist_gap_reference as HG
    from extrack_amd import synth
    from oracle import oracle_hist as OH
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=2000)
    ap.add_argument("--len", type=int, default=12)
    ap.add_argument("--max-nb-states", type=int, default=200)
    a = ap.parse_args()
    n, L, K = a.tracks, a.len, a.max_nb_states
    vals = dict(D0=1e-3, D1=0.25, LocErr=0.02, F0=0.6, F1=0.4, p01=0.1, p10=0.15, pBL=0.1)
    full = synth.brownian_tracks(n, L, [vals["D0"], vals["D1"]], [[0.9, 0.1], [0.15, 0.85]], [0.6, 0.4], seed=5)
    gapped = synth.drop_positions(full, 0.25, seed=6)
    deleted = {}
    for tr in gapped:
        keep = tr[~np.isnan(tr[:, 0])]
        deleted.setdefault(str(len(keep)), []).append(keep)
    deleted = {k: np.array(v) for k, v in deleted.items()}
    out = {"tracks": n, "len": L, "max_nb_states": K, "missing_rows": float(np.isnan(gapped[:, :, 0]).mean()),
           "complete": summary(OH.len_hist(vals, {str(L): full}, 0.02, [1.0], K), n),
           "gaps": summary(HG.len_hist_gaps(vals, {str(L): gapped}, 0.02, [1.0], K), n),
           "rows_deleted": summary(OH.len_hist(vals, deleted, 0.02, [1.0], K), n)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
