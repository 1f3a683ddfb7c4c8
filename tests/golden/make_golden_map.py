#!/usr/bin/env python3
"""Generate tests/golden/map_cases.{json,npz}: exact most-likely state paths taken from the REFERENCE's own sequence matrix.

Run in the build container only (needs the reference; see oracle/ref_loader.py for the import shims).  The produced files are data:
inputs, and for every track the argmax of the reference's per-sequence log-probabilities with its value and the gap to the runner-up.
Nothing of the reference's source travels.

    python tests/golden/make_golden_map.py

Reference entry point exercised: extrack/tracking.py:109 P_Cs_inter_bound_stats (first return value, :318), for tracks of at most
frame_len + 1 positions, where it fuses nothing and the matrix holds every state sequence of the track.  With isBL its newest digit is the
state AFTER the last position: it is summed out (log-sum-exp) before the argmax, as it is no position of the track.
"""
import contextlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import ref_loader as R  # noqa: E402

T = R.load("tracking")


def rand_model(rng, S):
    ds = np.sort(rng.uniform(0.004, 0.2, S))
    Fs = rng.dirichlet(np.ones(S) * 2)
    Tm = rng.uniform(0.02, 0.9 / max(S - 1, 1) if S > 3 else 0.3, (S, S))
    Tm[np.arange(S), np.arange(S)] = 0
    Tm[np.arange(S), np.arange(S)] = 1 - Tm.sum(1)
    return ds, Fs, Tm


def main():
    rng = np.random.default_rng(20261017)
    out, meta, cid = {}, [], 0
    N = 6
    for S, F in ((2, 4), (2, 6), (3, 4), (4, 3)):
        for L in sorted(set([2, 3, F, F + 1])):
            for D, le in [(1, "scalar"), (2, "scalar"), (2, "dim"), (2, "peak"), (3, "dim"), (3, "peak")]:
                for isBL in (0, 1):
                    min_len = int(rng.choice([2, 3, 5]))
                    ds, Fs, Tm = rand_model(rng, S)
                    pBL = float(rng.uniform(0.02, 0.2))
                    cell = [float(rng.uniform(0.5, 2.0))] if rng.random() < 0.6 else [0.6, 2.5]
                    step = ds[rng.integers(0, S, (N, L, 1))]
                    Cs = np.cumsum(rng.normal(0, 1, (N, L, D)) * step, 1) + rng.normal(0, 0.02, (N, L, D)) + rng.uniform(0, 5, (N, 1, D))
                    if le == "scalar":
                        LE = np.array([[[0.02]]])
                    elif le == "dim":
                        LE = rng.uniform(0.01, 0.04, (1, 1, D))
                    else:
                        LE = rng.uniform(0.01, 0.04, (N, L, D))
                    with contextlib.redirect_stdout(io.StringIO()):
                        LP = np.asarray(T.P_Cs_inter_bound_stats(Cs, LE, ds, Fs, Tm, pBL, isBL, cell, 1, F, 0, min_len)[0], float)
                    assert LP.shape == (N, S ** (L + isBL)), LP.shape
                    if isBL:
                        LPr = LP.reshape(N, S ** L, S)
                        mx = LPr.max(axis=2, keepdims=True)
                        LP = np.log(np.exp(LPr - mx).sum(axis=2)) + mx[:, :, 0]
                    best = np.argmax(LP, axis=1)
                    srt = np.sort(LP, axis=1)
                    path = np.stack([(best // S ** (L - 1 - p)) % S for p in range(L)], axis=1).astype(np.int8)
                    pre = "m%04d_" % cid
                    out[pre + "Cs"], out[pre + "LE"] = Cs, LE
                    out[pre + "ds"], out[pre + "Fs"], out[pre + "T"] = ds, Fs, Tm
                    out[pre + "path"], out[pre + "logp"], out[pre + "margin"] = path, LP[np.arange(N), best], srt[:, -1] - srt[:, -2]
                    meta.append(dict(id=cid, S=S, F=F, L=L, D=D, le=le, isBL=isBL, min_len=min_len, pBL=pBL, cell_dims=cell))
                    cid += 1
    np.savez_compressed(os.path.join(HERE, "map_cases.npz"), **out)
    with open(os.path.join(HERE, "map_cases.json"), "w") as f:
        json.dump(meta, f, indent=0)
    print("map cases:", cid)


if __name__ == "__main__":
    main()
