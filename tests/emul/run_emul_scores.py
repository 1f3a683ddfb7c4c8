"""ctypes driver for tests/emul/libxt_emul_scores.so (test infrastructure): the per-track score store of the forward-mode gradient
bodies on CPU threads (emul_scores.cpp; emul_r2.cpp and emul_gradr.cpp compiled in under object names of their own)."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "libxt_emul_scores.so")
        units = ["emul_scores.cpp", "emul_r2.cpp", "emul_gradr.cpp"]
        csrc = os.path.join(HERE, "..", "..", "extrack_amd", "csrc")
        deps = [os.path.join(HERE, u) for u in units + ["emul_ctx.h"]] + [os.path.join(csrc, h) for h in os.listdir(csrc) if h.endswith(".h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            import subprocess
            objs = [os.path.join(HERE, "scores_" + u[:-4] + ".o") for u in units]
            procs = [subprocess.Popen(["g++", "-O1", "-std=c++17", "-fPIC", "-pthread", "-c", os.path.join(HERE, u), "-o", o]) for u, o in zip(units, objs)]
            if any(p.wait() != 0 for p in procs):
                raise RuntimeError("g++ failed on tests/emul (scores)")
            subprocess.check_call(["g++", "-shared", "-pthread", "-o", so] + objs)
        _lib = C.CDLL(so)
    return _lib


def run_scores(family, buckets, row0, le, ds, Fs, T, pBL, p_stay, ns, F, min_len, max_len, tangents, blocks_per_bucket=None, with_scores=True):
    """family: 2 xt_reg2.h | 3, 4 xt_gradr.h (directions per pass) | 0, 1 xt_grad.h (one / two passes).  buckets: arrays [N, L, D] in LAUNCH
    order; row0[i]: first row of bucket i in the score matrix.  tangents: list of dicts (keys ds2, Fs, TrMat, p_stay, locerr, pBL).
    Returns (sum LL, gradient [n], scores [sum N, n] (NaN where nothing was stored))."""
    f64 = lambda x: np.ascontiguousarray(x, dtype=np.float64)
    buckets = [f64(b) for b in buckets]
    S, D = len(ds), buckets[0].shape[2]
    G = S ** ns
    le = f64(np.asarray(le, float).reshape(-1))
    n = len(tangents)
    rows = np.zeros((n, 6 + 2 * S + S * S + G))
    for i, t in enumerate(tangents):
        v = np.atleast_1d(np.asarray(t.get("locerr", 0.0), float)).ravel()
        rows[i, :len(v)] = v
        rows[i, 5] = t.get("pBL", 0.0)
        rows[i, 6:6 + S] = np.broadcast_to(t.get("ds2", 0.0), (S,))
        rows[i, 6 + S:6 + 2 * S] = np.broadcast_to(t.get("Fs", 0.0), (S,))
        rows[i, 6 + 2 * S:6 + 2 * S + S * S] = np.broadcast_to(t.get("TrMat", 0.0), (S, S)).ravel()
        rows[i, 6 + 2 * S + S * S:] = np.broadcast_to(t.get("p_stay", 0.0), (G,))
    nb = len(buckets)
    ptrs = (C.c_void_p * nb)(*[b.ctypes.data for b in buckets])
    Ns = (C.c_longlong * nb)(*[len(b) for b in buckets])
    Ls = (C.c_int * nb)(*[b.shape[1] for b in buckets])
    r0 = (C.c_longlong * nb)(*[int(r) for r in row0])
    bpb = (C.c_int * nb)(*(blocks_per_bucket or [2] * nb))
    ntot = sum(len(b) for b in buckets)
    scores = np.full((ntot, n), np.nan)
    out = np.zeros(1 + n)
    vp = lambda x: f64(x).ctypes.data_as(C.c_void_p)
    keep = [f64(ds), f64(Fs), f64(T), f64(p_stay), f64(rows)]
    rc = lib().xt_emul_scores(int(family), nb, ptrs, Ns, Ls, r0, D, S, int(ns), int(F), int(max_len), int(min_len), len(le), le.ctypes.data_as(C.c_void_p),
                              C.c_double(pBL), *[k.ctypes.data_as(C.c_void_p) for k in keep[:4]], n, keep[4].ctypes.data_as(C.c_void_p), bpb,
                              1 if with_scores else 0, scores.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise RuntimeError("xt_emul_scores failed: %d" % rc)
    return out[0], out[1:], scores
