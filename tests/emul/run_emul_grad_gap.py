"""ctypes driver for tests/emul/libxt_emul_grad_gap.so (test infrastructure): the forward-mode gradient bodies (xt_gradr.h, xt_grad.h) with and
without their GAPS flag on CPU threads (emul_grad_gap.cpp), several length buckets per emulated launch through the bucket-descriptor table,
with per-track scores."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "libxt_emul_grad_gap.so")
        csrc = os.path.join(HERE, "..", "..", "extrack_amd", "csrc")
        deps = [os.path.join(HERE, u) for u in ("emul_grad_gap.cpp", "emul_ctx.h")] + [os.path.join(csrc, h) for h in os.listdir(csrc) if h.endswith(".h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            import subprocess
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-pthread", "-shared", os.path.join(HERE, "emul_grad_gap.cpp"), "-o", so])
        _lib = C.CDLL(so)
    return _lib


def pack_tangents(tangents, S):
    """Rows [locerr(3), slope, offset, pBL, ds2(S), Fs(S), TrMat(S*S), p_stay(S)] from tangent dicts (missing fields are zero)."""
    rows = np.zeros((len(tangents), 6 + 3 * S + S * S))
    for i, t in enumerate(tangents):
        le = np.atleast_1d(np.asarray(t.get("locerr", []), float)).ravel()
        rows[i, :len(le)] = le
        rows[i, 3], rows[i, 4], rows[i, 5] = t.get("slope", 0.0), t.get("offset", 0.0), t.get("pBL", 0.0)
        for k, (o, n) in (("ds2", (6, S)), ("Fs", (6 + S, S)), ("TrMat", (6 + 2 * S, S * S)), ("p_stay", (6 + 2 * S + S * S, S))):
            if k in t:
                rows[i, o:o + n] = np.asarray(t[k], float).ravel()
    return rows


def run_grad_gap(body, buckets, le, ds, Fs, T, pBL, p_stay, F, min_len, max_len, tangents, sigmas=None, slope_offset=None, blocks_per_bucket=None,
                 gaps=True):
    """body: 0 = xt_grad.h, 3 / 4 = xt_gradr.h with that many directions per pass.  buckets: arrays [N, L, D] in LAUNCH order; row r of the
    returned scores is track r of the concatenated buckets.  le / sigmas / slope_offset as run_emul_gap.run_gap.
    Returns (per bucket LL [N], sum LL, gradient [n_dir], scores [sum N, n_dir])."""
    f64 = lambda x: np.ascontiguousarray(x, dtype=np.float64)
    buckets = [f64(b) for b in buckets]
    S, D = len(ds), buckets[0].shape[2]
    nb = len(buckets)
    mode = 0 if sigmas is None else (2 if slope_offset is not None else 1)
    sig = [f64(s) for s in sigmas] if sigmas is not None else []
    KS = sig[0].shape[2] if sig else 0
    lev = np.zeros(3)
    v = np.atleast_1d(np.asarray(le, float)).ravel()
    lev[:len(v)] = v
    slope, offset = slope_offset if slope_offset is not None else (0.0, 0.0)
    ptrs = (C.c_void_p * nb)(*[b.ctypes.data for b in buckets])
    sptrs = (C.c_void_p * nb)(*[(s.ctypes.data if sig else None) for s in (sig or [None] * nb)])
    Ns = (C.c_longlong * nb)(*[len(b) for b in buckets])
    Ls = (C.c_int * nb)(*[b.shape[1] for b in buckets])
    r0 = np.concatenate([[0], np.cumsum([len(b) for b in buckets])])
    row0 = (C.c_longlong * nb)(*[int(x) for x in r0[:-1]])
    bpb = (C.c_int * nb)(*(blocks_per_bucket or [2] * nb))
    ll = [np.full(len(b), -12345.0) for b in buckets]
    llp = (C.c_void_p * nb)(*[x.ctypes.data for x in ll])
    rows = f64(pack_tangents(tangents, S))
    n_dir = len(rows)
    scores = np.full((int(r0[-1]), n_dir), -12345.0)
    out = np.zeros(1 + n_dir)
    keep = [f64(ds), f64(Fs), f64(T), f64(p_stay)]
    rc = lib().xt_emul_grad_gap(int(body), 1 if gaps else 0, nb, ptrs, sptrs, Ns, Ls, row0, D, KS, S, int(F), int(max_len), int(min_len), mode, len(v),
                                lev.ctypes.data_as(C.c_void_p), C.c_double(slope), C.c_double(offset), C.c_double(pBL),
                                *[k.ctypes.data_as(C.c_void_p) for k in keep], n_dir, rows.ctypes.data_as(C.c_void_p), bpb, llp,
                                scores.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise RuntimeError("xt_emul_grad_gap failed: %d" % rc)
    return ll, out[0], out[1:].copy(), scores
