"""ctypes driver for tests/emul/libxt_emul_map_gap.so (test infrastructure): the state-path decoder body (xt_map.h) with GAPS = true (or,
``gaps=False``, the plain body) on CPU threads (emul_map_gap.cpp), several length buckets per emulated launch through the
bucket-descriptor table."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "libxt_emul_map_gap.so")
        csrc = os.path.join(HERE, "..", "..", "extrack_amd", "csrc")
        deps = [os.path.join(HERE, u) for u in ("emul_map_gap.cpp", "emul_ctx.h")] + [os.path.join(csrc, h) for h in os.listdir(csrc) if h.endswith(".h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            import subprocess
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-pthread", "-shared", os.path.join(HERE, "emul_map_gap.cpp"), "-o", so])
        _lib = C.CDLL(so)
    return _lib


def run_map(buckets, le, ds, Fs, T, pBL, p_stay, F, min_len, max_len, sigmas=None, slope_offset=None, blocks_per_bucket=None, tpb=2,
            bp_global=False, gaps=True):
    """buckets: arrays [N, L, D] in LAUNCH order.  le: global localisation error (1 or D values), ignored with ``sigmas`` (per-peak errors
    [N, L, 1 | D] per bucket; ``slope_offset`` selects the affine mode).  Returns [(states int8 [N, L], score [N])] in the same order."""
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
    bpb = (C.c_int * nb)(*(blocks_per_bucket or [2] * nb))
    states = [np.full(b.shape[:2], 99, dtype=np.int8) for b in buckets]
    scores = [np.full(len(b), -12345.0) for b in buckets]
    st = (C.c_void_p * nb)(*[s.ctypes.data for s in states])
    sc = (C.c_void_p * nb)(*[s.ctypes.data for s in scores])
    keep = [f64(ds), f64(Fs), f64(T), f64(p_stay)]
    rc = lib().xt_emul_map_gap(nb, ptrs, sptrs, Ns, Ls, D, KS, S, int(F), int(max_len), int(min_len), mode, len(v), lev.ctypes.data_as(C.c_void_p),
                           C.c_double(slope), C.c_double(offset), C.c_double(pBL), *[k.ctypes.data_as(C.c_void_p) for k in keep], bpb, int(tpb),
                           1 if bp_global else 0, 1 if gaps else 0, st, sc)
    if rc != 0:
        raise RuntimeError("xt_emul_map_gap failed: %d" % rc)
    return list(zip(states, scores))
