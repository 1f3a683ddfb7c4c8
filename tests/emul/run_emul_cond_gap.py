"""ctypes driver for tests/emul/libxt_emul_cond_gap.so (test infrastructure): the fixed-state smoother body (xt_cond.h) with GAPS = true
(or, ``gaps=False``, the plain body) on CPU threads (emul_cond_gap.cpp), one bucket per emulated launch."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "libxt_emul_cond_gap.so")
        csrc = os.path.join(HERE, "..", "..", "extrack_amd", "csrc")
        deps = [os.path.join(HERE, u) for u in ("emul_cond_gap.cpp", "emul_ctx.h")] + [os.path.join(csrc, h) for h in os.listdir(csrc) if h.endswith(".h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            import subprocess
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-pthread", "-shared", os.path.join(HERE, "emul_cond_gap.cpp"), "-o", so])
        _lib = C.CDLL(so)
    return _lib


def run_cond(Cs, states, le, ds, sigma=None, slope_offset=None, nblocks=2, tpb=64, ws_global=False, logdens=True, gaps=True):
    """Cs [N, L, D]; states int8 [N, L]; le: global localisation error (1 or D values), ignored with ``sigma`` (per-peak errors
    [N, L, 1 | D]; ``slope_offset`` selects the affine mode); ds: diffusion lengths [S].  Returns (mu [N, L, D], sigma [N, L, K],
    logdens [N] or None)."""
    f64 = lambda x: np.ascontiguousarray(x, dtype=np.float64)
    Cs = f64(Cs)
    states = np.ascontiguousarray(states, dtype=np.int8)
    N, L, D = Cs.shape
    S = len(ds)
    mode = 0 if sigma is None else (2 if slope_offset is not None else 1)
    sig = f64(sigma) if sigma is not None else None
    KS = sig.shape[2] if sig is not None else 0
    lev = np.zeros(3)
    v = np.atleast_1d(np.asarray(le, float)).ravel()
    lev[:len(v)] = v
    K = len(v) if mode == 0 else KS
    slope, offset = slope_offset if slope_offset is not None else (0.0, 0.0)
    mu = np.full((N, L, D), -12345.0)
    so = np.full((N, L, K), -12345.0)
    ld = np.full(N, -12345.0) if logdens else None
    # the tables the smoother does not read (TrMat, Fs, p_stay) still go through the library's table builder
    keep = [f64(ds), f64(np.full(S, 1.0 / S)), f64(np.full((S, S), 1.0 / S)), f64(np.ones(S))]
    vp = lambda x: x.ctypes.data_as(C.c_void_p) if x is not None else None
    rc = lib().xt_emul_cond_gap(vp(Cs), vp(sig), vp(states), C.c_longlong(N), L, D, KS, S, mode, len(v), vp(lev), C.c_double(slope), C.c_double(offset),
                            *[vp(k) for k in keep], int(nblocks), int(tpb), 1 if ws_global else 0, 1 if gaps else 0, vp(mu), vp(so), vp(ld))
    if rc != 0:
        raise RuntimeError("xt_emul_cond_gap failed: %d" % rc)
    return mu, so, ld
