"""ctypes driver for tests/emul/libxt_emul_hist_gap.so (test infrastructure): the state-duration histogram body (xt_hist.h) with GAPS = true
(or, ``gaps=False``, the plain body) on CPU threads (emul_hist_gap.cpp), one bucket per emulated launch."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "libxt_emul_hist_gap.so")
        csrc = os.path.join(HERE, "..", "..", "extrack_amd", "csrc")
        deps = [os.path.join(HERE, u) for u in ("emul_hist_gap.cpp", "emul_ctx.h")] + [os.path.join(csrc, h) for h in os.listdir(csrc) if h.endswith(".h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            import subprocess
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-pthread", "-shared", os.path.join(HERE, "emul_hist_gap.cpp"), "-o", so])
        _lib = C.CDLL(so)
    return _lib


def dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def run_hist(Cs, LE, ds, Fs, T, pBL, isBL, p_stay, min_l, max_nb_states, nblocks=1, threads=64, par_lds=1, slope_offset=None, gaps=True):
    """Cs [N, L, D] (all-NaN rows: missed frames).  LE: global localisation error [1, 1, 1 | D], or per-peak errors [N, L, 1 | D] (NaN allowed
    at the gap rows; ``slope_offset`` selects the affine mode).  Returns hist[L - 1, S] summed over the tracks."""
    Cs = np.ascontiguousarray(Cs, float)
    N, L, D = Cs.shape
    S = len(ds)
    LE = np.asarray(LE, float)
    if LE.shape[1] == 1 and L != 1:
        mode, K, KS = 0, LE.shape[2], 1
        locerr = np.zeros(3)
        locerr[:K] = LE[0, 0]
        sigma = None
    else:
        mode, KS = (2 if slope_offset is not None else 1), LE.shape[2]
        K, locerr, sigma = KS, np.zeros(3), np.ascontiguousarray(np.broadcast_to(LE, (N, L, LE.shape[2])))
    slope, offset = slope_offset if slope_offset is not None else (0.0, 0.0)
    out = np.zeros((L - 1, S))
    ds, Fs, T, p_stay = [np.ascontiguousarray(x, float) for x in (ds, Fs, T, p_stay)]
    rc = lib().xt_emul_hist_gap(dp(Cs), dp(sigma), C.c_longlong(N), L, D, KS, S, int(isBL), int(min_l), mode, K, dp(locerr), C.c_double(slope),
                                C.c_double(offset), C.c_double(pBL), dp(ds), dp(Fs), dp(T), dp(p_stay), int(max_nb_states), int(nblocks), int(threads),
                                1 if par_lds else 0, 1 if gaps else 0, dp(out))
    if rc != 0:
        raise RuntimeError("xt_emul_hist_gap failed: %d" % rc)
    return out
