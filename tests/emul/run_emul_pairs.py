"""ctypes driver for tests/emul/libxt_emul_pairs.so (test infrastructure): the PAIRS instantiations of the fixed-window body (xt_kernel.h) on
CPU threads (emul_pairs.cpp), several length buckets per emulated launch through the bucket-descriptor table, and the pair launch's geometry
function (xt_pair_geom.h)."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
PICK_FIELDS = ("refusal", "tpb", "threads", "lds", "wide", "sel", "pred_lds_same_tpb", "gap_path", "gap_tpb", "gap_threads", "gap_lds", "pred_path")


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "libxt_emul_pairs.so")
        csrc = os.path.join(HERE, "..", "..", "extrack_amd", "csrc")
        deps = [os.path.join(HERE, u) for u in ("emul_pairs.cpp", "emul_ctx.h")] + [os.path.join(csrc, h) for h in os.listdir(csrc) if h.endswith(".h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            import subprocess
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-pthread", "-shared", os.path.join(HERE, "emul_pairs.cpp"), "-o", so])
        _lib = C.CDLL(so)
        _lib.xt_emul_pair_refusal_text.restype = C.c_char_p
    return _lib


def pair_pick(S, NS, F, D, K, n_cu=256):
    """xt_pair_pick beside xt_ll_pick for posteriors at the same point: dict of PICK_FIELDS, or None where xt_build_config refuses."""
    out = (C.c_longlong * 12)()
    if lib().xt_emul_pair_pick(int(S), int(NS), int(F), int(D), int(K), int(n_cu), out) != 0:
        return None
    return dict(zip(PICK_FIELDS, list(out)))


def refusal_text(r):
    return lib().xt_emul_pair_refusal_text(int(r)).decode()


def run_pairs(buckets, le, ds, Fs, T, pBL, p_stay, F, min_len, max_len, sigmas=None, slope_offset=None, blocks_per_bucket=None, gaps=True,
              tpb=0, pairs=True, counts=True):
    """buckets: arrays [N, L, D] in LAUNCH order.  le: global localisation error (1 or D values), ignored with ``sigmas`` (per-peak errors
    [N, L, 1 | D] per bucket; ``slope_offset`` selects the affine mode).  Returns (per bucket: pairs [N, L-1, S, S] or None; per bucket:
    counts [N, S, S] or None; launch info)."""
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
    pr = [np.full((len(b), b.shape[1] - 1, S, S), -12345.0) for b in buckets]
    ct = [np.full((len(b), S, S), -12345.0) for b in buckets]
    prp = (C.c_void_p * nb)(*[(x.ctypes.data if pairs else None) for x in pr])
    ctp = (C.c_void_p * nb)(*[(x.ctypes.data if counts else None) for x in ct])
    keep = [f64(ds), f64(Fs), f64(T), f64(p_stay)]
    info = (C.c_int * 3)()
    rc = lib().xt_emul_pairs(nb, ptrs, sptrs, Ns, Ls, D, KS, S, int(F), int(max_len), int(min_len), mode, len(v), lev.ctypes.data_as(C.c_void_p),
                             C.c_double(slope), C.c_double(offset), C.c_double(pBL), *[k.ctypes.data_as(C.c_void_p) for k in keep], bpb,
                             1 if gaps else 0, int(tpb), prp, ctp, info)
    if rc != 0:
        raise RuntimeError("xt_emul_pairs failed: %d" % rc)
    return (pr if pairs else None), (ct if counts else None), list(info)
