"""ctypes driver for tests/emul/libxt_emul_rev_gap.so (test infrastructure): the reverse-mode gradient body (xt_rev.h) with and without its GAPS
flag on CPU threads (emul_rev_gap.cpp), several length buckets per emulated launch through the bucket-descriptor table, and the launcher's
decisions of a gapped launch group (xt_grad_pick -> xt_grad_gap_reg2 -> xt_grad_gap_rev)."""
import ctypes as C
import os

import numpy as np

from run_emul_grad_gap import pack_tangents

HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None
PATHS = ("none", "rev", "reg2", "gradr", "lds", "gaps_reg2", "gaps_rev")  # XtGradPath
FIELDS = ("path", "refusal", "tpb", "threads", "lds", "nbuf", "max_blocks", "log_stride", "NPC")
GEOMETRY = ("tpb", "threads", "lds", "nbuf", "max_blocks", "log_stride")  # what an upgraded pick takes from its gap-free twin


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(HERE, "libxt_emul_rev_gap.so")
        csrc = os.path.join(HERE, "..", "..", "extrack_amd", "csrc")
        deps = [os.path.join(HERE, u) for u in ("emul_rev_gap.cpp", "emul_ctx.h")] + [os.path.join(csrc, h) for h in os.listdir(csrc) if h.endswith(".h")]
        if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
            import subprocess
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-pthread", "-shared", os.path.join(HERE, "emul_rev_gap.cpp"), "-o", so])
        _lib = C.CDLL(so)
    return _lib


def run_rev_gap(nbuf, buckets, le, ds, Fs, T, pBL, p_stay, F, min_len, max_len, tangents, sigmas=None, slope_offset=None, blocks_per_bucket=None,
                gaps=True):
    """nbuf: exchange buffers per track (1 | 2).  buckets: arrays [N, L, D] in LAUNCH order (longest first).  le / sigmas / slope_offset as
    run_emul_gap.run_gap.  Returns (per bucket LL [N], sum LL, gradient [n_dir])."""
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
    ll = [np.full(len(b), -12345.0) for b in buckets]
    llp = (C.c_void_p * nb)(*[x.ctypes.data for x in ll])
    rows = f64(pack_tangents(tangents, S))
    n_dir = len(rows)
    out = np.zeros(1 + n_dir)
    keep = [f64(ds), f64(Fs), f64(T), f64(p_stay)]
    rc = lib().xt_emul_rev_gap(int(nbuf), 1 if gaps else 0, nb, ptrs, sptrs, Ns, Ls, D, KS, S, int(F), int(max_len), int(min_len), mode, len(v),
                               lev.ctypes.data_as(C.c_void_p), C.c_double(slope), C.c_double(offset), C.c_double(pBL),
                               *[k.ctypes.data_as(C.c_void_p) for k in keep], n_dir, rows.ctypes.data_as(C.c_void_p), bpb, llp,
                               out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise RuntimeError("xt_emul_rev_gap failed: %d" % rc)
    return ll, out[0], out[1:].copy()


def decide(S=3, NS=1, F=5, D=2, K=1, locerr_mode=0, n_dir=13, Lmax=30, nbuckets=1, n_cu=256, gaps=1, scores=0, grad_reg2=1, grad_rev=1,
           rev_log_mb=16384, fmask=0xe0):
    """The picks of a launch group as dicts of FIELDS (path as text): (xt_grad_pick, after xt_grad_gap_reg2, after xt_grad_gap_rev, xt_grad_pick of
    the gap-free twin), or None where xt_build_config refuses the model."""
    out = (C.c_longlong * 36)()
    inp = (C.c_longlong * 16)(S, NS, F, D, K, locerr_mode, n_dir, Lmax, nbuckets, n_cu, gaps, scores, grad_reg2, grad_rev, rev_log_mb, fmask)
    if lib().xt_emul_grad_gap_rev(inp, out) != 0:
        return None
    o = list(out)
    picks = [dict(zip(FIELDS, o[i * 9:i * 9 + 9])) for i in range(4)]
    for p in picks:
        p["path"] = PATHS[p["path"]]
    return tuple(picks)
