"""TEST INFRASTRUCTURE: the cases of the gap-aware register-resident 2-state gradient kernels and their stored reference.
The reference itself is ``grad_gap_reference.reference`` (unchanged: Richardson differences of the numpy oracle); this module only names the four
cases, keeps their arrays in a file of their own - tests/golden/r2_grad_gap_reference.npz, same array names as grad_gap_reference.npz, written by
running this file - and drives the CPU emulation of the body (tests/emul/emul_r2_grad_gap.cpp, one library per frame_len).  Not a conftest; imported
by tests/test_emul_r2_grad_gaps.py, tests/test_grad_gap_reg2_cpu.py and tests/test_hip_reg2_grad_gaps.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "emul"))
if __name__ == "__main__":  # run as a script (regenerating the golden file): the repository root is not on the path yet
    sys.path.insert(0, os.path.dirname(HERE))

import gap_reference as R  # noqa: E402
import grad_gap_reference as GR  # noqa: E402
from oracle import oracle_np as O  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "r2_grad_gap_reference.npz")
# (D, frame_len): two states, one global localisation error.  Each: buckets L = 2, 3, F + 1, 14, 40 (gap_reference.gap_masks) and 10 directions -
# ds2 x 2, F x 2, T x 4, le0, pBL - i.e. two passes of full directions plus the uniform pBL, and a 40-row track across the 32-row staging chunk
CASES = [(1, 4), (2, 5), (2, 6), (3, 7)]
GAPS_REG2, REG2, GRADR, LDS = 5, 2, 3, 4  # XtGradPath
F_DEFAULT, F_ALL = 0xe0, 0xf0  # frame lengths a context upgrades (bit F): by default 5, 6, 7; frame_len 4 on request (EXTRACK_GAP_REG2_F)


def key(D, F):
    return (2, D, "global1", F)


def make(D, F):
    return R.make_case(2, D, "global1", F)


def golden(case, k):
    """``grad_gap_reference.reference(case, k, golden=True)`` from this module's file."""
    with np.load(GOLDEN) as z:
        ref = {a: z[GR._key(k) + "." + a] for a in ("ll", "fd", "est", "gfd", "gest")}
    ref["dirs"] = GR.directions(case)
    return ref


def assert_golden_is_current(case, k, ref):
    """``grad_gap_reference.assert_golden_is_current`` for this module's file: same inputs (LL to 1e-12), same differences up to their own estimates."""
    gold = golden(case, k)
    np.testing.assert_allclose(gold["ll"], ref["ll"], rtol=1e-12, atol=1e-10)
    for a, e in (("fd", "est"), ("gfd", "gest")):
        assert np.all(np.abs(gold[a] - ref[a]) <= 2 * (gold[e] + ref[e]) + 1e-7 * np.abs(ref[a])), (k, a)


def simple_case(buckets, D, F):
    """A case dict as ``gap_reference.make_case`` builds it (what ``grad_gap_reference.directions`` and ``test_emul_grad_gaps.emulate`` read) around
    given buckets [N, L, D], short -> long."""
    return dict(S=2, D=D, F=F, layout="global1", buckets=list(buckets), masks=[np.isnan(b).all(axis=2) for b in buckets], sig=None, le=[0.02],
                slope_offset=None, eff=[np.array([[[0.02]]])] * len(buckets))


# ---- CPU emulation of xt_r2_body<.., NP > 0, .., GAPS> under the product's decisions
_libs = {}
DIMS = {4: 1, 5: 2, 6: 2, 7: 3}  # the track dimensionality each library is built for


def lib(F):
    """tests/emul/emul_r2_grad_gap.cpp -DXT_EMUL_F=F -> tests/emul/libxt_emul_r2_grad_gap_f<F>.so (rebuilt when a source it includes is newer)."""
    if F not in _libs:
        emul = os.path.join(HERE, "emul")
        csrc = os.path.join(HERE, "..", "extrack_amd", "csrc")
        so, src = os.path.join(emul, "libxt_emul_r2_grad_gap_f%d.so" % F), os.path.join(emul, "emul_r2_grad_gap.cpp")
        deps = [src, os.path.join(emul, "emul_ctx.h")] + [os.path.join(csrc, h) for h in os.listdir(csrc) if h.endswith(".h")]
        if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in deps):
            subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-pthread", "-shared", "-DXT_EMUL_F=%d" % F, src, "-o", so])
        _libs[F] = C.CDLL(so)
        assert _libs[F].xt_emul_r2gg_frame_len() == F and _libs[F].xt_emul_r2gg_dims() == DIMS[F]
    return _libs[F]


def emulate(case, dirs, gaps=True, buckets=None, maxnp=8, grad_reg2=1, fmask=None, guarded=False, blocks=2, le=0.02, ds=None, fill=np.nan):
    """(LL [sum N], sum LL, gradient, scores [sum N, n_dir], info) in upload order (short -> long); launched longest first, all buckets in one
    emulated launch group.  info = [path, lazy variant, tracks per block, threads, passes, LDS bytes of the first pass]; the body has run only where
    info[0] is GAPS_REG2 (gaps) / REG2 (gaps=False: the plain body), else LL and scores come back as None.  fill: what the staging leaves in LDS in
    place of a NaN coordinate (the product: the NaN itself); the rows are classified from the input either way."""
    import run_emul_grad_gap as E
    F = case["F"]
    Ds, Tm, Fs = R.MODELS[2]
    ds = np.sqrt(2 * Ds * R.DT) if ds is None else np.asarray(ds, float)
    bk = case["buckets"] if buckets is None else buckets
    order = list(range(len(bk)))[::-1]
    f64 = lambda x: np.ascontiguousarray(x, dtype=np.float64)
    lb = [f64(bk[i]) for i in order]
    nb, D = len(lb), lb[0].shape[2]
    fmask = (F_DEFAULT if (F_DEFAULT >> F) & 1 else F_ALL) if fmask is None else fmask
    rows = f64(E.pack_tangents([d[1] for d in dirs], 2))
    n_dir = len(rows)
    r0 = np.concatenate([[0], np.cumsum([len(b) for b in lb])])
    ll = [np.full(len(b), -12345.0) for b in lb]
    scores = np.full((int(r0[-1]), n_dir), -12345.0)
    out, info = np.zeros(1 + n_dir), (C.c_int * 6)()
    keep = [f64(ds), f64(Fs), f64(Tm), f64(O.p_stay_table(ds, 2, 1, R.CELL))]
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    lib(F).xt_emul_r2gg_set_fill(C.c_double(fill))
    rc = lib(F).xt_emul_r2_grad_gap(
        1 if gaps else 0, nb, (C.c_void_p * nb)(*[b.ctypes.data for b in lb]), (C.c_longlong * nb)(*[len(b) for b in lb]),
        (C.c_int * nb)(*[b.shape[1] for b in lb]), (C.c_longlong * nb)(*[int(x) for x in r0[:-1]]), D, max(b.shape[1] for b in lb), R.MIN_LEN,
        C.c_double(le), C.c_double(R.PBL), *[vp(k) for k in keep], n_dir, vp(rows), (C.c_int * nb)(*([blocks] * nb)),
        (C.c_int * 4)(int(grad_reg2), int(maxnp), int(fmask), 1 if guarded else 0), (C.c_void_p * nb)(*[x.ctypes.data for x in ll]), vp(scores), vp(out), info)
    lib(F).xt_emul_r2gg_set_fill(C.c_double(np.nan))
    info = list(info)
    if rc == 1:
        return None, None, None, None, info
    assert rc == 0, rc
    lls, scs = [None] * nb, [None] * nb
    for j, i in enumerate(order):
        lls[i], scs[i] = ll[j], scores[r0[j]:r0[j + 1]]
    return np.concatenate(lls), out[0], out[1:].copy(), np.concatenate(scs), info


if __name__ == "__main__":  # regenerate the golden file
    out = {}
    for D, F in CASES:
        ref = GR.reference(make(D, F), key(D, F))
        GR.assert_condition("D %d frame_len %d" % (D, F), ref["gfd"], ref["gest"])
        for a in ("ll", "fd", "est", "gfd", "gest"):
            out[GR._key(key(D, F)) + "." + a] = ref[a]
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
