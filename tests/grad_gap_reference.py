"""TEST INFRASTRUCTURE: the reference of the gap-aware gradient and per-track scores: two Richardson levels (h and h / 2,
``test_grad_cpu._richardson``) of central differences of ``gap_reference.loglik_and_preds`` - the unchanged numpy oracle - along the directions
and steps of ``test_grad_cpu.model_directions``.  Not a conftest; imported by tests/test_emul_grad_gaps.py and tests/test_hip_grad_gaps.py.

Metric: ``test_grad_edges_cpu.check_gradient``, per direction |g - fd| <= 1e-6 |fd| + est with est = |level(h / 2) - level(h)|.  So that est
cannot hide a failure, ``assert_condition`` demands est <= 1e-6 |fd| of every tested figure whose |fd| is not exactly 0.

The sum over tracks meets the condition along every direction (measured: est / |fd| <= 2.2e-8 over the cases of the tests).  A single track's
score can sit next to a zero crossing, where the rounding of the differenced oracle - an ABSOLUTE error set by |LL| and the step, so about
the same for all tracks of a bucket along one direction - is no longer 1e-6 of it; one track's own est can also be 0 by coincidence of the two
levels while its neighbours show 2e-9.  ``score_mask`` therefore keeps a score only where max(est, median of est over the bucket's tracks along
that direction) <= 1e-6 |fd|: a rule that looks at the reference alone.  It drops 5 of 5184 scores of the CPU cases (le0 of one L = 14 track
with globalD errors; slope and offset of one L = 40 track with affine errors; ds2_0 of one L = 14 and one L = 40 track); the tests print what
it drops and refuse a mask that drops more than 0.5 %.  Dropped scores stay in the sum-gradient check."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # run as a script (regenerating the golden file): the repository root is not on the path yet
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import gap_reference as R  # noqa: E402
from test_grad_cpu import _richardson, model_directions  # noqa: E402

H_SLOPE, H_OFFSET = 1e-4, 1e-6  # the steps of test_grad_cpu's per-peak test


def case_model(case):
    Ds, Tm, Fs = R.MODELS[case["S"]]
    return 2 * Ds * R.DT, np.array(Tm, float), np.array(Fs, float)


def directions(case):
    """[(name, tangent dict for the kernels, perturbation dict for the reference, step)]: every model direction of ``model_directions``; the
    per-peak layouts have no global error (no le direction), the affine one adds slope and offset."""
    ds2, T, _ = case_model(case)
    le = np.array(case["le"] if case["le"] is not None else [0.02], float)
    dirs = model_directions(case["S"], len(le), 1, ds2, T, le, R.CELL)
    if case["sig"] is not None:
        dirs = [d for d in dirs if not d[0].startswith("le")]
        if case["slope_offset"] is not None:
            dirs += [("slope", dict(slope=1.0), dict(slope=1.0), H_SLOPE), ("offset", dict(offset=1.0), dict(offset=1.0), H_OFFSET)]
    return dirs


def _ll(case, x, d):
    """Per-track LL of all buckets (upload order, concatenated) with the model displaced by x along the perturbation d."""
    ds2, T, Fs = case_model(case)
    Lmax = max(b.shape[1] for b in case["buckets"])
    out = []
    for i, b in enumerate(case["buckets"]):
        if case["sig"] is None:
            eff = (np.array(case["le"], float) + x * d.get("le", 0.0))[None, None]
        elif case["slope_offset"] is None:
            eff = case["sig"][i]
        else:
            eff = np.maximum(case["sig"][i] * (case["slope_offset"][0] + x * d.get("slope", 0.0)) + case["slope_offset"][1] + x * d.get("offset", 0.0), 1e-6)
        ll, _ = R.loglik_and_preds(b, eff, np.sqrt(ds2 + x * d.get("ds2", 0.0)), Fs + x * d.get("Fs", 0.0), T + x * d.get("T", 0.0),
                                   R.PBL + x * d.get("pBL", 0.0), int(b.shape[1] != Lmax), R.CELL, case["F"], R.MIN_LEN)
        out.append(ll)
    return np.concatenate(out)


_cache = {}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grad_gap_reference.npz")
# the cases of the CPU and the GPU test: (S, D, layout, frame_len) of gap_reference.make_case - every state count at frame_len 3, 2 and 3 states at
# frame_len 5 (up to 81 groups: more than one wavefront per track); every (D, K) pair - (1,1) (2,2) (3,1) (3,3) (2,1) - and every error layout
CASES = [(2, 1, "global1", 3), (3, 2, "globalD", 3), (4, 3, "affine", 3), (2, 3, "peak", 5), (3, 2, "global1", 5)]


def lds_case():
    """2 states at frame_len 10 (512 groups of sequences per track: beyond the 256 of xt_gradr.h, so the LDS-resident body: one track per 512-thread
    workgroup, one direction per pass), L = 14, N = 5: a gap at t = 1, at t = L - 2, a run of 8, every interior row, none.
    (4 states at frame_len 6 - 1024 groups - cannot take this path: 4^6 sequences x (1 + D + K) doubles are 128 KiB per primal region and
    xt_grad.h holds two of them plus one more per direction, against 160 KiB of LDS; that model is refused, see the refusal test.)"""
    from extrack_amd import synth
    Ds, Tm, Fs = R.MODELS[2]
    m = np.zeros((5, 14), bool)
    m[0, 1] = m[1, 12] = True
    m[2, 3:11] = True
    m[3, 1:-1] = True
    tr = synth.brownian_tracks(5, 14, list(Ds), Tm.tolist(), list(Fs), LocErr=0.02, dt=R.DT, dims=2, seed=77)
    tr[m] = np.nan
    return dict(S=2, D=2, F=10, layout="global1", buckets=[tr], masks=[m], sig=None, le=[0.02], slope_offset=None, eff=[np.array([[[0.02]]])])


def _key(key):
    return "_".join(str(k) for k in key) if isinstance(key, tuple) else str(key)


def reference(case, key, golden=False):
    """dict(ll [sum N], dirs, fd / est [sum N, n_dir] per-track scores, gfd / gest [n_dir] of the sum over tracks), computed once per key.
    ``golden``: read the arrays from tests/golden/grad_gap_reference.npz (written by running this file; the CPU test recomputes them and checks
    that the file is current) - the GPU tests then spend no time in the oracle."""
    if golden:
        with np.load(GOLDEN) as z:
            ref = {k: z[_key(key) + "." + k] for k in ("ll", "fd", "est", "gfd", "gest")}
        ref["dirs"] = directions(case)
        return ref
    if key not in _cache:
        dirs = directions(case)
        lv = []
        for hs in (1.0, 0.5):
            lv.append(np.stack([_richardson(lambda x: _ll(case, x, d), h * hs) for _, _, d, h in dirs], axis=1))
        fd, est = lv[1], np.abs(lv[1] - lv[0])
        gl = [l.sum(axis=0) for l in lv]
        ref = dict(ll=_ll(case, 0.0, {}), dirs=dirs, fd=fd, est=est, gfd=gl[1], gest=np.abs(gl[1] - gl[0]))
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[key] = ref
    return _cache[key]


def assert_condition(tag, fd, est):
    """est <= 1e-6 |fd| wherever |fd| is not exactly 0: the error estimate must not be what lets a wrong gradient pass."""
    nz = fd != 0
    worst = float((est[nz] / np.abs(fd[nz])).max()) if nz.any() else 0.0
    print("%s: reference alone, worst est / |fd| = %.3g" % (tag, worst))
    assert worst <= 1e-6, (tag, worst)


def score_mask(tag, case, ref):
    """bool [sum N, n_dir]: the per-track scores whose reference is good enough to test against (see the module docstring)."""
    fd, est = ref["fd"], ref["est"]
    floor, r0 = np.zeros_like(est), 0
    for b in case["buckets"]:
        floor[r0:r0 + len(b)] = np.median(est[r0:r0 + len(b)], axis=0)[None]
        r0 += len(b)
    keep = (fd == 0) | (np.maximum(est, floor) <= 1e-6 * np.abs(fd))
    for n, j in zip(*np.nonzero(~keep)):
        print("%s: score dropped, %s of track %d: fd %.3g, est %.3g, bucket median of est %.3g" % (tag, ref["dirs"][j][0], n, fd[n, j], est[n, j], floor[n, j]))
    assert (~keep).sum() <= 0.005 * keep.size, (tag, int((~keep).sum()), keep.size)
    return keep


def assert_golden_is_current(case, key, ref):
    """The stored arrays against freshly computed ones: the same inputs (LL to 1e-12) and the same differences up to their own error estimates."""
    gold = reference(case, key, golden=True)
    np.testing.assert_allclose(gold["ll"], ref["ll"], rtol=1e-12, atol=1e-10)
    for a, e in (("fd", "est"), ("gfd", "gest")):
        assert np.all(np.abs(gold[a] - ref[a]) <= 2 * (gold[e] + ref[e]) + 1e-7 * np.abs(ref[a])), (key, a)


if __name__ == "__main__":  # regenerate the golden file
    out = {}
    for key, case in [(c, R.make_case(*c)) for c in CASES] + [("lds", lds_case())]:
        ref = reference(case, key)
        for k in ("ll", "fd", "est", "gfd", "gest"):
            out[_key(key) + "." + k] = ref[k]
    np.savez_compressed(GOLDEN, **out)
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
