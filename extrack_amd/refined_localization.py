"""Drop-in replacement for ``extrack.refined_localization.position_refinement`` (extrack/refined_localization.py:304-338).

Same name, arguments and result as the reference; the two threshold-fusion passes (get_LC_Km_Ks, :48-204) and the combination of the
predictions from the future and from the past (get_pos_PDF, :207-298) run in HIP kernels through ``extrack_refine_positions`` of the
C ABI.  Built for what the reference's own array reshapes carry through: ONE global localisation error (a float or a 1-element array)
or a dict of per-peak errors ``{len: sigma[n_tracks, len, 1]}``, nb_substeps = 1.  Per-peak errors are used exactly as the reference uses
them - it reverses the error array but not the track in get_LC_Km_Ks (refined_localization.py:64-65 vs :115), so its pass "from the
future" pairs every position with its mirror image's error; that pairing is reproduced (pinned by 50 reference-generated buckets,
tests/golden/refine_pp_cases.*), per-dimension errors and ``[n, len, dims]`` dicts are refused as the reference's reshapes refuse them.
Like the reference, every length bucket is processed as one chunk: its first 30 tracks decide which state sequences are merged.

``get_pos_PDF_fixedBs`` and ``refine_along_states`` answer the other question - where the particle was GIVEN one state per position (the
output of ``tracking.predict_states``) - through ``extrack_refine_fixed_states``: one forward and one backward sweep per track, any number
of states, global, per-dimension or per-peak errors."""
import numpy as np

from . import engine
from .engine import TrackSet
from .lmfit_compat import is_parameters

__all__ = ["position_refinement", "get_pos_PDF", "get_pos_PDF_fixedBs", "refine_along_states"]


def position_refinement(all_tracks, LocErr, ds, Fs, TrMat, frame_len=7, threshold=0.1, max_nb_states=1000, device=0):
    """all_tracks: {str(len): ndarray[n_tracks, len, dims]}; LocErr: localisation error (std); ds: diffusion lengths sqrt(2 D dt);
    Fs: initial fractions; TrMat: per-step transition probabilities.  Returns ({len: refined positions [n, len, dims]},
    {len: refined stds [n, len]})."""
    per_peak = isinstance(LocErr, dict)
    if not per_peak:
        le = np.atleast_1d(np.asarray(LocErr, dtype=np.float64)).ravel()
        if len(le) != 1:
            raise ValueError("position refinement takes one global localisation error (float) or a dict of per-peak errors "
                             "{len: [n_tracks, len, 1]} (the reference's reshapes assume it, extrack/refined_localization.py:276)")
    print("LocErr_type", "dict" if per_peak else "array")
    ds, Fs, TrMat = np.asarray(ds, float), np.asarray(Fs, float), np.asarray(TrMat, float)
    S = len(ds)
    all_mus, all_sigmas = {}, {}
    for l, Cs in all_tracks.items():
        Cs = np.asarray(Cs, dtype=np.float64)
        if Cs.ndim != 3 or Cs.shape[1] != int(l):
            raise ValueError("all_tracks[%r] must be an array [n_tracks, %s, dims]" % (l, l))
        if len(Cs) == 0:
            all_mus[l], all_sigmas[l] = np.zeros((0, int(l), Cs.shape[2])), np.zeros((0, int(l)))
            continue
        sig = None
        if per_peak:
            sig = np.asarray(LocErr[l], dtype=np.float64)
            if sig.shape != (Cs.shape[0], Cs.shape[1], 1):
                raise ValueError("per-peak localisation errors must be arrays [n_tracks, len, 1] matching all_tracks[%r]" % l)
        ts = TrackSet([Cs], [sig] if per_peak else None, device=device)
        try:
            model = ts.make_model(None if per_peak else le[None, None], ds, Fs, TrMat, 0.0, [], 1, frame_len)
            all_mus[l], all_sigmas[l] = ts.ctx.refine_positions(model, 0, threshold, max_nb_states)
        finally:
            ts.close()
    return all_mus, all_sigmas


def get_pos_PDF(Cs, LocErr, ds, Fs, TrMat, frame_len=7, threshold=0.2, max_nb_states=1000, device=0):
    """Mirror of extrack/refined_localization.py:207-298 for one array of tracks ``Cs[n_tracks, len, dims]``: the Gaussian mixture that
    describes every position given all the others.  ``LocErr``: the 3-D array position_refinement hands over (``[[[error]]]`` or per-peak
    ``[n_tracks, len, 1]``) or a float.  Returns ``(all_pos_means, all_pos_stds, all_pos_weights)``: lists over the positions of
    ``[n_tracks, n_comp, dims]``, ``[n_tracks, n_comp, 1]``, ``[n_tracks, n_comp]`` (log-weights), components in the reference's order.
    Meant for inspection: every component of every track is copied to the host (position_refinement never materialises them)."""
    Cs = np.asarray(Cs, dtype=np.float64)
    if Cs.ndim != 3 or Cs.shape[1] < 2 or len(Cs) == 0:
        raise ValueError("Cs must be a non-empty array [n_tracks, len >= 2, dims]")
    le = np.asarray(LocErr, dtype=np.float64)
    per_peak = le.ndim == 3 and le.shape[1] == Cs.shape[1] and le.shape[1] > 1
    if per_peak:
        if le.shape != (Cs.shape[0], Cs.shape[1], 1):
            raise ValueError("per-peak localisation errors must be an array [n_tracks, len, 1] matching Cs")
    elif le.size != 1:
        raise ValueError("LocErr must be one global localisation error or per-peak errors [n_tracks, len, 1]")
    ts = TrackSet([Cs], [le] if per_peak else None, device=device)
    try:
        model = ts.make_model(None if per_peak else le.reshape(1, 1, 1), np.asarray(ds, float), np.asarray(Fs, float), np.asarray(TrMat, float), 0.0, [], 1,
                              frame_len)
        return ts.ctx.refine_pos_pdf(model, 0, threshold, max_nb_states)
    finally:
        ts.close()


def _squeeze_sigs(sg):
    """[n, len, K] -> [n, len] for one error channel, [n, len, dims] for one per dimension."""
    return sg[:, :, 0] if sg.shape[2] == 1 else sg


def _check_states(st, n, L, S, what):
    """int8 copy of an integer state array [n, len] with every entry < S (negative entries mark a track without a path)."""
    st = np.asarray(st)
    if not np.issubdtype(st.dtype, np.integer):
        raise TypeError("%s must be an integer array (int8, as predict_states returns it), not %s" % (what, st.dtype))
    if st.shape != (n, L):
        raise ValueError("%s must have shape (%d, %d), not %s" % (what, n, L, st.shape))
    if st.size and st.max() >= S:
        raise ValueError("%s holds state %d but the model has %d states" % (what, st.max(), S))
    return np.ascontiguousarray(np.maximum(st, -1), dtype=np.int8)


def get_pos_PDF_fixedBs(Cs, LocErr, ds, Fs, TrMat, Bs, device=0):
    """Posterior mean and standard deviation of every real position of the tracks ``Cs[n_tracks, len, dims]`` GIVEN the state of every
    position ``Bs`` (integers, ``[n_tracks, len]`` or the reference's ``[n_tracks, 1, len]``): the quantity
    extrack/refined_localization.py:483-519 (with get_LC_Km_Ks_fixed_Bs, :414-481) was written to compute, with its name and argument
    order.  ``LocErr``: a float, one value per dimension, or per-peak errors ``[n_tracks, len, 1 | dims]``.  Returns
    ``(mus [n_tracks, len, dims], sigs [n_tracks, len])``, ``sigs [n_tracks, len, dims]`` with per-dimension errors.  A track with a NaN
    position or error, or with a negative state, is NaN in both.

    The model: flat prior on the first real position, real steps N(0, (ds[b[t]]^2 + ds[b[t+1]]^2) / 2) - the likelihood's step variance -
    and observations N(real position, LocErr^2), independently per dimension; ``Fs`` and ``TrMat`` are checked for shape and otherwise
    unused (given the path they do not move the positions).  The numbers are NOT the reference's, whose function is inconsistent as
    shipped: it takes first_log_integrale_dif / log_integrale_dif / ds_froms_states from tracking_0 (:27), which work in variances, hands
    them standard deviations and squares the results again (:446, :460, :471); pairs ``all_Km1[-k]`` with ``all_Ks1[-1-k]`` (:505-506);
    and reads track 0 only (:478-480).  On a 7-position, 2-state track (LocErr 0.02, ds 0.01 / 0.1) it returns stds 0.0138 ... 0.0047
    where the exact conditional stds are 0.0196 ... 0.0128, and means off by up to 0.04.  What is returned here is checked against a
    dense solve of the same Gaussian model (tests/cond_reference.py)."""
    Cs = np.asarray(Cs, dtype=np.float64)
    if Cs.ndim != 3 or Cs.shape[1] < 2 or len(Cs) == 0 or not 1 <= Cs.shape[2] <= 3:
        raise ValueError("Cs must be a non-empty array [n_tracks, len >= 2, dims <= 3]")
    n, L, D = Cs.shape
    ds, Fs, TrMat = np.asarray(ds, float), np.asarray(Fs, float), np.asarray(TrMat, float)
    S = len(ds) if ds.ndim == 1 else 0
    if S < 2 or Fs.shape != (S,) or TrMat.shape != (S, S):
        raise ValueError("ds [S], Fs [S] and TrMat [S, S] must describe the same S >= 2 states")
    Bs = np.asarray(Bs)
    if Bs.ndim == 3 and Bs.shape[1] == 1:
        Bs = Bs[:, 0]
    Bs = _check_states(Bs, n, L, S, "Bs")
    le = np.asarray(LocErr, dtype=np.float64)
    per_peak = le.ndim == 3 and le.shape[:2] == (n, L)
    if per_peak:
        if le.shape[2] not in (1, D):
            raise ValueError("per-peak localisation errors must be an array [n_tracks, len, 1 | dims] matching Cs")
    elif le.size not in (1, D) or le.ndim > 3 or (le.ndim > 1 and le.size != le.shape[-1]):
        raise ValueError("LocErr must be a float, one value per dimension, or per-peak errors [n_tracks, len, 1 | dims]")
    ts = TrackSet([Cs], [le] if per_peak else None, device=device)
    try:
        model = ts.make_model(None if per_peak else le.reshape(1, 1, -1), ds, Fs, TrMat, 0.0, [], 1, 2)
        mu, sg = ts.ctx.refine_fixed_states(model, 0, Bs)
    finally:
        ts.close()
    return mu, _squeeze_sigs(sg)


def refine_along_states(all_tracks, dt, params, states=None, nb_states=2, frame_len=6, cell_dims=[1], input_LocErr=None,
                        return_logdensity=False, device=0, gaps=False):
    """Positions of a whole dataset refined along one state path per track.  ``all_tracks``: {str(len): ndarray[n_tracks, len, dims]};
    ``params``: lmfit-style parameters as for ``predict_states``; ``states``: {str(len): int8 ndarray[n_tracks, len]}, exactly what
    ``tracking.predict_states`` returns, or None to decode the most-likely paths with it first (``nb_states``, ``frame_len``,
    ``cell_dims`` go there; this is what the reference's get_best_estimates, extrack/refined_localization.py:551-560, does with the argmax
    of the posteriors).  ``input_LocErr``: optional per-peak errors {str(len): [n_tracks, len, 1 | dims]}.

    Returns ({len: mus [n, len, dims]}, {len: sigs [n, len]}) keyed by every input key - sigs [n, len, dims] with per-dimension errors -
    and with ``return_logdensity`` also {len: float64 [n]}, the log density of each track's displacements given its path (the path's own
    prior is not part of it).  A track with a NaN position or error, or whose path is -1 (``predict_states`` on such a track), is NaN;
    without ``gaps`` a missed detection written as a NaN row is such a position.

    ``gaps``: all-NaN rows are missed detections (``extrack_amd.gaps.insert_gaps``, DESIGN.md sections 18 and 19), checked on the host by
    the rules of ``TrackSet(gaps=True)`` (ValueError naming bucket and track, before any device call).  mus / sigs at such a row are the
    posterior mean and standard deviation of where the particle was at the frame it was not detected; the log density is that of the
    displacements between consecutive observed positions.  ``states`` carry one state per row, missed frames included, as
    ``predict_states(..., gaps=True)`` returns them; with ``states=None`` the paths are decoded with gaps first."""
    from . import tracking
    if not is_parameters(params):
        raise TypeError("params must be either of the class 'lmfit.parameter.Parameters' or a dictionary of the relevant parameters")
    if isinstance(dt, dict):
        raise NotImplementedError("refine_along_states is not built for per-track time steps (dt as a dict of arrays)")
    le, Ds, Fs, TrMat, pBL, so = tracking._extract_arrays(params, dt, 1, 1)
    S = len(Ds)
    shapes = {}
    for l, Cs in all_tracks.items():
        shp = np.shape(Cs)
        if len(shp) != 3 or shp[1] != int(l):
            raise ValueError("all_tracks[%r] must be an array [n_tracks, %s, dims]" % (l, l))
        if len(Cs) and not (shp[1] >= 2 and 1 <= shp[2] <= 3):
            raise ValueError("all_tracks[%r]: tracks need at least 2 positions and 1 to 3 dimensions" % l)
        shapes[str(l)] = shp
    if input_LocErr is not None:
        for l, shp in shapes.items():
            if shp[0] == 0:
                continue
            if not isinstance(input_LocErr, dict) or l not in input_LocErr:
                raise ValueError("input_LocErr must be a dict with the keys of all_tracks")
            es = np.shape(input_LocErr[l])
            if len(es) != 3 or es[:2] != shp[:2] or es[2] not in (1, shp[2]):
                raise ValueError("input_LocErr[%r] must be an array [n_tracks, len, 1 | dims] matching all_tracks" % l)
    if states is not None:
        if not isinstance(states, dict) or set(str(k) for k in states) != set(shapes):
            raise ValueError("states must be a dict with the keys of all_tracks: %s" % sorted(shapes, key=int))
        states = {str(k): _check_states(v, shapes[str(k)][0], shapes[str(k)][1], S, "states[%r]" % k) for k, v in states.items()}
    else:
        states = tracking.predict_states(all_tracks, dt, params, cell_dims=cell_dims, nb_states=nb_states, frame_len=frame_len,
                                         input_LocErr=input_LocErr, device=device, gaps=gaps)
    keys, tracks, sigmas = engine.sort_buckets(all_tracks, input_LocErr)
    ds = np.sqrt(2 * Ds * dt)
    K = None
    mus, sigs, lds = {}, {}, {l: np.empty(0) for l in keys}
    if tracks:
        ts = TrackSet(tracks, sigmas, device=device, min_len=max(int(keys[0]), 2), max_len=int(keys[-1]), gaps=gaps)
        try:
            if sigmas is not None:
                model = ts.make_model(None, ds, Fs, TrMat, pBL, cell_dims, 1, frame_len, slope_offset=so)
            else:
                model = ts.make_model(le[None, None], ds, Fs, TrMat, pBL, cell_dims, 1, frame_len)
            out = ts.refine_fixed_states(model, [states[str(arr.shape[1])] for arr in tracks], logdens=True)
            for arr, (mu, sg, ld) in zip(tracks, out):
                l = str(arr.shape[1])
                K = sg.shape[2]
                mus[l], sigs[l], lds[l] = mu, _squeeze_sigs(sg), ld
        finally:
            ts.close()
    for l in keys:  # empty buckets
        if l not in mus:
            shp = shapes[l]
            mus[l] = np.empty((0, shp[1], shp[2]))
            sigs[l] = np.empty((0, shp[1]) if K in (None, 1) else (0, shp[1], shp[2]))
    return (mus, sigs, lds) if return_logdensity else (mus, sigs)
