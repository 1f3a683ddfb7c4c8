"""Tracks with missed detections.

Trackers close gaps (TrackMate's gap closing, blinking fluorophores): consecutive rows of a track are then not consecutive frames.  The
readers return the frame numbers next to the positions (extrack/readers.py:173-203); ``insert_gaps`` turns both into what
``param_fitting(..., gaps=True)`` / ``predict_Bs(..., gaps=True)`` / ``TrackSet(..., gaps=True)`` take: one row per FRAME between a track's
first and last detection, NaN in every coordinate where nothing was detected, bucketed by that frame span.  The kernels integrate such a
position out exactly instead of treating its neighbours as one frame apart (which inflates the diffusion coefficients).
"""
import numpy as np


def _frame_rows(fr, what):
    f = np.asarray(fr, dtype=np.float64)
    if f.ndim == 2 and f.shape[1] == 1:
        f = f[:, 0]
    if f.ndim != 1:
        raise ValueError("%s: frames must be one number per position" % what)
    if not np.all(np.isfinite(f)) or np.any(f != np.round(f)):
        raise ValueError("%s: frames must be integers" % what)
    d = np.diff(f)
    if np.any(d == 0):
        raise ValueError("%s: a frame is repeated" % what)
    if np.any(d < 0):
        raise ValueError("%s: frames must increase along the track" % what)
    return f.astype(np.int64)


def insert_gaps(all_tracks, frames, input_LocErr=None, max_gap=None):
    """all_tracks {len: [n, len, dims]} and frames {len: [n, len]} (the readers' two dicts; [n, len, 1] is accepted) -> ``(tracks, frames,
    input_LocErr, origin)``, dicts keyed by the frame SPAN (str, like the input keys): tracks [n, span, dims] with a NaN row per missing
    frame, frames [n, span] (every frame of the span), the per-peak errors [n, span, k] with NaN at those rows (None without
    ``input_LocErr``) and origin [n, 2] = (source bucket length, source row) of every output track.
    ``max_gap``: a run of more than ``max_gap`` missing frames splits the track there (0: at every missing frame); pieces of fewer than 2
    positions are dropped.  Frames that are non-integer, repeated or decreasing raise ValueError."""
    if max_gap is not None and max_gap < 0:
        raise ValueError("max_gap must be None or >= 0")
    acc = {}
    for key in all_tracks:
        tr = np.asarray(all_tracks[key], dtype=np.float64)
        if len(tr) == 0:
            continue
        if key not in frames:
            raise ValueError("frames has no bucket %r" % (key,))
        fr_b = np.asarray(frames[key])
        if fr_b.shape[:2] != tr.shape[:2]:
            raise ValueError("bucket %r: frames must match all_tracks in (n_tracks, len)" % (key,))
        sg = None if input_LocErr is None else np.asarray(input_LocErr[key], dtype=np.float64)
        if sg is not None and sg.shape[:2] != tr.shape[:2]:
            raise ValueError("bucket %r: input_LocErr must match all_tracks in (n_tracks, len)" % (key,))
        for n in range(len(tr)):
            f = _frame_rows(fr_b[n], "bucket %r, track %d" % (key, n))
            cuts = [0] + ([] if max_gap is None else list(np.nonzero(np.diff(f) - 1 > max_gap)[0] + 1)) + [len(f)]
            for a, b in zip(cuts[:-1], cuts[1:]):
                if b - a < 2:
                    continue
                span = int(f[b - 1] - f[a] + 1)
                rows = f[a:b] - f[a]
                pos = np.full((span, tr.shape[2]), np.nan)
                pos[rows] = tr[n, a:b]
                err = None
                if sg is not None:
                    err = np.full((span, sg.shape[2]), np.nan)
                    err[rows] = sg[n, a:b]
                acc.setdefault(span, []).append((pos, np.arange(f[a], f[a] + span), err, (int(tr.shape[1]), n)))
    tracks, out_frames, errs, origin = {}, {}, ({} if input_LocErr is not None else None), {}
    for span in sorted(acc):
        k = str(span)
        tracks[k] = np.array([x[0] for x in acc[span]])
        out_frames[k] = np.array([x[1] for x in acc[span]])
        if errs is not None:
            errs[k] = np.array([x[2] for x in acc[span]])
        origin[k] = np.array([x[3] for x in acc[span]], dtype=np.int64)
    return tracks, out_frames, errs, origin
