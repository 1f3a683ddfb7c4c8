"""extrack_amd - MI355X (gfx950) implementation of ExTrack's track-likelihood hot path.

Public surface mirrors ``extrack.tracking`` for this path only:
``param_fitting``, ``predict_Bs``, ``cum_Proba_Cs``, ``extract_params``, ``generate_params``, ``get_params``,
plus what the reference lacks: ``predict_states`` (most-likely state path per track), ``predict_transitions`` / ``transition_matrix`` (posterior of every pair of consecutive states, expected transition counts),``refine_along_states`` / ``get_pos_PDF_fixedBs`` (positions refined along such a path, ``extrack_amd.refined_localization``), ``parameter_uncertainties`` / ``track_scores`` (standard errors of a fit, ``extrack_amd.uncertainty``), ``gaps=True`` / ``extrack_amd.gaps.insert_gaps`` (tracks with missed detections: fit - ``gradient="forward"`` for the exact gap-aware gradient -, posteriors, state paths, the positions at the missed frames, the state-duration histograms ``len_hist(..., gaps=True)``, and ``track_scores`` / ``parameter_uncertainties(..., gaps=True)`` for standard errors)
(and ``extrack.histograms.len_hist`` in ``extrack_amd.histograms``).
The recursion runs in hand-written HIP kernels behind the C ABI of ``include/extrack_hip.h``;
importing this package does not touch the GPU, calling into it without the built library or without
a gfx950 device raises.
"""
from . import gaps, histograms, tracking, uncertainty  # noqa: F401
from .lmfit_compat import Parameters, minimize  # noqa: F401
from .tracking import (P_Cs_inter_bound_stats, Proba_Cs, TrackSet, cum_Proba_Cs, extract_params, generate_params, get_params,  # noqa: F401
                       param_fitting, predict_Bs, predict_states, predict_transitions, transition_matrix)
from .refined_localization import get_pos_PDF_fixedBs, refine_along_states  # noqa: F401
from .uncertainty import hessian_from_gradient, parameter_uncertainties, track_scores  # noqa: F401

__version__ = "0.1.0"
