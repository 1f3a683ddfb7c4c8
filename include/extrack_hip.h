/* extrack_hip.h - C ABI of libextrack_hip.so: the MI355X (gfx950) implementation of ExTrack's
 * track-likelihood hot path.
 *
 * The reference (vanTeeffelenLab/ExTrack v1.6.3, pure Python/numpy) has no FFI seam for this path;
 * the functions below are what a binding for it replaces (file:line relative to the reference root):
 *
 *   extrack_upload_bucket / extrack_attach_bucket
 *       one length bucket of the {str(len): ndarray[N, len, D]} dict, as produced by
 *       extrack/readers.py:82-97 and consumed at extrack/tracking.py:1346-1367 (param_fitting) and
 *       :822-835 (predict_Bs); optional per-peak localisation errors = input_LocErr (tracking.py:1354).
 *   extrack_loglik / extrack_loglik_async
 *       sum over all buckets of Proba_Cs (extrack/tracking_0.py:440-458 -> P_Cs_inter_bound_stats,
 *       extrack/tracking.py:109-318), i.e. the body of cum_Proba_Cs after extract_params
 *       (extrack/tracking_0.py:654-700 / tracking.py:1009-1069): returns +sum(LL); the caller negates.
 *   extrack_predict
 *       P_Cs_inter_bound_stats(..., do_preds=1)[2] for one bucket (Pool_star_P_inter,
 *       extrack/tracking_0.py:460-461, driven by predict_Bs :463-563).
 *   extrack_map_states
 *       nothing in the reference: the most-likely state sequence of every track of one bucket (windowed Viterbi decoding of the same
 *       recursion), for the callers of predict_Bs (extrack/tracking.py:792-906) that segment tracks by the argmax of its posteriors.
 *   extrack_loglik_th
 *       the same sum for the THRESHOLD-FUSION kernel that extrack.tracking calls in v1.6.3: Proba_Cs
 *       (extrack/tracking.py:769-787) -> P_Cs_inter_bound_stats_th (:427-650) + fuse_tracks_th (:652-743),
 *       evaluated in chunks as cum_Proba_Cs does (tracking.py:1043-1069, 2000 tracks per chunk).
 *   extrack_predict_th
 *       P_Cs_inter_bound_stats_th(..., do_preds=1)[2] for one bucket in chunks of nb_max tracks (predict_Bs,
 *       extrack/tracking.py:792-906).
 *   extrack_th_plan_step
 *       the merge groups fuse_tracks_th decided for one chunk and step (tracking.py:681-701) - diagnostic.
 *   extrack_p_stay_table
 *       the field-of-view survival table, extrack/tracking.py:182-191.
 *   extrack_segment_len_hist
 *       P_segment_len(...)[2] (extrack/histograms.py:26-286) summed over one bucket: the state-duration histogram that len_hist
 *       (histograms.py:294-373) accumulates over chunks of 50 tracks.
 *   extrack_segment_len_hist_gaps
 *       extrack_segment_len_hist for tracks with missed detections (all-NaN rows, as extrack_loglik_gaps): nothing in the reference.
 *   extrack_refine_positions
 *       get_pos_PDF + the weighted read-out of position_refinement for one bucket (extrack/refined_localization.py:207-338).
 *   extrack_refine_pos_pdf
 *       get_pos_PDF's own return values (extrack/refined_localization.py:207-298): means / stds / log-weights of every component of the
 *       Gaussian mixture of every position, for inspection of small buckets.
 *   extrack_refine_fixed_states
 *       what get_pos_PDF_fixedBs / get_LC_Km_Ks_fixed_Bs (extrack/refined_localization.py:414-519, used by get_best_estimates :551-560)
 *       were written to compute: mean and std of every real position given ONE state per position.  Not that function's numbers, which
 *       are inconsistent as shipped: it hands standard deviations to the variance-based integrals it imports from tracking_0 (:27) and
 *       squares their results again (:446, :460, :471), pairs all_Km1[-k] with all_Ks1[-1-k] (:505-506) and reads track 0 only (:478-480).
 *   extrack_map_states_gaps / extrack_refine_fixed_states_gaps
 *       the two above for tracks with missed detections (all-NaN rows), as extrack_loglik_gaps / extrack_predict_gaps: nothing in the
 *       reference, which never reads the frame numbers its readers return (extrack/readers.py:173-203).
 *   extrack_loglik_grad
 *       extrack_loglik AND its exact gradient in one pass.  It replaces the finite-difference loop that the reference's
 *       optimiser runs around cum_Proba_Cs (lmfit.minimize at extrack/tracking.py:1371: BFGS evaluates the objective
 *       nvar + 1 times per iteration to difference it numerically).
 *   extrack_loglik_grad_gaps / extrack_loglik_scores_gaps
 *       extrack_loglik_grad / extrack_loglik_scores for tracks with missed detections (all-NaN rows, as extrack_loglik_gaps): nothing in
 *       the reference.
 *   extrack_loglik_scores
 *       the same evaluation keeping every track's own dLL_n/dtheta and their outer-product sum: what the parameter standard errors
 *       of a fit are computed from (the reference returns point estimates only).
 *   extrack_loglik_th_grad
 *       extrack_loglik_th AND the exact gradient of that value at the evaluation's own merge plan - the objective v1.6.3's
 *       param_fitting hands to lmfit.minimize (extrack/tracking.py:1371 -> cum_Proba_Cs :991 -> P_Cs_inter_bound_stats_th :427-650);
 *       the reference differences it numerically although the grouping decisions of fuse_tracks_th (:676-701) make it only
 *       piecewise smooth.
 *
 * Conventions: plain C, no exceptions cross the boundary.  Every function returns 0 on success or a
 * negative EXTRACK_E_* code; extrack_last_error() gives the message.  The caller owns every host
 * buffer it passes; the library owns device copies made by extrack_upload_bucket.  A context is
 * driven by one host thread at a time.  All arithmetic is IEEE fp64.
 */
#ifndef EXTRACK_HIP_H
#define EXTRACK_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EXTRACK_ABI_VERSION 6

#define EXTRACK_OK 0
#define EXTRACK_E_INVALID (-1)     /* bad argument / unsupported configuration */
#define EXTRACK_E_HIP (-2)         /* HIP runtime error (message has the HIP error string) */
#define EXTRACK_E_NODEVICE (-3)    /* no usable gfx950 device */
#define EXTRACK_E_UNSUPPORTED (-4) /* valid request outside the built kernel set (e.g. S^F too large for LDS) */

typedef struct extrack_ctx extrack_ctx;

/* Model parameters after extract_params (extrack/tracking.py:913-986) plus the dataset-global scalars
 * that cum_Proba_Cs derives from the bucket list (tracking.py:1009-1010). */
typedef struct extrack_model {
    int32_t n_states;    /* S, 2..8 */
    int32_t nb_substeps; /* ns, 1..4 */
    int32_t frame_len;   /* F > ns, window of exactly enumerated states; S^F <= 2^20 sequences per track.  Up to 1024 groups
                            (S^(F-ns)) and 160 KB per track the state lives in LDS / registers; beyond that - 5 states at the reference's default
                            frame_len 6, 6 states at frame_len 5 - 6, 2 states at frame_len 11 - 15, posteriors with 7 / 8 states - in global
                            memory, one lane per track (csrc/xt_big.h: likelihood and posteriors; the gradient entry points answer
                            EXTRACK_E_UNSUPPORTED there and the caller differences the objective) */
    int32_t min_len;     /* smallest track length of the WHOLE dataset (all shards); the stay-in-FOV term starts at step max(min_len, 2) */
    int32_t max_len;     /* largest track length of the WHOLE dataset: buckets of this length get isBL = 0 */
    int32_t locerr_mode; /* 0: global locerr[]; 1: per-peak sigma uploaded with the bucket;
                            2: per-peak, sigma' = clip(sigma*slope + offset, 1e-6, inf) (tracking.py:928-930) */
    int32_t locerr_dims; /* mode 0: 1 (one value for all dims) or D (one per dim) */
    int32_t n_p_stay;    /* 0 or 1: p_stay is ONE table; n > 1: p_stay holds n tables, one per chunk (per-track time steps, see
                            extrack_set_bucket_dt) */
    double locerr[3];    /* mode 0: localisation error (std) */
    double slope, offset;
    double pBL;          /* bleaching probability per step */
    const double* ds;    /* [S] diffusion lengths sqrt(2 D dt), non-decreasing */
    const double* Fs;    /* [S] initial fractions, > 0 */
    const double* TrMat; /* [S*S] row-major per-substep transition probabilities P(i->j), > 0 */
    const double* p_stay;/* [S^ns] probability of staying in the field of view; index r has digit c
                            (r / S^c) % S with c = 0 the newest sub-state (extrack_p_stay_table) */
} extrack_model;

int extrack_abi_version(void);

/* Creates a context on HIP device `device_id` (must be gfx950).  Owns one non-blocking stream. */
int extrack_create(int device_id, extrack_ctx** out);
void extrack_destroy(extrack_ctx* ctx);
/* Message for the last error on ctx (or for a failed extrack_create when ctx == NULL). */
const char* extrack_last_error(const extrack_ctx* ctx);

/* Use an external HIP stream (hipStream_t) for all subsequent work, or NULL to go back to the
 * context's own stream. */
int extrack_set_stream(extrack_ctx* ctx, void* hip_stream);

/* Copies one length bucket to the device.  tracks: host [n][len][dims] C-order fp64.
 * sigma: NULL or host [n][len][sigma_dims] per-peak localisation errors, sigma_dims in {1, dims}.
 * Buckets may be uploaded in any order; ids are dense from 0. */
int extrack_upload_bucket(extrack_ctx* ctx, const double* tracks, int64_t n, int32_t len, int32_t dims,
                          const double* sigma, int32_t sigma_dims, int32_t* bucket_id_out);
/* Same, for buffers that already live on this device (e.g. torch tensors): no copy, caller keeps
 * them alive until extrack_clear_buckets / extrack_destroy. */
int extrack_attach_bucket(extrack_ctx* ctx, const double* d_tracks, int64_t n, int32_t len, int32_t dims,
                          const double* d_sigma, int32_t sigma_dims, int32_t* bucket_id_out);
/* Per-track time steps of one bucket (extrack/tracking.py:979-982: dt given as {len: array[n][len]}): dt host [n][len], copied
 * to the device; NULL removes them.  Only the threshold-fusion entry points use them (the reference's fixed-window kernel has no
 * such input).  With time steps set, model->ds must be the diffusion lengths for a UNIT time step (sqrt(2 D)): the diffusion
 * term added at step t is scaled by dt[track][len - t] (tracking.py:494-499, 548-551 - the reference reads its UNREVERSED array
 * at column len - current_step), and model->p_stay must hold one table per chunk, buckets in id order, chunks in row order: the
 * field-of-view table of a chunk comes from the median over the chunk's tracks of sqrt(2 D dt[track][0]) (tracking.py:507-511). */
int extrack_set_bucket_dt(extrack_ctx* ctx, int32_t bucket_id, const double* dt);
int extrack_clear_buckets(extrack_ctx* ctx);
int extrack_bucket_count(const extrack_ctx* ctx);

/* One log-likelihood evaluation over every bucket of the context.
 * total_ll (host, required): sum of per-track log-likelihoods (NOT negated).
 * per_track (host, may be NULL): per-track log-likelihoods, buckets concatenated in id order. */
int extrack_loglik(extrack_ctx* ctx, const extrack_model* model, double* total_ll, double* per_track);
/* Enqueues the evaluation on the context's stream and leaves the scalar in device memory
 * (d_total_ll, 8 bytes, device pointer) without synchronising - for a following RCCL all-reduce. */
int extrack_loglik_async(extrack_ctx* ctx, const extrack_model* model, double* d_total_ll);

/* Per-sequence log-probabilities of one bucket, the first return value of P_Cs_inter_bound_stats (extrack/tracking.py:109-318, returned
 * at :318): lp host [n][n_cols], column i = the sequence of states whose digit c is (i / n_states^c) % n_states, c = 0 the newest state
 * (get_all_Bs, tracking.py:746-757); n_cols = extrack_sequence_columns(n_states, len, nb_substeps, frame_len, isBL) with isBL =
 * (len != model->max_len).  The likelihood path never forms this matrix (it is reduced in the kernel): this entry point exists for
 * callers of the reference function that read it, on small inputs (n * n_states^(frame_len + nb_substeps) doubles cross the host). */
int64_t extrack_sequence_columns(int32_t n_states, int32_t len, int32_t nb_substeps, int32_t frame_len, int32_t isBL);
int extrack_sequence_matrix(extrack_ctx* ctx, const extrack_model* model, int32_t bucket_id, double* lp, int64_t n_cols);

/* State posteriors of one bucket: preds host [n][len][S].  model->nb_substeps must be 1
 * (predict_Bs forces it, extrack/tracking.py:839). */
int extrack_predict(extrack_ctx* ctx, const extrack_model* model, int32_t bucket_id, double* preds);

/* Tracks with missed detections: extrack_loglik / extrack_predict with gaps.  A row of a bucket whose coordinates are ALL NaN is a frame
 * at which the particle was not detected (trackers close such gaps; extrack/readers.py:173-203 returns the frame numbers and nothing
 * downstream reads them).  The position is integrated out exactly: at such a step the state chain and the diffusion go on - transition
 * and stay factor, fusion and expansion as at any step - and no observation factor is applied; the variance carried forward is d2 + u.
 * This is the limit of an infinite localisation error at that row.  The bucket length is the frame span, gaps included: isBL, min_len,
 * max_len and the stay-in-field-of-view term follow from it as before.  The per-track constant counts the observed rows,
 * -(n_observed - 1) * dims / 2 * log(2 pi).  The first and the last row of a track must be observed; a NaN first or last row, or a row
 * with only some NaN coordinates, makes the track's results NaN (as any NaN does in extrack_loglik).  The per-peak error of a gap row
 * is never read and may be NaN.  Posteriors: the state posterior of the gap position is returned like any other; the predictive
 * density of a position that was not observed does not weight the posterior of the state leaving the window at that step.
 * Served by gap-aware instantiations of the general fixed-window kernel (csrc/xt_kernel.h); two-state likelihood launches (frame_len 5..7,
 * and 4 in a context created under EXTRACK_GAP_REG2_F=all; one global scalar localisation error, a well-scaled model) by the gap-aware
 * instantiation of the register-resident kernel (csrc/xt_reg2.h; EXTRACK_LL_PATH=lds keeps the general kernel; extrack_last_ll_path tells
 * which ran).  Decided on the
 * host, nothing is launched, EXTRACK_E_UNSUPPORTED: nb_substeps >= 2, n_states > 4, models whose sequence state does not fit a
 * workgroup (more than 1024 groups of sequences or more than 160 KiB of LDS per track), buckets with per-track time steps.
 * extrack_last_kernel_ms / extrack_last_launch_info cover the launches. */
int extrack_loglik_gaps(extrack_ctx* ctx, const extrack_model* model, double* total_ll, double* per_track);
int extrack_predict_gaps(extrack_ctx* ctx, const extrack_model* model, int32_t bucket_id, double* preds);

/* Most-likely state path of every track of one bucket (windowed Viterbi decoding): states host [n][len] (int8, the state of every
 * position), score host [n] or NULL (log joint density of the track and that path).  Replaces nothing in the reference, which has no
 * such function; it sits beside predict_Bs (extrack/tracking.py:792-906), whose callers segment tracks by the per-position argmax of the
 * posteriors.  The recursion is that of extrack_predict with every sum over sequences replaced by a selection: a sequence older than
 * frame_len states survives only as the most probable member of its group, the last position takes the most probable of the
 * n_states^(frame_len + 1) sequences left (with isBL the state after the last position is summed out), and the older states follow from
 * the recorded choices.  For len <= frame_len + 1 the path is the exact maximiser of the sequence matrix (extrack_sequence_matrix).
 * A track with a NaN position or error gets states -1 and score NaN.  model->nb_substeps must be 1.  EXTRACK_E_UNSUPPORTED (decided on
 * the host, nothing is launched): n_states > 4, n_states^(frame_len - 1) > 1024 or a sequence state beyond the LDS of a CU, buckets
 * with per-track time steps.  extrack_last_kernel_ms covers the launch. */
int extrack_map_states(extrack_ctx* ctx, const extrack_model* model, int32_t bucket_id, int8_t* states, double* score);

/* extrack_map_states for tracks with missed detections (all-NaN rows, as extrack_loglik_gaps defines them): at such a row the select
 * and its recorded choice are those of any step, the expand applies the transition / stay factor alone, and the state at the row is
 * decoded like any other.  score: log joint density of the OBSERVED positions and the path, constant -(n_observed - 1) * dims / 2 *
 * log(2 pi).  A NaN first or last row, a row with only some NaN coordinates, or a NaN error at an observed row gives states -1 and score
 * NaN; the per-peak error of a gap row is never read.  Inside a run of two or more consecutive gap rows distinct paths can have exactly
 * the same density (it depends on how many rows of the run each state occupies, not on where): the tie rule of extrack_map_states
 * picks one.  Same launch path, back-pointer placement, scratch and refusals as extrack_map_states, except that nb_substeps != 1 is
 * EXTRACK_E_UNSUPPORTED here (as in extrack_loglik_gaps); gap-free data gives the same bits. */
int extrack_map_states_gaps(extrack_ctx* ctx, const extrack_model* model, int32_t bucket_id, int8_t* states, double* score);

/* Pairwise state posteriors of one bucket (nothing of the kind in the reference): pairs host [n][len-1][n_states][n_states] or NULL,
 * pairs[k][t][i][j] = P(state of position t = i, state of position t+1 = j | track k); counts host [n][n_states][n_states] or NULL,
 * counts[k][i][j] = sum over t of pairs[k][t][i][j], the expected number of i -> j transitions of the track (summed in the order of t).
 * With pairs NULL only the counts leave the device.  nb_substeps is 1.
 * Definition: the pair is taken from exactly the weights from which extrack_predict takes the posterior of position t.  A position that
 * leaves the window (t <= len - 2 - frame_len) is read when it is the oldest digit of the window, weighted by the predictive density of the
 * next position as the reference weights it (extrack/tracking.py:255-271, its missing 1/2 on the log term included): the pair is the oldest
 * and the second-oldest digit.  The remaining positions come from the final sequence weights, as neighbouring digits.  So
 *     sum over j of pairs[k][t][i][j] = preds[k][t][i] of extrack_predict for EVERY t (to rounding), while
 *     sum over i of pairs[k][t][i][j] = preds[k][t+1][j] holds only for t >= len - 1 - frame_len (inside the last window); before that the
 * two sides are read at different lags of the fixed-lag approximation.  For len <= frame_len + 1 nothing is fused and the pairs are exact.
 * extrack_predict_pairs_gaps: all-NaN rows are missed detections with the weights of extrack_predict_gaps (at a gap step the transition
 * factor alone weights the leaving digit); pairs that involve a missed frame are returned like any other.  A track that extrack_predict
 * (extrack_predict_gaps) makes NaN is NaN everywhere, counts included.
 * Served by the PAIRS instantiations of the fixed-window kernel (csrc/xt_kernel.h), two states included; extrack_last_ll_path reports
 * "general" or "gaps".  Both outputs NULL: EXTRACK_E_INVALID.  Decided on the host, nothing is launched: nb_substeps != 1 (refused as
 * extrack_predict / extrack_predict_gaps refuse it), and EXTRACK_E_UNSUPPORTED for n_states > 4, for n_states^(frame_len - 1) > 1024 or a
 * sequence state with pair accumulators beyond the 160 KiB LDS of a CU, and for buckets with per-track time steps.
 * extrack_last_kernel_ms / extrack_last_launch_info cover the launch. */
int extrack_predict_pairs(extrack_ctx* ctx, const extrack_model* model, int32_t bucket_id, double* pairs, double* counts);
int extrack_predict_pairs_gaps(extrack_ctx* ctx, const extrack_model* model, int32_t bucket_id, double* pairs, double* counts);

/* Tangent of a model along one direction theta: d(field)/d(theta) for every differentiable field of extrack_model.
 * The diffusion lengths enter as the derivative of their SQUARES (ds^2 = 2 D dt is what the recursion uses, and it keeps the
 * derivative finite at D = 0).  p_stay is a function of ds and cell_dims computed by the caller (extrack_p_stay_table), so its
 * tangent comes from the caller too. */
typedef struct extrack_model_tangent {
    double locerr[3];     /* d locerr (std), mode 0 */
    double slope, offset; /* mode 2 */
    double pBL;
    const double* ds2;    /* [S]    d (ds^2) */
    const double* Fs;     /* [S] */
    const double* TrMat;  /* [S*S] */
    const double* p_stay; /* [S^ns] */
} extrack_model_tangent;

/* One evaluation of the fixed-window log-likelihood (as extrack_loglik) together with its derivative along n_dir model
 * directions, by forward-mode differentiation inside the recursion (window fusion included: it is the exact gradient of the
 * value extrack_loglik returns, not an approximation).  total_ll: sum of per-track log-likelihoods; grad[i] = d total_ll /
 * d theta_i (host, n_dir entries).  n_dir may be 0 (then it is extrack_loglik).  Two-state models with one substep run with the
 * sequence state and its tangents in registers (csrc/xt_reg2.h), <= 8 directions per pass; 3 / 4 states by reverse mode (csrc/xt_rev.h);
 * other models with the tangents in registers + LDS exchange (csrc/xt_gradr.h) or in LDS (csrc/xt_grad.h).  Restriction: all uploaded
 * buckets must share the track dimensionality and the per-peak error layout (ONE launch group; a real dataset does) - otherwise
 * EXTRACK_E_UNSUPPORTED (extrack_loglik itself serves such mixed sets, group by group). */
int extrack_loglik_grad(extrack_ctx* ctx, const extrack_model* model, int32_t n_dir, const extrack_model_tangent* tangents,
                        double* total_ll, double* grad);
/* The same evaluation enqueued on the context's stream (extrack_set_stream) without waiting for it: d_out (DEVICE, 1 + n_dir
 * doubles) receives {sum LL, d sum LL / d theta_i} in stream order - the multi-GPU objective all-reduces that buffer on the same
 * stream (RCCL), like extrack_loglik_async does for the scalar.  The tangent arrays are consumed before the call returns. */
int extrack_loglik_grad_async(extrack_ctx* ctx, const extrack_model* model, int32_t n_dir, const extrack_model_tangent* tangents,
                              double* d_out);
/* Threshold-fusion log-likelihood (as extrack_loglik_th: same threshold / max_nb_states / chunk semantics, same value up to rounding)
 * together with its derivative along n_dir model directions AT THE FROZEN PLAN of this evaluation: the plan kernel decides the merge
 * groups of every chunk from its pilot tracks at `model`, then one forward and one backward sweep over every track (reverse mode, csrc/
 * xt_thgrad.h) return sum LL and the adjoint of every model table, contracted with the directions' tangents - the cost does not
 * depend on n_dir.  With the groups held fixed the value is a smooth function of the model and grad is its exact derivative; where a
 * parameter change flips a grouping decision the objective itself jumps (by ~1e-9 relative) and no derivative exists - finite
 * differences of the reference's optimiser sample those jumps, this gradient does not.  n_dir may be 0.  Not built: per-track time
 * steps (extrack_set_bucket_dt) and models whose n_states^(nb_substeps + 1) table adjoints exceed the LDS (EXTRACK_E_UNSUPPORTED). */
int extrack_loglik_th_grad(extrack_ctx* ctx, const extrack_model* model, double threshold, int32_t max_nb_states, int32_t chunk,
                           int32_t n_dir, const extrack_model_tangent* tangents, double* total_ll, double* grad);
/* The same, enqueued on the context's stream: d_out (DEVICE, 1 + n_dir doubles) receives {sum LL, gradient} in stream order (the plan
 * kernel's sequence counts are still read back once inside the call, as in extrack_loglik_th_async). */
int extrack_loglik_th_grad_async(extrack_ctx* ctx, const extrack_model* model, double threshold, int32_t max_nb_states, int32_t chunk,
                                 int32_t n_dir, const extrack_model_tangent* tangents, double* d_out);
/* Frozen plan: with on = 1 the threshold-fusion evaluations of this context (extrack_loglik_th[_async], extrack_loglik_th_grad[_async])
 * skip the plan kernel and follow the merge plan the LAST planning evaluation left with the buckets (same chunk size required;
 * EXTRACK_E_INVALID if there is none).  The value is then a smooth function of the model (the objective fuse_tracks_th would give if its
 * grouping decisions, /root/reference/extrack/tracking.py:676-701, did not react to the parameters) - what an optimiser should be
 * handed between two re-plannings (extrack_amd.tracking.param_fitting does: plan, minimise at that plan with the exact gradient,
 * re-plan, until the plan no longer changes).  on = 0: every evaluation decides its own plan again (the reference's semantics). */
int extrack_th_freeze_plan(extrack_ctx* ctx, int32_t on);
/* Per-sequence log-probabilities of the threshold-fusion kernel for ONE bucket taken as ONE chunk - the first return value of
 * P_Cs_inter_bound_stats_th (extrack/tracking.py:427, returned at :650) before Proba_Cs' log-sum (:780-787): lp host [n][n_cols], n_cols =
 * (state sequences alive after the last merge) x n_states^nb_substeps, column g * n_states^nb_substeps + r as in the reference; for isBL
 * buckets (len != model->max_len) WITHOUT the leaving / bleaching term, a further expansion by n_states^nb_substeps whose factors depend
 * on the model only (tracking.py:611-630; extrack_amd.tracking.P_Cs_inter_bound_stats_th adds it).  Call with lp == NULL first: *n_cols_out
 * receives n_cols (it depends on the merges, i.e. on the data).  For callers of the reference function that read the matrix, on small
 * inputs (n * n_cols doubles cross the host); the likelihood path never forms it. */
int extrack_sequence_matrix_th(extrack_ctx* ctx, const extrack_model* model, int32_t bucket_id, double threshold, int32_t max_nb_states,
                               double* lp, int64_t n_cols_cap, int64_t* n_cols_out);
/* Per-track scores.  One evaluation as extrack_loglik_grad that also keeps every track's own derivative s_n = d LL_n / d theta (the
 * forward-mode kernels hold it just before they sum over tracks) and, tracks being independent, reduces it on the device to the outer
 * product of gradients opg[i][j] = sum_n s_ni s_nj (fp64, fixed summation order: bit-reproducible; exactly symmetric) - an estimate of
 * the Fisher information whose inverse is the BHHH covariance of a fitted theta.  total_ll and grad (n_dir entries, or NULL) as
 * extrack_loglik_grad; opg: host [n_dir * n_dir] row-major, or NULL (then the reduction is skipped); scores: host [sum N][n_dir], the
 * buckets concatenated in id order as the per_track output of extrack_loglik, or NULL (the N x n_dir matrix then never leaves the
 * device).  A track with a NaN position has a NaN row, and opg is then not finite.  Always the forward-mode kernels (csrc/xt_reg2.h,
 * xt_gradr.h, xt_grad.h) - the reverse-mode kernels accumulate their adjoints across tracks and have no per-track score - so for 3 / 4
 * states one call costs several extrack_loglik_grad calls: meant to be called once per fit, not once per iteration.  1 <= n_dir <= 32
 * (n_dir == 0: EXTRACK_E_INVALID).  Restriction as extrack_loglik_grad: ONE launch group, EXTRACK_E_UNSUPPORTED otherwise.  The device
 * score matrix (sum N * n_dir doubles) stays allocated with the context.  The first reduction stage sums tiles of EXTRACK_OPG_TILE
 * tracks. */
#define EXTRACK_OPG_TILE 1024
int extrack_loglik_scores(extrack_ctx* ctx, const extrack_model* model, int32_t n_dir, const extrack_model_tangent* tangents,
                          double* total_ll, double* grad, double* opg, double* scores);
/* The same, enqueued on the context's stream: d_out (DEVICE, 1 + n_dir + n_dir * n_dir doubles) receives {sum LL, gradient, opg
 * row-major} in stream order - a multi-GPU caller all-reduces that buffer; the scores themselves are never gathered. */
int extrack_loglik_scores_async(extrack_ctx* ctx, const extrack_model* model, int32_t n_dir, const extrack_model_tangent* tangents,
                                double* d_out);
/* extrack_loglik_grad / extrack_loglik_scores (and their _async forms) for tracks with missed detections: all-NaN rows as
 * extrack_loglik_gaps defines them, same arguments and outputs as the plain calls.  At a gap step the merged state and its tangents go
 * through the transition alone (rz' = R + d log T[q], dm' = d m_bar, du' = d d2_q + d u_bar): no Gaussian factor, and neither the
 * position nor the per-peak error of the row is read (the error may be NaN).  total_ll is the value extrack_loglik_gaps returns; its
 * + n_gaps * dims / 2 * log(2 pi) per track does not depend on the model and adds nothing to gradient and scores.  A NaN first or last
 * row, a row with only some NaN coordinates or a NaN error at an observed row gives the track a NaN LL and NaN scores.  Served by
 * gap-aware instantiations of the two forward-mode bodies (csrc/extrack_grad_gaps.hip): csrc/xt_gradr.h for up to 256 groups of
 * sequences per track, else csrc/xt_grad.h for up to 1024; two states with one global localisation error (locerr_mode 0, locerr_dims 1) at
 * frame_len 5..7 (4 under EXTRACK_GAP_REG2_F) run on gap-aware instantiations of the register-resident kernels instead (csrc/xt_reg2.h,
 * csrc/extrack_reg2_grad_gaps_f*.hip; EXTRACK_GRAD_PATH=gradr | lds keep the general ones; extrack_last_grad_path tells which ran).  A gradient
 * call (not a scores call: reverse mode has no per-track scores) whose gap-free twin - the same group through extrack_loglik_grad - would run
 * the reverse-mode kernels runs their gap-aware instantiations instead (csrc/xt_rev.h, csrc/extrack_rev_gaps.hip: 3 and 4 states; two states
 * with per-peak errors or frame_len 3), one forward and one backward sweep whatever n_dir; EXTRACK_GRAD_PATH=gradr | lds |
 * reg2, or a log budget (EXTRACK_REV_LOG_MB) too small for the group, keep the forward-mode kernels.  Decided on the host before anything is enqueued, EXTRACK_E_UNSUPPORTED: nb_substeps >= 2,
 * n_states > 4, buckets with per-track time steps, models that fit neither kernel.  n_dir == 0 is extrack_loglik_gaps (for the _async
 * form: evaluated synchronously, the sum then copied to d_out).  Scores: rows in bucket-upload order, ONE launch group, opg as in
 * extrack_loglik_scores.  Gap-free data gives the values of the plain calls up to the rounding of another kernel family (two states: the
 * plain call runs csrc/xt_reg2.h).  extrack_last_grad_ms / extrack_last_launch_info cover the launches. */
int extrack_loglik_grad_gaps(extrack_ctx* ctx, const extrack_model* model, int32_t n_dir, const extrack_model_tangent* tangents,
                             double* total_ll, double* grad);
int extrack_loglik_grad_gaps_async(extrack_ctx* ctx, const extrack_model* model, int32_t n_dir, const extrack_model_tangent* tangents,
                                   double* d_out);
int extrack_loglik_scores_gaps(extrack_ctx* ctx, const extrack_model* model, int32_t n_dir, const extrack_model_tangent* tangents,
                               double* total_ll, double* grad, double* opg, double* scores);
int extrack_loglik_scores_gaps_async(extrack_ctx* ctx, const extrack_model* model, int32_t n_dir, const extrack_model_tangent* tangents,
                                     double* d_out);
/* Device time (ms) of the gradient kernels of the last extrack_loglik_grad / extrack_loglik_th_grad (or _async) call (waits for them). */
int extrack_last_grad_ms(extrack_ctx* ctx, float* ms);

/* State-duration histogram of one bucket (extrack/histograms.py:26-286 P_segment_len, third return value, summed over the bucket's
 * tracks): hist host [(len - 1)][S], hist[k - 1][s] = expected number of segments of exactly k consecutive positions in state s
 * (segments as long as the whole track are not counted, histograms.py:279).  Every state sequence is followed with its full
 * history; after each position at most max_nb_states sequences survive, ranked by their probability including the next position's
 * predictive density (histograms.py:185-203; len_hist's default is 500).  model->nb_substeps must be 1; model->min_len is the
 * reference's min_l (smallest track length of the dataset), isBL = (len != model->max_len) as elsewhere.
 * Limits: len * bits_per_state <= 4096 (bits = 1 / 2 / 3 for <= 2 / 4 / 8 states), max_nb_states * n_states <= 16384, and the staged track +
 * candidate arrays + histogram must fit the 160 KiB LDS of a CU (refused with EXTRACK_E_UNSUPPORTED otherwise). */
int extrack_segment_len_hist(extrack_ctx* ctx, const extrack_model* model, int32_t bucket_id, int32_t max_nb_states, double* hist);
/* The same for tracks with missed detections: an interior row whose coordinates are all NaN is a frame without detection (the limit of an
 * infinite localisation error at that row, as extrack_loglik_gaps), and the bucket's len is the frame span.  At such a row the sequences
 * are expanded by the new state and take its transition factor, but no Gaussian factor; the mean stays and the variance is carried
 * unreduced; a ranking key drops the predictive density of a missed next frame.  The state histories keep one digit per frame and run
 * lengths are counted in frames, missed ones included; min_len, isBL and the stay-in-field-of-view terms follow from len as above.  The
 * per-peak error of a gap row is never read (NaN allowed).  The first and the last row must be observed and a row is finite or NaN as a
 * whole: a track that breaks this, or has a NaN error at an observed row, makes the bucket's histogram NaN (as any NaN does in
 * extrack_segment_len_hist).  Same arguments, limits and error codes as extrack_segment_len_hist; gap-free data gives the same bits.
 * Inside a run of two or more missed frames distinct histories tie exactly; with pruning the order of such ties is decided by rounding
 * and, through the last-K quirk of the reference's LL terms, visible in the result. */
int extrack_segment_len_hist_gaps(extrack_ctx* ctx, const extrack_model* model, int32_t bucket_id, int32_t max_nb_states, double* hist);

/* Refined positions of one bucket (extrack/refined_localization.py:304-338 position_refinement -> get_pos_PDF :207 -> get_LC_Km_Ks :48):
 * mu host [n][len][dims], sigma host [n][len].  Two passes of the threshold-fusion recursion (merge decisions from the first 30
 * tracks of the bucket, fuse_tracks_th with per-track histories) - over the time-reversed tracks with model->TrMat and over the tracks
 * as they are with its transpose - record every position's surviving state sequences (mean, std, log-weight, newest state); for each
 * position the sequences of both passes that agree on its state are paired and the three Gaussians (prediction from the future,
 * localisation, prediction from the past) multiplied; mu / sigma are the probability-weighted mean / root mean variance of the pairs.
 * model: n_states, ds, TrMat, Fs (position 0 only, through a quirk of the reference), locerr[0] (one global error: locerr_mode 0,
 * locerr_dims 1), frame_len; nb_substeps must be 1; p_stay / pBL / min_len / max_len are not used.  Tracks need >= 3 positions. */
int extrack_refine_positions(extrack_ctx* ctx, const extrack_model* model, int32_t bucket_id, double threshold, int32_t max_nb_states,
                             double* mu, double* sigma);

/* The mixture extrack_refine_positions reads out, as get_pos_PDF returns it (extrack/refined_localization.py:207-298: all_pos_means,
 * all_pos_stds, all_pos_weights).  counts host [len]: components of every position, in the reference's order (end positions: the
 * sequences of the pass's last record; between: for every state, sequences from the future x sequences from the past that agree on it).
 * With cum[k] = counts[0] + ... + counts[k - 1], component j of position k of track x is means[((cum[k] + j) * n + x) * dims + d],
 * stds / logw[(cum[k] + j) * n + x] (host; `capacity` = rows each array holds >= the sum of the counts).  means == NULL: counts only
 * (the sizing call).  Same model fields and limits as extrack_refine_positions; the bucket's records must fit one row block
 * (EXTRACK_REFINE_BUDGET_MB), EXTRACK_E_UNSUPPORTED otherwise - the components of a large bucket are not meant to leave the GPU. */
int extrack_refine_pos_pdf(extrack_ctx* ctx, const extrack_model* model, int32_t bucket_id, double threshold, int32_t max_nb_states,
                           int32_t* counts, int64_t capacity, double* means, double* stds, double* logw);

/* Positions of one bucket refined along a given state path (fixed-state smoother, csrc/xt_cond.h): states host [n][len] (int8, the state
 * of every position, as extrack_map_states writes them), mu host [n][len][dims], sigma host [n][len][K] with K = 1 (one error for all
 * dimensions) or dims (locerr_dims = dims, or per-peak errors uploaded per dimension), logdens host [n] or NULL.  Model of one track, per
 * dimension: flat prior on the first real position, real steps N(0, q[t]) with q[t] = (ds[b[t]]^2 + ds[b[t+1]]^2) / 2 - the step variance
 * of the likelihood's tables -, observations N(real position, error^2) with the error of locerr_mode 0 / 1 / 2.  mu / sigma: posterior mean
 * and standard deviation of every real position given the whole track and the path; logdens: log density of the len - 1 observed
 * displacements given the path (the path's own prior - Fs, TrMat, p_stay, pBL - is not part of it, and none of those fields is read;
 * frame_len, min_len, max_len are not used either).  Any n_states in 2..8, dims 1..3, every track length.  A track with a NaN position or
 * error, or with a negative state (extrack_map_states writes -1 for such tracks), is NaN in all three outputs.  Decided on the host,
 * nothing launched: EXTRACK_E_INVALID for nb_substeps != 1 and for a state >= n_states anywhere; EXTRACK_E_UNSUPPORTED for buckets with
 * per-track time steps.  Rows of 64 tracks live in LDS while they fit a CU, else in mu / sigma themselves (EXTRACK_COND_WS=global forces
 * that; extrack_last_launch_info then reports the LDS bytes of the step-variance table alone, 8 * n_states^2 rounded up to 16); both give
 * the same bits.  extrack_last_kernel_ms and extrack_last_launch_info cover the launch. */
int extrack_refine_fixed_states(extrack_ctx* ctx, const extrack_model* model, int32_t bucket_id, const int8_t* states, double* mu,
                                double* sigma, double* logdens);

/* extrack_refine_fixed_states for tracks with missed detections (all-NaN rows, as extrack_loglik_gaps defines them): such a row is an
 * observation of infinite error.  mu / sigma at the row are the interpolated posterior of the real position there (given the states of
 * the row and its neighbours, as everywhere); logdens is the log density of the displacements between consecutive OBSERVED positions
 * given the path, constant -(n_observed - 1) * dims / 2 * log(2 pi).  The position and the per-peak error of a gap row are never read.
 * NaN in all three outputs: a NaN first or last row, a row with only some NaN coordinates, a NaN error at an observed row, a negative
 * state anywhere (gap rows included).  Same launch path, placements and refusals as extrack_refine_fixed_states, except that
 * nb_substeps != 1 is EXTRACK_E_UNSUPPORTED here (as in extrack_loglik_gaps); gap-free data gives the same bits. */
int extrack_refine_fixed_states_gaps(extrack_ctx* ctx, const extrack_model* model, int32_t bucket_id, const int8_t* states, double* mu,
                                     double* sigma, double* logdens);

/* Threshold-fusion log-likelihood (the kernel extrack.tracking.param_fitting / cum_Proba_Cs call in v1.6.3,
 * extrack/tracking.py:427-743).  Which state sequences are merged at a step is decided from the first 30 tracks
 * of every chunk of `chunk` consecutive tracks of a bucket (tracking.py:678-679; cum_Proba_Cs uses chunk = 2000,
 * tracking.py:1043) and applied to the whole chunk, so the value depends on `chunk` and on the track order.
 * model->frame_len is the number of most recent states whose equality forces a merge; threshold and
 * max_nb_states as in tracking.py:427 (threshold is multiplied by 1.2 at every step with more than
 * max_nb_states live sequences).  Time steps: fixed (in model->ds) or per track (extrack_set_bucket_dt).
 * total_ll / per_track as in extrack_loglik.  Limit: 32 768 expanded sequences (live sequences x n_states^nb_substeps) at any step
 * (EXTRACK_E_UNSUPPORTED beyond; 8192 for extrack_predict_th / extrack_refine_positions). */
int extrack_loglik_th(extrack_ctx* ctx, const extrack_model* model, double threshold, int32_t max_nb_states, int32_t chunk,
                      double* total_ll, double* per_track);
/* Same evaluation, the scalar left in device memory (d_total_ll, 8 bytes) for a following RCCL all-reduce on the context's
 * stream; nothing is copied back to the host at the end (counterpart of extrack_loglik_async for the threshold-fusion kernel). */
int extrack_loglik_th_async(extrack_ctx* ctx, const extrack_model* model, double threshold, int32_t max_nb_states, int32_t chunk,
                            double* d_total_ll);
/* Threshold-fusion state posteriors of one bucket (P_Cs_inter_bound_stats_th(..., do_preds=1), extrack/tracking.py:427-650,
 * driven as predict_Bs drives it, tracking.py:792-906): preds host [n][len][S].  The bucket is cut into chunks of nb_max
 * consecutive tracks (predict_Bs default: 1, i.e. every track decides its own merges); with nb_max > 30 the first 30 tracks of a
 * chunk decide the merges (tracking.py:676-691) and the others follow them with their own merge weights (tracking.py:703-741).
 * model->nb_substeps must be 1 (tracking.py:839). */
int extrack_predict_th(extrack_ctx* ctx, const extrack_model* model, int32_t bucket_id, double threshold, int32_t max_nb_states,
                       int32_t nb_max, double* preds);

/* Diagnostic: merge groups of the last extrack_loglik_th call for chunk `chunk_index` of a bucket at step t
 * (t = 1 .. len-1; merges happen for t < len-1).  n_expanded = sequences before the merge, n_groups = after
 * (0 when the step has no merge).  members[0..n_expanded) are the expanded sequence indices sorted by group,
 * gstart[0..n_groups] the group boundaries; both may be NULL; cap = capacity of both arrays in elements. */
int extrack_th_plan_step(extrack_ctx* ctx, int32_t bucket_id, int64_t chunk_index, int32_t t, int32_t* n_expanded,
                         int32_t* n_groups, uint16_t* members, uint16_t* gstart, int32_t cap);

/* Device time (ms, HIP events on the context's stream) spent in the track kernels of the last
 * extrack_loglik / extrack_loglik_async / extrack_predict call (valid after the stream is idle). */
int extrack_last_kernel_ms(extrack_ctx* ctx, float* ms);
/* Launch geometry of the last track kernel: info[0] blocks, [1] threads/block, [2] LDS bytes/block,
 * [3] tracks/block, [4] occupancy (blocks/CU), [5] compute units. */
int extrack_last_launch_info(const extrack_ctx* ctx, int32_t info[6]);
/* Kernel family of the last launch group of extrack_loglik* / extrack_predict* / extrack_sequence_matrix (XtLlPath, csrc/xt_ll_geom.h):
 * 1 register-resident 2-state, 2 LDS-resident 2-state, 3 entry-parallel, 4 general, 5 general with missed detections, 6 global-state,
 * 7 register-resident 2-state with missed detections; 0 before any launch. */
int extrack_last_ll_path(const extrack_ctx* ctx, int32_t* path);
/* Kernel family of the last launch group of extrack_loglik_grad* / extrack_loglik_scores* (XtGradPath, csrc/xt_grad_geom.h): 1 reverse mode,
 * 2 register-resident 2-state, 3 registers + LDS exchange (xt_gradr.h), 4 LDS-resident (xt_grad.h), 5 register-resident 2-state with missed
 * detections (a two-state _gaps launch with one global localisation error, frame_len 5..7, or 4 under EXTRACK_GAP_REG2_F;
 * EXTRACK_GRAD_PATH=gradr | lds keep the general gap kernels), 6 reverse mode with missed detections (a _gaps gradient launch whose gap-free
 * twin would run reverse mode); 0 before any launch.  A call without directions runs the likelihood kernels and
 * leaves the value as it was. */
int extrack_last_grad_path(const extrack_ctx* ctx, int32_t* path);

/* Host helper: p_stay table (extrack/tracking.py:182-191).  out has S^ns entries. */
int extrack_p_stay_table(const double* ds, int32_t n_states, int32_t nb_substeps, const double* cell_dims,
                         int32_t n_cell_dims, double* out);

/* ---- one process, several GPUs -------------------------------------------------------------------------------------------------------
 * The reference parallelises with multiprocessing.Pool.map over track chunks and sums the per-chunk results (extrack/tracking.py:1061-1069).
 * A host without torch.distributed (option B) drives all the GPUs of a node from one thread through these entry points:
 * every device keeps a contiguous row range of every uploaded bucket, an evaluation runs the likelihood kernel on all devices at once and ends
 * with ONE all-reduce of the scalar over RCCL / xGMI (ncclCommInitAll over the listed devices at creation, ncclAllReduce(sum, double, 1) per
 * evaluation).  use_rccl: 0 = sum the per-device totals on the host; 1 = RCCL when librccl.so can be loaded (at run time, no link-time
 * dependency) and the devices are distinct, else the host sum; 2 = RCCL or EXTRACK_E_UNSUPPORTED.  The multi-PROCESS form of the same
 * partitioning (one rank per GPU, torch.distributed) is extrack_amd/distributed.py. */
typedef struct extrack_multi extrack_multi;
int extrack_multi_create(int32_t n_devices, const int32_t* device_ids, int32_t use_rccl, extrack_multi** out);
void extrack_multi_destroy(extrack_multi* m);
const char* extrack_multi_last_error(const extrack_multi* m);
int32_t extrack_multi_device_count(const extrack_multi* m);
int32_t extrack_multi_uses_rccl(const extrack_multi* m);
/* The per-device context i (owned by m): for the single-device entry points above on one shard, e.g. extrack_predict. */
extrack_ctx* extrack_multi_context(extrack_multi* m, int32_t i);
/* One length bucket, host [n][len][dims] (+ per-peak errors): device r receives the rows [r n / w, (r + 1) n / w) (balanced to one row). */
int extrack_multi_upload_bucket(extrack_multi* m, const double* tracks, int64_t n, int32_t len, int32_t dims, const double* sigma,
                                int32_t sigma_dims);
int extrack_multi_clear_buckets(extrack_multi* m);
/* sum(LL) over all buckets on all devices (as extrack_loglik; model->min_len / max_len are the dataset-global values). */
int extrack_multi_loglik(extrack_multi* m, const extrack_model* model, double* total_ll);

#ifdef __cplusplus
}
#endif
#endif /* EXTRACK_HIP_H */
