// libextrack_hip.so, translation unit: position refinement (extrack/refined_localization.py:207-338) behind extrack_refine_positions /
// extrack_refine_pos_pdf - two recording passes of the prediction-mode plan kernel (xt_th.h, refine mode; launched through
// xt_th_launch_predict of extrack_th.hip) + the combination of the "future" and "past" predictions of every position.
#include "xt_host.h"

struct XtRefineArgs {
    const double* tracks;  // [N][L][D] original time order (rows of this launch)
    const double* fut;     // records of the pass over the time-reversed track: entry e = state after positions L-1 .. L-1-e
    const double* past;    // records of the pass over the track as it is:      entry e = state after positions 0 .. e
    const uint8_t* fut_new;
    const uint8_t* past_new;
    const int32_t* fut_cnt;
    const int32_t* past_cnt;
    double* mu_out;        // [N][L][D]
    double* sig_out;       // [N][L]
    int64_t N;             // rows of this launch (the records are [L - 1][cap][2 + D][N]: a wavefront reads 64 neighbouring tracks' values of a field)
    int32_t L, S, cap_f, cap_p;  // sequences recorded per (entry, track) by the two passes
    double l2;             // squared localisation error (global), or
    const double* sigma;   // per-peak localisation errors [N][L] of these rows (nullptr: the global one)
    double logF[XT_MAX_STATES];
    // the mixture itself (get_pos_PDF's return values, refined_localization.py:298), xt_refine_components only: component j of position k at
    // row comp_off[k] + j of means [.][N][D], stds [.][N], logw [.][N]
    const int64_t* comp_off;
    double* comp_mean;
    double* comp_std;
    double* comp_logw;
};

// One thread per (track, position): softmax-weighted mean of the pair means / root mean of the pair variances
// (refined_localization.py:222-298 get_pos_PDF + :329-337).  ONE sweep over the pairs with a running maximum of the log-weights (the sums
// are rescaled when it grows): every record is read once.  Adjacent threads serve adjacent tracks of the same position, so a wavefront
// walks 64 neighbouring record rows.
template <int D>
__global__ void __launch_bounds__(256) xt_refine_combine(XtRefineArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N * a.L) return;
    const int k = (int)(i / a.N);
    const int64_t x = i - (int64_t)k * a.N;
    const int L = a.L, R = 2 + D;
    double c[D];
    for (int d = 0; d < D; ++d) c[d] = a.tracks[(x * L + k) * D + d];
    // this position's own localisation variance (get_pos_PDF, refined_localization.py:222, 271, 289).  Per-peak errors: the in-place update
    // of the last record inside get_LC_Km_Ks (:186-193) takes the error of index len - 1 of the array it was given - for position 0 (pass
    // over the unreversed array) that is the LAST position's error, reproduced as it is; for position len - 1 it is its own
    const double l2k = a.sigma ? a.sigma[x * L + k] * a.sigma[x * L + k] : a.l2;
    const double l2q = a.sigma ? a.sigma[x * L + (L - 1)] * a.sigma[x * L + (L - 1)] : a.l2;
    double wmax = -INFINITY, sw = 0.0, smu[D], ssg = 0.0;
    for (int d = 0; d < D; ++d) smu[d] = 0.0;
    auto add = [&](double w, const double* mu, double var) {
        if (w > wmax) {  // rescale what has been summed to the new maximum (exp(-inf) = 0 the first time, when the sums are 0 anyway)
            const double sc = exp(wmax - w);
            sw *= sc;
            ssg *= sc;
            for (int d = 0; d < D; ++d) smu[d] *= sc;
            wmax = w;
        }
        const double p = exp(w - wmax);
        sw += p;
        for (int d = 0; d < D; ++d) smu[d] += p * mu[d];
        ssg += p * var;
    };
    // record field f of sequence q of entry e of this thread's track: rec[((e * cap + q) * R + f) * N + x]
    if (k == 0 || k == L - 1) {
        // end positions: one pass only; the reference's last record already carries the density of this position (and the
        // initial fractions for position 0) through its in-place update (refined_localization.py:188-193), and get_pos_PDF adds the
        // overlap term once more
        const int cap = k == 0 ? a.cap_f : a.cap_p;
        const double* rec = (k == 0 ? a.fut : a.past) + ((int64_t)(L - 2) * cap * R) * a.N + x;
        const uint8_t* nw = (k == 0 ? a.fut_new : a.past_new) + (int64_t)(L - 2) * cap;
        const int n = (k == 0 ? a.fut_cnt : a.past_cnt)[L - 2];
        for (int q = 0; q < n; ++q) {
            const double* r = rec + (int64_t)q * R * a.N;
            const double lp = r[0], sd = r[(int64_t)(1 + D) * a.N], v = sd * sd + l2k, vq = sd * sd + l2q;
            double dsq = 0.0, mu[D];
            for (int d = 0; d < D; ++d) {
                const double m = r[(int64_t)(1 + d) * a.N];
                dsq += (c[d] - m) * (c[d] - m);
                mu[d] = (m * l2k + c[d] * sd * sd) / v;
            }
            const double lk = -0.5 * D * log(2.0 * M_PI * v) - dsq / (2.0 * v);       // get_pos_PDF's overlap term
            const double lkq = -0.5 * D * log(2.0 * M_PI * vq) - dsq / (2.0 * vq);    // the in-place update of the last record
            add(lp + lk + lkq + (k == 0 ? a.logF[nw[q]] : 0.0), mu, l2k * sd * sd / v);
        }
    } else {
        const double* rf = a.fut + ((int64_t)(L - 2 - k) * a.cap_f * R) * a.N + x;
        const double* rp = a.past + ((int64_t)(k - 1) * a.cap_p * R) * a.N + x;
        const uint8_t* nf = a.fut_new + (int64_t)(L - 2 - k) * a.cap_f;
        const uint8_t* np_ = a.past_new + (int64_t)(k - 1) * a.cap_p;
        const int n1 = a.fut_cnt[L - 2 - k], n2 = a.past_cnt[k - 1];
        for (int q1 = 0; q1 < n1; ++q1) {
            const double* r1 = rf + (int64_t)q1 * R * a.N;
            const double lp1 = r1[0], s1 = r1[(int64_t)(1 + D) * a.N];
            const double v12 = s1 * s1 + l2k, vA = s1 * s1 * l2k / v12;
            double muA[D], d1 = 0.0;
            for (int d = 0; d < D; ++d) {
                const double m1 = r1[(int64_t)(1 + d) * a.N];
                muA[d] = (m1 * l2k + c[d] * s1 * s1) / v12;
                d1 += (m1 - c[d]) * (m1 - c[d]);
            }
            const double lk1 = -0.5 * D * log(2.0 * M_PI * v12) - d1 / (2.0 * v12);
            for (int q2 = 0; q2 < n2; ++q2) {
                if (np_[q2] != nf[q1]) continue;  // pairs that agree on the state at this position
                const double* r2 = rp + (int64_t)q2 * R * a.N;
                const double s3 = r2[(int64_t)(1 + D) * a.N], v3 = vA + s3 * s3;
                double d2 = 0.0, mu[D];
                for (int d = 0; d < D; ++d) {
                    const double m3 = r2[(int64_t)(1 + d) * a.N];
                    d2 += (muA[d] - m3) * (muA[d] - m3);
                    mu[d] = (muA[d] * s3 * s3 + m3 * vA) / v3;
                }
                add(lp1 + r2[0] + lk1 - 0.5 * D * log(2.0 * M_PI * v3) - d2 / (2.0 * v3), mu, vA * s3 * s3 / v3);
            }
        }
    }
    for (int d = 0; d < D; ++d) a.mu_out[(x * L + k) * D + d] = smu[d] / sw;
    a.sig_out[x * L + k] = sqrt(ssg / sw);
}

// The Gaussian mixture of every position as the reference returns it from get_pos_PDF (refined_localization.py:207-298): same pair walk as
// xt_refine_combine, in the reference's component order - end positions: the sequences of the pass's last record; positions between: for
// every state s, (sequences from the future whose state at this position is s) x (sequences from the past with state s), the former outer.
// For inspection of small inputs (every component of every track goes through HBM); the refinement proper never materialises them.
template <int D>
__global__ void __launch_bounds__(256) xt_refine_components(XtRefineArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.N * a.L) return;
    const int k = (int)(i / a.N);
    const int64_t x = i - (int64_t)k * a.N;
    const int L = a.L, R = 2 + D;
    double c[D];
    for (int d = 0; d < D; ++d) c[d] = a.tracks[(x * L + k) * D + d];
    const double l2k = a.sigma ? a.sigma[x * L + k] * a.sigma[x * L + k] : a.l2;
    const double l2q = a.sigma ? a.sigma[x * L + (L - 1)] * a.sigma[x * L + (L - 1)] : a.l2;
    int64_t row = a.comp_off[k];
    // the recording kernel keeps the -dims/2 log(2 pi) of every integration step out of the weights (the likelihood kernels add them once per
    // track): the records this position combines went through len - 2 (end positions) or len - 3 steps together
    const double wconst = -0.5 * D * log(2.0 * M_PI) * (double)((k == 0 || k == L - 1) ? L - 2 : L - 3);
    auto put = [&](double w, const double* mu, double var) {
        for (int d = 0; d < D; ++d) a.comp_mean[(row * a.N + x) * D + d] = mu[d];
        a.comp_std[row * a.N + x] = sqrt(var);
        a.comp_logw[row * a.N + x] = w + wconst;
        ++row;
    };
    if (k == 0 || k == L - 1) {
        const int cap = k == 0 ? a.cap_f : a.cap_p;
        const double* rec = (k == 0 ? a.fut : a.past) + ((int64_t)(L - 2) * cap * R) * a.N + x;
        const uint8_t* nw = (k == 0 ? a.fut_new : a.past_new) + (int64_t)(L - 2) * cap;
        const int n = (k == 0 ? a.fut_cnt : a.past_cnt)[L - 2];
        for (int q = 0; q < n; ++q) {
            const double* r = rec + (int64_t)q * R * a.N;
            const double lp = r[0], sd = r[(int64_t)(1 + D) * a.N], v = sd * sd + l2k, vq = sd * sd + l2q;
            double dsq = 0.0, mu[D];
            for (int d = 0; d < D; ++d) {
                const double m = r[(int64_t)(1 + d) * a.N];
                dsq += (c[d] - m) * (c[d] - m);
                mu[d] = (m * l2k + c[d] * sd * sd) / v;
            }
            const double lk = -0.5 * D * log(2.0 * M_PI * v) - dsq / (2.0 * v);
            const double lkq = -0.5 * D * log(2.0 * M_PI * vq) - dsq / (2.0 * vq);
            // the pass from the past runs with neutral initial fractions 1 / S (refined_localization.py:216): a constant the read-out cancels
            put(lp + lk + lkq + (k == 0 ? a.logF[nw[q]] : -log((double)a.S)), mu, l2k * sd * sd / v);
        }
    } else {
        const double* rf = a.fut + ((int64_t)(L - 2 - k) * a.cap_f * R) * a.N + x;
        const double* rp = a.past + ((int64_t)(k - 1) * a.cap_p * R) * a.N + x;
        const uint8_t* nf = a.fut_new + (int64_t)(L - 2 - k) * a.cap_f;
        const uint8_t* np_ = a.past_new + (int64_t)(k - 1) * a.cap_p;
        const int n1 = a.fut_cnt[L - 2 - k], n2 = a.past_cnt[k - 1];
        for (int st = 0; st < a.S; ++st)
            for (int q1 = 0; q1 < n1; ++q1) {
                if (nf[q1] != st) continue;
                const double* r1 = rf + (int64_t)q1 * R * a.N;
                const double lp1 = r1[0], s1 = r1[(int64_t)(1 + D) * a.N];
                const double v12 = s1 * s1 + l2k, vA = s1 * s1 * l2k / v12;
                double muA[D], d1 = 0.0;
                for (int d = 0; d < D; ++d) {
                    const double m1 = r1[(int64_t)(1 + d) * a.N];
                    muA[d] = (m1 * l2k + c[d] * s1 * s1) / v12;
                    d1 += (m1 - c[d]) * (m1 - c[d]);
                }
                const double lk1 = -0.5 * D * log(2.0 * M_PI * v12) - d1 / (2.0 * v12);
                for (int q2 = 0; q2 < n2; ++q2) {
                    if (np_[q2] != st) continue;
                    const double* r2 = rp + (int64_t)q2 * R * a.N;
                    const double s3 = r2[(int64_t)(1 + D) * a.N], v3 = vA + s3 * s3;
                    double d2 = 0.0, mu[D];
                    for (int d = 0; d < D; ++d) {
                        const double m3 = r2[(int64_t)(1 + d) * a.N];
                        d2 += (muA[d] - m3) * (muA[d] - m3);
                        mu[d] = (muA[d] * s3 * s3 + m3 * vA) / v3;
                    }
                    put(lp1 + r2[0] + lk1 - 0.5 * D * log(2.0 * M_PI * v3) - d2 / (2.0 * v3), mu, vA * s3 * s3 / v3);
                }
            }
    }
}

// Time-reversed copy of a bucket [N][L][D] on the device (the pass "from the future" walks the track backwards).
__global__ void __launch_bounds__(256) xt_reverse_tracks(const double* __restrict__ src, double* __restrict__ dst, int64_t N, int L, int D)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= N * L * D) return;
    const int64_t x = i / ((int64_t)L * D);
    const int r = (int)(i - x * L * D), p = r / D, d = r - p * D;
    dst[i] = src[(x * L + (L - 1 - p)) * D + d];
}

// Grow-only device buffers of the refinement path, kept in the context between calls: a hipMalloc / hipFree pair per record array and
// call cost more than the kernels (r02: 0.25 s wall for 30 ms of kernels on 1e5 x 30).
static int xt_rf_reserve(extrack_ctx* ctx, int slot, size_t bytes)
{
    const std::string what = "refinement buffer (" + std::to_string(bytes >> 20) + " MiB)";
    return xt_grow_device(ctx, &ctx->rf_buf[slot], &ctx->rf_cap_bytes[slot], bytes, what.c_str());
}
enum { XT_RF_REV = 0, XT_RF_REC0, XT_RF_REC1, XT_RF_NEW0, XT_RF_NEW1, XT_RF_CNT0, XT_RF_CNT1, XT_RF_MU, XT_RF_SIG, XT_RF_STATUS };

// One launch of the recording kernel over bucket `d_tracks` ([N][L][D] on the device).  rows == 0: capacity probe on the pilot tracks
// (nothing recorded; *cap_out = sequences to record per entry); else: the tracks [row0, row0 + rows) are recorded into a.rf_out.
static int xt_refine_launch(extrack_ctx* ctx, const extrack_model* m, const double* d_tracks, const double* d_sigma, int64_t N, int L, int D, double threshold,
                            int32_t max_nb_states, int64_t row0, int64_t rows, int rf_cap, double* d_rec, uint8_t* d_new, int32_t* d_cnt, int* cap_out)
{
    const int S = m->n_states, F = m->frame_len, G = S;
    XtThArgs a;
    memset(&a, 0, sizeof(a));
    a.tracks = d_tracks;
    a.blob = ctx->d_blob;
    a.L = L;
    a.S = S;
    a.NS = 1;
    a.G = G;
    a.F = F;
    a.isBL = 0;
    a.min_len = L + 2;  // no field-of-view / bleaching factors in the recorded weights
    a.sigma = d_sigma;  // per-peak errors [N][L][1], read at the SAME index as the position of d_tracks (see extrack_refine_positions)
    a.locerr_mode = d_sigma ? 1 : 0;
    a.KS = 1;
    a.max_nb = max_nb_states;
    a.threshold = threshold;
    a.pcap = (int)std::min<int64_t>(N, XT_TH_PILOT);
    a.pair_lanes_max_p = ctx->th_pair_lanes;
    a.refine = 1;
    int rc = xt_rf_reserve(ctx, XT_RF_STATUS, 4 * sizeof(int32_t));
    if (rc) return rc;
    int32_t* d_status = (int32_t*)ctx->rf_buf[XT_RF_STATUS];
    a.status = d_status;
    const bool probe = rows == 0;
    if (!probe) {
        a.rf_cap = rf_cap;
        a.rf_out = d_rec;
        a.rf_new = d_new;
        a.rf_cnt = d_cnt;
        a.rf_row0 = row0;
        a.rf_rows = rows;
    }
    hipError_t e = hipSuccess;
    for (;;) {
        int capE = ctx->th_capE;
        while (capE < S * G) capE *= 2;
        ctx->th_capE = capE;
        a.capE = a.wsP = a.wsE = capE;
        a.ws_lds = 0;
        a.N = probe ? std::min<int64_t>(N, XT_TH_PILOT) : N;
        a.chunk = (int32_t)std::min<int64_t>(a.N, (int64_t)1 << 30);
        a.nchunks = 1;
        a.cmat_words = 0;
        const int64_t first = std::max<int64_t>(row0, a.pcap), last = std::min<int64_t>(N, row0 + rows);
        const int64_t nbatch = (!probe && last > first) ? (last - first + a.pcap - 1) / a.pcap : 0;
        const int grid = probe ? 1 : (int)std::max<int64_t>(1, std::min<int64_t>(nbatch, (int64_t)ctx->n_cu * xt_th_pred_waves(S)));
        const size_t lds = (size_t)xt_th_plan_lds_doubles(S, G, capE, D, 1) * sizeof(double);
        a.ws_stride = xt_th_hist_doubles(a.wsE, a.pcap, true, L) + xt_th_ws_doubles(a.wsP, a.wsE, D, 1, F, 1, S, a.pcap, true);
        extrack_ctx::ThSlot& sl = ctx->th_slot[0];  // the plan kernel's workspace
        if ((rc = xt_grow_device(ctx, (void**)&sl.d_ws, &sl.ws_cap, (size_t)a.ws_stride * grid * sizeof(double), "refinement workspace"))) return rc;
        a.ws = sl.d_ws;
        if (lds > 160 * 1024) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "plan tables do not fit the 160 KiB LDS of a CU");
        e = xt_th_launch_predict(ctx, a, D, 1, grid, 256, lds);
        int32_t st[4] = {0, 0, 0, 0};
        if (e == hipSuccess) e = hipMemcpyAsync(st, d_status, sizeof(st), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return xt_fail(ctx, EXTRACK_E_HIP, std::string("refinement pass: ") + hipGetErrorString(e));
        if (st[0]) {  // capacity overflow: grow and repeat
            int ncap = capE;
            while (ncap < std::max(st[1], st[2])) ncap *= 2;
            if (ncap == capE) ncap *= 2;
            if (ncap > XT_TH_MAXCAP)
                return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "more than 8192 live state sequences per step (threshold fusion expands every sequence by n_states^nb_substeps before it merges): raise threshold, lower max_nb_states or nb_substeps - or use the fixed-window kernel (fusion='window' / extrack_loglik), which serves this model");
            ctx->th_capE = ncap;
            continue;
        }
        if (cap_out) *cap_out = std::max(std::max(st[1], st[2]), S * G);
        return EXTRACK_OK;
    }
}

// Request for the mixture components (extrack_refine_pos_pdf); nullptr: the refined positions only.
struct XtPdfOut {
    int32_t* counts;   // [L] components per position (always filled)
    int64_t capacity;  // rows the three arrays below hold
    double* means;     // nullptr: counts only
    double* stds;
    double* logw;
};

static int xt_refine_run(extrack_ctx* ctx, const extrack_model* m, int32_t bucket_id, double threshold, int32_t max_nb_states, double* mu, double* sigma,
                         const XtPdfOut* pdf)
{
    int rc = xt_validate_model(ctx, m);
    if (rc) return rc;
    if (bucket_id < 0 || bucket_id >= (int)ctx->buckets.size()) return xt_fail(ctx, EXTRACK_E_INVALID, "bucket id out of range");
    if (m->nb_substeps != 1) return xt_fail(ctx, EXTRACK_E_INVALID, "position refinement is defined for nb_substeps == 1");
    if (m->locerr_mode == 2 || (m->locerr_mode == 0 && m->locerr_dims != 1))
        return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "position refinement takes one global localisation error or per-peak errors [n][len][1] (what the reference's reshapes carry through)");
    if (!(threshold >= 0.0)) return xt_fail(ctx, EXTRACK_E_INVALID, "threshold must be >= 0");
    if (m->frame_len <= 1 || m->frame_len > 15) return xt_fail(ctx, EXTRACK_E_INVALID, "frame_len must be in (1, 15]");
    XtBucket& b = ctx->buckets[bucket_id];
    const int S = m->n_states, L = b.L, D = b.D, R = 2 + D;
    if (L < 2) return xt_fail(ctx, EXTRACK_E_INVALID, "position refinement needs tracks of at least 2 positions");
    if (m->locerr_mode == 1 && (!b.d_sigma || b.KS != 1))
        return xt_fail(ctx, EXTRACK_E_INVALID, "position refinement with per-peak errors needs the bucket's sigma [n][len][1]");
    // Per-peak errors (refined_localization.py:59-70): get_LC_Km_Ks reverses the error array but walks an UNREVERSED track from its end, so the
    // k-th position it injects meets the error of index k counted from the START of the array it was given - the same array in both passes
    // (:211, :216).  Here both passes walk their track from index 0, the pass "from the future" on the time-reversed copy: handing BOTH the
    // bucket's sigma as it is reproduces exactly that pairing (mirrored errors in the pass from the future, the right ones from the past).
    const double* d_sig_in = m->locerr_mode == 1 ? b.d_sigma : nullptr;
    XT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nel = (size_t)b.N * L * D;
    // time-reversed copy of the bucket for the pass "from the future", made on the device
    if ((rc = xt_rf_reserve(ctx, XT_RF_REV, nel * sizeof(double)))) return rc;
    double* d_rev = (double*)ctx->rf_buf[XT_RF_REV];
    hipLaunchKernelGGL(xt_reverse_tracks, dim3((unsigned)((nel + 255) / 256)), dim3(256), 0, ctx->stream, b.d_tracks, d_rev, b.N, L, D);
    XT_HIP(ctx, hipGetLastError());
    // pass 0: from the future (reversed track, the matrix as given, refined_localization.py:211); pass 1: from the past (track as it is,
    // transposed matrix, :213-216).  No initial fractions in the recorded weights (:93).
    std::vector<double> ones(S, 1.0), Tt((size_t)S * S);
    for (int i = 0; i < S; ++i)
        for (int j = 0; j < S; ++j) Tt[(size_t)i * S + j] = m->TrMat[(size_t)j * S + i];
    std::vector<double> blobs[2];
    for (int pass = 0; pass < 2; ++pass) {
        XtModelHost mh;
        xt_model_host(m, mh);
        mh.Fs = ones.data();
        mh.TrMat = pass == 0 ? m->TrMat : Tt.data();
        int G = 0;
        std::string err = xt_th_build_blob(mh, blobs[pass], G);
        if (!err.empty()) return xt_fail(ctx, EXTRACK_E_INVALID, err);
    }
    const double* src[2] = {d_rev, b.d_tracks};
    // capacity probes on the pilot tracks: sequences to record per entry of either pass
    int cap[2] = {0, 0};
    for (int pass = 0; pass < 2; ++pass) {
        if ((rc = xt_upload_blob(ctx, blobs[pass]))) return rc;
        if ((rc = xt_refine_launch(ctx, m, src[pass], d_sig_in, b.N, L, D, threshold, max_nb_states, 0, 0, 0, nullptr, nullptr, nullptr, &cap[pass]))) return rc;
    }
    // row blocks: both passes' records of a block stay within the memory budget (EXTRACK_REFINE_BUDGET_MB, default 16 GiB of the 288 GB);
    // the merge plan only depends on the pilot tracks, which every launch re-walks, so the blocks are independent
    size_t budget = (size_t)16 << 30;
    if (const char* ev = getenv("EXTRACK_REFINE_BUDGET_MB")) {
        const long v = atol(ev);
        if (v >= 1) budget = (size_t)v << 20;
    }
    const size_t per_row = (size_t)(L - 1) * (size_t)(cap[0] + cap[1]) * R * sizeof(double);
    int64_t RB = (int64_t)std::max<size_t>(XT_TH_PILOT, budget / per_row);
    RB = std::min<int64_t>(RB, b.N);
    if (pdf && RB < b.N)
        return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "the mixture components are returned for buckets whose records fit ONE row block (EXTRACK_REFINE_BUDGET_MB, default 16 GiB): pass fewer tracks");
    for (int pass = 0; pass < 2; ++pass) {
        if ((rc = xt_rf_reserve(ctx, XT_RF_REC0 + pass, (size_t)(L - 1) * (size_t)RB * cap[pass] * R * sizeof(double)))) return rc;
        if ((rc = xt_rf_reserve(ctx, XT_RF_NEW0 + pass, (size_t)(L - 1) * cap[pass]))) return rc;
        if ((rc = xt_rf_reserve(ctx, XT_RF_CNT0 + pass, (size_t)(L - 1) * sizeof(int32_t)))) return rc;
    }
    if ((rc = xt_rf_reserve(ctx, XT_RF_MU, nel * sizeof(double)))) return rc;
    if ((rc = xt_rf_reserve(ctx, XT_RF_SIG, (size_t)b.N * L * sizeof(double)))) return rc;
    double* d_mu = (double*)ctx->rf_buf[XT_RF_MU];
    double* d_sig = (double*)ctx->rf_buf[XT_RF_SIG];
    XT_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    for (int64_t row0 = 0; row0 < b.N; row0 += RB) {
        const int64_t rows = std::min<int64_t>(RB, b.N - row0);
        for (int pass = 0; pass < 2; ++pass) {
            if ((rc = xt_upload_blob(ctx, blobs[pass]))) return rc;
            if ((rc = xt_refine_launch(ctx, m, src[pass], d_sig_in, b.N, L, D, threshold, max_nb_states, row0, rows, cap[pass], (double*)ctx->rf_buf[XT_RF_REC0 + pass],
                                       (uint8_t*)ctx->rf_buf[XT_RF_NEW0 + pass], (int32_t*)ctx->rf_buf[XT_RF_CNT0 + pass], nullptr)))
                return rc;
        }
        XtRefineArgs ra;
        memset(&ra, 0, sizeof(ra));
        ra.tracks = b.d_tracks + (size_t)row0 * L * D;
        ra.fut = (const double*)ctx->rf_buf[XT_RF_REC0];
        ra.past = (const double*)ctx->rf_buf[XT_RF_REC1];
        ra.fut_new = (const uint8_t*)ctx->rf_buf[XT_RF_NEW0];
        ra.past_new = (const uint8_t*)ctx->rf_buf[XT_RF_NEW1];
        ra.fut_cnt = (const int32_t*)ctx->rf_buf[XT_RF_CNT0];
        ra.past_cnt = (const int32_t*)ctx->rf_buf[XT_RF_CNT1];
        ra.mu_out = d_mu + (size_t)row0 * L * D;
        ra.sig_out = d_sig + (size_t)row0 * L;
        ra.N = rows;
        ra.L = L;
        ra.S = S;
        ra.cap_f = cap[0];
        ra.cap_p = cap[1];
        ra.l2 = m->locerr[0] * m->locerr[0];
        ra.sigma = d_sig_in ? d_sig_in + (size_t)row0 * L : nullptr;
        for (int s2 = 0; s2 < S; ++s2) ra.logF[s2] = log(m->Fs[s2]);
        const int grid = (int)(((int64_t)rows * L + 255) / 256);
        if (!pdf) {
            if (D == 1) hipLaunchKernelGGL(xt_refine_combine<1>, dim3(grid), dim3(256), 0, ctx->stream, ra);
            else if (D == 2) hipLaunchKernelGGL(xt_refine_combine<2>, dim3(grid), dim3(256), 0, ctx->stream, ra);
            else hipLaunchKernelGGL(xt_refine_combine<3>, dim3(grid), dim3(256), 0, ctx->stream, ra);
            XT_HIP(ctx, hipGetLastError());
            continue;
        }
        // ---- mixture components (one row block): count them on the host from the passes' plans, then one thread per (track, position)
        std::vector<int32_t> cnt[2];
        std::vector<uint8_t> nw[2];
        for (int pass = 0; pass < 2; ++pass) {
            cnt[pass].resize(L - 1);
            nw[pass].resize((size_t)(L - 1) * cap[pass]);
            XT_HIP(ctx, hipMemcpyAsync(cnt[pass].data(), ctx->rf_buf[XT_RF_CNT0 + pass], (size_t)(L - 1) * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
            XT_HIP(ctx, hipMemcpyAsync(nw[pass].data(), ctx->rf_buf[XT_RF_NEW0 + pass], nw[pass].size(), hipMemcpyDeviceToHost, ctx->stream));
        }
        XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        std::vector<int64_t> off(L + 1, 0);
        for (int k = 0; k < L; ++k) {
            int64_t n = 0;
            if (k == 0 || k == L - 1) {
                n = cnt[k == 0 ? 0 : 1][L - 2];
            } else {
                for (int st = 0; st < S; ++st) {
                    int64_t n1 = 0, n2 = 0;
                    for (int q = 0; q < cnt[0][L - 2 - k]; ++q) n1 += nw[0][(size_t)(L - 2 - k) * cap[0] + q] == st;
                    for (int q = 0; q < cnt[1][k - 1]; ++q) n2 += nw[1][(size_t)(k - 1) * cap[1] + q] == st;
                    n += n1 * n2;
                }
            }
            if (n > INT32_MAX) return xt_fail(ctx, EXTRACK_E_UNSUPPORTED, "too many mixture components at one position");
            pdf->counts[k] = (int32_t)n;
            off[k + 1] = off[k] + n;
        }
        if (!pdf->means) continue;
        if (off[L] > pdf->capacity) return xt_fail(ctx, EXTRACK_E_INVALID, "mixture component arrays too small (sum of the counts of a counts-only call)");
        const size_t rows_c = (size_t)off[L] * (size_t)rows;
        double* d_comp = nullptr;
        int64_t* d_off = nullptr;
        hipError_t e = hipMalloc(&d_comp, std::max<size_t>(rows_c, 1) * (D + 2) * sizeof(double));
        if (e == hipSuccess) e = hipMalloc(&d_off, (size_t)(L + 1) * sizeof(int64_t));
        if (e == hipSuccess) e = hipMemcpyAsync(d_off, off.data(), (size_t)(L + 1) * sizeof(int64_t), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) {
            ra.comp_off = d_off;
            ra.comp_mean = d_comp;
            ra.comp_std = d_comp + rows_c * D;
            ra.comp_logw = d_comp + rows_c * (D + 1);
            if (D == 1) hipLaunchKernelGGL(xt_refine_components<1>, dim3(grid), dim3(256), 0, ctx->stream, ra);
            else if (D == 2) hipLaunchKernelGGL(xt_refine_components<2>, dim3(grid), dim3(256), 0, ctx->stream, ra);
            else hipLaunchKernelGGL(xt_refine_components<3>, dim3(grid), dim3(256), 0, ctx->stream, ra);
            e = hipGetLastError();
        }
        if (e == hipSuccess && rows_c) e = hipMemcpyAsync(pdf->means, ra.comp_mean, rows_c * D * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && rows_c) e = hipMemcpyAsync(pdf->stds, ra.comp_std, rows_c * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && rows_c) e = hipMemcpyAsync(pdf->logw, ra.comp_logw, rows_c * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        (void)hipFree(d_comp);
        (void)hipFree(d_off);
        if (e != hipSuccess) return xt_fail(ctx, EXTRACK_E_HIP, std::string("mixture components: ") + hipGetErrorString(e));
    }
    XT_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    ctx->timed = true;
    if (!pdf) {
        XT_HIP(ctx, hipMemcpyAsync(mu, d_mu, nel * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        XT_HIP(ctx, hipMemcpyAsync(sigma, d_sig, (size_t)b.N * L * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    }
    XT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return EXTRACK_OK;
}

extern "C" int extrack_refine_positions(extrack_ctx* ctx, const extrack_model* m, int32_t bucket_id, double threshold, int32_t max_nb_states,
                                        double* mu, double* sigma)
{
    if (!ctx || !mu || !sigma) return xt_fail(ctx, EXTRACK_E_INVALID, "null argument");
    return xt_refine_run(ctx, m, bucket_id, threshold, max_nb_states, mu, sigma, nullptr);
}

extern "C" int extrack_refine_pos_pdf(extrack_ctx* ctx, const extrack_model* m, int32_t bucket_id, double threshold, int32_t max_nb_states,
                                      int32_t* counts, int64_t capacity, double* means, double* stds, double* logw)
{
    if (!ctx || !counts || capacity < 0 || (means && (!stds || !logw))) return xt_fail(ctx, EXTRACK_E_INVALID, "null argument");
    XtPdfOut pdf = {counts, capacity, means, stds, logw};
    return xt_refine_run(ctx, m, bucket_id, threshold, max_nb_states, nullptr, nullptr, &pdf);
}
