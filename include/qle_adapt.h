/*
 * qle_adapt.h -- adaptive tag-pose noise: every filter estimates its R_r / R_ang from its innovations, on the device
 * (libqle_adapt.so).
 *
 * qle_score.h, qle_bank.h and qle_imm.h answer "which tag-pose noise is right?" by enumeration over M hand-picked
 * candidates, at M filters per vehicle.  Here each filter estimates its own diagonal R from the innovations it already
 * forms, and the next tick uses the estimate.  Per tag tick, against the PREDICTED state (what qle_score.h evaluates):
 *     R_k = N diag(R) N^T,   n_k = the k-th column of the noise Jacobian N (EKF.cpp:462-472),
 *     S = G P G^T + R_k = L D L^T,   a_k = n_k^T S^-1 nu,   c_k = n_k^T S^-1 n_k   (one factorisation, seven forward solves),
 *     sample  r^_k = R_k + R_k^2 (a_k^2 - c_k),   k = 0..5  (r x, y, z, then theta x, y, z -- the entries of R_r, R_ang):
 * the E-step of EM for a diagonal measurement noise, E[n_k^2 | nu] = (R_k a_k)^2 + (R_k - R_k^2 c_k), non-negative in exact
 * arithmetic, with the fixed point E[a_k^2] = c_k, which holds exactly when S is the covariance of nu.  After `window` tag
 * ticks the M-step with forgetting,
 *     R_k <- clamp(R_k + gain (sum r^_k / n - R_k), R_lo[k], R_hi[k]),
 * evaluated in fp64 from the R_k the record holds and rounded once to the compute dtype, is stored into words 18..23 of
 * the filter's per-filter parameter record (qle_set_filter_params), which every tick kernel reads.
 *
 * What the estimate means: the R under which this filter's own model explains its innovations.  That is not the noise
 * of the sensor wherever the model is off (the linearisation, a mis-set Q, the reading of the angle-noise columns of N).
 *
 * Two kernels.  k_adapt_observe, one launch per observed tag tick: read-only on the state, the input records (it never
 * writes the mask word, so an observed run is the plain run until the first apply) and the parameter records; a
 * read-modify-write of the filter's accumulator record.  k_adapt_apply, one launch per window: writes the six R words
 * and resets the window of every filter with n >= n_min; a filter with n < n_min is not written at all and keeps its
 * open window.  One lane owns one filter: no atomics, the result is deterministic.
 *
 * The accumulators: acc[QAD_WORDS][padded_batch] doubles, plane-major (word w of filter i at acc[w * padded_batch + i]),
 * fp64 whatever the handle's dtype, zeroed by the caller before the first tick:
 *     0        n           scored ticks in the open window
 *     1        n_bad       the filter was on, but S was not positive definite, or NIS or a sample not finite
 *     2..7     sum of r^_k
 *     8..13    sum of a_k^2
 *     14..19   sum of c_k       (sum a_k^2 / sum c_k is 1 where the filter's R explains its innovations)
 *     20       n_total     scored ticks since the accumulators were zeroed
 *     21       windows     applies that wrote this filter
 *     22       n_rejected  the filter was on and scorable, but NIS > chi2_max
 *     23       zero
 * A filter is "on" at a tick when its mask word != 0 and it holds a state; it is "scored" when it is on, S is positive
 * definite, NIS and the six samples are finite and NIS <= chi2_max (+inf: no limit).  n_bad and n_rejected change no
 * other word; not on changes no word.  An apply zeroes words 0 and 2..19 of the filters it writes and increments word 21.
 *
 * Conventions: those of qle_score.h.  qad_observe_tick, qad_apply and qad_run are asynchronous on the handle's stream;
 * acc, applied and R_out are device pointers on its device.  Every call returns 0 or a negative error class of
 * qle_ekf.h; the message is in qad_last_error() (thread-local).  Every refusal is made before any GPU call: null or
 * misaligned pointers, a short struct_size, window < 1, gain outside (0, 1], n_min < 1, chi2_max NaN or <= 0, R_lo not
 * finite or <= 0, R_hi < R_lo, num_states against est_bias, a tick without a tag slot, params->multirate_ekf
 * (QLE_ERR_STATE, the gate's rule) and a view whose filter_params is NULL (QLE_ERR_STATE: per-filter parameters are
 * not in force -- qle_set_filter_params first, the estimate has nowhere else to go).  `params` are the qle_params the
 * handle was created with (the library links libqle_ekf.so for qle_params_derive, qle_run, qle_get_filter_params and the
 * two view calls).
 *
 * Not provided: adaptation of Q; multirate handles; a full (non-diagonal) R; per-filter bounds; adaptation inside
 * qle_run, qsq_run or qsc_run -- those keep their bits, qad_run is the sequence form.
 */
#ifndef QLE_ADAPT_H
#define QLE_ADAPT_H

#include "qle_ekf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QAD_WORDS 24 /* doubles per filter of an accumulator array */

typedef struct qad_config {
    uint32_t struct_size; /* sizeof(qad_config); a smaller value is refused                               */
    int32_t window;       /* qad_run: an apply after every window-th tag-slot tick of the call, >= 1       */
    double gain;          /* forgetting: in (0, 1]; 1 replaces R by the window's mean sample               */
    int32_t n_min;        /* a filter is applied when it scored at least n_min ticks in its window, >= 1   */
    int32_t reserved;
    double chi2_max;      /* qad_run: ticks with NIS above it are not scored (> 0; +inf: no limit)         */
    double R_lo[6];       /* bounds of the applied R, shared by the batch: finite, > 0                     */
    double R_hi[6];       /* >= R_lo                                                                       */
} qad_config;

const char *qad_last_error(void);
/* Diagnostics: kernel launches this library has made in this process so far (all threads). */
int64_t qad_launch_count(void);
/* Diagnostics: the launch census of this library, the contract of qle_launch_census_begin / _end (qle_ekf.h): the distinct
 * kernels this library has launched since begin, process-wide; end stops the census and writes their mangled names, sorted,
 * each followed by '\n', by the two-call size protocol.  Off, the census costs one relaxed atomic load per launch. */
int qad_launch_census_begin(void);
int qad_launch_census_end(char *names, int64_t cap, int64_t *needed);

/* Add the tag poses of one tick to acc: `in` is the tick's inputs view and must have a tag slot (in->z) and IMU
 * records, already packed, and the tick must not have run yet.  Writes acc, nothing else.  ONE kernel launch
 * (k_adapt_observe). */
int qad_observe_tick(const qle_device_view *view, const qle_inputs_view *in, const qle_params *params, double *acc, double chi2_max);
/* The M-step: of every filter with n >= cfg->n_min the six R words of its parameter record (through
 * view->filter_params), its window zeroed, word 21 incremented.  applied = [batch] bytes (1 where written) and
 * R_out = [batch][6] doubles, the six values now in force whether applied or not; either may be NULL.  cfg->window
 * and cfg->chi2_max are checked and not used.  ONE kernel launch (k_adapt_apply). */
int qad_apply(const qle_device_view *view, double *acc, const qad_config *cfg, uint8_t *applied, double *R_out);
/* Ticks [t0, t0 + n) of a device-resident sequence, adapted: for every tick qle_inputs_get_device_view,
 * qad_observe_tick where the tick has a tag slot, qle_run(h, in, t, 1), and qad_apply after every cfg->window-th
 * tag-slot tick, counted from the start of the call.  Plain launches on the handle's stream. */
int qad_run(qle_batch *h, const qle_inputs *in, int64_t t0, int64_t n, const qle_params *params, double *acc, const qad_config *cfg);
/* qad_run for callers without device tensors: zeroed accumulators of its own on the handle's stream, the run,
 * acc_host = [QAD_WORDS][batch] doubles and R_host = [batch][6] doubles (the R in force after the run, read back
 * through qle_get_filter_params) copied back; the stream is synchronised. */
int qad_run_host(qle_batch *h, const qle_inputs *in, int64_t t0, int64_t n, const qle_params *params, const qad_config *cfg,
                 double *acc_host, double *R_host);

#ifdef __cplusplus
}
#endif
#endif /* QLE_ADAPT_H */
