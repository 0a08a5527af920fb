/*
 * qle_score.h -- innovation scoring for noise sweeps: per-filter likelihood over a run (libqle_score.so).
 *
 * A sweep over per-filter noise parameters (qle_set_filter_params, qle_synth_generate with perturb_filter_params) ends
 * with the question which parameter set is better.  The criterion that needs no truth is the innovation
 * log-likelihood of each filter, summed over the run,
 *     log L = -1/2 sum_t ( NIS_t + log det S_t + 6 ln 2 pi ),   NIS = nu^T S^-1 nu,   S = G P G^T + R_k,
 * with nu and S of every tag pose taken against the PREDICTED state (EKF.cpp:447-450, :475), plus innovation
 * consistency statistics per component: sum nu_k^2 / sum S_kk names the mis-set entry of R_r / R_ang (1 for a
 * consistent filter), sum nu_k nu_k^- / sum nu_k^2 is the whiteness test (0 for a consistent filter).
 *
 * One kernel per scored tag tick, k_score: per filter the arithmetic of the gate (k_pregate of qle_gate.h: predict in
 * registers, nu, S, its L D L^T factor, whose pivots give log det S = sum log d_m) and a read-modify-write of the
 * filter's accumulator record.  It is read-only on the state and on the input records -- it never writes the mask
 * word, so a scored run is the plain run -- and one lane owns one filter: no atomics, the result is deterministic.
 *
 * The accumulators: acc[QSC_WORDS][padded_batch] doubles, plane-major (word w of filter i at acc[w * padded_batch + i]),
 * fp64 whatever the handle's dtype, zeroed by the caller before the first tick:
 *     0        n        scored innovations
 *     1        sum of NIS
 *     2        sum of NIS^2
 *     3        sum of log det S
 *     4        n_bad    the filter was on, but NIS was not finite or S not positive definite
 *     5        n_pairs  lag products added
 *     6..11    sum of nu_k            (k: r x, y, z, then theta x, y, z -- the entries of R_r, R_ang)
 *     12..17   sum of nu_k^2
 *     18..23   sum of S_kk
 *     24..29   sum of nu_k nu_k^-     nu^-: the filter's previous scored innovation, however many ticks ago
 *     30..35   nu^- itself
 *     36..39   zero
 * A filter is "on" at a tick when its mask word != 0 and it holds a state; it is "scored" when it is on and its NIS is
 * finite.  On but not scored only increments n_bad; not on changes no word.  The lag product and n_pairs are added
 * only when n >= 1 before the tick.
 *
 * Conventions: those of qle_gate.h.  qsc_score_tick, qsc_run and qsc_summary are asynchronous on the handle's stream;
 * acc, mask and out30 are device pointers on its device.  Every call returns 0 or a negative error class of qle_ekf.h;
 * the message is in qsc_last_error() (thread-local).  Every refusal is made before any GPU call:
 * params->multirate_ekf (QLE_ERR_STATE: the gate's own rule, a delayed measurement's innovation belongs to a history
 * entry), an acc that is not 16-byte aligned, a wrong struct_size, ticks outside the sequence, a tick without a tag
 * slot given to qsc_score_tick.  `params` are the qle_params the handle was created with (the library links
 * libqle_ekf.so for qle_params_derive, qle_run and the two view calls).  A gate inside a scored run is not provided.
 */
#ifndef QLE_SCORE_H
#define QLE_SCORE_H

#include "qle_ekf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QSC_WORDS 40 /* doubles per filter of an accumulator array                     */
#define QSC_SUMS 30  /* words 0..29: what qsc_summary adds over the batch              */

const char *qsc_last_error(void);
/* Diagnostics: kernel launches this library has made in this process so far (all threads). */
int64_t qsc_launch_count(void);
/* Diagnostics: the launch census of this library, the contract of qle_launch_census_begin / _end (qle_ekf.h): the distinct
 * kernels this library has launched since begin, process-wide; end stops the census and writes their mangled names, sorted,
 * each followed by '\n', by the two-call size protocol.  Off, the census costs one relaxed atomic load per launch. */
int qsc_launch_census_begin(void);
int qsc_launch_census_end(char *names, int64_t cap, int64_t *needed);

/* Score the tag poses of one tick: `in` is the tick's inputs view and must have a tag slot (in->z) and IMU records,
 * already packed, and the tick must not have run yet (the innovation is taken against the state one prediction ahead
 * of the stored one).  Writes acc, nothing else.  ONE kernel launch (k_score). */
int qsc_score_tick(const qle_device_view *view, const qle_inputs_view *in, const qle_params *params, double *acc);
/* Ticks [t0, t0 + n) of a device-resident sequence, scored: for every tick qle_inputs_get_device_view, qsc_score_tick
 * where the tick has a tag slot, then qle_run(h, in, t, 1).  Plain launches on the handle's stream.  State and
 * sequence end with the bits qle_run(h, in, t0, n) leaves. */
int qsc_run(qle_batch *h, const qle_inputs *in, int64_t t0, int64_t n, const qle_params *params, double *acc);
/* Words 0..29 of acc added over the filters with mask[i] != 0 (mask = [batch] bytes, NULL = all): out30 = 30 doubles.
 * TWO launches (per-tile partials by a fixed shuffle tree, then one workgroup adds the tiles in a fixed order) and a
 * partials buffer the library keeps per (device, stream); deterministic, and additive over shards. */
int qsc_summary(const qle_device_view *view, const double *acc, const uint8_t *mask, double *out30);
/* qsc_run for callers without device tensors: zeroed accumulators of its own on the handle's stream, the run, and
 * acc_host = [QSC_WORDS][batch] doubles copied back (the stream is synchronised). */
int qsc_run_host(qle_batch *h, const qle_inputs *in, int64_t t0, int64_t n, const qle_params *params, double *acc_host);

#ifdef __cplusplus
}
#endif
#endif /* QLE_SCORE_H */
