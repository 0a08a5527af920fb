/*
 * qle_bank.h -- filter banks: posterior weights and one fused estimate per bank on the device, read-only (libqle_bank.so).
 *
 * A sweep runs many parameter sets at once (qle_set_filter_params) and qle_score.h answers which set is better.  The standard
 * use of that answer is multiple-model estimation: a bank of M filters with different noise parameters, fed the same IMU samples
 * and tag poses, publishes ONE estimate, the moment-matched mixture under the members' posterior weights -- for the landing
 * filter the answer to a tag-pose noise that changes with range: a few R_r / R_ang hypotheses run side by side and the data
 * chooses.  qbk_fuse computes it in ONE read-only launch (k_bank_fuse: csrc/ekf_bank.hpp).
 *
 * Geometry.  A handle of B filters is G = B / members banks of `members` consecutive filters: bank g is filters
 * [g * members, (g + 1) * members).  members is a power of two in 2..64 and B a multiple of it, so a bank never leaves one
 * 64-filter wave tile.  NOT PROVIDED: banks that cross tiles, and a member count that is not a power of two.
 *
 * Arithmetic, per bank, from the members' unnormalised log-weights logw (float64; qsc's loglik, or anything else):
 *   valid member   mask[i] != 0 (mask NULL: all), the filter holds a state, logw[i] is finite
 *   weights        w_i = exp(logw_i - lmax) / sum exp(logw_j - lmax) over the valid members, lmax their maximum; else w_i = 0
 *   reference      the lowest-index valid member with logw_i == lmax; best[g] is its filter index
 *   differences    d_i = x_i (-) x_ref, 15 words: plain for r, v, ab, wb; log(norm(q_ref^-1 (x) q_i)) for the attitude (the error
 *                  of qcs_nees, with the w < -0.75 flip: a member stored as -q is the same attitude); m = sum w_i d_i
 *   fused state    r, v, ab, wb: x_ref + m;  q = norm(q_ref (x) exp(m_theta))
 *   fused cov.     P_ab = sum w_i (P_i,ab + (d_i,a - m_a)(d_i,b - m_b)), first order: the member covariances are taken as
 *                  expressed in the fused tangent space, the usual error-state approximation
 * d is formed in the compute dtype; the weights, every term and every sum are fp64, cast to the compute dtype once.  The sums are
 * a fixed tree over the bank's members: deterministic, and the same bits wherever the bank sits in the batch.
 * A bank without a valid member is EMPTY: its fused record is all zero -- the engine's "not initialised" -- best[g] = -1 and
 * every w_i = 0.  A valid member's non-finite words reach its own bank's record (qhl_health flags them) and no other bank's.
 *
 * The result is a VIEW, as a forecast is (qle_lookahead.h).  The kernel stores fused records in the wave-tile layout into a
 * workspace the caller supplies (qbk_workspace_bytes; the library allocates nothing) and fills `fused`, a copy of the input
 * view with batch = G, padded_batch = padded(G), state = workspace and filter_params = NULL.  Every read-only consumer of a
 * qle_device_view works on it unchanged: qdv_unpack_state, qdv_unpack_report, qhl_health, qcs_nees against a truth [G][16].
 * Of a record the view->record_words words a tick moves are written (x and the covariance words), for all padded(G) records
 * (those beyond G are empty).  NOT PROVIDED: qlk_lookahead of a fused view -- which Q a fused estimate coasts under is a
 * modelling choice this library does not make (the fused view carries no per-filter parameters for that reason).
 *
 * Served: fp32 and fp64 handles, 15 and 9 states, compact records, per-filter parameters, multirate_ekf (the current state
 * is what is fused).  Conventions: those of qle_gate.h.  Every pointer of qbk_fuse is a device pointer on view->device; ONE
 * launch per call, asynchronous on view->stream, no allocation, no synchronisation.  Every call returns 0 or a negative error
 * class of qle_ekf.h; the message is in qbk_last_error() (thread-local).  Every refusal is made before any GPU call
 * (QLE_ERR_INVALID): a wrong struct_size, members not a power of two in 2..64, batch % members != 0, logw == NULL, a misaligned
 * pointer, a workspace that is too small or overlaps view->state.
 */
#ifndef QLE_BANK_H
#define QLE_BANK_H

#include "qle_ekf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QBK_MAX_MEMBERS 64

const char *qbk_last_error(void);
/* Diagnostics: kernel launches this library has made in this process so far (all threads). */
int64_t qbk_launch_count(void);
/* Diagnostics: the launch census of this library, the contract of qle_launch_census_begin / _end (qle_ekf.h): the distinct
 * kernels this library has launched since begin, process-wide; end stops the census and writes their mangled names, sorted,
 * each followed by '\n', by the two-call size protocol.  Off, the census costs one relaxed atomic load per launch. */
int qbk_launch_census_begin(void);
int qbk_launch_census_end(char *names, int64_t cap, int64_t *needed);

/* Bytes of the workspace the fused records of this view need (state_words words of the compute dtype for padded(batch /
 * members) filters), or a negative error class. */
int64_t qbk_workspace_bytes(const qle_device_view *view, int32_t members);

/* The fused record of every bank of `view` into `workspace` (16-byte aligned, >= qbk_workspace_bytes(view, members), not
 * overlapping view->state), and the view of them into *fused (may be the same struct as *view).
 * logw = [batch] float64 (8-byte aligned); mask = [batch] bytes or NULL (all); w = [batch] float64 (8-byte aligned) or NULL;
 * best = [batch / members] int32 (4-byte aligned) or NULL. */
int qbk_fuse(const qle_device_view *view, int32_t members, const double *logw, const uint8_t *mask, void *workspace,
             int64_t workspace_bytes, qle_device_view *fused, double *w, int32_t *best);
/* The same with logw, mask, w and best as host arrays: staged through device buffers of its own on view->stream, which it
 * synchronises.  workspace is still a device pointer: the fused records stay on the device. */
int qbk_fuse_host(const qle_device_view *view, int32_t members, const double *logw, const uint8_t *mask, void *workspace,
                  int64_t workspace_bytes, qle_device_view *fused, double *w, int32_t *best);

#ifdef __cplusplus
}
#endif
#endif /* QLE_BANK_H */
