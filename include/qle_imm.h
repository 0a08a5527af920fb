/*
 * qle_imm.h -- filter banks as an interacting multiple model (IMM) estimator: the mixing step and the mode-probability recursion
 * on the device (libqle_imm.so).
 *
 * qle_bank.h fuses a bank of M filters that run different noise parameters under posterior weights; qle_score.h supplies the
 * likelihoods.  That is a STATIC multiple-model estimator: the weights never forget, and the members never interact.  For a
 * tag-pose noise that changes with range both matter: after a few hundred tag ticks at altitude the cumulative log-likelihoods
 * differ by hundreds of nats, and a member whose R was wrong all that time has drifted or grown over-confident when its hypothesis
 * becomes right.  IMM adds a Markov transition between the modes -- recursive mode probabilities that forget at a chosen rate --
 * and a mixing step in front of every measurement cycle that re-initialises member j from the moment-matched mixture of all
 * members under the mixing weights mu_{i|j}.  One IMM cycle around a tag tick is
 *     qim_mix  ->  the likelihood of the tick (qsc_score_tick into zeroed accumulators)  ->  the tick  ->  qim_update
 * and the combination step is qbk_fuse with logmu as the log-weights.
 *
 * Geometry and validity: those of qle_bank.h.  members M is a power of two in 2..64, batch a multiple of M, bank g is filters
 * [g M, (g + 1) M): a bank never leaves one 64-filter wave tile.  Member i is VALID when mask[i] != 0 (mask NULL: all), it holds
 * a state and logmu[i] is finite.
 *
 * qim_mix, per bank, from logmu [batch] (float64, unnormalised log mode probabilities) and Pi [M][M] (float64, row-major, on the
 * device, shared by all banks; Pi[i][j] = P(mode i -> mode j); non-negative entries and rows that add to 1 are the caller's
 * responsibility):
 *   mu_i     = exp(logmu_i - lmax) / sum_valid exp(logmu_k - lmax)     the weights of qbk_fuse; 0 for an invalid member
 *   c_j      = sum_{i valid} Pi[i][j] mu_i                              the predicted mode probability, i ascending
 *   mu_{i|j} = Pi[i][j] mu_i / c_j                                      0 for an invalid i
 *   d_ij     = x_i (-) x_j                                              the difference of qbk_fuse; member j is ITS OWN reference
 *   m_j      = sum_i mu_{i|j} d_ij
 *   x0_j     = x_j (+) m_j                                              r, v, ab, wb: x_j + m_j;  q = norm(q_j (x) exp(m_theta))
 *   P0_j,ab  = sum_i mu_{i|j} (P_i,ab + (d_ij,a - m_j,a)(d_ij,b - m_j,b))
 * d is formed in the compute dtype; weights, terms and sums are fp64 and cast once.  Every sum over i runs in ascending member
 * order: deterministic, and the same bits wherever the bank sits in the batch.  FIRST ORDER, as qbk_fuse: P_i is not transported
 * between tangent spaces.
 * Destination j is MIXED when j is valid, c_j is finite and > 0, and at least one valid i != j has mu_{i|j} > 0.  Only mixed
 * members are written, in place into view->state, for the view->record_words words a tick moves; every other record keeps its
 * bits.  So an identity Pi is a bit-exact no-op, a retired filter stays retired and a bank with one valid member is untouched.
 * A term takes part where mu_{i|j} > 0, by a select (0 * NaN is NaN): a zero in Pi isolates j from the non-finite words of i, a
 * block-diagonal Pi gives independent sub-banks, and nothing crosses a bank.
 * Outputs: logc [batch] float64 = log c_j, -inf for an invalid member or a c_j that is not positive and finite; mixed [batch]
 * bytes (1 = written), optional.
 *
 * qim_update, per bank, after the members have ticked:
 *   logmu_j = logc_j + loglik_j - logsumexp_k (logc_k + loglik_k)       over the members with mask != 0 and finite logc
 *   logmu_j = max(logmu_j, logmu_min)                                   for those members: the floor against mode extinction
 *                                                                       (-inf disables it); not renormalised, the next mix / fuse does
 *   logmu_j = -inf                                                      for every other member
 * A NaN loglik counts as -inf.  loglik [batch] is any float64 array: the loglik of a one-tick scorer (qle_score.h) is the intended
 * source -- it is 0 for a member without a tag pose this tick, whose probability is then its prediction c_j.  The bank sums are
 * the fixed butterfly of qbk_fuse.
 *
 * Conventions, error classes and the rule that every refusal is made before any GPU call: those of qle_bank.h.  Every pointer
 * of qim_mix / qim_update is a device pointer on view->device; ONE launch per call, asynchronous on view->stream, no allocation,
 * no synchronisation.  Refused with QLE_ERR_INVALID: a wrong struct_size, members not a power of two in 2..64, batch % members
 * != 0, a NULL logmu, Pi, logc (qim_update: logc, loglik, logmu) or params, a misaligned pointer (8 bytes for the float64 arrays,
 * 16 for view->state), a NaN logmu_min.  Refused with QLE_ERR_STATE: params->multirate_ekf, the gate's and the scorer's rule --
 * there the next correcting tick replays from the history and would discard what was mixed into the current state.  params is
 * read for that flag only: the library links the HIP runtime alone.
 *
 * NOT PROVIDED: IMM inside qsq_run (a C loop over whole sequences), transition matrices per bank, multirate handles, transport
 * of P_i between tangent spaces, qlk_lookahead of anything fused, banks that cross a 64-filter tile.
 */
#ifndef QLE_IMM_H
#define QLE_IMM_H

#include "qle_ekf.h"

#ifdef __cplusplus
extern "C" {
#endif

const char *qim_last_error(void);
/* Diagnostics: kernel launches this library has made in this process so far (all threads). */
int64_t qim_launch_count(void);
/* Diagnostics: the launch census of this library, the contract of qle_launch_census_begin / _end (qle_ekf.h): the distinct
 * kernels this library has launched since begin, process-wide; end stops the census and writes their mangled names, sorted,
 * each followed by '\n', by the two-call size protocol.  Off, the census costs one relaxed atomic load per launch. */
int qim_launch_census_begin(void);
int qim_launch_census_end(char *names, int64_t cap, int64_t *needed);

/* The mixing step of every bank of `view`, in place.  logmu = [batch] float64; Pi = [members][members] float64; mask = [batch]
 * bytes or NULL (all); logc = [batch] float64 (written); mixed = [batch] bytes or NULL (written).  ONE launch, writes view->state. */
int qim_mix(const qle_device_view *view, const qle_params *params, int32_t members, const double *logmu, const double *Pi,
            const uint8_t *mask, double *logc, uint8_t *mixed);
/* The mode-probability recursion of every bank.  logc, loglik = [batch] float64; mask = [batch] bytes or NULL (all);
 * logmu = [batch] float64 (written; may be the array qim_mix read).  ONE launch; view->state is not touched. */
int qim_update(const qle_device_view *view, int32_t members, const double *logc, const double *loglik, const uint8_t *mask,
               double logmu_min, double *logmu);
/* qim_mix with logmu, Pi, mask, logc and mixed as host arrays: staged through device buffers of its own on view->stream, which
 * it synchronises.  view->state stays on the device. */
int qim_mix_host(const qle_device_view *view, const qle_params *params, int32_t members, const double *logmu, const double *Pi,
                 const uint8_t *mask, double *logc, uint8_t *mixed);

#ifdef __cplusplus
}
#endif
#endif /* QLE_IMM_H */
