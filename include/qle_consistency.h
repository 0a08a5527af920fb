/*
 * qle_consistency.h -- filter consistency against a truth, evaluated on the device (libqle_consistency.so).
 *
 * The innovation side (qle_innovation, include/qle_gate.h) says whether the filters' innovations fit their predicted
 * covariance; qle_synth_rmse says how large the errors are and ignores the covariance.  This library answers what a
 * Monte-Carlo sweep ends with: is the covariance each filter reports the covariance of the error it makes?  Per filter
 *     NEES = e^T P^-1 e
 * over all n states or over the marginal of a selection of the five 3-state blocks, chi-square with
 * dof = 3 popcount(blocks) degrees of freedom for a consistent filter, plus a deterministic batch summary.  The error is
 * truth minus estimate in the filter's error-state convention (the correction injects q <- q (x) exp(dtheta),
 * EKF.cpp:486-501):
 *     e_r = r_true - r,  e_v = v_true - v,  e_theta = quaternion_log(quaternion_norm(q^-1 (x) q_true))   (EKF.cpp:447-450)
 *     e_ab = ab_true - (ab_nom + ab_static),  e_wb = wb_true - (wb_nom + wb_static)      (the biases of qle_get_report)
 * with the static biases of the per-filter parameter record while qle_set_filter_params is in force, else the shared ones.
 *
 * Two launches per call, both read-only with respect to the handle: k_nees (one lane per filter: P = L D L^T in
 * registers, eight fp64 partial sums per 64-filter tile) and k_nees_reduce (one workgroup adds the tiles in a fixed
 * order).  No atomics: two calls on the same state return bit-identical summaries.  The sums are additive, so ranks and
 * shards combine them on the host as they do the RMSE sums.
 *
 * Conventions: those of qle_gate.h.  qcs_nees is asynchronous on view->stream; every pointer it takes is a device
 * pointer on view->device.  x_true = [batch][16] rows (r 3, v 3, q xyzw 4, ab 3, wb 3: the layout of the state, with the
 * TOTAL true biases), row-major, contiguous, 16-byte aligned, of true_dtype; nees = [batch], err = [batch][n] of
 * dst_dtype (QCS_F32 | QCS_F64); a value changes dtype by the plain C cast, the truth before any subtraction.
 * mask = [batch] bytes or NULL (all).  A filter with mask 0 or without state gets NEES = NaN and err = 0 and takes no part
 * in the summary; one whose selected covariance is not positive definite gets NEES = NaN and is counted in n_not_pd.
 * err holds all n components of e, whatever `blocks` selects.  Every call returns 0 or a negative error class of
 * qle_ekf.h; the message is in qcs_last_error() (thread-local).  Every refusal is made before any GPU call:
 * blocks == 0 or bits above QCS_BLOCK_WB, bias bits on an n = 9 handle, chi2_hi not > 0, a wrong struct_size, a
 * misaligned tensor.  It works with every handle, the multirate filter included (the stored state is what it reads).
 *
 * `params` are the qle_params the handle was created with (the library links libqle_ekf.so for qle_params_derive).
 */
#ifndef QLE_CONSISTENCY_H
#define QLE_CONSISTENCY_H

#include "qle_ekf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QCS_F32 0
#define QCS_F64 1

#define QCS_BLOCK_R 1u
#define QCS_BLOCK_V 2u
#define QCS_BLOCK_THETA 4u
#define QCS_BLOCK_AB 8u
#define QCS_BLOCK_WB 16u
#define QCS_BLOCKS_ALL 31u

/* The batch summary: eight doubles.  "Evaluated" = mask != 0, state initialised, NEES finite. */
typedef struct qcs_summary {
    double count;            /* filters evaluated with finite NEES                               */
    double sum_nees;         /* sum of NEES over those filters                                   */
    double sum_nees_sq;      /* sum of squared NEES                                              */
    double n_above;          /* count with nees > chi2_hi                                        */
    double n_not_pd;         /* filters (mask != 0, initialised) flagged not positive definite   */
    double sum_r_err_sq;     /* sum of |e_r|^2 over the counted filters                          */
    double sum_theta_err_sq; /* sum of |e_theta|^2 over the counted filters                      */
    double dof;              /* 3 popcount(blocks); not a sum: the same in every shard           */
} qcs_summary;

const char *qcs_last_error(void);
/* Diagnostics: kernel launches this library has made in this process so far (all threads). */
int64_t qcs_launch_count(void);
/* Diagnostics: the launch census of this library, the contract of qle_launch_census_begin / _end (qle_ekf.h): the distinct
 * kernels this library has launched since begin, process-wide; end stops the census and writes their mangled names, sorted,
 * each followed by '\n', by the two-call size protocol.  Off, the census costs one relaxed atomic load per launch. */
int qcs_launch_census_begin(void);
int qcs_launch_census_end(char *names, int64_t cap, int64_t *needed);

/* NEES of every filter of the view against x_true.  nees, err and summary may each be NULL.  chi2_hi > 0 is the bound
 * n_above counts against; +INFINITY gives 0.  With a summary: TWO launches (k_nees, k_nees_reduce) and a partials buffer
 * the library keeps per (device, stream); without: one. */
int qcs_nees(const qle_device_view *view, const qle_params *params, const void *x_true, int32_t true_dtype,
             const uint8_t *mask, uint32_t blocks, double chi2_hi, void *nees, void *err, qcs_summary *summary,
             int32_t dst_dtype);
/* The same from host fp64 arrays, for callers without device tensors: stages x_true, mask and the outputs through device
 * buffers of its own on view->stream and synchronises it.  nees = [batch], err = [batch][n], summary: any may be NULL. */
int qcs_nees_host(const qle_device_view *view, const qle_params *params, const double *x_true, const uint8_t *mask,
                  uint32_t blocks, double chi2_hi, double *nees, double *err, qcs_summary *summary);

#ifdef __cplusplus
}
#endif
#endif /* QLE_CONSISTENCY_H */
