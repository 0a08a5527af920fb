/*
 * qle_budget.h -- the per-component error budget of a batch against a truth, evaluated on the device (libqle_budget.so).
 *
 * qcs_nees (qle_consistency.h) reduces a batch to one number per filter and eight doubles; the deliverable of a Monte-Carlo
 * sweep is the budget per state: the ensemble mean of the error (the bias of every state), the sample covariance of the
 * error, and the covariance the filters report averaged over the same ensemble -- "RMS error against +-sigma" for each of
 * the 15 states.  The ratio sum e_k^2 / sum P_kk names the over-confident state, as the var_ratio of qle_score.h names the
 * mis-set entry of R.  Per group of filters this library returns QBG_WORDS = 256 doubles:
 *     [0]              n: the filters counted
 *     [1 + k]          sum e_k, k < 15
 *     [16 + tri(i,j)]  sum e_i e_j, i <= j            tri(i,j) = 15 i - i (i - 1) / 2 + (j - i): the row-major upper triangle
 *     [136 + tri(i,j)] sum P_ij
 * with e the error of qle_consistency.h (truth minus estimate in the filter's error-state convention: r, v, theta, ab, wb)
 * and P the stored covariance.  On a handle with n = 9 states e_k = 0 for k >= 9; compact records hold zeros in the bias
 * blocks of P.  A filter is counted when its mask is not 0, it has a state, and every e_k and every covariance word its
 * record holds is finite.
 *
 * Two launches per call, both read-only with respect to the handle: k_budget (one lane per filter; the 256 words of the 64
 * filters of a tile are added in fp64 by a fixed tree, the xor-butterfly over the offsets 32, 16, 8, 4, 2, 1) and
 * k_budget_reduce (one workgroup per group adds the group's tiles in ascending order from +0.0).  No atomics: two calls on
 * the same state return the same bits, and the sums of shards that are whole groups are the groups' sums of the whole batch,
 * bit for bit.  A group is `group_tiles` consecutive tiles of 64 filters (the last one may be shorter); group_tiles = 0 is one
 * group for the batch.  A sweep lays its parameter sets out in multiples of 64 filters.
 *
 * Conventions: those of qle_consistency.h.  qbg_budget is asynchronous on view->stream; every pointer it takes is a device
 * pointer on view->device.  x_true = [true_rows][16] rows (r 3, v 3, q xyzw 4, ab 3, wb 3, with the TOTAL true biases),
 * row-major, contiguous, 16-byte aligned, of true_dtype; true_rows = batch, or 1: one reference row for every filter (the
 * dispersion of the ensemble about a common point).  mask = [batch] bytes or NULL (all).  sums = [groups][256] doubles,
 * groups = qbg_groups(batch, group_tiles).  err = [batch][n] of dst_dtype (QBG_F32 | QBG_F64) or NULL: e, 0 where the filter
 * is off; status = [batch] bytes or NULL: 0 off, 1 counted, 2 on but not finite.  Every call returns 0 or a negative error
 * class of qle_ekf.h; the message is in qbg_last_error() (thread-local).  Every refusal is made before any GPU call: a wrong
 * struct_size, a misaligned tensor, true_rows not in {1, batch}, group_tiles < 0, sums == NULL.  It works with every handle
 * and every view, the multirate filter included (the stored state is what it reads).
 *
 * `params` are the qle_params the handle was created with (the library links libqle_ekf.so for qle_params_derive).
 */
#ifndef QLE_BUDGET_H
#define QLE_BUDGET_H

#include "qle_ekf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QBG_F32 0
#define QBG_F64 1
#define QBG_WORDS 256

const char *qbg_last_error(void);
/* Diagnostics: kernel launches this library has made in this process so far (all threads). */
int64_t qbg_launch_count(void);
/* Diagnostics: the launch census of this library, the contract of qle_launch_census_begin / _end (qle_ekf.h). */
int qbg_launch_census_begin(void);
int qbg_launch_census_end(char *names, int64_t cap, int64_t *needed);

/* The number of groups of a batch: 1 for group_tiles = 0, else ceil(ceil(batch / 64) / group_tiles).  < 0: refused
 * (batch <= 0 or group_tiles < 0). */
int64_t qbg_groups(int64_t batch, int64_t group_tiles);

/* The budget of every group of the view against x_true.  err and status may each be NULL.  TWO launches (k_budget,
 * k_budget_reduce) and a [tiles][256] partials buffer the library keeps per (device, stream). */
int qbg_budget(const qle_device_view *view, const qle_params *params, const void *x_true, int32_t true_dtype,
               int64_t true_rows, const uint8_t *mask, int64_t group_tiles, double *sums, void *err, int32_t dst_dtype,
               uint8_t *status);
/* The same from host arrays, for callers without device tensors: x_true = [true_rows][16] doubles; stages x_true, mask and
 * the outputs through device buffers of its own on view->stream and synchronises it.  sums = [groups][256],
 * err = [batch][n] doubles or NULL, status = [batch] bytes or NULL. */
int qbg_budget_host(const qle_device_view *view, const qle_params *params, const double *x_true, int64_t true_rows,
                    const uint8_t *mask, int64_t group_tiles, double *sums, double *err, uint8_t *status);

#ifdef __cplusplus
}
#endif
#endif /* QLE_BUDGET_H */
