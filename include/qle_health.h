/*
 * qle_health.h -- filter lifecycle from GPU memory: health check, retire, mask algebra (libqle_health.so).
 *
 * include/qle_devio.h feeds and reads filters from GPU memory; this library covers the moment a filter breaks.  With
 * qle_initialize_state_slot (include/qle_ekf.h: seeding from a device-resident tag slot) it closes the loop without a
 * host copy or a synchronisation:
 *     qhl_health(view, limits, mask, status, flagged, summary)   classify every filter, read-only
 *     qhl_retire(view, flagged)                                  flagged filters become "uninitialised": every tick skips them
 *     qhl_and_masks(view, flagged, detections, reseed)           the filters to seed again: flagged AND seen
 *     qdv_pack_inputs(view, slot, u, z, reseed, dtype); qle_initialize_state_slot(h, inputs, t, reinit_bias)
 * It works with every handle, the multirate filter included (where the chi-square gate is refused).
 *
 * status[i] is a byte of the bits below, defined on the stored record words cast to double, so that a restatement in numpy on
 * qle_get_state() is exact.  An initialised filter with mask[i] != 0 is EVALUATED; every other filter gets status 0:
 *     QHL_NONFINITE     any of the view->record_words words of the record (136, or 64 compact) is NaN or Inf.  When this bit is
 *                       set, no other bit is evaluated
 *     QHL_NOT_PD        a pivot of the L D L^T of the n x n covariance is <= 0 or not finite: the factorisation and the rule
 *                       under which qcs_nees (include/qle_consistency.h) counts n_not_pd with all blocks of the handle selected
 *     QHL_QNORM         |q.q - 1| > qnorm_tol, q.q = ((qx^2 + qy^2) + qz^2) + qw^2 in double
 *     QHL_SIGMA_R, QHL_SIGMA_V, QHL_SIGMA_THETA
 *                       the largest diagonal entry of that 3-state block of P is above sigma_*_max^2 (the square is formed on
 *                       the host in double; a limit of +INFINITY disables the bit)
 * flagged[i] = (status[i] & limits->select) != 0 for an evaluated filter, else 0: usable as it is as the mask of qhl_retire,
 * and ANDed with a detection mask (qhl_and_masks) as the mask of a seed.
 *
 * The summary is nine doubles of exact counts, reduced as qcs_nees reduces its sums: per-tile counts from a wave reduction,
 * then one workgroup adds the tiles in a fixed order.  No atomics: two calls on the same state give bit-identical
 * summaries, and the summaries of shards add to the whole batch's.
 *
 * Conventions: those of qle_consistency.h.  Every call is asynchronous on view->stream; every pointer is a device pointer on
 * view->device; masks, status and flagged are [batch] bytes; summary is 8-byte aligned.  Every call returns 0 or a negative
 * error class of qle_ekf.h; the message is in qhl_last_error() (thread-local).  Every refusal is made before any GPU call: a
 * wrong struct_size (view or limits), a misaligned pointer, a limit that is not > 0 (NaN included), select == 0 or bits above
 * QHL_ALL, a null mask where one is required.  The library works from the view struct alone and links the HIP runtime only.
 */
#ifndef QLE_HEALTH_H
#define QLE_HEALTH_H

#include "qle_ekf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QHL_NONFINITE 1u
#define QHL_NOT_PD 2u
#define QHL_QNORM 4u
#define QHL_SIGMA_R 8u
#define QHL_SIGMA_V 16u
#define QHL_SIGMA_THETA 32u
#define QHL_ALL 63u

typedef struct qhl_limits {
    uint32_t struct_size;   /* sizeof(qhl_limits) */
    uint32_t select;        /* the status bits that flag a filter: a non-empty subset of QHL_ALL */
    double sigma_r_max;     /* [m]     > 0, +INFINITY = no limit */
    double sigma_v_max;     /* [m/s]   > 0, +INFINITY = no limit */
    double sigma_theta_max; /* [rad]   > 0, +INFINITY = no limit */
    double qnorm_tol;       /* > 0 */
} qhl_limits;

/* The batch summary: nine doubles, all counts.  A filter with mask 0 enters no field. */
typedef struct qhl_summary {
    double evaluated;       /* mask != 0 and state initialised                                   */
    double flagged;         /* evaluated with (status & select) != 0                             */
    double uninitialised;   /* mask != 0 and no state                                            */
    double n_nonfinite;     /* one count per status bit, in bit order                            */
    double n_not_pd;
    double n_qnorm;
    double n_sigma_r;
    double n_sigma_v;
    double n_sigma_theta;
} qhl_summary;

const char *qhl_last_error(void);
/* Diagnostics: kernel launches this library has made in this process so far (all threads). */
int64_t qhl_launch_count(void);
/* Diagnostics: the launch census of this library, the contract of qle_launch_census_begin / _end (qle_ekf.h): the distinct
 * kernels this library has launched since begin, process-wide; end stops the census and writes their mangled names, sorted,
 * each followed by '\n', by the two-call size protocol.  Off, the census costs one relaxed atomic load per launch. */
int qhl_launch_census_begin(void);
int qhl_launch_census_end(char *names, int64_t cap, int64_t *needed);

/* Classify every filter of the view.  mask = [batch] bytes or NULL (all); status, flagged and summary may each be NULL.
 * Changes nothing in the handle.  With a summary: TWO launches (k_health, k_health_reduce) and a partials buffer the library
 * keeps per (device, stream); without: one. */
int qhl_health(const qle_device_view *view, const qhl_limits *limits, const uint8_t *mask, uint8_t *status, uint8_t *flagged,
               qhl_summary *summary);
/* The same from and into host arrays, for callers without device tensors: stages mask and the outputs through device buffers of
 * its own on view->stream and synchronises it.  status, flagged = [batch] bytes, summary: any may be NULL. */
int qhl_health_host(const qle_device_view *view, const qhl_limits *limits, const uint8_t *mask, uint8_t *status, uint8_t *flagged,
                    qhl_summary *summary);
/* The filters with mask[i] != 0 lose their state: the 16 words of x become zero, the engine's definition of "not initialised"
 * (qle_initialize_state_masked), and so do the covariance words of the record, so that the record equals that of a filter
 * that never had a state.  Every tick entry point then leaves them untouched, and a later seed treats them as fresh
 * (upds_since_correction = 0, a one-entry multirate history).  ONE launch.  mask must not be NULL. */
int qhl_retire(const qle_device_view *view, const uint8_t *mask);
/* out[i] = a[i] != 0 && b[i] != 0, [batch] bytes each; out may be a or b.  ONE launch. */
int qhl_and_masks(const qle_device_view *view, const uint8_t *a, const uint8_t *b, uint8_t *out);

#ifdef __cplusplus
}
#endif
#endif /* QLE_HEALTH_H */
