/*
 * qle_lookahead.h -- look-ahead on the device: state and covariance h ticks ahead, read-only (libqle_lookahead.so).
 *
 * While a filter coasts on the IMU alone (between two tag poses, or for a whole final descent once the corner gate rejects the
 * tag) a controller asks where the pad will be, and with what covariance, h ticks from now -- and a supervisor asks how many
 * more ticks the filter can coast before a sigma crosses the limit qhl_health would flag.  qlk_lookahead answers both in ONE
 * read-only launch (k_lookahead: csrc/ekf_lookahead.hpp): it loads every filter's record once, applies prediction_step
 * (EKF.cpp:346-415) h times in registers with the IMU sample u[i] held -- the zero-order hold filter_update itself applies
 * when no new sample has arrived (EKF.cpp:138-139), dT = dT_nom, so the horizon is h * dT_nom seconds -- and stores the result
 * somewhere else.  Not one word of the handle changes.
 *
 * The forecast is a VIEW.  The kernel stores forecast records in the wave-tile layout (include/qle_ekf.h) into a workspace
 * the caller supplies (qlk_workspace_bytes; the library allocates nothing) and fills `ahead`, a copy of the input view whose
 * `state` points into the workspace.  Every read-only consumer of a qle_device_view works on it unchanged: qdv_unpack_state,
 * qdv_unpack_report, qhl_health ("which filters will be flagged in h ticks"), qcs_nees against a truth at the horizon -- and
 * qlk_lookahead itself: forecasts chain, and lookahead(5) of lookahead(12) has the bits of lookahead(17).  Of a record the
 * view->record_words words a tick moves are written (x and the covariance words); no consumer reads the others.
 *
 * A filter is SKIPPED when mask[i] == 0, when it holds no state (stored quaternion all zero), or beyond the batch's ragged
 * end.  A skipped filter's forecast record is all zero -- the engine's "not initialised" -- so every consumer skips it by the
 * rules it already has, and its ticks_to_limit is -1.
 *
 * Coast budget: with `coast` and `ticks_to_limit` given, ticks_to_limit[i] is the smallest k in 0..h at which a diagonal
 * entry of P(r,r) exceeds sigma_r_max^2 or one of P(theta,theta) exceeds sigma_theta_max^2, else -1; k = 0 is the stored
 * state.  The squares are formed on the host in double and the stored word is cast to double for the comparison: the rule
 * of QHL_SIGMA_R / QHL_SIGMA_THETA (include/qle_health.h) on the states lookahead(k) returns, k = 0..h.
 *
 * Conventions: those of qle_gate.h.  params is the handle's qle_params (the parameter block is derived from it as the handle
 * derives it).  Every pointer of qlk_lookahead is a device pointer on view->device; ONE launch per call, asynchronous on
 * view->stream, no allocation, no synchronisation.  Every call returns 0 or a negative error class of qle_ekf.h; the message
 * is in qlk_last_error() (thread-local).  Every refusal is made before any GPU call: a wrong struct_size (view or coast), a
 * misaligned pointer, h outside 0..QLK_MAX_HORIZON, a workspace that is too small or overlaps view->state, u == NULL, a dtype
 * that is neither QLK_F32 nor QLK_F64, a limit that is not > 0 (NaN included), one of coast / ticks_to_limit without the other.
 */
#ifndef QLE_LOOKAHEAD_H
#define QLE_LOOKAHEAD_H

#include "qle_ekf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QLK_F32 0
#define QLK_F64 1
/* the largest horizon a call accepts: the kernel's run time is bounded by an argument the host has checked */
#define QLK_MAX_HORIZON 4096

typedef struct qlk_coast {
    uint32_t struct_size;   /* sizeof(qlk_coast) */
    uint32_t reserved;
    double sigma_r_max;     /* [m]   > 0, +INFINITY = no limit */
    double sigma_theta_max; /* [rad] > 0, +INFINITY = no limit */
} qlk_coast;

const char *qlk_last_error(void);
/* Diagnostics: kernel launches this library has made in this process so far (all threads). */
int64_t qlk_launch_count(void);
/* Diagnostics: the launch census of this library, the contract of qle_launch_census_begin / _end (qle_ekf.h): the distinct
 * kernels this library has launched since begin, process-wide; end stops the census and writes their mangled names, sorted,
 * each followed by '\n', by the two-call size protocol.  Off, the census costs one relaxed atomic load per launch. */
int qlk_launch_census_begin(void);
int qlk_launch_census_end(char *names, int64_t cap, int64_t *needed);

/* Bytes of the workspace a forecast of this view needs (state_words words of the compute dtype for padded_batch filters),
 * or a negative error class. */
int64_t qlk_workspace_bytes(const qle_device_view *view);

/* The forecast of every filter of `view` h ticks ahead into `workspace` (16-byte aligned, >= qlk_workspace_bytes(view), not
 * overlapping view->state), and the view of it into *ahead (may be the same struct as *view).
 * u = [batch][6] of u_dtype (QLK_F32 | QLK_F64; 16-byte aligned), cast to the compute dtype with the plain C++ cast, as
 * qdv_pack_inputs casts; mask = [batch] bytes or NULL (all); ticks_to_limit = [batch] int32 (4-byte aligned).
 * coast and ticks_to_limit: both NULL, or both given. */
int qlk_lookahead(const qle_device_view *view, const qle_params *params, const void *u, int32_t u_dtype, int32_t h,
                  const uint8_t *mask, void *workspace, int64_t workspace_bytes, qle_device_view *ahead, const qlk_coast *coast,
                  int32_t *ticks_to_limit);
/* The same with u ([batch][6] doubles), mask and ticks_to_limit as host arrays: staged through device buffers of its own on
 * view->stream, which it synchronises.  workspace is still a device pointer: the forecast stays on the device. */
int qlk_lookahead_host(const qle_device_view *view, const qle_params *params, const double *u, int32_t h, const uint8_t *mask,
                       void *workspace, int64_t workspace_bytes, qle_device_view *ahead, const qlk_coast *coast,
                       int32_t *ticks_to_limit);

#ifdef __cplusplus
}
#endif
#endif /* QLE_LOOKAHEAD_H */
