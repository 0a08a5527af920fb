/*
 * qle_gate.h -- chi-square outlier gate in front of the fused tick, fed from GPU memory (libqle_gate.so).
 *
 * The gated calls of include/qle_ekf.h (qle_step_gated, qle_update_gated) take host fp64 arrays, return accepted / nis to
 * the host and are three launches per tick; they refuse qle_enable_gating.  Here the gate is ONE read-only kernel,
 * k_pregate, launched between qdv_pack_inputs (include/qle_devio.h) and the unchanged tick of qle_run: per filter it
 * predicts in registers what the innovation covariance is read from, evaluates the normalised innovation squared
 *     NIS = delta_y^T S^-1 delta_y,   S = G P G^T + R_k   (EKF.cpp:447-450, :475)
 * against the PREDICTED state, and clears the mask word of the tick's tag record where the tag pose is not accepted:
 *     accepted = mask && state_initialized && isfinite(NIS) && NIS <= chi2_max.
 * The tick behind it -- the fused k_step, the workgroup-cooperative tick of the small batches, full or compact records,
 * with or without qle_enable_gating -- then applies exactly the accepted corrections.  A gated tick from device tensors is
 *     qdv_wait_stream(view, producer)
 *     qdv_pack_inputs(view, inputs_view(t), u, z, mask, dtype)
 *     qgt_gate_tick(view, inputs_view(t), params, chi2_max, nis, accepted, nu, S, dtype)
 *     qle_run(h, inputs, t, 1)
 *     qdv_signal_stream(view, consumer)
 *
 * With qle_enable_gating on, the mask word means measurement_ready (EKF.hpp:125): a rejected tag pose is treated as no
 * detection -- it is not consumed and does not reset the rate limiter -- and the decision logic of the tick
 * (EKF.cpp:147-186) runs on the accepted ones.
 *
 * Conventions: those of qle_devio.h.  Every call is asynchronous on view->stream; every tensor pointer is a device
 * pointer on view->device, row-major AoS, contiguous, of dst_dtype (QGT_F32 | QGT_F64; accepted: one byte per filter);
 * a value changes dtype by the plain C cast.  A filter with mask 0 or without state gets nu = 0, S = 0, NIS = NaN and is
 * never accepted; one whose S is not positive definite gets NIS = NaN and is never accepted.  Every call returns 0 or a
 * negative error class of qle_ekf.h; the message is in qgt_last_error() (thread-local).  Every refusal is made before
 * any GPU call.
 *
 * The view carries no noise or extrinsic parameters: `params` are the qle_params the handle was created with (or last
 * given to qle_set_params); the library derives from them the parameter block the handle's own kernels use (it links
 * libqle_ekf.so for qle_params_derive).  params->multirate_ekf set is refused with QLE_ERR_STATE: a delayed
 * measurement's innovation belongs to a history entry, and a gate inside the multirate replay remains a follow-up.
 * Host-array qle_step_gated stays what it is: three launches.
 */
#ifndef QLE_GATE_H
#define QLE_GATE_H

#include "qle_ekf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QGT_F32 0
#define QGT_F64 1

const char *qgt_last_error(void);

/* The gate of one tick: `in` is the tick's inputs view and must have a tag slot (in->z), already packed with u, z and
 * mask.  nis = [batch], accepted = [batch] (uint8), nu = [batch][6], S = [batch][36] (symmetric, row-major); any may
 * be NULL.  chi2_max > 0; +INFINITY accepts every finite NIS.  Writes the mask words of the tag record, never the state.
 * ONE kernel launch (k_pregate<PREDICT = true>). */
int qgt_gate_tick(const qle_device_view *view, const qle_inputs_view *in, const qle_params *params, double chi2_max,
                  void *nis, uint8_t *accepted, void *nu, void *S, int32_t dst_dtype);
/* qle_innovation from GPU memory: nu, S and NIS of the tag record of `in` against the STORED state (no prediction; the
 * IMU record is not read).  Changes nothing at all.  ONE kernel launch (k_pregate<PREDICT = false>). */
int qgt_innovation(const qle_device_view *view, const qle_inputs_view *in, const qle_params *params, void *nis, void *nu,
                   void *S, int32_t dst_dtype);
/* Diagnostics: kernel launches this library has made in this process so far (all threads). */
int64_t qgt_launch_count(void);
/* Diagnostics: the launch census of this library, the contract of qle_launch_census_begin / _end (qle_ekf.h): the distinct
 * kernels this library has launched since begin, process-wide; end stops the census and writes their mangled names, sorted,
 * each followed by '\n', by the two-call size protocol.  Off, the census costs one relaxed atomic load per launch. */
int qgt_launch_census_begin(void);
int qgt_launch_census_end(char *names, int64_t cap, int64_t *needed);

#ifdef __cplusplus
}
#endif
#endif /* QLE_GATE_H */
