/*
 * qle_devio.h -- device-tensor boundary of the batched relative-pose EKF engine (libqle_devio.so).
 *
 * include/qle_ekf.h takes and returns HOST fp64 arrays.  A caller whose IMU samples and tag poses already live in GPU
 * memory (a simulator, a Monte-Carlo sweep, a learned detector), usually as float32 tensors, packs them here straight
 * into the records the tick kernels read, and reads state and report back into device tensors: no host copy and no
 * synchronisation on the way.  Every call is asynchronous on the view's stream (the handle's own).
 *
 * The library works from the two view structs of qle_ekf.h alone (qle_get_device_view, qle_inputs_get_device_view) and
 * the layout they cite; it does not link libqle_ekf.so.  A tick from device tensors is
 *     qdv_wait_stream(view, producer)                  the handle's stream waits for whoever produced u, z
 *     qdv_pack_inputs(view, inputs_view(t), u, z, mask, dtype)
 *     qle_run(h, inputs, t, 1)                         the existing tick, every mode it serves
 *     qdv_unpack_state / qdv_unpack_report(view, ...)
 *     qdv_signal_stream(view, consumer)                the consumer's stream waits for the handle's
 *
 * Conventions
 *   - all tensor pointers are device pointers on view->device, row-major AoS, contiguous, 16-byte aligned, of the dtype
 *     the call names (QDV_F32 | QDV_F64); masks are one byte per filter (uint8 or bool).
 *   - a value changes dtype by the plain C cast in both directions, so every result equals, bit for bit, what the host
 *     path of qle_ekf.h gives for the same values ((T)double in, (double)T out; float32 out = (float) of that double).
 *   - every call returns 0 or a negative error class of qle_ekf.h (QLE_ERR_*); the message is in qdv_last_error()
 *     (thread-local).
 *   - out of scope, still host-fed through qle_ekf.h: the per-filter stamps of dynamic_meas_delay
 *     (qle_filter_update_stamped).  Writing the state from device tensors -- qle_set_state without the host, snapshot, restore,
 *     gather -- lives in include/qle_stateio.h (libqle_stateio.so).  The NIS-gated tick from device tensors lives in include/qle_gate.h (libqle_gate.so):
 *     one launch between qdv_pack_inputs and qle_run.  Seeding from device tensors is qdv_pack_inputs into a tag slot
 *     followed by qle_initialize_state_slot (qle_ekf.h); health check and retirement live in include/qle_health.h.
 */
#ifndef QLE_DEVIO_H
#define QLE_DEVIO_H

#include "qle_ekf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QDV_F32 0
#define QDV_F64 1

const char *qdv_last_error(void);
/* Diagnostics: the launch census of this library, the contract of qle_launch_census_begin / _end (qle_ekf.h): the distinct
 * kernels this library has launched since begin, process-wide; end stops the census and writes their mangled names, sorted,
 * each followed by '\n', by the two-call size protocol.  Off, the census costs one relaxed atomic load per launch. */
int qdv_launch_census_begin(void);
int qdv_launch_census_end(char *names, int64_t cap, int64_t *needed);

/* u = [batch][6] (accel, gyro) -> the IMU records of the tick `in` describes; when that tick has a tag slot also
 * z = [batch][7] (NULL = identity pose) and mask = [batch] (NULL = all set) -> its tag records, as qle_inputs_upload_tick
 * writes them.  z or mask given for a tick without a tag slot is refused.  ONE kernel launch. */
int qdv_pack_inputs(const qle_device_view *view, const qle_inputs_view *in, const void *u, const void *z, const uint8_t *mask,
                    int32_t src_dtype);
/* qle_get_state into device tensors: x = [batch][16], P = [batch][n][n] full symmetric, n = view->num_states; full and
 * compact records.  Either pointer may be NULL. */
int qdv_unpack_state(const qle_device_view *view, void *x, void *P, int32_t dst_dtype);
/* qle_get_report into device tensors (NODE.cpp:192-220): pose = [batch][7] (r, q xyzw), pose_cov = [batch][36] (rows/cols
 * {0-2,6-8} of cov_pert), vel = [batch][3], bias = [batch][6] = ab_nom+ab_static, wb_nom+wb_static.  Any pointer may be NULL. */
int qdv_unpack_report(const qle_device_view *view, void *pose, void *pose_cov, void *vel, void *bias, int32_t dst_dtype);
/* The handle's stream waits for everything submitted so far to producer_stream (a hipStream_t; NULL = the default stream):
 * an event record plus a stream wait, no host synchronisation. */
int qdv_wait_stream(const qle_device_view *view, void *producer_stream);
/* consumer_stream waits for everything submitted so far to the handle's stream, the same way. */
int qdv_signal_stream(const qle_device_view *view, void *consumer_stream);

#ifdef __cplusplus
}
#endif
#endif /* QLE_DEVIO_H */
