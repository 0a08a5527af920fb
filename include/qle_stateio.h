/*
 * qle_stateio.h -- device state I/O: write, copy and permute filter states in GPU memory (libqle_stateio.so).
 *
 * Everything a caller reads from a handle stays on the GPU (include/qle_devio.h and the libraries beside it); this library is the
 * other direction.  qsi_pack_state is the inverse of qdv_unpack_state: x = [batch][16] and P = [batch][n][n] tensors in GPU memory
 * become state records, bit for bit the records qle_set_state writes for the same values.  qsi_copy makes filter i of one view a
 * bitwise copy of filter index[i] of another: with a workspace as the destination that is a snapshot (a checkpoint), with a
 * snapshot as the source a restore, with an index a gather -- a permutation, a resampling step, the members of a bank forked from one
 * filter, a small population carried into a larger handle.
 *
 * A snapshot is a VIEW.  It is a copy of the handle's qle_device_view whose `state` points into a workspace the caller supplies
 * (qsi_workspace_bytes; the library allocates nothing), so every read-only consumer of a view works on it unchanged:
 * qdv_unpack_state, qdv_unpack_report, qhl_health, qcs_nees, qlk_lookahead.
 *
 * The handle's host flags: a state written through the view is not yet a state to the handle (qle_ekf.h: a fresh handle refuses to
 * tick, a multirate history still describes the old state).  After writing a handle's records with qsi_pack_state or qsi_copy the
 * caller says so with qle_mark_state_written(h) (qle_ekf.h), which does what qle_set_state does after it has staged its arrays.
 *
 * What a state record is, and is not: the record_words words a tick moves (x, the packed covariance).  A copy carries neither the
 * multirate history (ring, anchors) nor the per-filter counters (upds_since_correction, the rate limiter): after
 * qle_mark_state_written the history restarts at the next tick for every filter, as after qle_set_state, and the counters go on.
 * The copy is bitwise: NaN payloads arrive as they are, and an all-zero record -- the engine's "not initialised" -- copied over a
 * filter retires it.
 *
 * Conventions: those of qle_lookahead.h / qle_health.h.  Every pointer is a device pointer on view->device; ONE launch per call,
 * asynchronous on the destination view's stream, no allocation, no synchronisation (qsi_copy_host stages its host arrays through
 * buffers of its own and synchronises).  Every call returns 0 or a negative error class of qle_ekf.h; the message is in
 * qsi_last_error() (thread-local).  Every refusal is made before any GPU call: a wrong struct_size, a misaligned pointer, a dtype
 * that is neither QSI_F32 nor QSI_F64, views that disagree, x and P both NULL, and what qsi_copy lists below.
 */
#ifndef QLE_STATEIO_H
#define QLE_STATEIO_H

#include "qle_ekf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QSI_F32 0
#define QSI_F64 1

const char *qsi_last_error(void);
/* Diagnostics: kernel launches this library has made in this process so far (all threads). */
int64_t qsi_launch_count(void);
/* Diagnostics: the launch census of this library, the contract of qle_launch_census_begin / _end (qle_ekf.h): the distinct
 * kernels this library has launched since begin, process-wide; end stops the census and writes their mangled names, sorted,
 * each followed by '\n', by the two-call size protocol.  Off, the census costs one relaxed atomic load per launch. */
int qsi_launch_census_begin(void);
int qsi_launch_census_end(char *names, int64_t cap, int64_t *needed);

/* Bytes of a snapshot of this view (state_words words of the compute dtype for padded_batch filters), or a negative error class. */
int64_t qsi_workspace_bytes(const qle_device_view *view);

/* x = [batch][16], P = [batch][n][n] (n = view->num_states) of src_dtype (QSI_F32 | QSI_F64; 16-byte aligned) -> the state records
 * of view, full and compact: ONE launch (k_si_pack).  Either pointer may be NULL: that part of the record is kept.  The words
 * written are the words qle_set_state writes for the same values converted to double: x by the plain C++ cast, the covariance as
 * the symmetric part 0.5 * (P(a,b) + P(b,a)) formed in double and cast (k_pack_P_off), zero where a record holds a word for a state
 * the filter does not estimate.  The three padding words that end the covariance rows of a compact record are written as zero, as
 * every tick writes them.  Not written: filters with mask[i] == 0 (mask = [batch] bytes or NULL = all), the lanes beyond batch in
 * the last tile, and the words at or beyond record_words. */
int qsi_pack_state(const qle_device_view *view, const void *x, const void *P, int32_t src_dtype, const uint8_t *mask);

/* dst filter i becomes a bitwise copy of src filter index[i] (index = [dst->batch] int32, 4-byte aligned, or NULL = i): all
 * record_words words, ONE launch (k_si_copy) on dst->stream.  Filter i is not written when mask[i] == 0 (mask = [dst->batch] bytes
 * or NULL = all) or when its index is outside 0..src->batch-1; written = [dst->batch] bytes or NULL receives 1 for the filters that
 * were written and 0 for the others.  with_params != 0: the 24-word filter_params record travels too.
 * Refused: views that differ in dtype, num_states, compact, record_words or device; without an index, views that differ in batch;
 * src->state and dst->state that overlap (an in-place permutation races: copy into a snapshot first; and a copy onto itself has
 * nothing to do); with_params while either view has no filter_params, or while the two overlap. */
int qsi_copy(const qle_device_view *src, const qle_device_view *dst, const int32_t *index, const uint8_t *mask, int32_t with_params,
             uint8_t *written);
/* The same with index, mask and written as host arrays: staged through device buffers of its own on dst->stream, which it
 * synchronises. */
int qsi_copy_host(const qle_device_view *src, const qle_device_view *dst, const int32_t *index, const uint8_t *mask, int32_t with_params,
                  uint8_t *written);

#ifdef __cplusplus
}
#endif
#endif /* QLE_STATEIO_H */
