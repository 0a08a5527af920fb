/*
 * qle_sequence.h -- a whole tensor sequence per call at the device-tensor boundary (libqle_sequence.so).
 *
 * include/qle_devio.h feeds the filters from GPU memory one tick per call.  A caller that has the whole trajectory on
 * the GPU before the first tick (u [K][B][6], tag poses for the M ticks that have one, masks) packs it here into a
 * device-resident sequence (qle_inputs) with ceil(K / 32) launches, and runs it from one C loop that interleaves the
 * existing read-only launches -- the chi-square gate, the report, the NEES -- with the ticks:
 *     qdv_wait_stream(view, producer)
 *     qsq_pack(view, inputs, 0, K, u_seq, z_seq, mask_seq, dtype)        ceil(K / 32) launches of k_sq_pack
 *     qsq_run(h, inputs, 0, K, &opts)                                    per tick: [qgt_gate_tick] qle_run(.., 1) [qdv_unpack_report] [qcs_nees]
 *     qdv_signal_stream(view, consumer)
 * Every kernel of libqle_ekf.so, libqle_devio.so, libqle_gate.so and libqle_consistency.so is used as it is; this library
 * links them and adds one kernel of its own, k_sq_pack.  The records qsq_pack writes and the results qsq_run leaves are, bit
 * for bit, those of the per-tick path (qdv_pack_inputs, qgt_gate_tick, qle_run, qdv_unpack_report, qcs_nees called tick
 * by tick).
 *
 * Conventions: those of qle_devio.h.  Every entry is asynchronous on the handle's stream; every tensor pointer is a device
 * pointer on the handle's device, row-major, contiguous; a value changes dtype by the plain C cast.  Every entry returns 0
 * or a negative error class of qle_ekf.h with the message in qsq_last_error() (thread-local); the message of a callee
 * that fails (qdv_ / qgt_ / qcs_last_error, qle_last_error) is carried over into it.  Every refusal listed below is made
 * before any GPU call.
 */
#ifndef QLE_SEQUENCE_H
#define QLE_SEQUENCE_H

#include "qle_consistency.h"
#include "qle_devio.h"
#include "qle_ekf.h"
#include "qle_gate.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QSQ_F32 0
#define QSQ_F64 1
#define QSQ_CHUNK 32 /* ticks one launch of k_sq_pack fills */

const char *qsq_last_error(void);
/* Diagnostics: launches of k_sq_pack this library has made in this process so far (all threads).  The launches qsq_run
 * causes are counted by the libraries that make them (qgt_launch_count, qcs_launch_count, the tick library's census). */
int64_t qsq_launch_count(void);
/* Diagnostics: the launch census of this library, the contract of qle_launch_census_begin / _end (qle_ekf.h): the distinct
 * kernels this library has launched since begin, process-wide; end stops the census and writes their mangled names, sorted,
 * each followed by '\n', by the two-call size protocol.  Off, the census costs one relaxed atomic load per launch. */
int qsq_launch_census_begin(void);
int qsq_launch_census_end(char *names, int64_t cap, int64_t *needed);

/* Fill ticks [t0, t0 + n) of `in`: u_seq = [n][batch][6]; z_seq = [m][batch][7] and mask_seq = [m][batch] (one byte per
 * filter, uint8 or bool; NULL = all set), m being the number of those ticks that have a tag slot, in tick order; all of
 * src_dtype (QSQ_F32 | QSQ_F64).  ceil(n / QSQ_CHUNK) launches of k_sq_pack and nothing else; n = 0 does nothing.  Only
 * the BASES of the tensors must be 16-byte aligned: the slab of a tick may start anywhere an element may.
 * Refused: t0 < 0, n < 0 or t0 + n beyond the sequence; z_seq NULL while m > 0; z_seq or mask_seq given while m = 0; a
 * base pointer that is not 16-byte aligned; a view and inputs that do not go together (another struct size, or records
 * of two ticks of the range closer to each other than one record array of the view's batch and dtype is long). */
int qsq_pack(const qle_device_view *view, const qle_inputs *in, int64_t t0, int64_t n, const void *u_seq, const void *z_seq,
             const uint8_t *mask_seq, int32_t src_dtype);

/* What qsq_run does besides the ticks.  Set struct_size = sizeof(qsq_run_opts); any pointer may be NULL.
 * EVERY per-tick output slice has a pitch of padded_batch filters (qle_device_view): pose is [J][padded_batch][7], nis is
 * [m][padded_batch], and so on, so that every slice starts on the 16-byte boundary the entries that fill it insist on;
 * the rows at and beyond `batch` of a slice are never written.  summary is [J][8] doubles.  x_true_seq is plain
 * [J][batch][16]: a slice of it is 64 (128) bytes per filter and so always 16-byte aligned.
 * J = n / trace_every slices: slice j is taken after tick t0 + (j + 1) * trace_every - 1. */
typedef struct qsq_run_opts {
    uint32_t struct_size;
    int32_t dst_dtype;        /* QSQ_F32 | QSQ_F64: nis, the report tensors, nees                                   */
    double chi2_max;          /* > 0: qgt_gate_tick in front of every tick that has a tag slot; 0 = no gate         */
    const qle_params *params; /* the handle's parameters; needed by the gate and by the NEES                        */
    int64_t trace_every;      /* > 0: report / NEES after every trace_every-th tick of the range; 0 = none          */
    uint8_t *accepted;        /* gate: [m][padded_batch], one slice per tag tick of the range, in tick order        */
    void *nis;                /* gate: [m][padded_batch]                                                            */
    void *pose;               /* report: [J][padded_batch][7]                                                       */
    void *pose_cov;           /* report: [J][padded_batch][36]                                                      */
    void *vel;                /* report: [J][padded_batch][3]                                                       */
    void *bias;               /* report: [J][padded_batch][6]                                                       */
    const void *x_true_seq;   /* NEES: the truth after each traced tick, [J][batch][16] of true_dtype               */
    int32_t true_dtype;       /* QSQ_F32 | QSQ_F64                                                                  */
    uint32_t blocks;          /* NEES: QCS_BLOCK_* selection                                                        */
    double chi2_hi;           /* NEES: the bound n_above counts against (> 0, +INFINITY = none)                     */
    void *nees;               /* NEES: [J][padded_batch]                                                            */
    double *summary;          /* NEES: [J][8] (qcs_summary)                                                         */
} qsq_run_opts;

/* Ticks [t0, t0 + n) of `in` on handle h, and for each tick t0 + k, in this order, the calls the per-tick path makes:
 *   1. qgt_gate_tick on the tick's inputs view, if opts->chi2_max > 0 and the tick has a tag slot;
 *   2. qle_run(h, in, t0 + k, 1);
 *   3. if (k + 1) % trace_every == 0: qdv_unpack_report (any of pose, pose_cov, vel, bias given) and qcs_nees (x_true_seq
 *      with nees or summary given) into slice j = (k + 1) / trace_every - 1.
 * Plain launches on the handle's stream: no graph capture, no second stream.  opts NULL: the ticks alone.
 * Refused: t0 < 0, n < 0, t0 + n beyond the sequence (no wrap here); a gate with params->multirate_ekf (QLE_ERR_STATE,
 * the gate's own rule); chi2_max < 0 or NaN; gate outputs without a gate; trace outputs without trace_every; a gate or a
 * NEES without params; x_true_seq without nees and summary, or those without x_true_seq; blocks, chi2_hi and dtypes as
 * qcs_nees refuses them; an output that is not 16-byte aligned (accepted: any).
 *
 * A gated run leaves the ACCEPTED masks in the sequence's mask words, because k_pregate writes them: running the same
 * ticks again without a gate, on a handle in the same start state, replays exactly the accepted corrections. */
int qsq_run(qle_batch *h, const qle_inputs *in, int64_t t0, int64_t n, const qsq_run_opts *opts);

#ifdef __cplusplus
}
#endif
#endif /* QLE_SEQUENCE_H */
