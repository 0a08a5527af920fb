// sequence_capi.hip -- C ABI of include/qle_sequence.h over sequence_kernels.hpp and sequence_plan.hpp.  Host side: argument checks
// (every refusal before any GPU call), the launches of k_sq_pack on the view's stream, and the C loop of qsq_run over the entries of
// libqle_gate.so, libqle_ekf.so, libqle_devio.so and libqle_consistency.so, which it links.
#include "../../include/qle_sequence.h"

#include <cmath>
#include <vector>

#include "sequence_kernels.hpp"
#include "side_host.hpp"

using namespace qsq;
using namespace qle::side;

static_assert(QSQ_CHUNK == kSeqChunk, "the header publishes the chunk of k_sq_pack");
static_assert(sizeof(SeqEntry<float>) == 24 && sizeof(SeqChunk<double>) == 24 * kSeqChunk, "the chunk travels by value: 768 bytes of kernel arguments");
static_assert(sizeof(qcs_summary) == 8 * sizeof(double), "summary slices are eight doubles");

QLE_SIDE_LAST_ERROR(qsq_last_error)
QLE_SIDE_LAUNCH_COUNT(qsq_launch_count)
QLE_SIDE_LAUNCH_CENSUS(qsq)

static int check_dtype(int32_t d, const char* what)
{
    if (d != QSQ_F32 && d != QSQ_F64) return fail(QLE_ERR_INVALID, "%s must be QSQ_F32 or QSQ_F64 (got %d)", what, d);
    return QLE_OK;
}
static int check_aligned(const void* p, const char* what)
{
    if (!aligned(p, 16)) return fail(QLE_ERR_INVALID, "%s is not 16-byte aligned", what);
    return QLE_OK;
}
static int inputs_view(const qle_inputs* in, int64_t t, qle_inputs_view* iv)
{
    iv->struct_size = sizeof(qle_inputs_view);
    const int rc = qle_inputs_get_device_view(in, t, iv);
    return rc == QLE_OK ? QLE_OK : fail(rc, "%s", qle_last_error());
}
// [t0, t0 + n) inside the sequence: the tick library is the one that knows its length, and says so without a GPU call
static int check_range(const qle_inputs* in, int64_t t0, int64_t n)
{
    if (!in) return fail(QLE_ERR_INVALID, "inputs is null");
    if (t0 < 0 || n < 0) return fail(QLE_ERR_INVALID, "t0 and n must be >= 0 (got %lld, %lld)", (long long)t0, (long long)n);
    if (n == 0) return QLE_OK;
    qle_inputs_view iv;
    if (inputs_view(in, t0, &iv) != QLE_OK || inputs_view(in, t0 + n - 1, &iv) != QLE_OK)
        return fail(QLE_ERR_INVALID, "ticks [%lld, %lld) reach beyond the sequence: %s", (long long)t0, (long long)(t0 + n), qle_last_error());
    return QLE_OK;
}

template <typename T, typename S>
static int pack_t(const qle_device_view* v, const std::vector<PlanChunk>& plan, const std::vector<qle_inputs_view>& ivs, int64_t t0, const void* u_seq,
                  const void* z_seq, const uint8_t* mask_seq)
{
    for (const PlanChunk& c : plan) {
        SeqChunk<T> chunk = {};
        for (int y = 0; y < c.count; ++y) {
            const qle_inputs_view& iv = ivs[(size_t)(c.e[y].tick - t0)];
            chunk.e[y].u = (T*)iv.u;
            chunk.e[y].z = (T*)iv.z;
            chunk.e[y].zsrc = c.e[y].zsrc;
        }
        QLE_TRY(launch(k_sq_pack<T, S>, dim3((unsigned)(v->padded_batch / kTile), (unsigned)c.count), dim3(kTile), 0, stream_of(v), (const S*)u_seq, (const S*)z_seq,
                       mask_seq, v->batch, c.k0, chunk));
    }
    return QLE_OK;
}

extern "C" int qsq_pack(const qle_device_view* view, const qle_inputs* in, int64_t t0, int64_t n, const void* u_seq, const void* z_seq,
                        const uint8_t* mask_seq, int32_t src_dtype)
{
    QLE_TRY(check_view(view, ViewSize::exact, false));
    QLE_TRY(check_dtype(src_dtype, "src_dtype"));
    QLE_TRY(check_range(in, t0, n));
    if (!u_seq) return fail(QLE_ERR_INVALID, "u_seq is null");
    std::vector<qle_inputs_view> ivs((size_t)n);
    for (int64_t k = 0; k < n; ++k) QLE_TRY(inputs_view(in, t0 + k, &ivs[(size_t)k]));
    int64_t m = 0;
    const std::vector<PlanChunk> plan = sequence_plan(t0, n, [&](int64_t t) { return ivs[(size_t)(t - t0)].z != nullptr; }, &m);
    if (m > 0 && !z_seq) return fail(QLE_ERR_INVALID, "%lld ticks of the range have a tag slot but z_seq is null", (long long)m);
    if (m == 0 && (z_seq || mask_seq)) return fail(QLE_ERR_INVALID, "no tick of the range has a tag slot but z_seq or mask_seq is given");
    QLE_TRY(check_aligned(u_seq, "u_seq"));
    QLE_TRY(check_aligned(z_seq, "z_seq"));
    QLE_TRY(check_aligned(mask_seq, "mask_seq"));
    // the records of two ticks must lie at least one record array of this view apart: inputs made for a smaller batch or dtype do not
    const size_t wsz = view->dtype == QLE_F32 ? 4 : 8;
    const uintptr_t ub = (uintptr_t)qle::kUW * (uintptr_t)view->padded_batch * wsz, zb = (uintptr_t)qle::kZW * (uintptr_t)view->padded_batch * wsz;
    const qle_inputs_view* last_z = nullptr;
    for (int64_t k = 0; k < n; ++k) {
        const qle_inputs_view& iv = ivs[(size_t)k];
        if (!iv.u || !aligned(iv.u, 16) || !aligned(iv.z, 16)) return fail(QLE_ERR_INVALID, "tick %lld: records are null or not 16-byte aligned", (long long)(t0 + k));
        if (k > 0) {
            const uintptr_t a = (uintptr_t)ivs[(size_t)k - 1].u, b = (uintptr_t)iv.u;
            if ((a < b ? b - a : a - b) < ub) return fail(QLE_ERR_INVALID, "view and inputs do not go together: the IMU records of ticks %lld and %lld overlap for a batch of %lld", (long long)(t0 + k - 1), (long long)(t0 + k), (long long)view->batch);
        }
        if (iv.z) {
            if (last_z) {
                const uintptr_t a = (uintptr_t)last_z->z, b = (uintptr_t)iv.z;
                if ((a < b ? b - a : a - b) < zb) return fail(QLE_ERR_INVALID, "view and inputs do not go together: tag records overlap at tick %lld for a batch of %lld", (long long)(t0 + k), (long long)view->batch);
            }
            last_z = &iv;
        }
    }
    if (n == 0) return QLE_OK;
    QLE_TRY(use_device(view));
    if (view->dtype == QLE_F32)
        return src_dtype == QSQ_F32 ? pack_t<float, float>(view, plan, ivs, t0, u_seq, z_seq, mask_seq) : pack_t<float, double>(view, plan, ivs, t0, u_seq, z_seq, mask_seq);
    return src_dtype == QSQ_F32 ? pack_t<double, float>(view, plan, ivs, t0, u_seq, z_seq, mask_seq) : pack_t<double, double>(view, plan, ivs, t0, u_seq, z_seq, mask_seq);
}

// ---- qsq_run
static char* at(void* base, int64_t slice, int64_t pitch_bytes) { return base ? (char*)base + slice * pitch_bytes : nullptr; }

static int check_run(const qle_inputs* in, int64_t t0, int64_t n, const qsq_run_opts* o, const qle_device_view* v)
{
    QLE_TRY(check_range(in, t0, n));
    if (!o) return QLE_OK;
    if (o->struct_size != sizeof(qsq_run_opts)) return fail(QLE_ERR_INVALID, "opts: struct_size %u, this library was built for %zu", o->struct_size, sizeof(qsq_run_opts));
    const bool gate = o->chi2_max > 0.0;
    const bool report = o->pose || o->pose_cov || o->vel || o->bias;
    const bool nees = o->nees || o->summary;
    if (!(o->chi2_max >= 0.0)) return fail(QLE_ERR_INVALID, "chi2_max must be > 0, or 0 for no gate (got %g)", o->chi2_max);
    if (gate && !o->params) return fail(QLE_ERR_INVALID, "a gate needs params");
    if (gate && o->params->multirate_ekf) return fail(QLE_ERR_STATE, "the gate does not support multirate_ekf: a delayed measurement's innovation belongs to a history entry");
    if (!gate && (o->accepted || o->nis)) return fail(QLE_ERR_INVALID, "gate outputs given without a gate (chi2_max = 0)");
    if (o->trace_every < 0) return fail(QLE_ERR_INVALID, "trace_every must be >= 0 (got %lld)", (long long)o->trace_every);
    if (o->trace_every == 0 && (report || nees || o->x_true_seq)) return fail(QLE_ERR_INVALID, "trace outputs given without trace_every");
    if (nees != (o->x_true_seq != nullptr)) return fail(QLE_ERR_INVALID, "x_true_seq goes with nees or summary, and they with it");
    if (gate || report || nees) QLE_TRY(check_dtype(o->dst_dtype, "dst_dtype"));
    if (nees) {
        if (!o->params) return fail(QLE_ERR_INVALID, "the NEES needs params");
        QLE_TRY(check_dtype(o->true_dtype, "true_dtype"));
        if (o->blocks == 0 || (o->blocks & ~QCS_BLOCKS_ALL)) return fail(QLE_ERR_INVALID, "blocks 0x%x: expected a non-empty selection of bits 0..4 (r, v, theta, ab, wb)", o->blocks);
        if (v->num_states == 9 && (o->blocks & ~7u)) return fail(QLE_ERR_INVALID, "blocks 0x%x selects a bias block, the handle has n = 9 states (est_bias = false)", o->blocks);
        if (!(o->chi2_hi > 0.0)) return fail(QLE_ERR_INVALID, "chi2_hi must be > 0 (got %g)", o->chi2_hi);
        QLE_TRY(check_aligned(o->x_true_seq, "x_true_seq"));
        QLE_TRY(check_aligned(o->nees, "nees"));
        QLE_TRY(check_aligned(o->summary, "summary"));
    }
    if ((gate || nees) && v->num_states != (o->params->est_bias ? 15 : 9)) return fail(QLE_ERR_INVALID, "handle: num_states %d, params: est_bias %d", v->num_states, o->params->est_bias);
    QLE_TRY(check_aligned(o->nis, "nis"));
    QLE_TRY(check_aligned(o->pose, "pose"));
    QLE_TRY(check_aligned(o->pose_cov, "pose_cov"));
    QLE_TRY(check_aligned(o->vel, "vel"));
    QLE_TRY(check_aligned(o->bias, "bias"));
    return QLE_OK;
}

extern "C" int qsq_run(qle_batch* h, const qle_inputs* in, int64_t t0, int64_t n, const qsq_run_opts* o)
{
    if (!h) return fail(QLE_ERR_INVALID, "handle is null");
    qle_device_view v;
    v.struct_size = sizeof(v);
    if (int rc = qle_get_device_view(h, &v)) return fail(rc, "%s", qle_last_error());
    QLE_TRY(check_run(in, t0, n, o, &v));
    const bool gate = o && o->chi2_max > 0.0;
    const bool report = o && (o->pose || o->pose_cov || o->vel || o->bias);
    const bool nees = o && (o->nees || o->summary);
    const int64_t every = o ? o->trace_every : 0;
    const int64_t Bp = v.padded_batch, B = v.batch;
    const int64_t dsz = o && o->dst_dtype == QSQ_F64 ? 8 : 4, tsz = o && o->true_dtype == QSQ_F64 ? 8 : 4;
    int64_t slot = 0;
    for (int64_t k = 0; k < n; ++k) {
        const int64_t t = t0 + k;
        if (gate) {
            qle_inputs_view iv;
            QLE_TRY(inputs_view(in, t, &iv));
            if (iv.z) {
                if (int rc = qgt_gate_tick(&v, &iv, o->params, o->chi2_max, at(o->nis, slot, Bp * dsz), (uint8_t*)at(o->accepted, slot, Bp), nullptr, nullptr, o->dst_dtype))
                    return fail(rc, "qgt_gate_tick at tick %lld: %s", (long long)t, qgt_last_error());
                ++slot;
            }
        }
        if (int rc = qle_run(h, in, t, 1)) return fail(rc, "qle_run at tick %lld: %s", (long long)t, qle_last_error());
        const bool traced = every > 0 && (k + 1) % every == 0;
        if (gate || traced) {
            // the state a tick leaves may live elsewhere than the one it read (the multirate history is a ring): ask again
            v.struct_size = sizeof(v);
            if (int rc = qle_get_device_view(h, &v)) return fail(rc, "%s", qle_last_error());
        }
        if (!traced) continue;
        const int64_t j = (k + 1) / every - 1;
        if (report)
            if (int rc = qdv_unpack_report(&v, at(o->pose, j, Bp * 7 * dsz), at(o->pose_cov, j, Bp * 36 * dsz), at(o->vel, j, Bp * 3 * dsz), at(o->bias, j, Bp * 6 * dsz), o->dst_dtype))
                return fail(rc, "qdv_unpack_report after tick %lld: %s", (long long)t, qdv_last_error());
        if (nees)
            if (int rc = qcs_nees(&v, o->params, (const char*)o->x_true_seq + j * B * 16 * tsz, o->true_dtype, nullptr, o->blocks, o->chi2_hi, at(o->nees, j, Bp * dsz), nullptr,
                                  (qcs_summary*)at(o->summary, j, (int64_t)sizeof(qcs_summary)), o->dst_dtype))
                return fail(rc, "qcs_nees after tick %lld: %s", (long long)t, qcs_last_error());
    }
    return QLE_OK;
}
