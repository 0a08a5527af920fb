// devio_capi.hip -- C ABI of include/qle_devio.h over devio_kernels.hpp.  Host side: argument checks and launches on the view's
// stream.  Works from the view structs of include/qle_ekf.h alone; links libamdhip64 only.
#include "../../include/qle_devio.h"

#include <mutex>

#include "devio_kernels.hpp"
#include "side_host.hpp"

using namespace qdv;
using namespace qle::side;

QLE_SIDE_LAST_ERROR(qdv_last_error)
QLE_SIDE_LAUNCH_CENSUS(qdv)

// This library takes a view of exactly its own size and does not ask for aligned records (include/qle_devio.h).  No GPU call: every
// entry refuses what it refuses first and calls use_device() behind that.
static int check_view(const qle_device_view* v) { return check_view(v, ViewSize::exact, false); }
static int check_dtype(int32_t d, const char* what)
{
    if (d != QDV_F32 && d != QDV_F64) return fail(QLE_ERR_INVALID, "%s must be QDV_F32 or QDV_F64 (got %d)", what, d);
    return QLE_OK;
}
static int check_aligned(const void* p, const char* what)
{
    if (((uintptr_t)p & 15u) != 0) return fail(QLE_ERR_INVALID, "%s is not 16-byte aligned", what);
    return QLE_OK;
}

template <typename T, typename S>
static int pack_t(const qle_device_view* v, const qle_inputs_view* in, const void* u, const void* z, const uint8_t* mask)
{
    return launch(k_dv_pack<T, S>, tiles(v), dim3(kTile), 0, stream_of(v), (const S*)u, (const S*)z, mask, (T*)in->u, (T*)in->z, v->batch);
}

extern "C" int qdv_pack_inputs(const qle_device_view* view, const qle_inputs_view* in, const void* u, const void* z, const uint8_t* mask, int32_t src_dtype)
{
    QLE_TRY(check_view(view));
    QLE_TRY(check_dtype(src_dtype, "src_dtype"));
    if (!in || in->struct_size != sizeof(qle_inputs_view) || !in->u) return fail(QLE_ERR_INVALID, "inputs view is null or of another size");
    if (!u) return fail(QLE_ERR_INVALID, "u is null");
    if (!in->z && (z || mask)) return fail(QLE_ERR_INVALID, "the tick has no tag slot but z or mask is given");
    QLE_TRY(check_aligned(u, "u"));
    QLE_TRY(check_aligned(z, "z"));
    QLE_TRY(use_device(view));
    if (view->dtype == QLE_F32) return src_dtype == QDV_F32 ? pack_t<float, float>(view, in, u, z, mask) : pack_t<float, double>(view, in, u, z, mask);
    return src_dtype == QDV_F32 ? pack_t<double, float>(view, in, u, z, mask) : pack_t<double, double>(view, in, u, z, mask);
}

template <typename T, typename D>
static int state_t(const qle_device_view* v, void* x, void* P)
{
    if (v->num_states == 15) return launch(k_dv_state<T, D, 15>, tiles(v), dim3(kTile), 0, stream_of(v), (const T*)v->state, (D*)x, (D*)P, v->batch, 0);
    return launch(k_dv_state<T, D, 9>, tiles(v), dim3(kTile), 0, stream_of(v), (const T*)v->state, (D*)x, (D*)P, v->batch, (int)v->compact);
}

extern "C" int qdv_unpack_state(const qle_device_view* view, void* x, void* P, int32_t dst_dtype)
{
    QLE_TRY(check_view(view));
    QLE_TRY(check_dtype(dst_dtype, "dst_dtype"));
    if (!x && !P) return QLE_OK;
    QLE_TRY(check_aligned(x, "x"));
    QLE_TRY(check_aligned(P, "P"));
    QLE_TRY(use_device(view));
    if (view->dtype == QLE_F32) return dst_dtype == QDV_F32 ? state_t<float, float>(view, x, P) : state_t<float, double>(view, x, P);
    return dst_dtype == QDV_F32 ? state_t<double, float>(view, x, P) : state_t<double, double>(view, x, P);
}

template <typename T, typename D>
static int report_t(const qle_device_view* v, void* pose, void* cov, void* vel, void* bias)
{
    StaticBias sb;
    for (int k = 0; k < 3; ++k) { sb.v[k] = v->ab_static[k]; sb.v[3 + k] = v->wb_static[k]; }
    return launch(k_dv_report<T, D>, tiles(v), dim3(kTile), 0, stream_of(v), (const T*)v->state, (const T*)v->filter_params, (D*)pose, (D*)cov, (D*)vel, (D*)bias,
                  v->batch, (int)v->compact, sb);
}

extern "C" int qdv_unpack_report(const qle_device_view* view, void* pose, void* pose_cov, void* vel, void* bias, int32_t dst_dtype)
{
    QLE_TRY(check_view(view));
    QLE_TRY(check_dtype(dst_dtype, "dst_dtype"));
    if (!pose && !pose_cov && !vel && !bias) return QLE_OK;
    QLE_TRY(check_aligned(pose, "pose"));
    QLE_TRY(check_aligned(pose_cov, "pose_cov"));
    QLE_TRY(check_aligned(vel, "vel"));
    QLE_TRY(check_aligned(bias, "bias"));
    QLE_TRY(use_device(view));
    if (view->dtype == QLE_F32) return dst_dtype == QDV_F32 ? report_t<float, float>(view, pose, pose_cov, vel, bias) : report_t<float, double>(view, pose, pose_cov, vel, bias);
    return dst_dtype == QDV_F32 ? report_t<double, float>(view, pose, pose_cov, vel, bias) : report_t<double, double>(view, pose, pose_cov, vel, bias);
}

// ---- stream ordering: one event per device and direction, made on first use and re-recorded by every call (a wait that was queued
// on an earlier record keeps that record's position).
static constexpr int kMaxDevices = 64;
static std::mutex g_ev_mu;
static hipEvent_t g_ev[kMaxDevices][2] = {};

static int order(const qle_device_view* v, hipStream_t first, hipStream_t then, int dir)
{
    if (v->device < 0 || v->device >= kMaxDevices) return fail(QLE_ERR_INVALID, "device %d", v->device);
    QLE_TRY(use_device(v));
    if (first == then) return QLE_OK;
    std::lock_guard<std::mutex> lock(g_ev_mu);
    hipEvent_t& ev = g_ev[v->device][dir];
    if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(ev, first));
    HIP_TRY(hipStreamWaitEvent(then, ev, 0));
    return QLE_OK;
}

extern "C" int qdv_wait_stream(const qle_device_view* view, void* producer_stream)
{
    QLE_TRY(check_view(view));
    return order(view, (hipStream_t)producer_stream, stream_of(view), 0);
}

extern "C" int qdv_signal_stream(const qle_device_view* view, void* consumer_stream)
{
    QLE_TRY(check_view(view));
    return order(view, stream_of(view), (hipStream_t)consumer_stream, 1);
}
