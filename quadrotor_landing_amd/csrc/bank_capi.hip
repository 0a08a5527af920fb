// bank_capi.hip -- C ABI of include/qle_bank.h over ekf_bank.hpp.  Host side: argument checks (every refusal before any GPU call) and
// ONE launch on the view's stream.  Works from the view struct of include/qle_ekf.h alone; links the HIP runtime only.  Allocates
// nothing: the fused records go into the caller's workspace (the host entry stages its host arrays through buffers of its own).
#include "../../include/qle_bank.h"

#include "ekf_bank.hpp"
#include "side_host.hpp"

using namespace qle;
using namespace qle::side;

static_assert(QBK_MAX_MEMBERS == kBankMaxMembers && kBankMaxMembers == kTile, "a bank never leaves one wave tile");

QLE_SIDE_LAST_ERROR(qbk_last_error)
QLE_SIDE_LAUNCH_COUNT(qbk_launch_count)
QLE_SIDE_LAUNCH_CENSUS(qbk)

static int64_t elt(const qle_device_view* v) { return v->dtype == QLE_F64 ? 8 : 4; }

// what every entry refuses about the view and the geometry; no GPU call.  A view of exactly this library's size (the fused view is a
// copy of it), with 16-byte aligned records.
static int check_geometry(const qle_device_view* v, int32_t members)
{
    QLE_TRY(check_view(v, ViewSize::exact, true));
    if (!bank_members_ok(members)) return fail(QLE_ERR_INVALID, "members %d: expected a power of two in 2..%d", members, kBankMaxMembers);
    if (v->batch % members != 0) return fail(QLE_ERR_INVALID, "batch %lld is not a multiple of members %d", (long long)v->batch, members);
    return QLE_OK;
}

static int64_t workspace_bytes(const qle_device_view* v, int32_t members) { return padded_filters(v->batch / members) * (int64_t)kSW * elt(v); }

extern "C" int64_t qbk_workspace_bytes(const qle_device_view* view, int32_t members)
{
    QLE_TRY(check_geometry(view, members));
    return workspace_bytes(view, members);
}

// Everything include/qle_bank.h lists as refused, the view first; no GPU call.  host: logw, mask, w and best are host arrays (no
// alignment to ask for).
static int check_args(const qle_device_view* v, int32_t members, const double* logw, const void* workspace, int64_t ws_bytes, const qle_device_view* fused,
                      const double* w, const int32_t* best, bool host)
{
    QLE_TRY(check_geometry(v, members));
    if (!logw) return fail(QLE_ERR_INVALID, "logw is null");
    if (!workspace) return fail(QLE_ERR_INVALID, "workspace is null");
    if (!aligned(workspace, 16)) return fail(QLE_ERR_INVALID, "workspace must be 16-byte aligned");
    const int64_t need = workspace_bytes(v, members);
    if (ws_bytes < need) return fail(QLE_ERR_INVALID, "workspace of %lld bytes is too small: qbk_workspace_bytes says %lld", (long long)ws_bytes, (long long)need);
    const uintptr_t w0 = reinterpret_cast<uintptr_t>(workspace), s0 = reinterpret_cast<uintptr_t>(v->state);
    const uintptr_t state_bytes = (uintptr_t)(v->padded_batch * (int64_t)kSW * elt(v));
    if (w0 < s0 + state_bytes && s0 < w0 + (uintptr_t)ws_bytes) return fail(QLE_ERR_INVALID, "workspace overlaps view->state: the fuse never writes the records it reads");
    if (!fused) return fail(QLE_ERR_INVALID, "fused is null");
    if (!host) {
        if (!aligned(logw, 8) || !aligned(w, 8)) return fail(QLE_ERR_INVALID, "logw and w must be 8-byte aligned");
        if (!aligned(best, 4)) return fail(QLE_ERR_INVALID, "best must be 4-byte aligned");
    }
    return QLE_OK;
}

// the launch and the fused view; the arguments are checked
template <typename T>
static int launch_t(const qle_device_view* v, int32_t members, const double* logw, const uint8_t* mask, void* workspace, double* w, int32_t* best)
{
    const int64_t out_tiles = padded_filters(v->batch / members) / kTile;
    const dim3 grid((unsigned)(out_tiles * members));   // >= the input tiles; the workgroups past them fill the last output tile
    return with(v->compact != 0, [&](auto k) {
        return launch(k_bank_fuse<T, decltype(k)::value>, grid, dim3(kTile), 0, stream_of(v), (const T*)v->state, (T*)workspace, logw, mask, w, best,
                      v->batch, members, (int32_t)(v->padded_batch / kTile));
    });
}

static int run(const qle_device_view* v, int32_t members, const double* logw, const uint8_t* mask, void* workspace, qle_device_view* fused, double* w,
               int32_t* best)
{
    const qle_device_view in = *v;   // fused may be the struct the caller passed as view
    QLE_TRY(in.dtype == QLE_F32 ? launch_t<float>(&in, members, logw, mask, workspace, w, best) : launch_t<double>(&in, members, logw, mask, workspace, w, best));
    *fused = in;
    fused->batch = in.batch / members;
    fused->padded_batch = padded_filters(fused->batch);
    fused->state = workspace;
    fused->filter_params = nullptr;
    return QLE_OK;
}

extern "C" int qbk_fuse(const qle_device_view* view, int32_t members, const double* logw, const uint8_t* mask, void* workspace, int64_t ws_bytes,
                        qle_device_view* fused, double* w, int32_t* best)
{
    QLE_TRY(check_args(view, members, logw, workspace, ws_bytes, fused, w, best, false));
    QLE_TRY(use_device(view));
    return run(view, members, logw, mask, workspace, fused, w, best);
}

extern "C" int qbk_fuse_host(const qle_device_view* view, int32_t members, const double* logw, const uint8_t* mask, void* workspace, int64_t ws_bytes,
                             qle_device_view* fused, double* w, int32_t* best)
{
    QLE_TRY(check_args(view, members, logw, workspace, ws_bytes, fused, w, best, true));
    QLE_TRY(use_device(view));
    hipStream_t s = stream_of(view);
    const size_t B = (size_t)view->batch, G = B / (size_t)members;
    DeviceMem own;
    void* d[4] = {};
    HIP_TRY(own.acquire({{d[0], B * sizeof(double)}, {d[1], mask ? B : 0}, {d[2], w ? B * sizeof(double) : 0}, {d[3], best ? G * sizeof(int32_t) : 0}}));
    HIP_TRY(hipMemcpyAsync(d[0], logw, B * sizeof(double), hipMemcpyHostToDevice, s));
    if (mask) HIP_TRY(hipMemcpyAsync(d[1], mask, B, hipMemcpyHostToDevice, s));
    QLE_TRY(run(view, members, (const double*)d[0], (const uint8_t*)d[1], workspace, fused, (double*)d[2], (int32_t*)d[3]));
    if (w) HIP_TRY(hipMemcpyAsync(w, d[2], B * sizeof(double), hipMemcpyDeviceToHost, s));
    if (best) HIP_TRY(hipMemcpyAsync(best, d[3], G * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return QLE_OK;
}
