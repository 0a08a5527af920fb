// lookahead_capi.hip -- C ABI of include/qle_lookahead.h over ekf_lookahead.hpp.  Host side: argument checks (every refusal before any
// GPU call) and ONE launch on the view's stream.  Works from the view struct of include/qle_ekf.h and the public parameters; links
// libqle_ekf.so for qle_params_derive and derives the launch's parameter block as the handle does (ekf_params.hpp).  Allocates nothing:
// the forecast goes into the caller's workspace (the host entry stages its host arrays through buffers of its own).
#include "../../include/qle_lookahead.h"

#include <cmath>

#include "ekf_lookahead.hpp"
#include "ekf_params.hpp"
#include "side_host.hpp"

using namespace qle;
using namespace qle::side;

static_assert(QLK_MAX_HORIZON == kMaxHorizon, "the horizon cap of the header");

QLE_SIDE_LAST_ERROR(qlk_last_error)
QLE_SIDE_LAUNCH_COUNT(qlk_launch_count)
QLE_SIDE_LAUNCH_CENSUS(qlk)

// what every entry refuses about the view; no GPU call.  A view of exactly this library's size (the forecast is a copy of it), with
// 16-byte aligned records.
static int check_view(const qle_device_view* v) { return check_view(v, ViewSize::exact, true); }

static int64_t workspace_bytes(const qle_device_view* v) { return v->padded_batch * (int64_t)kSW * (v->dtype == QLE_F64 ? 8 : 4); }

extern "C" int64_t qlk_workspace_bytes(const qle_device_view* view)
{
    QLE_TRY(check_view(view));
    return workspace_bytes(view);
}

// Everything include/qle_lookahead.h lists as refused, the view first; no GPU call.  host: u, mask and ticks_to_limit are host arrays
// (no alignment to ask for).
static int check_args(const qle_device_view* v, const qle_params* p, const void* u, int32_t u_dtype, int32_t h, const void* workspace,
                      int64_t ws_bytes, const qle_device_view* ahead, const qlk_coast* coast, const int32_t* ticks, bool host, CoastLimits* lim)
{
    QLE_TRY(check_view(v));
    if (!p) return fail(QLE_ERR_INVALID, "params is null");
    if (v->num_states != (p->est_bias ? 15 : 9)) return fail(QLE_ERR_INVALID, "view: num_states %d, params: est_bias %d", v->num_states, p->est_bias);
    if (!u) return fail(QLE_ERR_INVALID, "u is null");
    if (u_dtype != QLK_F32 && u_dtype != QLK_F64) return fail(QLE_ERR_INVALID, "u_dtype must be QLK_F32 or QLK_F64 (got %d)", u_dtype);
    if (h < 0 || h > QLK_MAX_HORIZON) return fail(QLE_ERR_INVALID, "h %d: the horizon must be in 0..%d", h, QLK_MAX_HORIZON);
    if (!workspace) return fail(QLE_ERR_INVALID, "workspace is null");
    if (!aligned(workspace, 16)) return fail(QLE_ERR_INVALID, "workspace must be 16-byte aligned");
    const int64_t need = workspace_bytes(v);
    if (ws_bytes < need) return fail(QLE_ERR_INVALID, "workspace of %lld bytes is too small: qlk_workspace_bytes says %lld", (long long)ws_bytes, (long long)need);
    const uintptr_t w0 = reinterpret_cast<uintptr_t>(workspace), s0 = reinterpret_cast<uintptr_t>(v->state);
    if (w0 < s0 + (uintptr_t)need && s0 < w0 + (uintptr_t)ws_bytes) return fail(QLE_ERR_INVALID, "workspace overlaps view->state: the forecast never writes the records it reads");
    if (!ahead) return fail(QLE_ERR_INVALID, "ahead is null");
    if ((coast == nullptr) != (ticks == nullptr)) return fail(QLE_ERR_INVALID, "coast and ticks_to_limit: both NULL, or both given");
    lim->r2 = lim->th2 = INFINITY;
    if (coast) {
        if (coast->struct_size != sizeof(qlk_coast)) return fail(QLE_ERR_INVALID, "coast: struct_size %u, this library was built for %zu", coast->struct_size, sizeof(qlk_coast));
        if (!(coast->sigma_r_max > 0.0)) return fail(QLE_ERR_INVALID, "sigma_r_max must be > 0 (got %g)", coast->sigma_r_max);
        if (!(coast->sigma_theta_max > 0.0)) return fail(QLE_ERR_INVALID, "sigma_theta_max must be > 0 (got %g)", coast->sigma_theta_max);
        lim->r2 = coast->sigma_r_max * coast->sigma_r_max;
        lim->th2 = coast->sigma_theta_max * coast->sigma_theta_max;
    }
    if (!host) {
        if (!aligned(u, 16)) return fail(QLE_ERR_INVALID, "u must be 16-byte aligned");
        if (!aligned(ticks, 4)) return fail(QLE_ERR_INVALID, "ticks_to_limit must be 4-byte aligned");
    }
    return QLE_OK;
}

struct Call { const void* u; int32_t u_f64; int32_t h; const uint8_t* mask; void* workspace; CoastLimits lim; int32_t* ticks; };

template <typename T>
static int launch_t(const qle_device_view* v, const qle_params& pub, const qle_derived& der, const Call& c)
{
    DevParams<T> dp = make_dev<T>(pub, der);
    dp.compact = v->compact ? 1 : 0;
    auto go = [&](auto pfp, auto compact) {
        return launch(k_lookahead<T, decltype(pfp)::value, decltype(compact)::value>, tiles(v), dim3(kTile), 0, stream_of(v), (const T*)v->state, (T*)c.workspace, c.u,
                      v->batch, c.h, c.u_f64, c.mask, (const T*)v->filter_params, c.ticks, c.lim, dp);
    };
    return with(v->filter_params != nullptr, [&](auto f) { return with(v->compact != 0, [&](auto k) { return go(f, k); }); });
}

// the launch and the forecast view; the arguments are checked
static int run(const qle_device_view* v, const qle_params* p, const qle_derived& der, const Call& c, qle_device_view* ahead)
{
    const qle_device_view in = *v;   // ahead may be the struct the caller passed as view
    QLE_TRY(in.dtype == QLE_F32 ? launch_t<float>(&in, *p, der, c) : launch_t<double>(&in, *p, der, c));
    *ahead = in;
    ahead->state = c.workspace;
    return QLE_OK;
}

extern "C" int qlk_lookahead(const qle_device_view* view, const qle_params* params, const void* u, int32_t u_dtype, int32_t h, const uint8_t* mask,
                             void* workspace, int64_t ws_bytes, qle_device_view* ahead, const qlk_coast* coast, int32_t* ticks_to_limit)
{
    CoastLimits lim;
    QLE_TRY(check_args(view, params, u, u_dtype, h, workspace, ws_bytes, ahead, coast, ticks_to_limit, false, &lim));
    qle_derived der;
    if (qle_params_derive(params, &der) != QLE_OK) return fail(QLE_ERR_INVALID, "params: %s", qle_last_error());
    QLE_TRY(use_device(view));
    return run(view, params, der, Call{u, u_dtype == QLK_F64, h, mask, workspace, lim, ticks_to_limit}, ahead);
}

extern "C" int qlk_lookahead_host(const qle_device_view* view, const qle_params* params, const double* u, int32_t h, const uint8_t* mask,
                                  void* workspace, int64_t ws_bytes, qle_device_view* ahead, const qlk_coast* coast, int32_t* ticks_to_limit)
{
    CoastLimits lim;
    QLE_TRY(check_args(view, params, u, QLK_F64, h, workspace, ws_bytes, ahead, coast, ticks_to_limit, true, &lim));
    qle_derived der;
    if (qle_params_derive(params, &der) != QLE_OK) return fail(QLE_ERR_INVALID, "params: %s", qle_last_error());
    QLE_TRY(use_device(view));
    hipStream_t s = (hipStream_t)view->stream;
    const size_t B = (size_t)view->batch;
    DeviceMem own;
    void* d[3] = {};
    HIP_TRY(own.acquire({{d[0], B * kUW * sizeof(double)}, {d[1], mask ? B : 0}, {d[2], ticks_to_limit ? B * sizeof(int32_t) : 0}}));
    HIP_TRY(hipMemcpyAsync(d[0], u, B * kUW * sizeof(double), hipMemcpyHostToDevice, s));
    if (mask) HIP_TRY(hipMemcpyAsync(d[1], mask, B, hipMemcpyHostToDevice, s));
    QLE_TRY(run(view, params, der, Call{d[0], 1, h, (const uint8_t*)d[1], workspace, lim, (int32_t*)d[2]}, ahead));
    if (ticks_to_limit) HIP_TRY(hipMemcpyAsync(ticks_to_limit, d[2], B * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return QLE_OK;
}
