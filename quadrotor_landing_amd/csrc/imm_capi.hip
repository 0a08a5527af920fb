// imm_capi.hip -- C ABI of include/qle_imm.h over ekf_imm.hpp.  Host side: argument checks (every refusal before any GPU call) and ONE
// launch on the view's stream per call.  Works from the view struct of include/qle_ekf.h and one flag of the parameter struct; links the
// HIP runtime only.  Allocates nothing (the host entry stages its host arrays through buffers of its own).
#include "../../include/qle_imm.h"

#include "ekf_imm.hpp"
#include "side_host.hpp"

using namespace qle;
using namespace qle::side;

static_assert(kBankMaxMembers == kTile, "a bank never leaves one wave tile");

QLE_SIDE_LAST_ERROR(qim_last_error)
QLE_SIDE_LAUNCH_COUNT(qim_launch_count)
QLE_SIDE_LAUNCH_CENSUS(qim)

// what every entry refuses about the view and the geometry (the rules of bank_capi.hip); no GPU call
static int check_geometry(const qle_device_view* v, int32_t members)
{
    QLE_TRY(check_view(v, ViewSize::exact, true));
    if (!bank_members_ok(members)) return fail(QLE_ERR_INVALID, "members %d: expected a power of two in 2..%d", members, kBankMaxMembers);
    if (v->batch % members != 0) return fail(QLE_ERR_INVALID, "batch %lld is not a multiple of members %d", (long long)v->batch, members);
    return QLE_OK;
}

// multirate_ekf is QLE_ERR_STATE, the gate's and the scorer's rule, and stays ahead of everything that is refused about the view
static int check_params(const qle_params* p)
{
    if (!p) return fail(QLE_ERR_INVALID, "params is null");
    if (p->multirate_ekf)
        return fail(QLE_ERR_STATE, "mixing does not support multirate_ekf: the next correcting tick replays from the history and would discard what was mixed into the current state");
    return QLE_OK;
}

// host: logmu, Pi, mask, logc and mixed are host arrays (no alignment to ask for)
static int check_mix(const qle_device_view* v, const qle_params* p, int32_t members, const double* logmu, const double* Pi, const double* logc, bool host)
{
    QLE_TRY(check_params(p));
    QLE_TRY(check_geometry(v, members));
    if (!logmu) return fail(QLE_ERR_INVALID, "logmu is null");
    if (!Pi) return fail(QLE_ERR_INVALID, "Pi is null");
    if (!logc) return fail(QLE_ERR_INVALID, "logc is null");
    if (!host && (!aligned(logmu, 8) || !aligned(Pi, 8) || !aligned(logc, 8))) return fail(QLE_ERR_INVALID, "logmu, Pi and logc must be 8-byte aligned");
    return QLE_OK;
}

template <typename T>
static int launch_mix(const qle_device_view* v, int32_t members, const double* logmu, const double* Pi, const uint8_t* mask, double* logc, uint8_t* mixed)
{
    return with(v->compact != 0, [&](auto k) {
        return launch(k_imm_mix<T, decltype(k)::value>, tiles(v), dim3(kTile), 0, stream_of(v), (T*)v->state, logmu, Pi, mask, logc, mixed, v->batch, members);
    });
}

// behind every refusal and use_device
static int mix(const qle_device_view* v, int32_t members, const double* logmu, const double* Pi, const uint8_t* mask, double* logc, uint8_t* mixed)
{
    return v->dtype == QLE_F32 ? launch_mix<float>(v, members, logmu, Pi, mask, logc, mixed) : launch_mix<double>(v, members, logmu, Pi, mask, logc, mixed);
}

extern "C" int qim_mix(const qle_device_view* view, const qle_params* params, int32_t members, const double* logmu, const double* Pi, const uint8_t* mask,
                       double* logc, uint8_t* mixed)
{
    QLE_TRY(check_mix(view, params, members, logmu, Pi, logc, false));
    QLE_TRY(use_device(view));
    return mix(view, members, logmu, Pi, mask, logc, mixed);
}

extern "C" int qim_update(const qle_device_view* view, int32_t members, const double* logc, const double* loglik, const uint8_t* mask, double logmu_min,
                          double* logmu)
{
    QLE_TRY(check_geometry(view, members));
    if (!logc) return fail(QLE_ERR_INVALID, "logc is null");
    if (!loglik) return fail(QLE_ERR_INVALID, "loglik is null");
    if (!logmu) return fail(QLE_ERR_INVALID, "logmu is null");
    if (!aligned(logc, 8) || !aligned(loglik, 8) || !aligned(logmu, 8)) return fail(QLE_ERR_INVALID, "logc, loglik and logmu must be 8-byte aligned");
    if (logmu_min != logmu_min) return fail(QLE_ERR_INVALID, "logmu_min is NaN");
    QLE_TRY(use_device(view));
    return launch(k_imm_update, tiles(view), dim3(kTile), 0, stream_of(view), logc, loglik, mask, logmu_min, logmu, view->batch, members);
}

extern "C" int qim_mix_host(const qle_device_view* view, const qle_params* params, int32_t members, const double* logmu, const double* Pi, const uint8_t* mask,
                            double* logc, uint8_t* mixed)
{
    QLE_TRY(check_mix(view, params, members, logmu, Pi, logc, true));
    QLE_TRY(use_device(view));
    hipStream_t s = stream_of(view);
    const size_t B = (size_t)view->batch, MM = (size_t)members * (size_t)members;
    DeviceMem own;
    void* d[5] = {};
    HIP_TRY(own.acquire({{d[0], B * sizeof(double)}, {d[1], MM * sizeof(double)}, {d[2], mask ? B : 0}, {d[3], B * sizeof(double)}, {d[4], mixed ? B : 0}}));
    HIP_TRY(hipMemcpyAsync(d[0], logmu, B * sizeof(double), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d[1], Pi, MM * sizeof(double), hipMemcpyHostToDevice, s));
    if (mask) HIP_TRY(hipMemcpyAsync(d[2], mask, B, hipMemcpyHostToDevice, s));
    QLE_TRY(mix(view, members, (const double*)d[0], (const double*)d[1], (const uint8_t*)d[2], (double*)d[3], (uint8_t*)d[4]));
    HIP_TRY(hipMemcpyAsync(logc, d[3], B * sizeof(double), hipMemcpyDeviceToHost, s));
    if (mixed) HIP_TRY(hipMemcpyAsync(mixed, d[4], B, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return QLE_OK;
}
