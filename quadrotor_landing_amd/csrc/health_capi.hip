// health_capi.hip -- C ABI of include/qle_health.h over ekf_health.hpp.  Host side: argument checks (every refusal before any GPU
// call), the partials buffer of the batch summary, and the launches on the view's stream.  Works from the view struct of
// include/qle_ekf.h alone; links the HIP runtime only.
#include "../../include/qle_health.h"

#include <cmath>

#include "ekf_health.hpp"
#include "side_host.hpp"

using namespace qle;
using namespace qle::side;

static_assert(sizeof(qhl_summary) == kHealthSums * sizeof(double), "k_health_reduce writes the summary as nine doubles");
static_assert(QHL_ALL == kHealthAllBits && QHL_NONFINITE == kHealthNonfinite && QHL_NOT_PD == kHealthNotPd && QHL_QNORM == kHealthQnorm &&
              QHL_SIGMA_R == kHealthSigmaR && QHL_SIGMA_V == kHealthSigmaV && QHL_SIGMA_THETA == kHealthSigmaTheta, "the bits of the header");

QLE_SIDE_LAST_ERROR(qhl_last_error)
QLE_SIDE_LAUNCH_COUNT(qhl_launch_count)
QLE_SIDE_LAUNCH_CENSUS(qhl)

// what every entry refuses about the view; no GPU call.  The view may be larger than this library's (a smaller one is refused); the
// kernels read the records in 16-byte rows, so the records have to be aligned.
static int check_view(const qle_device_view* v) { return check_view(v, ViewSize::at_least, true); }

static int check_limits(const qhl_limits* l)
{
    if (!l) return fail(QLE_ERR_INVALID, "limits is null");
    if (l->struct_size != sizeof(qhl_limits)) return fail(QLE_ERR_INVALID, "limits: struct_size %u, this library was built for %zu", l->struct_size, sizeof(qhl_limits));
    if (l->select == 0 || (l->select & ~kHealthAllBits)) return fail(QLE_ERR_INVALID, "select 0x%x: expected a non-empty selection of the status bits 0x%x", l->select, kHealthAllBits);
    const struct { const char* name; double v; } lims[] = {{"sigma_r_max", l->sigma_r_max}, {"sigma_v_max", l->sigma_v_max}, {"sigma_theta_max", l->sigma_theta_max}, {"qnorm_tol", l->qnorm_tol}};
    for (const auto& m : lims)
        if (!(m.v > 0.0)) return fail(QLE_ERR_INVALID, "%s must be > 0 (got %g)", m.name, m.v);
    return QLE_OK;
}

static Partials g_partials(kHealthSums);   // the [tiles][9] partials of a summary

template <typename T>
static int health_t(const qle_device_view* v, const HealthLimits& lim, const uint8_t* mask, uint8_t* status, uint8_t* flagged, double* summary)
{
    const int64_t tiles = v->padded_batch / kTile;
    double* partials = nullptr;
    if (summary) QLE_TRY(g_partials.get(v, tiles, &partials));
    const dim3 grid((unsigned)tiles), block(kTile);
    hipStream_t s = (hipStream_t)v->stream;
    auto go = [&](auto compact, auto n) {
        return launch(k_health<T, decltype(compact)::value, decltype(n)::value>, grid, block, 0, s, (const T*)v->state, v->batch, mask, status, flagged,
                      partials, lim);
    };
    if (v->compact) QLE_TRY(go(std::true_type{}, std::integral_constant<int, 9>{}));
    else if (v->num_states == 9) QLE_TRY(go(std::false_type{}, std::integral_constant<int, 9>{}));
    else QLE_TRY(go(std::false_type{}, std::integral_constant<int, 15>{}));
    if (summary) QLE_TRY(launch(k_health_reduce, dim3(1), dim3(kBlock), 0, s, (const double*)partials, tiles, summary));
    return QLE_OK;
}

extern "C" int qhl_health(const qle_device_view* view, const qhl_limits* limits, const uint8_t* mask, uint8_t* status, uint8_t* flagged,
                          qhl_summary* summary)
{
    QLE_TRY(check_view(view));
    QLE_TRY(check_limits(limits));
    if (!aligned(summary, 8)) return fail(QLE_ERR_INVALID, "summary must be 8-byte aligned");
    if (!status && !flagged && !summary) return QLE_OK;
    HealthLimits lim;
    lim.r2 = limits->sigma_r_max * limits->sigma_r_max;
    lim.v2 = limits->sigma_v_max * limits->sigma_v_max;
    lim.th2 = limits->sigma_theta_max * limits->sigma_theta_max;
    lim.qnorm_tol = limits->qnorm_tol;
    lim.select = limits->select;
    QLE_TRY(use_device(view));
    double* sum = reinterpret_cast<double*>(summary);
    return view->dtype == QLE_F32 ? health_t<float>(view, lim, mask, status, flagged, sum) : health_t<double>(view, lim, mask, status, flagged, sum);
}

extern "C" int qhl_retire(const qle_device_view* view, const uint8_t* mask)
{
    QLE_TRY(check_view(view));
    if (!mask) return fail(QLE_ERR_INVALID, "mask is null: retiring every filter has to be asked for with a mask of ones");
    QLE_TRY(use_device(view));
    const dim3 grid((unsigned)(view->padded_batch / kTile)), block(kTile);
    hipStream_t s = (hipStream_t)view->stream;
    if (view->dtype == QLE_F32) return launch(k_retire<float>, grid, block, 0, s, (float*)view->state, mask, view->batch, view->compact);
    return launch(k_retire<double>, grid, block, 0, s, (double*)view->state, mask, view->batch, view->compact);
}

extern "C" int qhl_and_masks(const qle_device_view* view, const uint8_t* a, const uint8_t* b, uint8_t* out)
{
    QLE_TRY(check_view(view));
    if (!a || !b || !out) return fail(QLE_ERR_INVALID, "a, b and out must not be null");
    QLE_TRY(use_device(view));
    return launch(k_and_masks, dim3((unsigned)((view->batch + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)view->stream, a, b, out, view->batch);
}

extern "C" int qhl_health_host(const qle_device_view* view, const qhl_limits* limits, const uint8_t* mask, uint8_t* status, uint8_t* flagged,
                               qhl_summary* summary)
{
    QLE_TRY(check_view(view));
    QLE_TRY(check_limits(limits));
    if (!status && !flagged && !summary) return QLE_OK;
    QLE_TRY(use_device(view));
    hipStream_t s = (hipStream_t)view->stream;
    const size_t B = (size_t)view->batch;
    DeviceMem own;
    void* d[4] = {};
    HIP_TRY(own.acquire({{d[0], mask ? B : 0}, {d[1], status ? B : 0}, {d[2], flagged ? B : 0}, {d[3], summary ? sizeof(qhl_summary) : 0}}));
    if (mask) HIP_TRY(hipMemcpyAsync(d[0], mask, B, hipMemcpyHostToDevice, s));
    QLE_TRY(qhl_health(view, limits, (const uint8_t*)d[0], (uint8_t*)d[1], (uint8_t*)d[2], (qhl_summary*)d[3]));
    if (status) HIP_TRY(hipMemcpyAsync(status, d[1], B, hipMemcpyDeviceToHost, s));
    if (flagged) HIP_TRY(hipMemcpyAsync(flagged, d[2], B, hipMemcpyDeviceToHost, s));
    if (summary) HIP_TRY(hipMemcpyAsync(summary, d[3], sizeof(qhl_summary), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return QLE_OK;
}
