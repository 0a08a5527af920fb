// health_capi.hip -- C ABI of include/qle_health.h over ekf_health.hpp.  Host side: argument checks (every refusal before any GPU
// call), the partials buffer of the batch summary, and the launches on the view's stream.  Works from the view struct of
// include/qle_ekf.h alone; links the HIP runtime only.
#include "../../include/qle_health.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>

#include "ekf_health.hpp"

using namespace qle;

static_assert(sizeof(qhl_summary) == kHealthSums * sizeof(double), "k_health_reduce writes the summary as nine doubles");
static_assert(QHL_ALL == kHealthAllBits && QHL_NONFINITE == kHealthNonfinite && QHL_NOT_PD == kHealthNotPd && QHL_QNORM == kHealthQnorm &&
              QHL_SIGMA_R == kHealthSigmaR && QHL_SIGMA_V == kHealthSigmaV && QHL_SIGMA_THETA == kHealthSigmaTheta, "the bits of the header");

static thread_local std::string g_err;
static std::atomic<int64_t> g_launches{0};

static int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(QLE_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
#define QHL_TRY(expr)                  \
    do {                               \
        int rc_ = (expr);              \
        if (rc_ != QLE_OK) return rc_; \
    } while (0)

extern "C" const char* qhl_last_error(void) { return g_err.c_str(); }
extern "C" int64_t qhl_launch_count(void) { return g_launches.load(std::memory_order_relaxed); }

static bool aligned(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

// what every entry refuses about the view; no GPU call
static int check_view(const qle_device_view* v)
{
    if (!v) return fail(QLE_ERR_INVALID, "view is null");
    if (v->struct_size < sizeof(qle_device_view)) return fail(QLE_ERR_INVALID, "view: struct_size %u, this library was built for %zu", v->struct_size, sizeof(qle_device_view));
    if (v->dtype != QLE_F32 && v->dtype != QLE_F64) return fail(QLE_ERR_INVALID, "view: dtype %d", v->dtype);
    if (v->batch <= 0 || v->padded_batch != padded_filters(v->batch)) return fail(QLE_ERR_INVALID, "view: batch %lld / padded %lld", (long long)v->batch, (long long)v->padded_batch);
    if (!v->state || v->state_words != kSW) return fail(QLE_ERR_INVALID, "view: state records of %d words (this library: %d)", v->state_words, kSW);
    if (!aligned(v->state, 16)) return fail(QLE_ERR_INVALID, "view: state must be 16-byte aligned");
    if (v->num_states != 15 && v->num_states != 9) return fail(QLE_ERR_INVALID, "view: num_states %d", v->num_states);
    if (v->compact && v->num_states != 9) return fail(QLE_ERR_INVALID, "view: compact records with num_states %d", v->num_states);
    return QLE_OK;
}

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

// The [tiles][9] partials of a summary: one buffer per (device, stream), grown on demand and kept -- two calls on one stream are
// ordered, two streams never share a buffer.
static std::mutex g_mu;
static std::map<std::pair<int, void*>, std::pair<double*, int64_t>> g_partials;

static int partials_for(const qle_device_view* v, int64_t tiles, double** out)
{
    std::lock_guard<std::mutex> lk(g_mu);
    auto& slot = g_partials[{v->device, v->stream}];
    if (slot.second < tiles) {
        if (slot.first) {
            HIP_TRY(hipStreamSynchronize((hipStream_t)v->stream));   // a launch that reads the old buffer may be in flight
            HIP_TRY(hipFree(slot.first));
            slot = {nullptr, 0};
        }
        double* buf = nullptr;
        HIP_TRY(hipMalloc(&buf, (size_t)tiles * kHealthSums * sizeof(double)));
        slot = {buf, tiles};
    }
    *out = slot.first;
    return QLE_OK;
}

static int launched()
{
    HIP_TRY(hipGetLastError());
    g_launches.fetch_add(1, std::memory_order_relaxed);   // counts launches the runtime took, not attempts
    return QLE_OK;
}

template <typename T>
static int health_t(const qle_device_view* v, const HealthLimits& lim, const uint8_t* mask, uint8_t* status, uint8_t* flagged, double* summary)
{
    const int64_t tiles = v->padded_batch / kTile;
    double* partials = nullptr;
    if (summary) QHL_TRY(partials_for(v, tiles, &partials));
    const dim3 grid((unsigned)tiles), block(kTile);
    hipStream_t s = (hipStream_t)v->stream;
    auto go = [&](auto compact, auto n) {
        hipLaunchKernelGGL((k_health<T, decltype(compact)::value, decltype(n)::value>), grid, block, 0, s, (const T*)v->state, v->batch, mask, status, flagged,
                           partials, lim);
    };
    if (v->compact) go(std::true_type{}, std::integral_constant<int, 9>{});
    else if (v->num_states == 9) go(std::false_type{}, std::integral_constant<int, 9>{});
    else go(std::false_type{}, std::integral_constant<int, 15>{});
    QHL_TRY(launched());
    if (summary) {
        hipLaunchKernelGGL(k_health_reduce, dim3(1), dim3(kBlock), 0, s, (const double*)partials, tiles, summary);
        QHL_TRY(launched());
    }
    return QLE_OK;
}

extern "C" int qhl_health(const qle_device_view* view, const qhl_limits* limits, const uint8_t* mask, uint8_t* status, uint8_t* flagged,
                          qhl_summary* summary)
{
    QHL_TRY(check_view(view));
    QHL_TRY(check_limits(limits));
    if (!aligned(summary, 8)) return fail(QLE_ERR_INVALID, "summary must be 8-byte aligned");
    if (!status && !flagged && !summary) return QLE_OK;
    HealthLimits lim;
    lim.r2 = limits->sigma_r_max * limits->sigma_r_max;
    lim.v2 = limits->sigma_v_max * limits->sigma_v_max;
    lim.th2 = limits->sigma_theta_max * limits->sigma_theta_max;
    lim.qnorm_tol = limits->qnorm_tol;
    lim.select = limits->select;
    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(view->device));
    double* sum = reinterpret_cast<double*>(summary);
    return view->dtype == QLE_F32 ? health_t<float>(view, lim, mask, status, flagged, sum) : health_t<double>(view, lim, mask, status, flagged, sum);
}

extern "C" int qhl_retire(const qle_device_view* view, const uint8_t* mask)
{
    QHL_TRY(check_view(view));
    if (!mask) return fail(QLE_ERR_INVALID, "mask is null: retiring every filter has to be asked for with a mask of ones");
    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(view->device));
    const dim3 grid((unsigned)(view->padded_batch / kTile)), block(kTile);
    hipStream_t s = (hipStream_t)view->stream;
    if (view->dtype == QLE_F32) hipLaunchKernelGGL(k_retire<float>, grid, block, 0, s, (float*)view->state, mask, view->batch, view->compact);
    else hipLaunchKernelGGL(k_retire<double>, grid, block, 0, s, (double*)view->state, mask, view->batch, view->compact);
    return launched();
}

extern "C" int qhl_and_masks(const qle_device_view* view, const uint8_t* a, const uint8_t* b, uint8_t* out)
{
    QHL_TRY(check_view(view));
    if (!a || !b || !out) return fail(QLE_ERR_INVALID, "a, b and out must not be null");
    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(view->device));
    hipLaunchKernelGGL(k_and_masks, dim3((unsigned)((view->batch + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)view->stream, a, b, out, view->batch);
    return launched();
}

namespace {
// device buffers of one qhl_health_host call, freed however the call ends
struct Staging {
    void* p[4] = {nullptr, nullptr, nullptr, nullptr};
    ~Staging() { for (void* q : p) if (q) (void)hipFree(q); }
};
}  // namespace

extern "C" int qhl_health_host(const qle_device_view* view, const qhl_limits* limits, const uint8_t* mask, uint8_t* status, uint8_t* flagged,
                               qhl_summary* summary)
{
    QHL_TRY(check_view(view));
    QHL_TRY(check_limits(limits));
    if (!status && !flagged && !summary) return QLE_OK;
    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(view->device));
    hipStream_t s = (hipStream_t)view->stream;
    const size_t B = (size_t)view->batch;
    Staging d;
    if (mask) {
        HIP_TRY(hipMalloc(&d.p[0], B));
        HIP_TRY(hipMemcpyAsync(d.p[0], mask, B, hipMemcpyHostToDevice, s));
    }
    if (status) HIP_TRY(hipMalloc(&d.p[1], B));
    if (flagged) HIP_TRY(hipMalloc(&d.p[2], B));
    if (summary) HIP_TRY(hipMalloc(&d.p[3], sizeof(qhl_summary)));
    QHL_TRY(qhl_health(view, limits, (const uint8_t*)d.p[0], (uint8_t*)d.p[1], (uint8_t*)d.p[2], (qhl_summary*)d.p[3]));
    if (status) HIP_TRY(hipMemcpyAsync(status, d.p[1], B, hipMemcpyDeviceToHost, s));
    if (flagged) HIP_TRY(hipMemcpyAsync(flagged, d.p[2], B, hipMemcpyDeviceToHost, s));
    if (summary) HIP_TRY(hipMemcpyAsync(summary, d.p[3], sizeof(qhl_summary), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return QLE_OK;
}
