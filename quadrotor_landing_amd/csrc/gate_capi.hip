// gate_capi.hip -- C ABI of include/qle_gate.h over ekf_pregate.hpp.  Host side: argument checks (every refusal before any GPU call)
// and ONE launch on the view's stream.  Works from the view structs of include/qle_ekf.h and the public parameters; links
// libqle_ekf.so for qle_params_derive and derives the launch's parameter block as the handle does (ekf_params.hpp).
#include "../../include/qle_gate.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>

#include "ekf_params.hpp"
#include "ekf_pregate.hpp"

using namespace qle;

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
#define QGT_TRY(expr)                  \
    do {                               \
        int rc_ = (expr);              \
        if (rc_ != QLE_OK) return rc_; \
    } while (0)

extern "C" const char* qgt_last_error(void) { return g_err.c_str(); }
extern "C" int64_t qgt_launch_count(void) { return g_launches.load(std::memory_order_relaxed); }

// Everything that can be refused, in the order include/qle_gate.h lists it; no GPU call.
static int check_args(const qle_device_view* v, const qle_inputs_view* in, const qle_params* p, bool gate, double chi2_max, int32_t dst_dtype)
{
    if (!v) return fail(QLE_ERR_INVALID, "view is null");
    if (v->struct_size < sizeof(qle_device_view)) return fail(QLE_ERR_INVALID, "view: struct_size %u, this library was built for %zu", v->struct_size, sizeof(qle_device_view));
    if (!in) return fail(QLE_ERR_INVALID, "inputs view is null");
    if (in->struct_size < sizeof(qle_inputs_view)) return fail(QLE_ERR_INVALID, "inputs view: struct_size %u, this library was built for %zu", in->struct_size, sizeof(qle_inputs_view));
    if (!p) return fail(QLE_ERR_INVALID, "params is null");
    if (p->multirate_ekf) return fail(QLE_ERR_STATE, "the gate does not support multirate_ekf: a delayed measurement's innovation belongs to a history entry");
    if (!in->z) return fail(QLE_ERR_INVALID, "the tick has no tag slot");
    if (gate && !in->u) return fail(QLE_ERR_INVALID, "the tick has no IMU records");
    if (gate && !(chi2_max > 0.0)) return fail(QLE_ERR_INVALID, "chi2_max must be > 0 (got %g)", chi2_max);
    if (dst_dtype != QGT_F32 && dst_dtype != QGT_F64) return fail(QLE_ERR_INVALID, "dst_dtype must be QGT_F32 or QGT_F64 (got %d)", dst_dtype);
    if (v->dtype != QLE_F32 && v->dtype != QLE_F64) return fail(QLE_ERR_INVALID, "view: dtype %d", v->dtype);
    if (v->batch <= 0 || v->padded_batch != padded_filters(v->batch)) return fail(QLE_ERR_INVALID, "view: batch %lld / padded %lld", (long long)v->batch, (long long)v->padded_batch);
    if (!v->state || v->state_words != kSW) return fail(QLE_ERR_INVALID, "view: state records of %d words (this library: %d)", v->state_words, kSW);
    if (v->num_states != (p->est_bias ? 15 : 9)) return fail(QLE_ERR_INVALID, "view: num_states %d, params: est_bias %d", v->num_states, p->est_bias);
    if (v->compact && v->num_states != 9) return fail(QLE_ERR_INVALID, "view: compact records with num_states %d", v->num_states);
    return QLE_OK;
}

struct Outs { void* nis; uint8_t* accepted; void* nu; void* S; int32_t f64; double chi2_max; };

template <typename T, bool PREDICT>
static int launch_t(const qle_device_view* v, const qle_inputs_view* in, const qle_params& pub, const qle_derived& der, const Outs& o)
{
    DevParams<T> dp = make_dev<T>(pub, der);
    dp.compact = v->compact ? 1 : 0;
    const dim3 grid((unsigned)(v->padded_batch / kTile)), block(kTile);
    hipStream_t s = (hipStream_t)v->stream;
    auto go = [&](auto direct, auto pfp, auto compact) {
        hipLaunchKernelGGL((k_pregate<T, decltype(direct)::value, decltype(pfp)::value, decltype(compact)::value, PREDICT>), grid, block, 0, s,
                           (const T*)v->state, (const T*)in->u, (T*)in->z, v->batch, (const T*)v->filter_params, o.nis, o.accepted, o.nu, o.S, o.f64, o.chi2_max, dp);
    };
    auto with = [](bool b, auto&& f) { if (b) f(std::true_type{}); else f(std::false_type{}); };
    with(pub.direct_orien_method != 0, [&](auto d) { with(v->filter_params != nullptr, [&](auto f) { with(v->compact != 0, [&](auto c) { go(d, f, c); }); }); });
    HIP_TRY(hipGetLastError());
    g_launches.fetch_add(1, std::memory_order_relaxed);   // counts launches the runtime took, not attempts
    return QLE_OK;
}

template <bool PREDICT>
static int run(const qle_device_view* v, const qle_inputs_view* in, const qle_params* p, const Outs& o)
{
    QGT_TRY(check_args(v, in, p, PREDICT, o.chi2_max, o.f64));
    qle_derived der;
    if (qle_params_derive(p, &der) != QLE_OK) return fail(QLE_ERR_INVALID, "params: %s", qle_last_error());
    if (!PREDICT && !o.nis && !o.nu && !o.S) return QLE_OK;
    (void)hipGetLastError();
    HIP_TRY(hipSetDevice(v->device));
    return v->dtype == QLE_F32 ? launch_t<float, PREDICT>(v, in, *p, der, o) : launch_t<double, PREDICT>(v, in, *p, der, o);
}

extern "C" int qgt_gate_tick(const qle_device_view* view, const qle_inputs_view* in, const qle_params* params, double chi2_max, void* nis,
                             uint8_t* accepted, void* nu, void* S, int32_t dst_dtype)
{
    return run<true>(view, in, params, Outs{nis, accepted, nu, S, dst_dtype, chi2_max});
}

extern "C" int qgt_innovation(const qle_device_view* view, const qle_inputs_view* in, const qle_params* params, void* nis, void* nu, void* S,
                              int32_t dst_dtype)
{
    return run<false>(view, in, params, Outs{nis, nullptr, nu, S, dst_dtype, INFINITY});
}
