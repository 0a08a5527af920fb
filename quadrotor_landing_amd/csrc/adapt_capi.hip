// adapt_capi.hip -- C ABI of include/qle_adapt.h over ekf_adapt.hpp.  Host side: argument checks (every refusal before any GPU call),
// ONE launch per observed tick and ONE per apply on the view's stream, and the C loop of qad_run over qad's own launches and qle_run of
// the tick library (qsc_run's loop with another kernel and an apply every window-th tag-slot tick).  Links libqle_ekf.so for
// qle_params_derive, the two view calls, qle_run and qle_get_filter_params, and derives the launch's parameter block as the handle does
// (ekf_params.hpp); derive, inputs_view and check_run are side_run_host.hpp's.
#include "../../include/qle_adapt.h"

#include <cmath>
#include <vector>

#include "ekf_adapt.hpp"
#include "ekf_params.hpp"
#include "side_run_host.hpp"

using namespace qle;
using namespace qle::side;

static_assert(QAD_WORDS == kAdaptWords, "the header publishes the accumulator record of ekf_adapt.hpp");

QLE_SIDE_LAST_ERROR(qad_last_error)
QLE_SIDE_LAUNCH_COUNT(qad_launch_count)

// What every entry refuses about params, about a device accumulator array and about a configuration; no GPU call.  multirate_ekf is
// QLE_ERR_STATE, the gate's own rule, and stays ahead of everything that is refused about the handle or the view.
static int check_params(const qle_params* p)
{
    if (!p) return fail(QLE_ERR_INVALID, "params is null");
    if (p->multirate_ekf) return fail(QLE_ERR_STATE, "noise adaptation does not support multirate_ekf: a delayed measurement's innovation belongs to a history entry");
    return QLE_OK;
}
static int check_acc(const double* acc)
{
    if (!acc) return fail(QLE_ERR_INVALID, "acc is null");
    if (!aligned(acc, 16)) return fail(QLE_ERR_INVALID, "acc must be 16-byte aligned");
    return QLE_OK;
}
static int check_chi2(double chi2_max)
{
    if (std::isnan(chi2_max) || chi2_max <= 0.0) return fail(QLE_ERR_INVALID, "chi2_max must be > 0 (+inf: no limit), got %g", chi2_max);
    return QLE_OK;
}
static int check_cfg(const qad_config* c)
{
    if (!c) return fail(QLE_ERR_INVALID, "cfg is null");
    if (c->struct_size < sizeof(qad_config)) return fail(QLE_ERR_INVALID, "cfg: struct_size %u, this library was built for %zu", c->struct_size, sizeof(qad_config));
    if (c->window < 1) return fail(QLE_ERR_INVALID, "cfg: window must be >= 1, got %d", c->window);
    if (!(c->gain > 0.0 && c->gain <= 1.0)) return fail(QLE_ERR_INVALID, "cfg: gain must lie in (0, 1], got %g", c->gain);
    if (c->n_min < 1) return fail(QLE_ERR_INVALID, "cfg: n_min must be >= 1, got %d", c->n_min);
    QLE_TRY(check_chi2(c->chi2_max));
    for (int k = 0; k < 6; ++k) {
        if (!std::isfinite(c->R_lo[k]) || c->R_lo[k] <= 0.0) return fail(QLE_ERR_INVALID, "cfg: R_lo[%d] must be finite and > 0, got %g", k, c->R_lo[k]);
        if (!(c->R_hi[k] >= c->R_lo[k])) return fail(QLE_ERR_INVALID, "cfg: R_hi[%d] = %g is below R_lo[%d] = %g", k, c->R_hi[k], k, c->R_lo[k]);
    }
    return QLE_OK;
}
// the estimate is written into the per-filter parameter records: they have to be in force
static int check_pfp(const qle_device_view* v)
{
    if (!v->filter_params) return fail(QLE_ERR_STATE, "per-filter parameters are not in force (qle_set_filter_params first)");
    return QLE_OK;
}
// The view and the tick's inputs view; the view may be larger than this library's (a smaller one is refused).
static int check_tick(const qle_device_view* v, const qle_inputs_view* in, const qle_params* p)
{
    if (!in) return fail(QLE_ERR_INVALID, "inputs view is null");
    if (in->struct_size < sizeof(qle_inputs_view)) return fail(QLE_ERR_INVALID, "inputs view: struct_size %u, this library was built for %zu", in->struct_size, sizeof(qle_inputs_view));
    QLE_TRY(check_view(v, ViewSize::at_least, false));
    if (!in->z) return fail(QLE_ERR_INVALID, "the tick has no tag slot");
    if (!in->u) return fail(QLE_ERR_INVALID, "the tick has no IMU records");
    if (v->num_states != (p->est_bias ? 15 : 9)) return fail(QLE_ERR_INVALID, "view: num_states %d, params: est_bias %d", v->num_states, p->est_bias);
    return check_pfp(v);
}

template <typename T>
static int observe_t(const qle_device_view* v, const qle_inputs_view* in, const qle_params& pub, const qle_derived& der, double* acc, double chi2_max)
{
    DevParams<T> dp = make_dev<T>(pub, der);
    dp.compact = v->compact ? 1 : 0;
    auto go = [&](auto direct, auto compact) {
        hipLaunchKernelGGL((k_adapt_observe<T, decltype(direct)::value, decltype(compact)::value>), tiles(v), dim3(kTile), 0, stream_of(v), (const T*)v->state,
                           (const T*)in->u, (const T*)in->z, v->batch, (const T*)v->filter_params, acc, v->padded_batch, chi2_max, dp);
    };
    with(pub.direct_orien_method != 0, [&](auto d) { with(v->compact != 0, [&](auto c) { go(d, c); }); });
    return launched();
}
// behind every refusal and use_device
static int observe_tick(const qle_device_view* v, const qle_inputs_view* in, const qle_params& pub, const qle_derived& der, double* acc, double chi2_max)
{
    return v->dtype == QLE_F32 ? observe_t<float>(v, in, pub, der, acc, chi2_max) : observe_t<double>(v, in, pub, der, acc, chi2_max);
}
static int apply(const qle_device_view* v, double* acc, const qad_config& c, uint8_t* applied, double* R_out)
{
    AdaptApplyCfg k;
    k.gain = c.gain;
    k.n_min = (double)c.n_min;
    for (int j = 0; j < 6; ++j) { k.lo[j] = c.R_lo[j]; k.hi[j] = c.R_hi[j]; }
    if (v->dtype == QLE_F32)
        hipLaunchKernelGGL(k_adapt_apply<float>, tiles(v), dim3(kTile), 0, stream_of(v), (float*)v->filter_params, acc, v->batch, v->padded_batch, k, applied, R_out);
    else
        hipLaunchKernelGGL(k_adapt_apply<double>, tiles(v), dim3(kTile), 0, stream_of(v), (double*)v->filter_params, acc, v->batch, v->padded_batch, k, applied, R_out);
    return launched();
}

extern "C" int qad_observe_tick(const qle_device_view* view, const qle_inputs_view* in, const qle_params* params, double* acc, double chi2_max)
{
    QLE_TRY(check_params(params));
    QLE_TRY(check_acc(acc));
    QLE_TRY(check_chi2(chi2_max));
    QLE_TRY(check_tick(view, in, params));
    qle_derived der;
    QLE_TRY(derive(params, &der));
    QLE_TRY(use_device(view));
    return observe_tick(view, in, *params, der, acc, chi2_max);
}

extern "C" int qad_apply(const qle_device_view* view, double* acc, const qad_config* cfg, uint8_t* applied, double* R_out)
{
    QLE_TRY(check_view(view, ViewSize::at_least, false));
    QLE_TRY(check_acc(acc));
    QLE_TRY(check_cfg(cfg));
    if (R_out && !aligned(R_out, 8)) return fail(QLE_ERR_INVALID, "R_out must be 8-byte aligned");
    QLE_TRY(check_pfp(view));
    QLE_TRY(use_device(view));
    return apply(view, acc, *cfg, applied, R_out);
}

// ---- qad_run
// behind every refusal and use_device
static int run_loop(qle_batch* h, const qle_device_view* v, const qle_inputs* in, int64_t t0, int64_t n, const qle_params& pub, const qle_derived& der, double* acc,
                    const qad_config& c)
{
    int64_t tags = 0;
    for (int64_t t = t0; t < t0 + n; ++t) {
        qle_inputs_view iv;
        QLE_TRY(inputs_view(in, t, &iv));
        if (iv.z) {
            if (!iv.u) return fail(QLE_ERR_INVALID, "tick %lld has no IMU records", (long long)t);
            QLE_TRY(observe_tick(v, &iv, pub, der, acc, c.chi2_max));
        }
        if (int rc = qle_run(h, in, t, 1)) return fail(rc, "qle_run at tick %lld: %s", (long long)t, qle_last_error());
        if (iv.z && ++tags % c.window == 0) QLE_TRY(apply(v, acc, c, nullptr, nullptr));
    }
    return QLE_OK;
}

extern "C" int qad_run(qle_batch* h, const qle_inputs* in, int64_t t0, int64_t n, const qle_params* params, double* acc, const qad_config* cfg)
{
    QLE_TRY(check_params(params));
    QLE_TRY(check_acc(acc));
    QLE_TRY(check_cfg(cfg));
    qle_device_view v;
    QLE_TRY(check_run(h, in, t0, n, params, &v));
    QLE_TRY(check_pfp(&v));
    qle_derived der;
    QLE_TRY(derive(params, &der));
    if (n == 0) return QLE_OK;
    QLE_TRY(use_device(&v));
    return run_loop(h, &v, in, t0, n, *params, der, acc, *cfg);
}

extern "C" int qad_run_host(qle_batch* h, const qle_inputs* in, int64_t t0, int64_t n, const qle_params* params, const qad_config* cfg, double* acc_host,
                            double* R_host)
{
    QLE_TRY(check_params(params));
    if (!acc_host) return fail(QLE_ERR_INVALID, "acc_host is null");   // host arrays: no alignment to ask for
    if (!R_host) return fail(QLE_ERR_INVALID, "R_host is null");
    QLE_TRY(check_cfg(cfg));
    qle_device_view v;
    QLE_TRY(check_run(h, in, t0, n, params, &v));
    QLE_TRY(check_pfp(&v));
    qle_derived der;
    QLE_TRY(derive(params, &der));
    QLE_TRY(use_device(&v));
    hipStream_t s = stream_of(&v);
    const size_t B = (size_t)v.batch, Bp = (size_t)v.padded_batch;
    DeviceMem own;
    double* acc = nullptr;
    HIP_TRY(own.acquire({{acc, (size_t)kAdaptWords * Bp * sizeof(double), true}}, s));
    QLE_TRY(run_loop(h, &v, in, t0, n, *params, der, acc, *cfg));
    HIP_TRY(hipMemcpy2DAsync(acc_host, B * sizeof(double), acc, Bp * sizeof(double), B * sizeof(double), kAdaptWords, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    // the records are the only copy of the adapted values: read them back as every caller does
    std::vector<double> pfp(B * kFW);
    if (int rc = qle_get_filter_params(h, pfp.data())) return fail(rc, "qle_get_filter_params: %s", qle_last_error());
    for (size_t i = 0; i < B; ++i)
        for (int k = 0; k < 6; ++k) R_host[i * 6 + k] = pfp[i * kFW + 18 + k];
    return QLE_OK;
}
