// adapt_capi.hip -- C ABI of include/qle_adapt.h over ekf_adapt.hpp.  Host side: ONE launch per observed tick and ONE per apply on the
// view's stream, and qad_run as side_run_host.hpp's loop over the observe launch and qle_run of the tick library with an apply behind
// every window-th tag-slot tick.  The refusals it shares with scoring (every one before any GPU call), the launch ladder, the loop and
// the copy to the host are side_run_host.hpp's.  Links libqle_ekf.so for qle_params_derive, the two view calls, qle_run and
// qle_get_filter_params.
#include "../../include/qle_adapt.h"

#include <cmath>
#include <vector>

#include "ekf_adapt.hpp"
#include "side_run_host.hpp"

using namespace qle;
using namespace qle::side;

static_assert(QAD_WORDS == kAdaptWords, "the header publishes the accumulator record of ekf_adapt.hpp");

QLE_SIDE_LAST_ERROR(qad_last_error)
QLE_SIDE_LAUNCH_COUNT(qad_launch_count)
QLE_SIDE_LAUNCH_CENSUS(qad)

static int check_params(const qle_params* p) { return check_observer_params(p, "noise adaptation"); }
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

// behind every refusal and use_device; per-filter parameters are in force (check_pfp)
template <typename T>
static int observe_t(const qle_device_view* v, const qle_inputs_view* in, const qle_params& pub, const qle_derived& der, double* acc, double chi2_max)
{
    return launch_flags<T>(v, pub, der, [&](const DevParams<T>& dp, auto direct, auto, auto compact) {
        return launch(k_adapt_observe<T, decltype(direct)::value, decltype(compact)::value>, tiles(v), dim3(kTile), 0, stream_of(v), (const T*)v->state,
                      (const T*)in->u, (const T*)in->z, v->batch, (const T*)v->filter_params, acc, v->padded_batch, chi2_max, dp);
    });
}
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
        return launch(k_adapt_apply<float>, tiles(v), dim3(kTile), 0, stream_of(v), (float*)v->filter_params, acc, v->batch, v->padded_batch, k, applied, R_out);
    return launch(k_adapt_apply<double>, tiles(v), dim3(kTile), 0, stream_of(v), (double*)v->filter_params, acc, v->batch, v->padded_batch, k, applied, R_out);
}

extern "C" int qad_observe_tick(const qle_device_view* view, const qle_inputs_view* in, const qle_params* params, double* acc, double chi2_max)
{
    QLE_TRY(check_params(params));
    QLE_TRY(check_acc(acc));
    QLE_TRY(check_chi2(chi2_max));
    QLE_TRY(check_tick(view, in, params));
    QLE_TRY(check_pfp(view));
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
// behind every refusal and use_device: an apply behind every window-th tag-slot tick, counted from the start of the call
static int run_loop(qle_batch* h, const qle_device_view* v, const qle_inputs* in, int64_t t0, int64_t n, const qle_params& pub, const qle_derived& der, double* acc,
                    const qad_config& c)
{
    int64_t tags = 0;
    return run_ticks(h, in, t0, n, [&](const qle_inputs_view& iv) { return observe_tick(v, &iv, pub, der, acc, c.chi2_max); },
                     [&] { return ++tags % c.window == 0 ? apply(v, acc, c, nullptr, nullptr) : (int)QLE_OK; });
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
    QLE_TRY(run_to_host(&v, kAdaptWords, acc_host, [&](double* acc) { return run_loop(h, &v, in, t0, n, *params, der, acc, *cfg); }));
    const size_t B = (size_t)v.batch;
    // the records are the only copy of the adapted values: read them back as every caller does
    std::vector<double> pfp(B * kFW);
    if (int rc = qle_get_filter_params(h, pfp.data())) return fail(rc, "qle_get_filter_params: %s", qle_last_error());
    for (size_t i = 0; i < B; ++i)
        for (int k = 0; k < 6; ++k) R_host[i * 6 + k] = pfp[i * kFW + 18 + k];
    return QLE_OK;
}
