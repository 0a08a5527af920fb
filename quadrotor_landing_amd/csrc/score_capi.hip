// score_capi.hip -- C ABI of include/qle_score.h over ekf_score.hpp.  Host side: ONE launch per scored tick on the view's stream, qsc_run
// as side_run_host.hpp's loop over that launch and qle_run of the tick library, and the two launches of the batch summary.  The
// refusals (every one before any GPU call), the launch ladder, the loop and the copy to the host are side_run_host.hpp's.  Links
// libqle_ekf.so for qle_params_derive, the two view calls and qle_run.
#include "../../include/qle_score.h"

#include "ekf_score.hpp"
#include "side_run_host.hpp"

using namespace qle;
using namespace qle::side;

static_assert(QSC_WORDS == kScoreWords && QSC_SUMS == kScoreSums, "the header publishes the accumulator record of ekf_score.hpp");

QLE_SIDE_LAST_ERROR(qsc_last_error)
QLE_SIDE_LAUNCH_COUNT(qsc_launch_count)
QLE_SIDE_LAUNCH_CENSUS(qsc)

static int check_params(const qle_params* p) { return check_observer_params(p, "scoring"); }

// behind every refusal and use_device
template <typename T>
static int launch_t(const qle_device_view* v, const qle_inputs_view* in, const qle_params& pub, const qle_derived& der, double* acc)
{
    return launch_flags<T>(v, pub, der, [&](const DevParams<T>& dp, auto direct, auto pfp, auto compact) {
        return launch(k_score<T, decltype(direct)::value, decltype(pfp)::value, decltype(compact)::value>, tiles(v), dim3(kTile), 0, stream_of(v), (const T*)v->state,
                      (const T*)in->u, (const T*)in->z, v->batch, (const T*)v->filter_params, acc, v->padded_batch, dp);
    });
}
static int score_tick(const qle_device_view* v, const qle_inputs_view* in, const qle_params& pub, const qle_derived& der, double* acc)
{
    return v->dtype == QLE_F32 ? launch_t<float>(v, in, pub, der, acc) : launch_t<double>(v, in, pub, der, acc);
}

extern "C" int qsc_score_tick(const qle_device_view* view, const qle_inputs_view* in, const qle_params* params, double* acc)
{
    QLE_TRY(check_params(params));
    QLE_TRY(check_acc(acc));
    QLE_TRY(check_tick(view, in, params));
    qle_derived der;
    QLE_TRY(derive(params, &der));
    QLE_TRY(use_device(view));
    return score_tick(view, in, *params, der, acc);
}

// ---- qsc_run
// behind every refusal and use_device
static int run_loop(qle_batch* h, const qle_device_view* v, const qle_inputs* in, int64_t t0, int64_t n, const qle_params& pub, const qle_derived& der, double* acc)
{
    return run_ticks(h, in, t0, n, [&](const qle_inputs_view& iv) { return score_tick(v, &iv, pub, der, acc); }, [] { return (int)QLE_OK; });
}

extern "C" int qsc_run(qle_batch* h, const qle_inputs* in, int64_t t0, int64_t n, const qle_params* params, double* acc)
{
    QLE_TRY(check_params(params));
    QLE_TRY(check_acc(acc));
    qle_device_view v;
    QLE_TRY(check_run(h, in, t0, n, params, &v));
    qle_derived der;
    QLE_TRY(derive(params, &der));
    if (n == 0) return QLE_OK;
    QLE_TRY(use_device(&v));
    return run_loop(h, &v, in, t0, n, *params, der, acc);
}

extern "C" int qsc_run_host(qle_batch* h, const qle_inputs* in, int64_t t0, int64_t n, const qle_params* params, double* acc_host)
{
    QLE_TRY(check_params(params));
    if (!acc_host) return fail(QLE_ERR_INVALID, "acc_host is null");   // a host array: no alignment to ask for
    qle_device_view v;
    QLE_TRY(check_run(h, in, t0, n, params, &v));
    qle_derived der;
    QLE_TRY(derive(params, &der));
    QLE_TRY(use_device(&v));
    return run_to_host(&v, kScoreWords, acc_host, [&](double* acc) { return run_loop(h, &v, in, t0, n, *params, der, acc); });
}

// ---- qsc_summary
static Partials g_partials(kScoreSums);   // the [tiles][30] partials of a summary

extern "C" int qsc_summary(const qle_device_view* view, const double* acc, const uint8_t* mask, double* out30)
{
    QLE_TRY(check_view(view, ViewSize::at_least, false));
    QLE_TRY(check_acc(acc));
    if (!out30) return fail(QLE_ERR_INVALID, "out30 is null");
    if (!aligned(out30, 8)) return fail(QLE_ERR_INVALID, "out30 must be 8-byte aligned");
    QLE_TRY(use_device(view));
    const int64_t nt = view->padded_batch / kTile;
    double* partials = nullptr;
    QLE_TRY(g_partials.get(view, nt, &partials));
    QLE_TRY(launch(k_score_tiles, tiles(view), dim3(kTile), 0, stream_of(view), acc, view->batch, view->padded_batch, mask, partials));
    return launch(k_score_reduce, dim3(1), dim3(kBlock), 0, stream_of(view), (const double*)partials, nt, out30);
}
