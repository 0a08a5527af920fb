// score_capi.hip -- C ABI of include/qle_score.h over ekf_score.hpp.  Host side: argument checks (every refusal before any GPU call),
// ONE launch per scored tick on the view's stream, the C loop of qsc_run over qsc's own launch and qle_run of the tick library, and the
// two launches of the batch summary.  Links libqle_ekf.so for qle_params_derive, the two view calls and qle_run, and derives the
// launch's parameter block as the handle does (ekf_params.hpp); derive, inputs_view and check_run are side_run_host.hpp's.
#include "../../include/qle_score.h"

#include "ekf_params.hpp"
#include "ekf_score.hpp"
#include "side_run_host.hpp"

using namespace qle;
using namespace qle::side;

static_assert(QSC_WORDS == kScoreWords && QSC_SUMS == kScoreSums, "the header publishes the accumulator record of ekf_score.hpp");

QLE_SIDE_LAST_ERROR(qsc_last_error)
QLE_SIDE_LAUNCH_COUNT(qsc_launch_count)

// What every scoring entry refuses about params and about a device accumulator array; no GPU call.  multirate_ekf is QLE_ERR_STATE,
// the gate's own rule, and stays ahead of everything that is refused about the handle or the view.
static int check_params(const qle_params* p)
{
    if (!p) return fail(QLE_ERR_INVALID, "params is null");
    if (p->multirate_ekf) return fail(QLE_ERR_STATE, "scoring does not support multirate_ekf: a delayed measurement's innovation belongs to a history entry");
    return QLE_OK;
}
static int check_acc(const double* acc)
{
    if (!acc) return fail(QLE_ERR_INVALID, "acc is null");
    if (!aligned(acc, 16)) return fail(QLE_ERR_INVALID, "acc must be 16-byte aligned");
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
    return QLE_OK;
}

template <typename T>
static int launch_t(const qle_device_view* v, const qle_inputs_view* in, const qle_params& pub, const qle_derived& der, double* acc)
{
    DevParams<T> dp = make_dev<T>(pub, der);
    dp.compact = v->compact ? 1 : 0;
    auto go = [&](auto direct, auto pfp, auto compact) {
        hipLaunchKernelGGL((k_score<T, decltype(direct)::value, decltype(pfp)::value, decltype(compact)::value>), tiles(v), dim3(kTile), 0, stream_of(v), (const T*)v->state,
                           (const T*)in->u, (const T*)in->z, v->batch, (const T*)v->filter_params, acc, v->padded_batch, dp);
    };
    with(pub.direct_orien_method != 0, [&](auto d) { with(v->filter_params != nullptr, [&](auto f) { with(v->compact != 0, [&](auto c) { go(d, f, c); }); }); });
    return launched();
}
// behind every refusal and use_device
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
    for (int64_t t = t0; t < t0 + n; ++t) {
        qle_inputs_view iv;
        QLE_TRY(inputs_view(in, t, &iv));
        if (iv.z) {
            if (!iv.u) return fail(QLE_ERR_INVALID, "tick %lld has no IMU records", (long long)t);
            QLE_TRY(score_tick(v, &iv, pub, der, acc));
        }
        if (int rc = qle_run(h, in, t, 1)) return fail(rc, "qle_run at tick %lld: %s", (long long)t, qle_last_error());
    }
    return QLE_OK;
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
    hipStream_t s = stream_of(&v);
    const size_t B = (size_t)v.batch, Bp = (size_t)v.padded_batch;
    DeviceMem own;
    double* acc = nullptr;
    HIP_TRY(own.acquire({{acc, (size_t)kScoreWords * Bp * sizeof(double), true}}, s));
    QLE_TRY(run_loop(h, &v, in, t0, n, *params, der, acc));
    HIP_TRY(hipMemcpy2DAsync(acc_host, B * sizeof(double), acc, Bp * sizeof(double), B * sizeof(double), kScoreWords, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return QLE_OK;
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
    hipLaunchKernelGGL(k_score_tiles, tiles(view), dim3(kTile), 0, stream_of(view), acc, view->batch, view->padded_batch, mask, partials);
    QLE_TRY(launched());
    hipLaunchKernelGGL(k_score_reduce, dim3(1), dim3(kBlock), 0, stream_of(view), (const double*)partials, nt, out30);
    return launched();
}
