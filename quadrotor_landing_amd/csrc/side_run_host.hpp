// side_run_host.hpp -- what the side libraries that put a kernel of their own in front of a tag tick share on the host: the parameter
// block and the launch ladder (gate, score, adapt), and for the observers that loop over qle_run of the tick library (score, adapt: the
// kernel in front of every tick of a device-resident sequence that has a tag slot) their refusals, the loop and the copy of the
// accumulator planes to the host.  Behind side_host.hpp; host code only, every symbol internal.  A library that includes it links
// libqle_ekf.so for qle_params_derive, and for the two view calls and qle_run where it uses what needs them.
#pragma once

#include "ekf_params.hpp"
#include "side_host.hpp"

namespace qle {
namespace side {
namespace {

// the launch's parameter block as the handle derives it (ekf_params.hpp)
int derive(const qle_params* p, qle_derived* der)
{
    return qle_params_derive(p, der) == QLE_OK ? QLE_OK : fail(QLE_ERR_INVALID, "params: %s", qle_last_error());
}
// One launch on the view's records: go(dp, direct, pfp, compact) with the device parameter block and the three flags of the view and the
// parameters as std::true_type / std::false_type; go launches through launch() (side_host.hpp) and returns its status.  Behind every
// refusal and use_device.
template <typename T, typename Go>
int launch_flags(const qle_device_view* v, const qle_params& pub, const qle_derived& der, Go&& go)
{
    DevParams<T> dp = make_dev<T>(pub, der);
    dp.compact = v->compact ? 1 : 0;
    return with(pub.direct_orien_method != 0, [&](auto d) {
        return with(v->filter_params != nullptr, [&](auto f) { return with(v->compact != 0, [&](auto c) { return go(dp, d, f, c); }); });
    });
}

int inputs_view(const qle_inputs* in, int64_t t, qle_inputs_view* iv)
{
    iv->struct_size = sizeof(qle_inputs_view);
    const int rc = qle_inputs_get_device_view(in, t, iv);
    return rc == QLE_OK ? QLE_OK : fail(rc, "%s", qle_last_error());
}

// What every observer entry refuses about params and about a device accumulator array; no GPU call.  multirate_ekf is QLE_ERR_STATE,
// the gate's own rule, and stays ahead of everything that is refused about the handle or the view.  what: "scoring", "noise adaptation".
int check_observer_params(const qle_params* p, const char* what)
{
    if (!p) return fail(QLE_ERR_INVALID, "params is null");
    if (p->multirate_ekf) return fail(QLE_ERR_STATE, "%s does not support multirate_ekf: a delayed measurement's innovation belongs to a history entry", what);
    return QLE_OK;
}
int check_acc(const double* acc)
{
    if (!acc) return fail(QLE_ERR_INVALID, "acc is null");
    if (!aligned(acc, 16)) return fail(QLE_ERR_INVALID, "acc must be 16-byte aligned");
    return QLE_OK;
}
// The view and the tick's inputs view; the view may be larger than this library's (a smaller one is refused).
int check_tick(const qle_device_view* v, const qle_inputs_view* in, const qle_params* p)
{
    if (!in) return fail(QLE_ERR_INVALID, "inputs view is null");
    if (in->struct_size < sizeof(qle_inputs_view)) return fail(QLE_ERR_INVALID, "inputs view: struct_size %u, this library was built for %zu", in->struct_size, sizeof(qle_inputs_view));
    QLE_TRY(check_view(v, ViewSize::at_least, false));
    if (!in->z) return fail(QLE_ERR_INVALID, "the tick has no tag slot");
    if (!in->u) return fail(QLE_ERR_INVALID, "the tick has no IMU records");
    if (v->num_states != (p->est_bias ? 15 : 9)) return fail(QLE_ERR_INVALID, "view: num_states %d, params: est_bias %d", v->num_states, p->est_bias);
    return QLE_OK;
}

// The handle's view and [t0, t0 + n) inside the sequence (the tick library is the one that knows its length, and says so without a
// GPU call); no GPU call.
int check_run(qle_batch* h, const qle_inputs* in, int64_t t0, int64_t n, const qle_params* p, qle_device_view* v)
{
    if (!h) return fail(QLE_ERR_INVALID, "handle is null");
    if (!in) return fail(QLE_ERR_INVALID, "inputs is null");
    v->struct_size = sizeof(*v);
    if (int rc = qle_get_device_view(h, v)) return fail(rc, "%s", qle_last_error());
    QLE_TRY(check_view(v, ViewSize::at_least, false));
    if (v->num_states != (p->est_bias ? 15 : 9)) return fail(QLE_ERR_INVALID, "handle: num_states %d, params: est_bias %d", v->num_states, p->est_bias);
    if (t0 < 0 || n < 0) return fail(QLE_ERR_INVALID, "t0 and n must be >= 0 (got %lld, %lld)", (long long)t0, (long long)n);
    qle_inputs_view iv;
    if (n > 0 && (inputs_view(in, t0, &iv) != QLE_OK || inputs_view(in, t0 + n - 1, &iv) != QLE_OK))
        return fail(QLE_ERR_INVALID, "ticks [%lld, %lld) reach beyond the sequence: %s", (long long)t0, (long long)(t0 + n), qle_last_error());
    return QLE_OK;
}

// Ticks [t0, t0 + n) by qle_run, one at a time; around every tick that has a tag slot before_tag(iv) in front of it and after_tag()
// behind it, each returning a status.  Behind every refusal and use_device.
template <typename Before, typename After>
int run_ticks(qle_batch* h, const qle_inputs* in, int64_t t0, int64_t n, Before&& before_tag, After&& after_tag)
{
    for (int64_t t = t0; t < t0 + n; ++t) {
        qle_inputs_view iv;
        QLE_TRY(inputs_view(in, t, &iv));
        if (iv.z) {
            if (!iv.u) return fail(QLE_ERR_INVALID, "tick %lld has no IMU records", (long long)t);
            QLE_TRY(before_tag(iv));
        }
        if (int rc = qle_run(h, in, t, 1)) return fail(rc, "qle_run at tick %lld: %s", (long long)t, qle_last_error());
        if (iv.z) QLE_TRY(after_tag());
    }
    return QLE_OK;
}

// body(acc) on zeroed accumulator planes acc [words][padded batch] of its own, then the batch's columns into acc_host [words][batch];
// returns behind a synchronisation of the view's stream.
template <typename Body>
int run_to_host(const qle_device_view* v, int words, double* acc_host, Body&& body)
{
    hipStream_t s = stream_of(v);
    const size_t B = (size_t)v->batch, Bp = (size_t)v->padded_batch;
    DeviceMem own;
    double* acc = nullptr;
    HIP_TRY(own.acquire({{acc, (size_t)words * Bp * sizeof(double), true}}, s));
    QLE_TRY(body(acc));
    HIP_TRY(hipMemcpy2DAsync(acc_host, B * sizeof(double), acc, Bp * sizeof(double), B * sizeof(double), words, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return QLE_OK;
}

}  // namespace
}  // namespace side
}  // namespace qle
