// gate_capi.hip -- C ABI of include/qle_gate.h over ekf_pregate.hpp.  Host side: argument checks (every refusal before any GPU call)
// and ONE launch on the view's stream.  Works from the view structs of include/qle_ekf.h and the public parameters; links
// libqle_ekf.so for qle_params_derive; derive and the launch ladder are side_run_host.hpp's.
#include "../../include/qle_gate.h"

#include <cmath>

#include "ekf_pregate.hpp"
#include "side_run_host.hpp"

using namespace qle;
using namespace qle::side;

QLE_SIDE_LAST_ERROR(qgt_last_error)
QLE_SIDE_LAUNCH_COUNT(qgt_launch_count)
QLE_SIDE_LAUNCH_CENSUS(qgt)

// Everything include/qle_gate.h lists as refused; no GPU call.  multirate_ekf is QLE_ERR_STATE, another class of error than the rest,
// and stays ahead of what is refused about the view's fields; the view may be larger than this library's (a smaller one is refused).
static int check_args(const qle_device_view* v, const qle_inputs_view* in, const qle_params* p, bool gate, double chi2_max, int32_t dst_dtype)
{
    if (!in) return fail(QLE_ERR_INVALID, "inputs view is null");
    if (in->struct_size < sizeof(qle_inputs_view)) return fail(QLE_ERR_INVALID, "inputs view: struct_size %u, this library was built for %zu", in->struct_size, sizeof(qle_inputs_view));
    if (!p) return fail(QLE_ERR_INVALID, "params is null");
    if (p->multirate_ekf) return fail(QLE_ERR_STATE, "the gate does not support multirate_ekf: a delayed measurement's innovation belongs to a history entry");
    QLE_TRY(check_view(v, ViewSize::at_least, false));
    if (!in->z) return fail(QLE_ERR_INVALID, "the tick has no tag slot");
    if (gate && !in->u) return fail(QLE_ERR_INVALID, "the tick has no IMU records");
    if (gate && !(chi2_max > 0.0)) return fail(QLE_ERR_INVALID, "chi2_max must be > 0 (got %g)", chi2_max);
    if (dst_dtype != QGT_F32 && dst_dtype != QGT_F64) return fail(QLE_ERR_INVALID, "dst_dtype must be QGT_F32 or QGT_F64 (got %d)", dst_dtype);
    if (v->num_states != (p->est_bias ? 15 : 9)) return fail(QLE_ERR_INVALID, "view: num_states %d, params: est_bias %d", v->num_states, p->est_bias);
    return QLE_OK;
}

struct Outs { void* nis; uint8_t* accepted; void* nu; void* S; int32_t f64; double chi2_max; };

template <typename T, bool PREDICT>
static int launch_t(const qle_device_view* v, const qle_inputs_view* in, const qle_params& pub, const qle_derived& der, const Outs& o)
{
    return launch_flags<T>(v, pub, der, [&](const DevParams<T>& dp, auto direct, auto pfp, auto compact) {
        return launch(k_pregate<T, decltype(direct)::value, decltype(pfp)::value, decltype(compact)::value, PREDICT>, tiles(v), dim3(kTile), 0, stream_of(v),
                      (const T*)v->state, (const T*)in->u, (T*)in->z, v->batch, (const T*)v->filter_params, o.nis, o.accepted, o.nu, o.S, o.f64, o.chi2_max, dp);
    });
}

template <bool PREDICT>
static int run(const qle_device_view* v, const qle_inputs_view* in, const qle_params* p, const Outs& o)
{
    QLE_TRY(check_args(v, in, p, PREDICT, o.chi2_max, o.f64));
    qle_derived der;
    QLE_TRY(derive(p, &der));
    if (!PREDICT && !o.nis && !o.nu && !o.S) return QLE_OK;
    QLE_TRY(use_device(v));
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
