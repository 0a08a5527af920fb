// side_run_host.hpp -- what the side libraries that loop over qle_run of the tick library share on the host (score, adapt: a kernel of
// their own in front of every tick of a device-resident sequence that has a tag slot).  Behind side_host.hpp; host code only, every
// symbol internal.  A library that includes it links libqle_ekf.so for qle_params_derive, the two view calls and qle_run.
#pragma once

#include "side_host.hpp"

namespace qle {
namespace side {
namespace {

// the launch's parameter block as the handle derives it (ekf_params.hpp)
int derive(const qle_params* p, qle_derived* der)
{
    return qle_params_derive(p, der) == QLE_OK ? QLE_OK : fail(QLE_ERR_INVALID, "params: %s", qle_last_error());
}
int inputs_view(const qle_inputs* in, int64_t t, qle_inputs_view* iv)
{
    iv->struct_size = sizeof(qle_inputs_view);
    const int rc = qle_inputs_get_device_view(in, t, iv);
    return rc == QLE_OK ? QLE_OK : fail(rc, "%s", qle_last_error());
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

}  // namespace
}  // namespace side
}  // namespace qle
