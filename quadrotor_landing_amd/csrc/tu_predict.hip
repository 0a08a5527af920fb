// tu_predict.hip -- launchers of k_predict (one lane per filter, predict-only tick; the body is in ekf_lane_launch.hpp) and of k_innov
// (innovation diagnostics and the chi-square gate, ekf_innov.hpp).  Compiled once per compute dtype (-DQLE_TU_T=float|double); see
// ekf_host.hpp.
#include "ekf_lane_launch.hpp"
#include "ekf_innov.hpp"

#ifndef QLE_TU_T
#error "compile with -DQLE_TU_T=float or -DQLE_TU_T=double"
#endif

// k_innov over the handle's state and the tag records `z` (h->tick_z): gate = false writes nu / S into h->innov, gate = true clears the
// mask word of every record whose NIS is not <= chi2_max; both write NIS into h->innov_nis.  Launched as k_update.
template <typename T>
int launch_innov(qle_batch* h, void* z, bool gate, double chi2_max)
{
    const DevParams<T>& p = dev<T>(h);
    const dim3 g = grid_for(h, h->block), b(h->block);
    return with_bool(h->pub.direct_orien_method, [&](auto D) {
    return with_bool(h->pfp_on, [&](auto F) {
    return with_bool(h->compact, [&](auto C) {
    return with_bool(gate, [&](auto G) {
        return launch(h, k_innov<T, D, F, C, G>, g, b, 0, (const T*)state_cur(h), (T*)z, h->B, (int32_t)g.x, (int32_t)b.x, (const T*)h->pfp,
                      (T*)h->innov, (T*)h->innov_nis, chi2_max, p);
    }); }); }); });
}

template int predict_lanes<QLE_TU_T, false>(qle_batch*, const void*, const void*, void*, bool);
template int launch_innov<QLE_TU_T>(qle_batch*, void*, bool, double);
