// tu_misc.hip -- launchers of k_step_mr, k_update, k_run_resident (the bodies of the last two are in ekf_lane_launch.hpp)
// Compiled once per compute dtype (-DQLE_TU_T=float|double); see ekf_host.hpp.
#include "ekf_lane_launch.hpp"
#include "ekf_multirate.hpp"
#ifndef QLE_TU_T
#error "compile with -DQLE_TU_T=float or -DQLE_TU_T=double"
#endif

#if defined(QLE_MR_STAMPS)
// diagnostic build only (make dbg): the per-wave s_memtime stamps of the last k_step_mr launch of this dtype's translation unit
#define QLE_CAT2(a, b) a##b
#define QLE_CAT(a, b) QLE_CAT2(a, b)
extern "C" int QLE_CAT(qle_debug_clocks_, QLE_TU_T)(unsigned long long* out, int n)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(qle::qle_dbg_clock), sizeof(unsigned long long) * (size_t)n);
}
extern "C" int QLE_CAT(qle_debug_split_clocks_, QLE_TU_T)(unsigned long long* out, int n)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(qle::qle_dbg_split_clock), sizeof(unsigned long long) * (size_t)n);
}
#endif

// One multirate tick that carries tag poses (predict-only multirate ticks go through launch_predict).
template <typename T>
int launch_step_mr(qle_batch* h, const void* u, const void* z)
{
    QLE_TRY(mr_prepare(h));
    const DevParams<T>& p = dev<T>(h);
    const GateParams gp = make_gate(h);
    const MrParams m = make_mr(h);
    const dim3 g = grid_for(h, h->block), b(h->block);
    T *acc = h->aux ? (T*)h->aux_accel : (T*)nullptr, *obs = h->aux ? (T*)h->aux_obs : (T*)nullptr;
    const double* stamp = (h->have_stamps && h->pub.dynamic_meas_delay) ? h->stamp : nullptr;
    QLE_TRY(with_bool(h->pub.direct_orien_method, [&](auto D) {
    return with_bool(h->pfp_on, [&](auto F) {
        return launch(h, k_step_mr<T, D, F>, g, b, split_lds<T>(h), (T*)state_cur(h), (const T*)u, (const T*)z, h->B, (int32_t)g.x, (int32_t)b.x,
                      h->hist_first, (T*)h->mr_u, (T*)h->mr_ckpt, (T*)h->mr_anchor, (const T*)h->pfp, stamp, acc, obs, h->last_corr, h->flags,
                      h->delay_cur, p, gp, m);
    }); }));
    mr_schedule_extra(h);
    return QLE_OK;
}

template int launch_step_mr<QLE_TU_T>(qle_batch*, const void*, const void*);
template int update_lanes<QLE_TU_T, false>(qle_batch*, const void*);
template int resident_lanes<QLE_TU_T, false>(qle_batch*, const qle_inputs*, int64_t, int64_t);
