// ekf_lane_launch.hpp -- the bodies of the lane-per-filter launchers declared in ekf_host.hpp, seen by the tu_*.hip units that instantiate
// them: each unit instantiates its side, and ekf_capi.hip (which sees the declarations only) instantiates no tick kernel.
#pragma once

#include "ekf_host.hpp"
#include "ekf_kernels.hpp"

// prediction_step from `src` into `dst`; history: the tick also appends to the multirate history (full records only: compact records
// never carry it, qle_set_params).
template <typename T, bool COMPACT>
int predict_lanes(qle_batch* h, const void* u, const void* src, void* dst, bool history)
{
    const DevParams<T>& p = dev<T>(h);
    const dim3 g = grid_for(h, h->block), b(h->block);
    T* acc = h->aux ? (T*)h->aux_accel : (T*)nullptr;
    history = history && !COMPACT;
    // multirate history of this tick: the IMU sample's ring slot and, on checkpoint ticks, the checkpoint slot
    T* hu = history ? (T*)mr_u_slot_host(h, h->tick) : (T*)nullptr;
    bool extra_ck = false;
    T* hc = history ? (T*)mr_ck_for_predict(h, h->tick, &extra_ck) : (T*)nullptr;
    // the extra checkpoint stays in the Infinity Cache when it fits there next to the state (cached stores), else it is streamed
    const int32_t ck_cached = extra_ck && 2 * slot_bytes(h) <= ((size_t)200 << 20) ? 1 : 0;
    // "loads first" (predict_tick): the fp32 tick of a batch that gives every SIMD at most one wave
    return with_bool(h->pfp_on, [&](auto F) {
    return with_int<0, 1, 2, 3>(effective_nt(h), [&](auto N) {
    return with_bool_if<!COMPACT>(history, [&](auto M) {
    return with_bool_if<sizeof(T) == 4 && !COMPACT>(h->loads_first, [&](auto L) {
        return launch(h, k_predict<T, F, N, M, COMPACT, L>, g, b, 0, (const T*)src, (T*)dst, (const T*)u, h->B, (int64_t)0, (int32_t)g.x,
                      (int32_t)b.x, h->split, ck_cached, (const T*)h->pfp, acc, hu, hc, p);
    }); }); }); });
}

template <typename T, bool COMPACT>
int step_lanes(qle_batch* h, const void* u, const void* z)
{
    const DevParams<T>& p = dev<T>(h);
    const GateParams gp = make_gate(h);
    const dim3 g = grid_for(h, h->block), b(h->block);
    T *st = (T*)state_cur(h), *acc = h->aux ? (T*)h->aux_accel : (T*)nullptr, *obs = h->aux ? (T*)h->aux_obs : (T*)nullptr;
    return with_bool(h->pub.direct_orien_method, [&](auto D) {
    return with_bool(h->gating, [&](auto G) {
    return with_bool(h->pfp_on, [&](auto F) {
    return with_int<0, 1, 2, 3>(effective_nt(h), [&](auto N) {
        return launch(h, k_step<T, D, F, G, N, COMPACT>, g, b, 0, st, (const T*)u, (const T*)z, h->B, (int64_t)0, (int32_t)g.x, (int32_t)b.x,
                      h->split, (const T*)h->pfp, acc, obs, h->last_corr, h->flags, p, gp);
    }); }); }); });
}

template <typename T, bool COMPACT>
int update_lanes(qle_batch* h, const void* z)
{
    const DevParams<T>& p = dev<T>(h);
    const dim3 g = grid_for(h, h->block), b(h->block);
    T *st = (T*)state_cur(h), *obs = h->aux ? (T*)h->aux_obs : (T*)nullptr;
    return with_bool(h->pub.direct_orien_method, [&](auto D) {
    return with_bool(h->pfp_on, [&](auto F) {
        return launch(h, k_update<T, D, F, COMPACT>, g, b, split_lds<T>(h), st, (const T*)z, h->B, (int32_t)g.x, (int32_t)b.x, (const T*)h->pfp,
                      obs, p);
    }); });
}

// On-chip-resident variant: ONE launch advances every filter by n ticks with x and P held in
// registers; HBM traffic is the state once plus the inputs.  Not the unit of work of the headline
// metric (one launch per tick); reported separately.
template <typename T, bool COMPACT>
int resident_lanes(qle_batch* h, const qle_inputs* in, int64_t t0, int64_t n)
{
    const DevParams<T>& p = dev<T>(h);
    const dim3 g = grid_for(h, h->block), b(h->block);
    const int64_t pu = (int64_t)(in->pitch_u / h->wsz), pz = (int64_t)(in->pitch_z / h->wsz);
    return with_bool(h->pub.direct_orien_method, [&](auto D) {
    return with_bool(h->pfp_on, [&](auto F) {
        return launch(h, k_run_resident<T, D, F, COMPACT>, g, b, split_lds<T>(h), p, (T*)state_cur(h), (const T*)in->u, (const T*)in->z,
                      (const int32_t*)in->d_slot, pu, pz, in->T, t0, n, (const T*)h->pfp, h->B);
    }); });
}
