// ekf_gate.hpp -- the per-tick parameter blocks the host fills in (GateParams, MrParams) and the corner gate of filter_update's decision
// whether a filter corrects on this tick (EKF.cpp:147-186; the decision itself is spelled out in step_tick, k_step_mr and wg_tick).
// Light: no covariance arithmetic, so the host side includes it for the structs alone.
#pragma once

#include "ekf_layout.hpp"

namespace qle {

// --------------------------------------------------------- measurement gate
// Decision logic of filter_update, EKF.cpp:147-186, per filter on the device:
//   consume  = measurement_ready && (!limit_measurement_freq || upds_since_correction + 1 >= upd_per_meas)
//   perform  = consume && (!corner_margin_enbl || some tag of the bundle projects inside the image margins)
// upds_since_correction is kept implicitly: last_corr[i] is the index of the filter's last correcting
// tick (-1 = never), so upds_since_correction before tick n is n - last_corr[i] - 1 and predict-only
// ticks never touch the array.  The projection runs in fp64 whatever the compute dtype, so the
// discrete decision matches the fp64 reference for the same (dtype-rounded) tag pose.
struct GateParams {
    int32_t limit;              // limit_measurement_freq (EKF.hpp:75)
    int32_t upd_per_meas;       // EKF.cpp:91
    int32_t corner_enbl;        // corner_margin_enbl (EKF.hpp:76)
    int32_t n_tags;             // EKF.hpp:117
    int32_t tick;               // index of this tick
    double K[9];                // camera_K row-major
    double x_lo, x_hi, y_lo, y_hi;  // camera_width*margin, camera_width*(1-margin), same for height (EKF.cpp:175-178)
    double hw[16], px[16], py[16];  // tag_widths/2, tag_positions x,y (EKF.cpp:163-164)
};

__device__ inline bool corner_gate(const GateParams& g, const double (&z)[7])
{
    double q[4] = {z[3], z[4], z[5], z[6]}, C[9];
    quat_to_rot<double>(q, C);  // T_ct = Translation(r_c_tc) * q_ct, EKF.cpp:154
    for (int t = 0; t < g.n_tags; ++t) {
        const double hw = g.hw[t];
        const double cx[4] = {hw + g.px[t], -hw + g.px[t], -hw + g.px[t], hw + g.px[t]};
        const double cy[4] = {hw + g.py[t], hw + g.py[t], -hw + g.py[t], -hw + g.py[t]};
        double mnx = 0, mny = 0, mxx = 0, mxy = 0;
        for (int k = 0; k < 4; ++k) {
            double pc[3];
            for (int r = 0; r < 3; ++r) pc[r] = C[3 * r] * cx[k] + C[3 * r + 1] * cy[k] + C[3 * r + 2] * 0.0 + z[r];
            const double iz = 1.0 / pc[2];                                   // EKF.cpp:168
            const double nx = pc[0] * iz, ny = pc[1] * iz, nz = pc[2] * iz;  // EKF.cpp:169
            const double u = g.K[0] * nx + g.K[1] * ny + g.K[2] * nz;        // EKF.cpp:170
            const double v = g.K[3] * nx + g.K[4] * ny + g.K[5] * nz;
            if (k == 0) { mnx = mxx = u; mny = mxy = v; }
            else { mnx = fmin(mnx, u); mxx = fmax(mxx, u); mny = fmin(mny, v); mxy = fmax(mxy, v); }
        }
        if (mnx > g.x_lo && mny > g.y_lo && mxx < g.x_hi && mxy < g.y_hi) return true;  // EKF.cpp:175-180
    }
    return false;
}

// Per-tick parameters of the multirate EKF (the history scheme: ekf_multirate.hpp).
struct MrParams {
    int32_t k;            // checkpoint period in ticks
    int32_t Nc;           // checkpoint slots
    int32_t Cu;           // IMU ring slots = k * Nc
    int32_t tick;         // index n of this tick; the newest history entry is tick n-1 (= cur)
    int32_t fixed_step;   // measurement_step_delay (EKF.cpp:93) when !dynamic
    int32_t dynamic;      // dynamic_meas_delay (EKF.hpp:79)
    int32_t gate;         // 1: mask word = measurement_ready, decide on device; 0: mask word = perform
    int32_t e_tick;       // tick whose state the EXTRA checkpoint slot (index Nc) holds; far negative = none (see k_step_mr)
    int64_t slot_words;   // words per state slot (kSW x padded batch)
    int64_t u_words;      // words per IMU ring slot (kHW x padded batch)
    double dT, offset, delay_max, t_curr, uniform_age;  // EKF.cpp:199-200
};

}  // namespace qle
