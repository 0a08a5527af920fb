// ekf_params.hpp -- the uniform parameter block of a launch (DevParams, ekf_device.hpp) from the public parameters and the values
// initialize_params derives from them (qle_params_derive, EKF.cpp:87-125).  Shared by every library that launches the engine's
// arithmetic on a handle's records (libqle_ekf.so for its own kernels, libqle_gate.so for the gate in front of the fused tick), so
// that they all hold the same values.
#pragma once

#include "../../include/qle_ekf.h"
#include "ekf_device.hpp"

template <typename T> static qle::DevParams<T> make_dev(const qle_params& p, const qle_derived& d)
{
    qle::DevParams<T> o;
    o.dT = (T)d.dT_nom;
    o.dTw = p.est_bias ? (T)d.dT_nom : T(0);
    o.bias_on = p.est_bias ? T(1) : T(0);
    o.small_ang_tol = (T)p.small_ang_tol;
    for (int i = 0; i < 3; ++i) { o.g[i] = (T)p.g[i]; o.r_v_cv[i] = (T)p.r_v_cv[i]; o.ab_static[i] = (T)p.ab_static[i]; o.wb_static[i] = (T)p.wb_static[i]; }
    for (int i = 0; i < 4; ++i) o.q_vc[i] = (T)d.q_vc[i];
    for (int i = 0; i < 9; ++i) o.C_vc[i] = (T)d.C_vc[i];
    for (int i = 0; i < 12; ++i) o.Q[i] = (T)d.Q[i];
    for (int i = 0; i < 6; ++i) o.R[i] = (T)d.R[i];
    o.compact = 0;   // set by qle_set_params
    return o;
}
