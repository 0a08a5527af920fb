// tu_step.hip -- launcher of k_step (one lane per filter, fused predict + masked update; the body is in ekf_lane_launch.hpp)
// Compiled once per compute dtype (-DQLE_TU_T=float|double); see ekf_host.hpp.
#include "ekf_lane_launch.hpp"

#ifndef QLE_TU_T
#error "compile with -DQLE_TU_T=float or -DQLE_TU_T=double"
#endif

template int step_lanes<QLE_TU_T, false>(qle_batch*, const void*, const void*);
