// tu_compact.hip -- launchers of the lane-per-filter kernels on COMPACT records (est_bias = false, relative_pose_EKF.cpp:92: the record
// keeps the 9 x 9 pose block of P only; ekf_layout.hpp).  Separate instantiations, so that the full-record kernels are compiled
// exactly as before; the launchers' bodies are shared with the full-record side (ekf_lane_launch.hpp).  Compiled once per compute dtype
// (-DQLE_TU_T=float|double); see ekf_host.hpp.
#include "ekf_lane_launch.hpp"

#ifndef QLE_TU_T
#error "compile with -DQLE_TU_T=float or -DQLE_TU_T=double"
#endif

template int predict_lanes<QLE_TU_T, true>(qle_batch*, const void*, const void*, void*, bool);
template int step_lanes<QLE_TU_T, true>(qle_batch*, const void*, const void*);
template int update_lanes<QLE_TU_T, true>(qle_batch*, const void*);
template int resident_lanes<QLE_TU_T, true>(qle_batch*, const qle_inputs*, int64_t, int64_t);
