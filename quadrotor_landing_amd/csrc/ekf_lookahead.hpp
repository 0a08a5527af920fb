// ekf_lookahead.hpp -- k_lookahead: state and covariance h ticks ahead, read-only (libqle_lookahead.so, include/qle_lookahead.h).  gfx950.
//
// The read-only sibling of k_run_resident (ekf_kernels.hpp): one lane per filter loads its record once, applies prediction_step h times
// in registers with the IMU sample held (the zero-order hold of filter_update, EKF.cpp:138-139), and stores the result into a record
// array of its own -- the forecast, in the wave-tile layout, so that every consumer of a qle_device_view reads it as it reads the handle.
//
//   loads      x (16) and the covariance words of the record (120, or the 48 of a compact record) through the wave-tile helpers of
//              ekf_layout.hpp (1 KiB-contiguous dwordx4 rows per wave), u (6, from the caller's [B][6] tensor of either dtype, cast with
//              the plain C++ cast), the mask byte, the noise record with per-filter parameters
//   loop       ekf_predict of ekf_device.hpp, h times: the arithmetic (and the bits) of h k_run_resident ticks without a tag pose.  The
//              trip count is the kernel argument, so the loop is wave-uniform by construction
//   coast      after every tick (and on the stored state, k = 0): does a diagonal entry of P(r,r) or P(th,th), cast to double, exceed
//              its limit squared?  The first such k is kept through a select; -1 when there is none
//   stores     x and the covariance words of the forecast record, ticks_to_limit [B] (int32, optional)
// Words moved per filter: 136 in and out (64 compact), 6 of u, one byte of mask, one word of ticks_to_limit.
//
// Every lane runs straight-line code: a filter that is masked out, holds no state or lies beyond the batch's ragged end computes on
// (with a unit quaternion where it holds none, so that its arithmetic stays finite) and what it stores is selected: an all-zero record
// -- the engine's "not initialised" -- and -1.  No early exit in front of the loads, nothing decided across the wave.
//
// The per-filter body (lookahead_filter) is written so that a host compiler accepts it: tests/cpp/lookahead_harness.cpp runs it on the
// CPU against h applications of the dense CPU restatement of the reference's predict.  The kernel and its loads follow under __HIPCC__.
#pragma once

#include <cmath>
#include <cstdint>

#include "ekf_device.hpp"

namespace qle {

constexpr int32_t kMaxHorizon = 4096;   // QLK_MAX_HORIZON of the header

// the coast limits as the kernel takes them: squares formed on the host in fp64; +inf never compares below a finite entry
struct CoastLimits {
    double r2, th2;
};

// Is a diagonal entry of P(r,r) above lim.r2, or one of P(th,th) above lim.th2?  On the words as stored, cast to double: the rule of
// QHL_SIGMA_R / QHL_SIGMA_THETA (ekf_health.hpp) -- "the largest entry exceeds" is "an entry exceeds".  Three compares per block.
template <typename T>
__host__ __device__ __forceinline__ bool coast_over(const T (&P)[120], const CoastLimits& lim)
{
    bool over = false;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        over = over || (double)P[sidx(j, j)] > lim.r2;
        over = over || (double)P[sidx(6 + j, 6 + j)] > lim.th2;
    }
    return over;
}

// The forecast of one filter.  x: the 16 state words, P: the 15-state register image of the packed covariance (zero bias blocks for a
// filter without bias states), both advanced in place by h calls of ekf_predict with the same u -- h = 0 leaves the input bits.
// asked: the filter is inside the batch and its mask is set.  A filter that is not asked or holds no state (stored quaternion all
// zero) is skipped: x and P come back all zero and ticks = -1.  ticks: the smallest k in 0..h at which coast_over holds (k = 0: the
// stored state), else -1.  No branch on a per-filter value: "skipped" and the coast bookkeeping are selects.
template <typename T>
__host__ __device__ __forceinline__ void lookahead_filter(const DevParams<T>& p, const Noise<T>& nz, T (&x)[16], T (&P)[120], const T (&u)[6],
                                                          int32_t h, const CoastLimits& lim, bool asked, int32_t& ticks)
{
    const bool no_state = filter_uninitialised(x);
    x[9] = no_state ? T(1) : x[9];
    int32_t t = coast_over<T>(P, lim) ? 0 : -1;
#pragma unroll 1
    for (int32_t k = 1; k <= h; ++k) {
        T accel[3];
        ekf_predict<T>(p, nz, x, P, u, accel);
        t = (t < 0 && coast_over<T>(P, lim)) ? k : t;
    }
    const bool skip = !asked || no_state;
#pragma unroll
    for (int k = 0; k < 16; ++k) x[k] = skip ? T(0) : x[k];
#pragma unroll
    for (int k = 0; k < 120; ++k) P[k] = skip ? T(0) : P[k];
    ticks = skip ? -1 : t;
}

}  // namespace qle

#if defined(__HIPCC__)
#include "ekf_layout.hpp"

namespace qle {

// One lane per filter, one wave per workgroup (a workgroup is one 64-filter tile).  Reads the state `st`, never writes it; writes the
// forecast records `out` (allocated for whole tiles, as the state is: every lane loads and stores, whole dwordx4 tile rows).
// u: [B][6] floats or doubles (u_f64, wave-uniform); mask [B] or null (all); ticks [B] or null.  The tensors are not padded: the lanes
// beyond the end read the last row.  h is checked by the host (0..kMaxHorizon).
// fp64 holds 240 registers of P: one wave per SIMD; fp32 fits two (the launch bounds cap it at 256 registers).
template <typename T, bool PFP, bool COMPACT>
__global__ __launch_bounds__(kTile, sizeof(T) == 8 ? 1 : 2) void k_lookahead(const T* __restrict__ st, T* __restrict__ out, const void* __restrict__ u_in,
                                                                             int64_t B, int32_t h, int32_t u_f64, const uint8_t* __restrict__ mask,
                                                                             const T* __restrict__ pfp, int32_t* __restrict__ ticks, CoastLimits lim,
                                                                             DevParams<T> p)
{
    args_early(st, out, u_in, B, h);
    const int64_t i = (int64_t)blockIdx.x * kTile + threadIdx.x;
    const int64_t row = i < B ? i : B - 1;
    T x[kXW], P[kPW], u[kUW];
    load_rec<T, kSW, 0, kXW>(st, i, x);
    if constexpr (COMPACT) load_P_compact<T>(st, i, P);
    else load_rec<T, kSW, kXW, kPW>(st, i, P);
    if (u_f64) {   // wave-uniform
#pragma unroll
        for (int k = 0; k < kUW; ++k) u[k] = (T) static_cast<const double*>(u_in)[row * kUW + k];
    } else {
#pragma unroll
        for (int k = 0; k < kUW; ++k) u[k] = (T) static_cast<const float*>(u_in)[row * kUW + k];
    }
    Noise<T> nz;
    load_noise<T, PFP>(p, pfp, i, nz);
    const bool asked = i < B && (mask ? mask[row] != 0 : true);
    int32_t t;
    lookahead_filter<T>(p, nz, x, P, u, h, lim, asked, t);
    store_rec<T, kSW, 0, kXW>(out, i, x);
    if constexpr (COMPACT) store_P_compact<T>(out, i, P);
    else store_rec<T, kSW, kXW, kPW>(out, i, P);
    if (i >= B) return;
    if (ticks) ticks[i] = t;
}

}  // namespace qle
#endif  // __HIPCC__
