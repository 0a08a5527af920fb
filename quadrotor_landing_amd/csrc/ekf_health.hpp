// ekf_health.hpp -- k_health, k_health_reduce, k_retire, k_and_masks: filter lifecycle on the device (libqle_health.so,
// include/qle_health.h).  gfx950.
//
// Which filters of a batch are broken?  One lane per filter reads its record and classifies it; nothing is written to the state.
//
//   loads      x (16) and every covariance word of the record (120, or the 48 of a compact record) through the wave-tile helpers of
//              ekf_layout.hpp (1 KiB-contiguous dwordx4 rows per wave), the mask byte
//   status     a byte of QHL_* bits per filter, defined on the stored words cast to double (include/qle_health.h):
//              NONFINITE  any record word is NaN or Inf -- when set, nothing else is evaluated
//              NOT_PD     a pivot of P = L D L^T over the handle's n x n covariance is <= 0 or not finite: ldl_solve of
//                         ekf_device.hpp, the factorisation (and the rule) under which k_nees counts n_not_pd with every block of the
//                         handle selected.  A full record with n = 9 factors its 9 x 9 pose block: k_nees puts the identity into the
//                         unselected bias blocks, whose pivots are 1 and whose rows change nothing
//              QNORM      |q.q - 1| > qnorm_tol, the sum ((q0^2 + q1^2) + q2^2) + q3^2 in fp64 without contraction
//              SIGMA_R / _V / _THETA   the largest diagonal entry of the block is above limit^2 (the square formed on the host in fp64)
//   stores     status [B], flagged [B] = (status & select) != 0 (bytes), and nine fp64 counts per 64-filter tile
// Words moved per filter: 136 in (64 compact), two bytes out.
//
// Every lane runs straight-line code: a filter that is masked out, holds no state or lies beyond the batch's ragged end is classified
// like any other and only what it stores and counts is selected.
//
// The batch summary keeps the arrangement of k_nees / k_nees_reduce: each wave counts its lanes per field (a ballot and a population
// count: a wave reduction with nothing to order), writes nine partials to a [tiles][9] buffer, and the one-workgroup k_health_reduce
// adds the tiles in a fixed order.  No atomics.
//
// The classification (health_classify) is written so that a host compiler accepts it: tests/cpp/health_harness.cpp runs it on the CPU
// against a numpy restatement.  The kernels follow under __HIPCC__.
#pragma once

#include <cmath>
#include <cstdint>

#include "ekf_device.hpp"

namespace qle {

constexpr uint32_t kHealthNonfinite = 1u, kHealthNotPd = 2u, kHealthQnorm = 4u, kHealthSigmaR = 8u, kHealthSigmaV = 16u, kHealthSigmaTheta = 32u;
constexpr uint32_t kHealthAllBits = 63u;
constexpr int kHealthBits = 6;
constexpr int kHealthSums = 9;   // the fields of qhl_summary (include/qle_health.h), in its order

// the limits as the kernel takes them: squares formed on the host in fp64
struct HealthLimits {
    double r2, v2, th2;   // sigma_*_max^2; +inf never compares below a finite entry
    double qnorm_tol;
    uint32_t select;
};

// Status byte of one filter.  x: the 16 state words.  P: the 15-state register image of the packed covariance (factored in place,
// destroyed).  N: the handle's number of states, 15 or 9; with 9 only the 9 x 9 pose block is factored.  COMPACT: only that block is a
// record word, the rest of the image is never read.  probe: 0, or NaN when a record word outside x and the image (the padding of a
// compact covariance) is not finite.  no_state: the stored quaternion is all zero (filter_uninitialised, ekf_device.hpp) -- the caller
// stores status 0 for such a filter.
template <typename T, bool COMPACT, int N>
__device__ __forceinline__ uint32_t health_classify(const T (&x)[16], T (&P)[120], T probe, const HealthLimits& lim, bool& no_state)
{
    static_assert(N == 9 || (N == 15 && !COMPACT), "15 states or 9; compact records hold 9");
    constexpr int NW = COMPACT ? 9 : 15;   // the covariance words of the record: all of them count for NONFINITE
    no_state = filter_uninitialised(x);
    // w * 0 is 0 for a finite word and NaN otherwise: one multiply-add per word
#pragma unroll
    for (int k = 0; k < 16; ++k) probe += x[k] * T(0);
#pragma unroll
    for (int a = 0; a < NW; ++a)
#pragma unroll
        for (int b = a; b < NW; ++b) probe += P[sidx(a, b)] * T(0);
    const bool nonfinite = !(probe == T(0));

    uint32_t st = 0;
    {   // the limits, on the words as stored
        double dmax[3];
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const double d0 = (double)P[sidx(3 * b, 3 * b)], d1 = (double)P[sidx(3 * b + 1, 3 * b + 1)], d2 = (double)P[sidx(3 * b + 2, 3 * b + 2)];
            const double m = d0 > d1 ? d0 : d1;
            dmax[b] = m > d2 ? m : d2;
        }
        st |= dmax[0] > lim.r2 ? kHealthSigmaR : 0u;
        st |= dmax[1] > lim.v2 ? kHealthSigmaV : 0u;
        st |= dmax[2] > lim.th2 ? kHealthSigmaTheta : 0u;
    }
    {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
        const double q0 = (double)x[6], q1 = (double)x[7], q2 = (double)x[8], q3 = (double)x[9];
        const double a0 = q0 * q0, a1 = q1 * q1, a2 = q2 * q2, a3 = q3 * q3;
        const double dev = ((a0 + a1) + a2) + a3 - 1.0;
        st |= (dev < 0.0 ? -dev : dev) > lim.qnorm_tol ? kHealthQnorm : 0u;
    }
    {   // P = L D L^T over the handle's N states
        T none[N];
        bool pd;
        (void)ldl_solve<N, false>([&](int i, int j) -> T& { return P[sidx(i, j)]; }, none, pd);
        T pp = T(0);   // the pivots are left on the diagonal: an overflowed one is not a pivot of a positive definite matrix either
#pragma unroll
        for (int c = 0; c < N; ++c) pp += P[sidx(c, c)] * T(0);
        st |= (!pd || !(pp == T(0))) ? kHealthNotPd : 0u;
    }
    return nonfinite ? kHealthNonfinite : st;
}

}  // namespace qle

#if defined(__HIPCC__)
#include "ekf_layout.hpp"

namespace qle {

// One lane per filter, one wave per workgroup (a workgroup is one 64-filter tile).  Reads the state, never writes it.
// mask [B] or null (all); status [B], flagged [B] (bytes) and partials [tiles][9] (fp64): any may be null (wave-uniform).
// fp64 holds 240 registers of P: one wave per SIMD, as k_nees<double>; fp32 fits two.
template <typename T, bool COMPACT, int N>
__global__ __launch_bounds__(kTile, sizeof(T) == 8 ? 1 : 2) void k_health(const T* __restrict__ st, int64_t B, const uint8_t* __restrict__ mask,
                                                                          uint8_t* __restrict__ status, uint8_t* __restrict__ flagged,
                                                                          double* __restrict__ partials, HealthLimits lim)
{
    args_early(st, B);
    const int64_t i = (int64_t)blockIdx.x * kTile + threadIdx.x;   // the records are allocated for whole tiles: every lane may load
    const int64_t row = i < B ? i : B - 1;                          // the tensors are not: the lanes beyond the end read the last byte
    T x[kXW], P[kPW];
    T probe = T(0);
    load_rec<T, kSW, 0, kXW>(st, i, x);
    if constexpr (COMPACT) {
        T t[kPWc];
        load_rec<T, kSW, kXW, kPWc>(st, i, t);
#pragma unroll
        for (int a = 0; a < 15; ++a)
#pragma unroll
            for (int b = a; b < 15; ++b) P[sidx(a, b)] = b < 9 ? t[sidx9(a, b)] : T(0);
#pragma unroll
        for (int k = 45; k < kPWc; ++k) probe += t[k] * T(0);   // the record's padding: words a tick moves, so words that count
    } else {
        load_rec<T, kSW, kXW, kPW>(st, i, P);
    }
    const bool asked = i < B && (mask ? mask[row] != 0 : true);
    bool no_state;
    const uint32_t raw = health_classify<T, COMPACT, N>(x, P, probe, lim, no_state);
    const bool on = asked && !no_state;
    const uint32_t s = on ? raw : 0u;
    const bool flag = (s & lim.select) != 0u;
    if (partials) {   // wave-uniform
        const int lane = (int)threadIdx.x;
        const double c0 = (double)__popcll(__ballot(on)), c1 = (double)__popcll(__ballot(flag)), c2 = (double)__popcll(__ballot(asked && no_state));
        double v = lane == 0 ? c0 : lane == 1 ? c1 : c2;
#pragma unroll
        for (int b = 0; b < kHealthBits; ++b) {
            const double cb = (double)__popcll(__ballot((s >> b) & 1u));
            v = lane == 3 + b ? cb : v;
        }
        if (lane < kHealthSums) partials[(int64_t)blockIdx.x * kHealthSums + lane] = v;
    }
    if (i >= B) return;
    if (status) status[i] = (uint8_t)s;
    if (flagged) flagged[i] = flag ? 1 : 0;
}

// One workgroup: the tiles' partials in a fixed order (reduce_tiles, ekf_layout.hpp; slices of 16 for the nine fields) into the nine
// doubles of a qhl_summary.
__global__ __launch_bounds__(kBlock) void k_health_reduce(const double* __restrict__ partials, int64_t tiles, double* __restrict__ summary)
{
    reduce_tiles<kHealthSums, 16>(partials, tiles, [&](int f, double tot) { summary[f] = tot; });
}

// "No state" for the filters with mask[i] != 0: the 16 x words become zero (filter_uninitialised, ekf_device.hpp), which every tick
// kernel leaves untouched and a later seed treats as fresh -- and so do the covariance words, so that a retired record is the record of
// a filter that never had a state (all zero), broken values included.  One lane per filter; compact is wave-uniform.
template <typename T>
__global__ __launch_bounds__(kTile) void k_retire(T* __restrict__ st, const uint8_t* __restrict__ mask, int64_t B, int32_t compact)
{
    const int64_t i = (int64_t)blockIdx.x * kTile + threadIdx.x;
    if (i >= B || mask[i] == 0) return;
    T x[kXW], P[kPW];
#pragma unroll
    for (int k = 0; k < kXW; ++k) x[k] = T(0);
#pragma unroll
    for (int k = 0; k < kPW; ++k) P[k] = T(0);
    store_rec<T, kSW, 0, kXW>(st, i, x);
    store_P_any<T>(st, i, P, compact != 0);
}

// out[i] = a[i] != 0 && b[i] != 0: flagged AND detections is a seed mask (out may be a or b: no __restrict__)
__global__ __launch_bounds__(kBlock) void k_and_masks(const uint8_t* a, const uint8_t* b, uint8_t* out, int64_t B)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < B) out[i] = (a[i] != 0 && b[i] != 0) ? 1 : 0;
}

}  // namespace qle
#endif  // __HIPCC__
