// ekf_consistency.hpp -- k_nees: filter consistency against a truth on the device (libqle_consistency.so, include/qle_consistency.h).  gfx950.
//
// The state-side counterpart of the innovation diagnostics (ekf_pregate.hpp): is the covariance a filter reports the covariance of the
// error it actually makes?  Per filter the normalised estimation error squared
//     NEES = e^T P^-1 e,   e = truth (-) estimate in the filter's own error-state convention,
// over all n states or over the marginal of a selection of the five 3-state blocks (r, v, th, ab, wb); chi-square with
// dof = 3 popcount(blocks) degrees of freedom for a consistent filter.  One lane per filter, x and the packed P in registers as in every
// tick kernel; the kernel reads the state and never writes it.
//
//   loads      x (16), all 120 covariance words (the 45 of a compact record), the truth row [16] (AoS, float32 or float64), the mask byte,
//              the static biases (shared, or words 12..17 of the per-filter parameter record)
//   error      e_r = r_true - r, e_v = v_true - v, e_th = log(norm(q^-1 (x) q_true)) -- the form of the attitude innovation
//              (EKF.cpp:447-450) with the w < -0.75 flip of quaternion_norm; the correction injects q <- q (x) exp(dth) (EKF.cpp:488) --
//              e_ab = ab_true - (ab_nom + ab_static), e_wb = wb_true - (wb_nom + wb_static): the biases qle_get_report publishes
//   marginal   no second code path: for an unselected state j, e_j = 0, P_jj = 1 and row and column j of P are zero, and the full matrix
//              is factored; the quadratic form of the result is exactly the marginal's.  `blocks` is wave-uniform: selects, no branch
//   factor     P = L D L^T in place on the packed words (sidx, compile-time indices), y = L^-1 e carried along, NEES = sum y_m^2 / d_m
//              -- ldl_solve of ekf_device.hpp, the routine of the 6 x 6 factor of pregate_eval.  A pivot <= 0 (or NaN): NEES = NaN, the
//              filter is flagged not positive definite
//   stores     nees [B], err [B][n] in the destination dtype, and eight fp64 partial sums per 64-filter tile
// Words moved per filter: full records 16 + 120 + 16 (truth) in, 1 + n out: 168 with every output, 153 with nees alone; compact records
// 16 + 48 + 16 in: 90 / 81.  Per-filter parameters add the two quad rows (fp32) or four (fp64) that hold the static biases.
//
// Every lane runs straight-line code: a filter that is masked out, not initialised or beyond the batch's ragged end computes on (with
// a unit quaternion where it holds none) and only what it stores is selected.
//
// The batch summary is deterministic: each wave reduces its eight partials by xor-shuffles (a fixed tree), writes them to a
// [tiles][8] buffer, and the one-workgroup k_nees_reduce adds the tiles in a fixed order.  No atomics.
//
// The arithmetic (nees_eval) is written so that a host compiler accepts it: tests/cpp/consistency_harness.cpp runs it on the CPU
// against numpy's dense solve.  The kernels follow under __HIPCC__.
#pragma once

#include <cmath>
#include <cstdint>

#include "ekf_device.hpp"

namespace qle {

constexpr uint32_t kNeesAllBlocks = 0x1Fu;   // bit 0 r, 1 v, 2 th, 3 ab, 4 wb
constexpr int kNeesSums = 8;                 // the fields of qcs_summary (include/qle_consistency.h), in its order

__host__ __device__ constexpr int nees_dof(uint32_t blocks)
{
    int n = 0;
    for (int b = 0; b < 5; ++b) n += (blocks >> b) & 1u ? 3 : 0;
    return n;
}

// e = truth (-) estimate (15 words: r, v, th, ab, wb) of state x against truth row xt (r, v, q xyzw, ab, wb; the TOTAL biases) and the
// returned NEES over the blocks selected.  P: the 15-state register image of the packed covariance, factored in place (destroyed).
// COMPACT: the bias blocks are not held (zero) and never selected -- the factor runs over the 9 pose states only.
// pd = false and NEES = NaN where a pivot is not > 0.
template <typename T, bool COMPACT>
__device__ __forceinline__ T nees_eval(const T (&x)[16], T (&P)[120], const T (&xt)[16], const T (&ab_static)[3], const T (&wb_static)[3],
                                       uint32_t blocks, T (&e)[15], bool& pd)
{
    constexpr int N = COMPACT ? 9 : 15;
    error_state<T>(x, xt, ab_static, wb_static, e);   // ekf_device.hpp: the two-sum bias errors, the attitude error of EKF.cpp:447-450
    // the marginal of the selected blocks as a full-size problem
    T y[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const bool si = ((blocks >> (i / 3)) & 1u) != 0;
        y[i] = si ? e[i] : T(0);
#pragma unroll
        for (int j = i; j < N; ++j) {
            const bool sj = ((blocks >> (j / 3)) & 1u) != 0;
            P[sidx(i, j)] = (si && sj) ? P[sidx(i, j)] : (i == j ? T(1) : T(0));
        }
    }
    // P = L D L^T in place, y = L^-1 e carried along: NEES = sum y_m^2 / d_m
    const T nees = ldl_solve<N, true>([&](int i, int j) -> T& { return P[sidx(i, j)]; }, y, pd);
    return pd ? nees : T(NAN);
}

}  // namespace qle

#if defined(__HIPCC__)
#include "ekf_layout.hpp"

namespace qle {

// One lane per filter, one wave per workgroup (a workgroup is one 64-filter tile).  Reads the state, never writes it.
// xt [B][16] of float32 / float64 (true_f64; load_truth, ekf_layout.hpp), mask [B] or null; nees [B], err [B][n_err] of dst dtype and partials [tiles][8] (fp64):
// any may be null (wave-uniform).  fp64 holds 240 registers of P: one wave per SIMD, as k_predict<double>; fp32 fits two.
template <typename T, bool PFP, bool COMPACT>
__global__ __launch_bounds__(kTile, sizeof(T) == 8 ? 1 : 2) void k_nees(const T* __restrict__ st, const void* __restrict__ xt, int64_t B,
                                                                        const uint8_t* __restrict__ mask, const T* __restrict__ pfp,
                                                                        void* __restrict__ nees_out, void* __restrict__ err_out,
                                                                        double* __restrict__ partials, uint32_t blocks, int32_t n_err,
                                                                        int32_t true_f64, int32_t dst_f64, double chi2_hi, DevParams<T> p)
{
    args_early(st, xt, B);
    const int64_t i = (int64_t)blockIdx.x * kTile + threadIdx.x;   // the records are allocated for whole tiles: every lane may load
    const int64_t row = i < B ? i : B - 1;                          // the tensors are not: the lanes beyond the end read the last row
    T x[kXW], P[kPW], t[16];
    load_rec<T, kSW, 0, kXW>(st, i, x);
    if constexpr (COMPACT) load_P_compact<T>(st, i, P);
    else load_rec<T, kSW, kXW, kPW>(st, i, P);
    load_truth<T>(xt, row, true_f64 != 0, t);
    Noise<T> nz;
    load_noise<T, PFP>(p, pfp, i, nz);
    const bool dead = filter_uninitialised(x);
    if (dead) x[9] = T(1);
    const bool on = !dead && i < B && (mask ? mask[row] != 0 : true);
    T e[15];
    bool pd;
    const T nees_raw = nees_eval<T, COMPACT>(x, P, t, nz.ab_static, nz.wb_static, blocks, e, pd);
    const T nees = on ? nees_raw : T(NAN);
    const double nd = (double)nees;
    const bool counted = on && isfinite(nd);
    if (partials) {   // wave-uniform
        const double er = (double)e[0] * (double)e[0] + (double)e[1] * (double)e[1] + (double)e[2] * (double)e[2];
        const double et = (double)e[6] * (double)e[6] + (double)e[7] * (double)e[7] + (double)e[8] * (double)e[8];
        const double s0 = wave_sum(counted ? 1.0 : 0.0);
        const double s1 = wave_sum(counted ? nd : 0.0);
        const double s2 = wave_sum(counted ? nd * nd : 0.0);
        const double s3 = wave_sum(counted && nd > chi2_hi ? 1.0 : 0.0);
        const double s4 = wave_sum(on && !pd ? 1.0 : 0.0);
        const double s5 = wave_sum(counted ? er : 0.0);
        const double s6 = wave_sum(counted ? et : 0.0);
        const int lane = (int)threadIdx.x;
        const double v = lane == 0 ? s0 : lane == 1 ? s1 : lane == 2 ? s2 : lane == 3 ? s3 : lane == 4 ? s4 : lane == 5 ? s5 : lane == 6 ? s6 : (double)nees_dof(blocks);
        if (lane < kNeesSums) partials[(int64_t)blockIdx.x * kNeesSums + lane] = v;
    }
    if (i >= B) return;
    if (nees_out) put<T>(nees_out, i, nees, dst_f64 != 0);
    if (err_out) {
#pragma unroll
        for (int k = 0; k < 15; ++k)
            if (k < n_err) put<T>(err_out, i * n_err + k, on ? e[k] : T(0), dst_f64 != 0);
    }
}

// One workgroup: the tiles' partials in a fixed order (reduce_tiles, ekf_layout.hpp) into the eight doubles of a qcs_summary.  dof is
// not a sum.
__global__ __launch_bounds__(kBlock) void k_nees_reduce(const double* __restrict__ partials, int64_t tiles, double* __restrict__ summary)
{
    reduce_tiles<kNeesSums, 8>(partials, tiles, [&](int f, double tot) { summary[f] = f == kNeesSums - 1 ? partials[kNeesSums - 1] : tot; });
}

}  // namespace qle
#endif  // __HIPCC__
