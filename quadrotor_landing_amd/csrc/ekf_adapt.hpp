// ekf_adapt.hpp -- k_adapt_observe, k_adapt_apply: adaptive tag-pose noise, R estimated from the innovations on the device
// (libqle_adapt.so, include/qle_adapt.h).  gfx950.
//
// Scoring, banks and IMM answer "which R_r / R_ang is right?" by enumeration over hand-picked candidates.  Here every filter estimates its
// own diagonal R from the innovations it already forms, and the next tick uses the estimate: the EM iteration for a diagonal measurement
// noise, with the tag tick's innovation as the only datum.  Per tag tick, against the state one prediction_step ahead (what k_score
// evaluates, pregate_eval_pivots<T, DIRECT, true>):
//     R_k = N diag(R) N^T,  n_k = the k-th column of N (noise_columns below; what quad::update_noise multiplies out)
//     S = G P G^T + R_k = L D L^T, factored once; w_nu = L^-1 nu and w_k = L^-1 n_k, seven forward solves against the stored factor
//     a_k = sum_m w_k[m] w_nu[m] / d_m  (= n_k^T S^-1 nu),   c_k = sum_m w_k[m]^2 / d_m  (= n_k^T S^-1 n_k)
//     r^_k = R_k + R_k^2 (a_k^2 - c_k)
// the E-step: E[n_k^2 | nu] is the squared posterior mean (R_k a_k)^2 plus the posterior variance R_k - R_k^2 c_k >= 0, so the sample is
// non-negative in exact arithmetic, and its fixed point E[a_k^2] = c_k holds exactly when S is the covariance of nu.  No inverse of N
// and no back-substitution.  The M-step with forgetting (adapt_apply_one) moves R_k towards the window's mean sample and writes the six R
// words of the filter's parameter record, which every tick kernel reads.
//
// What the estimate means: "the R under which this filter's own model explains its innovations".  Wherever the model is off -- the
// linearisation, the process noise, the open reading of the angle-noise columns of N -- that is not the noise of the sensor.
//
//   k_adapt_observe
//   loads      those of k_score with per-filter parameters: x (16), the quad rows of P over pregate_needs, u (6), z (7 + mask word),
//              the 24-word parameter record; and the filter's accumulator record, words 0..22 (fp64)
//   evaluate   pregate_eval_pivots (nu, S), noise_columns (N), adapt_sample (the factor, a, c, r^)
//   accumulate adapt_accumulate; fp64 whatever T is
//   stores     the accumulator record, words 0..22, of the filters that are on -- never the state, the mask word or the parameter record
//   k_adapt_apply
//   loads      accumulator words 0, 2..7 and 21, the six R words of the parameter record
//   stores     applied [B] and optionally R_out [B][6] of every filter in the batch; of an applied filter (n >= n_min) the six R words,
//              accumulator words 0 and 2..19 (zero) and word 21 (windows, incremented)
// The accumulators are plane-major, acc[kAdaptWords][padded batch], as k_score's.  One lane owns one filter: no atomics, a deterministic
// result.  Words moved per filter by k_adapt_observe, fp32 / fp64, the record's doubles counted as two: the loads of k_pregate (full
// records 150 / 120, compact records 78 / 76), the 24-word parameter record and 2 x 23 doubles = 92: 266 / 236 and 194 / 192.
// k_adapt_apply: 8 doubles and 6 words in; out, applied or not, one byte and 6 doubles, and of an applied filter 6 words and 20 doubles.
//
// Every lane runs straight-line code up to the stores (k_pregate's rule): a filter that is masked, not initialised or beyond the batch's
// ragged end computes on and selects its own words back; nothing is decided across the wave.
//
// Not provided: adaptation of Q, multirate handles, a full (non-diagonal) R, per-filter bounds, adaptation inside the plain or the scored
// run of a sequence (qad_run is the sequence form).
//
// The arithmetic (noise_columns, adapt_sample, adapt_accumulate, adapt_apply_one) is written so that a host compiler accepts it:
// tests/cpp/adapt_harness.cpp runs it on the CPU, behind pregate_eval_pivots, over consecutive tag ticks.  The kernels follow under
// __HIPCC__.
#pragma once

#include <cmath>
#include <cstdint>

#include "ekf_pregate.hpp"

namespace qle {

constexpr int kAdaptWords = 24;   // QAD_WORDS: planes of an accumulator array
constexpr int kAdaptLive = 23;    // words 0..22 are read and written by k_adapt_observe; 23 stays zero
// the words of an accumulator record (include/qle_adapt.h)
enum AdaptWord { kAdN = 0, kAdBad = 1, kAdRhat = 2, kAdA2 = 8, kAdC = 14, kAdTotal = 20, kAdWindows = 21, kAdRejected = 22 };

// what k_adapt_apply takes of a qad_config
struct AdaptApplyCfg {
    double gain, n_min;
    double lo[6], hi[6];
};

// The noise Jacobian N (6 x 6, N[row][column]) with R_k = N diag(R) N^T as quad::update_noise forms it, at state x:
// N = [-Cc C_vc, [r]x (direct, else 0); 0, C_vc] (EKF.cpp:462-472).
template <typename T, bool DIRECT>
__host__ __device__ __forceinline__ void noise_columns(const DevParams<T>& p, const T (&x)[16], T (&N)[6][6])
{
    const T q[4] = {x[6], x[7], x[8], x[9]};
    const T r[3] = {x[0], x[1], x[2]};
    T Cc[9];
    quad::q_to_rot(q, Cc);
    const T Sr[3][3] = {{T(0), -r[2], r[1]}, {r[2], T(0), -r[0]}, {-r[1], r[0], T(0)}};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            N[i][j] = -(Cc[3 * i] * p.C_vc[j] + Cc[3 * i + 1] * p.C_vc[3 + j] + Cc[3 * i + 2] * p.C_vc[6 + j]);
            N[i][3 + j] = DIRECT ? Sr[i][j] : T(0);
            N[3 + i][j] = T(0);
            N[3 + i][3 + j] = p.C_vc[3 * i + j];
        }
    }
}

// S = L D L^T once (ldl_solve on a copy, w_nu = L^-1 nu carried along), then the six columns of N forward-solved against the stored
// factor: a_k = n_k^T S^-1 nu, c_k = n_k^T S^-1 n_k and the sample r^_k = R_k + R_k^2 (a_k^2 - c_k).  Returns NIS = nu^T S^-1 nu as the
// factor left it, pd: whether every pivot is > 0.
template <typename T>
__device__ __forceinline__ T adapt_sample(const T (&S)[6][6], const T (&nu)[6], const T (&N)[6][6], const T (&R)[6], T (&a)[6], T (&c)[6],
                                          T (&rhat)[6], bool& pd)
{
    T F[6][6], wn[6], inv[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        wn[i] = nu[i];
#pragma unroll
        for (int j = i; j < 6; ++j) F[i][j] = S[i][j];
    }
    const T nis = ldl_solve<6, true>([&](int i, int j) -> T& { return F[i][j]; }, wn, pd);
#pragma unroll
    for (int m = 0; m < 6; ++m) inv[m] = T(1) / F[m][m];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        T w[6];
#pragma unroll
        for (int m = 0; m < 6; ++m) w[m] = N[m][k];
        // row m of the factor holds d_m and the unscaled L^T row: L(j, m) = F[m][j] / d_m, the multiplier ldl_solve used
#pragma unroll
        for (int m = 0; m < 6; ++m) {
#pragma unroll
            for (int j = m + 1; j < 6; ++j) w[j] -= F[m][j] * inv[m] * w[m];
        }
        T ak = T(0), ck = T(0);
#pragma unroll
        for (int m = 0; m < 6; ++m) {
            ak += w[m] * wn[m] * inv[m];
            ck += w[m] * w[m] * inv[m];
        }
        a[k] = ak;
        c[k] = ck;
        rhat[k] = R[k] + R[k] * R[k] * (ak * ak - ck);
    }
    return nis;
}

// One tag tick of one filter into its record acc.  on: mask word != 0, the filter holds a state and lies inside the batch.  Scorable =
// S positive definite, NIS and all six r^_k finite.  Scored = on, scorable and NIS <= chi2_max (+inf: no limit).  On but not scorable
// counts in n_bad, on and scorable but NIS > chi2_max in n_rejected, and neither changes another word; not on changes no word (every word
// is selected, never "plus zero").
template <typename T>
__device__ __forceinline__ void adapt_accumulate(double (&acc)[kAdaptLive], bool on, T nis, bool pd, const T (&a)[6], const T (&c)[6],
                                                 const T (&rhat)[6], double chi2_max)
{
    const double nd = (double)nis;
    bool fin = std::isfinite(nd);
#pragma unroll
    for (int k = 0; k < 6; ++k) fin = fin && std::isfinite((double)rhat[k]);
    const bool scorable = on && pd && fin;
    const bool scored = scorable && nd <= chi2_max;
    acc[kAdN] = scored ? acc[kAdN] + 1.0 : acc[kAdN];
    acc[kAdTotal] = scored ? acc[kAdTotal] + 1.0 : acc[kAdTotal];
    acc[kAdBad] = on && !scorable ? acc[kAdBad] + 1.0 : acc[kAdBad];
    acc[kAdRejected] = scorable && !scored ? acc[kAdRejected] + 1.0 : acc[kAdRejected];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double ak = (double)a[k];
        acc[kAdRhat + k] = scored ? acc[kAdRhat + k] + (double)rhat[k] : acc[kAdRhat + k];
        acc[kAdA2 + k] = scored ? acc[kAdA2 + k] + ak * ak : acc[kAdA2 + k];
        acc[kAdC + k] = scored ? acc[kAdC + k] + (double)c[k] : acc[kAdC + k];
    }
}

// The M-step with forgetting for one filter: n scored ticks in the open window, sum[k] = sum of r^_k over them, R the six words the record
// holds.  Returns whether the filter is applied (n >= n_min); Rn[k] = clamp(R_k + gain (sum_k / n - R_k), lo_k, hi_k), evaluated in
// fp64 and rounded once to T (not meaningful where not applied).
template <typename T>
__host__ __device__ __forceinline__ bool adapt_apply_one(const AdaptApplyCfg& cfg, double n, const double (&sum)[6], const T (&R)[6], T (&Rn)[6])
{
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double r = (double)R[k];
        const double v = r + cfg.gain * (sum[k] / n - r);
        Rn[k] = (T)fmin(fmax(v, cfg.lo[k]), cfg.hi[k]);
    }
    return n >= cfg.n_min;
}

}  // namespace qle

#if defined(__HIPCC__)
#include "ekf_layout.hpp"

namespace qle {

// One lane per filter, one wave per workgroup (a workgroup is one 64-filter tile).  Reads the state, the tick's records and the
// parameter record, writes none of them.  acc [kAdaptWords][Bp] doubles, Bp = the padded batch (gridDim.x * kTile): every lane may load
// its record.  One wave per SIMD is what the registers are budgeted for, as for k_score and for its reason: the record is 46 registers
// next to what k_pregate holds, the factor and the seven solves.  Per-filter parameters are always in force here (the estimate has
// nowhere else to go).
template <typename T, bool DIRECT, bool COMPACT>
__global__ __launch_bounds__(kTile, 1) void k_adapt_observe(const T* __restrict__ st, const T* __restrict__ us, const T* __restrict__ zs, int64_t B,
                                                            const T* __restrict__ pfp, double* __restrict__ acc, int64_t Bp, double chi2_max,
                                                            DevParams<T> p)
{
    args_early(st, us, zs, B);
    const int64_t i = (int64_t)blockIdx.x * kTile + threadIdx.x;   // the records are allocated for whole tiles: every lane may load
    T x[kXW], P[kPW], u[kUW], zr[kZW];
    // cached loads: the IMU and tag records are read again by the tick right behind
    load_rec<T, kZW, 0, kZW, kCached>(zs, i, zr);
    load_rec<T, kUW, 0, kUW, kCached>(us, i, u);
    load_rec<T, kSW, 0, kXW>(st, i, x);
    load_P_rows<T, COMPACT, kPregateNeeds<true>>(st, i, P);
    Noise<T> nz;
    load_noise<T, true>(p, pfp, i, nz);
    double a[kAdaptLive];
#pragma unroll
    for (int w = 0; w < kAdaptLive; ++w) a[w] = acc[(int64_t)w * Bp + i];
    const bool dead = filter_uninitialised(x);
    if (dead) x[9] = T(1);
    const T z[7] = {zr[0], zr[1], zr[2], zr[3], zr[4], zr[5], zr[6]};
    T nu[6], S[6][6], d[6];
    bool pd0;
    pregate_eval_pivots<T, DIRECT, true>(p, nz, x, P, u, z, nu, S, d, pd0);   // x: advanced to the predicted state
    T N[6][6], ak[6], ck[6], rhat[6];
    noise_columns<T, DIRECT>(p, x, N);
    bool pd;
    const T nis = adapt_sample<T>(S, nu, N, nz.R, ak, ck, rhat, pd);
    const bool on = !dead && zr[7] != T(0) && i < B;
    adapt_accumulate<T>(a, on, nis, pd, ak, ck, rhat, chi2_max);
    if (!on) return;
#pragma unroll
    for (int w = 0; w < kAdaptLive; ++w) acc[(int64_t)w * Bp + i] = a[w];
}

// One lane per filter.  pfp: the parameter records; words 18..23 of an applied filter are written, no other.  applied [B] bytes and
// R_out [B][6] doubles (or null, wave-uniform): the six values now in force, applied or not.
template <typename T>
__global__ __launch_bounds__(kTile) void k_adapt_apply(T* __restrict__ pfp, double* __restrict__ acc, int64_t B, int64_t Bp, AdaptApplyCfg cfg,
                                                       uint8_t* __restrict__ applied, double* __restrict__ R_out)
{
    const int64_t i = (int64_t)blockIdx.x * kTile + threadIdx.x;   // < Bp: the planes and the records are allocated for whole tiles
    const double n = acc[(int64_t)kAdN * Bp + i];
    const double windows = acc[(int64_t)kAdWindows * Bp + i];
    double sum[6];
    T R[6], Rn[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        sum[k] = acc[(int64_t)(kAdRhat + k) * Bp + i];
        R[k] = pfp[word_off<T>(18 + k, i, kFW)];
    }
    const bool ok = adapt_apply_one<T>(cfg, n, sum, R, Rn);
    if (i >= B) return;
    if (applied) applied[i] = ok ? 1 : 0;
    if (R_out) {
#pragma unroll
        for (int k = 0; k < 6; ++k) R_out[i * 6 + k] = (double)(ok ? Rn[k] : R[k]);
    }
    if (!ok) return;
#pragma unroll
    for (int k = 0; k < 6; ++k) pfp[word_off<T>(18 + k, i, kFW)] = Rn[k];
    acc[(int64_t)kAdN * Bp + i] = 0.0;
#pragma unroll
    for (int w = kAdRhat; w < kAdTotal; ++w) acc[(int64_t)w * Bp + i] = 0.0;
    acc[(int64_t)kAdWindows * Bp + i] = windows + 1.0;
}

}  // namespace qle
#endif  // __HIPCC__
