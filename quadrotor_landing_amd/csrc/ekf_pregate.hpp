// ekf_pregate.hpp -- k_pregate: the chi-square gate IN FRONT of the unchanged fused tick (libqle_gate.so, include/qle_gate.h).  gfx950.
//
// The fused tick (ekf_step_fused_z, ekf_fused.hpp) forms the innovation after its covariance sweep, under the drain of its stores; a gate
// has to decide before the sweep.  So the decision is taken by a kernel of its own that never writes the state: one lane per filter, it
// predicts in registers only what the innovation covariance is read from, evaluates NIS = dy^T S^-1 dy and clears the mask word of
// the tag record where the tag pose is not accepted.  The tick launched right behind it applies exactly the accepted corrections.
//
//   loads      x (16), the quad rows of P that hold a word the three predicted blocks depend on, u (6), z (7 + mask word), noise
//   predict    the nominal state (predict_nominal_lean) and P(r,r), P(r,th), P(th,th) through predict_level3 / predict_level1 -- the calls
//              and the blocks ekf_step_fused_z hands to quad::update_factor; every other word they would produce is dead code here
//   innovation R_k and Gx (quad::update_noise), dy (quad::update_innovation) against the predicted nominal state, S = G P G^T + R_k
//              (the sums of quad::update_factor), its L D L^T factor with y' = L^-1 dy carried along: NIS = sum y'_m^2 / d_m, NaN as
//              soon as one d_m <= 0
//   stores     nis, accepted = mask && initialised && isfinite(NIS) && NIS <= chi2_max (k_innov's rules, ekf_innov.hpp), the mask word
//              (kept where accepted, cleared elsewhere), optionally nu = dy (6) and S (36, symmetric)
// PREDICT = false evaluates against the stored state and leaves the mask word alone: qle_innovation from device tensors.
//
// The predicted pose block does not depend on the accelerometer-bias rows and columns of P: of the 120 covariance words 78 are read
// (pregate_needs below).  Only the 16-byte quad rows that hold one of them are loaded (load_P_rows, ekf_layout.hpp, as for k_innov) -- which the packed
// order (ekf_device.hpp: the ab column of every block-row sits between its th and wb columns) turns into all 120 words in fp32 and 90 in
// fp64; compact records hold nothing else than what is needed (48 / 46 words).  Words moved per filter, fp32 / fp64: full records
// 16 + 120 / 90 + 6 + 8 in, 1 (mask) + 1 (nis) out and one byte (accepted): 152 / 122; compact records 16 + 48 / 46 + 6 + 8 in: 80 / 78.
// Per-filter noise adds its 24-word record.
//
// Every lane runs straight-line code: a filter that is masked, not initialised or beyond the batch's ragged end computes on (with a unit
// quaternion where it holds none, so that its arithmetic stays finite) and only what it stores is selected -- no early exit in front
// of the loads (predict_tick, ekf_kernels.hpp, measured what such an exit costs) and nothing decided across the wave.
//
// The arithmetic (pregate_eval) is written so that a host compiler accepts it: tests/cpp/pregate_harness.cpp runs it on the CPU
// against the dense CPU restatement of the reference.  The kernel and its loads follow under __HIPCC__.
#pragma once

#include <cmath>

#include "ekf_device.hpp"
#include "ekf_quad.hpp"

namespace qle {

// Does P(a, b), a <= b, feed one of the predicted blocks P(r,r), P(r,th), P(th,th)?  predict_level3 reads rows r and v without their ab
// columns as far as those blocks go, predict_level1 reads P(th,th), P(th,wb), P(wb,wb).
__host__ __device__ constexpr bool pregate_needs(int a, int b)
{
    const int ba = a / 3, bb = b / 3;
    if (ba == 3 || bb == 3) return false;   // accelerometer bias
    if (ba <= 1) return true;               // rows r, v: columns r, v, th, wb
    return (ba == 2 && (bb == 2 || bb == 4)) || (ba == 4 && bb == 4);
}

// S = G P G^T + R_k over the six state columns G touches, upper triangle (i <= k); the sums of quad::update_factor, which keeps only the
// factor.  in: the covariance blocks (r,r), (r,th), (th,th) as full 3 x 3, Gx and R_k.
template <typename T, bool DIRECT>
__host__ __device__ __forceinline__ void innovation_cov(const quad::FactorIn<T>& in, T (&S)[6][6])
{
    using quad::rk_idx;
    if (DIRECT) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (k >= i) { S[i][k] = in.rk[rk_idx(i, k)] + in.frr[3 * i + k]; S[3 + i][3 + k] = in.rk[rk_idx(3 + i, 3 + k)] + in.ftt[3 * i + k]; }
                S[i][3 + k] = in.rk[rk_idx(i, 3 + k)] + in.frt[3 * i + k];
            }
        }
    } else {
        const T (&Gx)[9] = in.gx;
        const T (&Frt)[9] = in.frt;
        const T (&Ftt)[9] = in.ftt;
        T E[3][3];   // P_rt + Gx P_tt
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int k = 0; k < 3; ++k) E[i][k] = Frt[3 * i + k] + (Gx[3 * i] * Ftt[k] + Gx[3 * i + 1] * Ftt[3 + k] + Gx[3 * i + 2] * Ftt[6 + k]);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (k >= i) {
                    S[i][k] = in.rk[rk_idx(i, k)] + in.frr[3 * i + k] + (Gx[3 * i] * Frt[3 * k] + Gx[3 * i + 1] * Frt[3 * k + 1] + Gx[3 * i + 2] * Frt[3 * k + 2]) +
                              (E[i][0] * Gx[3 * k] + E[i][1] * Gx[3 * k + 1] + E[i][2] * Gx[3 * k + 2]);
                    S[3 + i][3 + k] = in.rk[rk_idx(3 + i, 3 + k)] + Ftt[3 * i + k];
                }
                S[i][3 + k] = in.rk[rk_idx(i, 3 + k)] + E[i][k];
            }
        }
    }
}

// nu = dy (EKF.cpp:447-450), S = G P G^T + R_k (EKF.cpp:475; symmetric, both triangles filled) and the returned NIS = dy^T S^-1 dy of
// tag pose z.  PREDICT: against the state one prediction_step (EKF.cpp:346-415) with IMU sample u ahead of (x, Po); x is advanced in
// place.  Otherwise against (x, Po) as they are, and u is not read.  Of Po only the words pregate_needs names are read (PREDICT) or the
// pose block (otherwise).  pregate_eval_pivots also hands back the pivots d_m of S = L D L^T (log det S = sum log d_m: k_score,
// ekf_score.hpp) and pd, whether every one of them is > 0; it returns the quadratic form as the factor left it.  pregate_eval is that
// with NaN where S is not positive definite.
template <typename T, bool DIRECT, bool PREDICT>
__device__ __forceinline__ T pregate_eval_pivots(const DevParams<T>& p, const Noise<T>& nzl, T (&x)[16], const T (&Po)[120], const T (&u)[6],
                                                 const T (&z)[7], T (&nu)[6], T (&S)[6][6], T (&d)[6], bool& pd)
{
    using SQ = quad::ScalarQ<T>;
    quad::FactorIn<T> in;
    if constexpr (PREDICT) {
        T Pn[120];
        PredictCtx<T> c;
        T accel[3];
        predict_nominal_lean<T>(p, nzl, x, u, accel, c);
        predict_level3<T>(c, Po, Pn);
        predict_level1<T>(c, nzl, Po, Pn);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                in.frr[3 * i + k] = Pn[sidx(i, k)]; in.frt[3 * i + k] = Pn[sidx(i, 6 + k)]; in.ftt[3 * i + k] = Pn[sidx(6 + i, 6 + k)];
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                in.frr[3 * i + k] = Po[sidx(i, k)]; in.frt[3 * i + k] = Po[sidx(i, 6 + k)]; in.ftt[3 * i + k] = Po[sidx(6 + i, 6 + k)];
            }
        }
    }
    quad::NoiseV<T> nz;
#pragma unroll
    for (int k = 0; k < 6; ++k) nz.R[k] = nzl.R[k];
    quad::update_noise<SQ, T, DIRECT>(p, nz, x, in.gx, in.rk);
    quad::update_innovation<SQ, T, DIRECT>(p, x, z, nu, [](const T (&)[7]) {});
    innovation_cov<T, DIRECT>(in, S);
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int b = a + 1; b < 6; ++b) S[b][a] = S[a][b];
    }
    // S = L D L^T on a copy, y' = L^-1 dy carried along: NIS = sum y'_m^2 / d_m
    T F[6][6], y[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        y[a] = nu[a];
#pragma unroll
        for (int b = a; b < 6; ++b) F[a][b] = S[a][b];
    }
    const T nis = ldl_solve<6, true>([&](int i, int j) -> T& { return F[i][j]; }, y, pd);
#pragma unroll
    for (int a = 0; a < 6; ++a) d[a] = F[a][a];
    return nis;
}

template <typename T, bool DIRECT, bool PREDICT>
__device__ __forceinline__ T pregate_eval(const DevParams<T>& p, const Noise<T>& nzl, T (&x)[16], const T (&Po)[120], const T (&u)[6],
                                          const T (&z)[7], T (&nu)[6], T (&S)[6][6])
{
    T d[6];
    bool pd;
    const T nis = pregate_eval_pivots<T, DIRECT, PREDICT>(p, nzl, x, Po, u, z, nu, S, d, pd);
    return pd ? nis : T(NAN);
}

}  // namespace qle

#if defined(__HIPCC__)
#include "ekf_layout.hpp"

namespace qle {

// the covariance words pregate_eval reads: pregate_needs (PREDICT) or the pose block
template <bool PREDICT> constexpr CovNeeds kPregateNeeds = PREDICT ? pregate_needs : pose_needs;
// words of the covariance the kernel moves per filter (whole quad rows)
template <int VW, bool COMPACT, bool PREDICT> constexpr int pregate_cov_words = CovSrc<VW, COMPACT, kPregateNeeds<PREDICT>>{}.words;
static_assert(pregate_cov_words<4, false, true> == 120 && pregate_cov_words<2, false, true> == 90 && pregate_cov_words<4, true, true> == 48 &&
              pregate_cov_words<2, true, true> == 46, "the word counts stated at the top of this file");

// One lane per filter, one wave per workgroup (a workgroup is one 64-filter tile).  Reads the state, never writes it.
// zs: the tag records (z 7 words + mask word); PREDICT stores the mask word back, kept where accepted and cleared elsewhere.
// nis [B], accepted [B], nu [B][6], S [B][36] of dst dtype: any may be null (wave-uniform).
template <typename T, bool DIRECT, bool PFP, bool COMPACT, bool PREDICT>
__global__ __launch_bounds__(kTile, 2) void k_pregate(const T* __restrict__ st, const T* __restrict__ us, T* zs, int64_t B,
                                                      const T* __restrict__ pfp, void* __restrict__ nis_out, uint8_t* __restrict__ acc_out,
                                                      void* __restrict__ nu_out, void* __restrict__ S_out, int32_t dst_f64, double chi2_max,
                                                      DevParams<T> p)
{
    args_early(st, us, zs, B);
    const int64_t i = (int64_t)blockIdx.x * kTile + threadIdx.x;   // the records are allocated for whole tiles: every lane may load
    T x[kXW], P[kPW], u[kUW], zr[kZW];
    // cached loads: the IMU and tag records are read again by the tick right behind (load_rec reads them non-temporally by default --
    // right for a kernel that is their last reader)
    load_rec<T, kZW, 0, kZW, kCached>(zs, i, zr);
    if constexpr (PREDICT) load_rec<T, kUW, 0, kUW, kCached>(us, i, u);
    else {
#pragma unroll
        for (int k = 0; k < kUW; ++k) u[k] = T(0);
    }
    load_rec<T, kSW, 0, kXW>(st, i, x);
    load_P_rows<T, COMPACT, kPregateNeeds<PREDICT>>(st, i, P);
    Noise<T> nz;
    load_noise<T, PFP>(p, pfp, i, nz);
    const bool dead = filter_uninitialised(x);
    if (dead) x[9] = T(1);
    const T z[7] = {zr[0], zr[1], zr[2], zr[3], zr[4], zr[5], zr[6]};
    T nu[6], S[6][6];
    const T nis_raw = pregate_eval<T, DIRECT, PREDICT>(p, nz, x, P, u, z, nu, S);
    const bool on = !dead && zr[7] != T(0);   // nothing to evaluate otherwise: nu = 0, S = 0, NIS = NaN, not accepted
    const T nis = on ? nis_raw : T(NAN);
    // NaN compares false: a non-finite NIS is never accepted; +Inf only passes an infinite threshold, which accepts finite NIS only
    const bool accepted = on && isfinite((double)nis) && (double)nis <= chi2_max;
    if (i >= B) return;
    if constexpr (PREDICT) zs[word_off<T>(7, i, kZW)] = accepted ? zr[7] : T(0);
    if (nis_out) put<T>(nis_out, i, nis, dst_f64 != 0);
    if (acc_out) acc_out[i] = accepted ? 1 : 0;
    if (nu_out) {
#pragma unroll
        for (int k = 0; k < 6; ++k) put<T>(nu_out, i * 6 + k, on ? nu[k] : T(0), dst_f64 != 0);
    }
    if (S_out) {
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = 0; b < 6; ++b) put<T>(S_out, i * 36 + a * 6 + b, on ? S[a][b] : T(0), dst_f64 != 0);
    }
}

}  // namespace qle
#endif  // __HIPCC__
