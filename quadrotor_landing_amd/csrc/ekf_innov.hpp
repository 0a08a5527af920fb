// ekf_innov.hpp -- innovation diagnostics of the tag-pose correction and the chi-square gate in front of it.
//
// correction_step forms the innovation delta_y (EKF.cpp:447-450) and its covariance S = G P G^T + R_k (EKF.cpp:475) and uses them only
// inside the gain.  k_innov evaluates them against the current state, one lane per filter, and reads nothing but x, the 21 words of the
// pose block P_JJ (J = r0..2, th0..2, the only columns G touches), the tag record and the filter's noise -- as whole 16-byte quad rows
// (load_P_rows, ekf_layout.hpp) 36 covariance words per filter in fp32 and 30 in fp64, 36 / 26 of a compact record.  It never writes
// the state:
//   diagnostics (GATE = false): nu = delta_y (6), S (21, packed upper triangle) into a kDW-word record per filter, and the normalised
//     innovation squared NIS = delta_y^T S^-1 delta_y into nis[i];
//   gate (GATE = true): accepted = mask && initialised && isfinite(NIS) && NIS <= chi2_max goes into the mask word of the tag record, so
//     that the unchanged k_update behind it applies exactly the accepted corrections; NIS into nis[i].
// A filter whose mask is 0 or that holds no state gets nu = 0, S = 0, NIS = NaN, accepted = 0.
//
// The arithmetic reuses ekf_update_prepare: y' = L^-1 delta_y, G' = L^-1 G and D of R_k = L D L^T.  With S' = G' P_JJ G'^T + D = L^-1 S L^-T,
// NIS = y'^T S'^-1 y' (an L D L^T factorisation of S'), and delta_y = L y', S = L S' L^T by forward substitution with L^-1.  L^-1 itself is
// read off G' exactly: in the direct method G = I, so G' = L^-1; otherwise R_k is block-diagonal (EKF.cpp:462-472), L^-1 is too, and G'
// carries it on its diagonal blocks (the upper-right block of G' is L^-1 G_x, the lower-left one is zero).
// Where S' is not positive definite (a corrupted covariance) NIS is NaN: such a measurement is never accepted.
// Every lane runs its own straight-line arithmetic; nothing is decided across the wave.
#pragma once

#include "ekf_layout.hpp"

namespace qle {

constexpr int kDW = 28;   // diagnostics record: nu (6), S packed upper triangle (21), 1 pad

__host__ __device__ constexpr int innov_state_col(int a) { return a < 3 ? a : a + 3; }   // J = {0,1,2,6,7,8}
__host__ __device__ constexpr int sidx6(int a, int b) { return a * 6 - a * (a - 1) / 2 + (b - a); }   // a <= b < 6
static_assert(CovSrc<4, false, pose_needs>{}.words == 36 && CovSrc<2, false, pose_needs>{}.words == 30 && CovSrc<4, true, pose_needs>{}.words == 36 &&
              CovSrc<2, true, pose_needs>{}.words == 26, "the word counts stated at the top of this file");

// nu, S (packed, a <= b) and NIS of one filter from its decorrelated measurement.
template <typename T, bool DIRECT>
__device__ __forceinline__ T innov_from_prep(const UpdatePrep<T>& u, const T (&Pj)[6][6], T (&nu)[6], T (&Sp)[21])
{
    const T (&Gm)[6][6] = u.Gm;
    // L^-1 (unit lower triangular), read off G'
    T Li[6][6];
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = 0; b < 6; ++b) Li[a][b] = (b < a && (DIRECT || a / 3 == b / 3)) ? Gm[a][b] : T(0);
    // S' = G' P_JJ G'^T + D (in the direct method G' is lower triangular)
    T M[6][6], Sd[6][6];
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            T acc = T(0);
#pragma unroll
            for (int m = 0; m < 6; ++m)
                if (!DIRECT || m <= a) acc += Gm[a][m] * Pj[m][c];
            M[a][c] = acc;
        }
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) {
            T acc = a == b ? u.d[a] : T(0);
#pragma unroll
            for (int m = 0; m < 6; ++m)
                if (!DIRECT || m <= b) acc += M[a][m] * Gm[b][m];
            Sd[a][b] = Sd[b][a] = acc;
        }
    // delta_y = L y':  solve L^-1 nu = y'
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        T acc = u.dy[a];
#pragma unroll
        for (int b = 0; b < a; ++b) acc -= Li[a][b] * nu[b];
        nu[a] = acc;
    }
    // S = L S' L^T:  W = L S' (solve L^-1 W = S'), then S^T = L W^T
    T W[6][6], S[6][6];
#pragma unroll
    for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            T acc = Sd[a][c];
#pragma unroll
            for (int b = 0; b < a; ++b) acc -= Li[a][b] * W[b][c];
            W[a][c] = acc;
        }
#pragma unroll
    for (int c = 0; c < 6; ++c)
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            T acc = W[c][a];
#pragma unroll
            for (int b = 0; b < a; ++b) acc -= Li[a][b] * S[c][b];
            S[c][a] = acc;
        }
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) Sp[sidx6(a, b)] = T(0.5) * (S[a][b] + S[b][a]);
    // NIS = y'^T S'^-1 y' through S' = Ls E Ls^T: the sum of (Ls^-1 y')_c^2 / e_c.  The loop of ldl_solve (ekf_device.hpp), written out:
    // called through it, 9 of this kernel's 32 instantiations change their register count (one from 128 to 129 VGPRs, an occupancy step).
    T y[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) y[a] = u.dy[a];
    T nis = T(0);
    bool pd = true;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const T e = Sd[c][c];
        pd = pd && e > T(0);
        const T inv = T(1) / e;
#pragma unroll
        for (int j = c + 1; j < 6; ++j) {
            const T l = Sd[c][j] * inv;
#pragma unroll
            for (int j2 = j; j2 < 6; ++j2) Sd[j][j2] -= l * Sd[c][j2];
            y[j] -= l * y[c];
        }
        nis += y[c] * y[c] * inv;
    }
    return pd ? nis : T(NAN);
}

// One lane per filter, launched and addressed as k_update (ekf_kernels.hpp).  Reads the state, never writes it.
template <typename T, bool DIRECT, bool PFP, bool COMPACT, bool GATE>
__global__ __launch_bounds__(kBlock) void k_innov(const T* __restrict__ st, T* __restrict__ zs, int64_t B, int32_t grid_x, int32_t block_x,   // (argument order: see k_predict)
                                                  const T* __restrict__ pfp, T* __restrict__ diag, T* __restrict__ nis_out, double chi2_max,
                                                  DevParams<T> p)
{
    args_early(st, zs, B, grid_x, block_x);
    const int64_t i = batch_block((unsigned)grid_x) * block_x + threadIdx.x;
    if (i >= B) return;
    T zr[kZW];
    load_rec<T, kZW, 0, kZW>(zs, i, zr);
    T x[kXW];
    load_rec<T, kSW, 0, kXW>(st, i, x);
    if (zr[7] == T(0) || filter_uninitialised(x)) {   // nothing to evaluate: nu = 0, S = 0, NIS = NaN, not accepted
        if constexpr (GATE) {
            if (zr[7] != T(0)) zs[word_off<T>(7, i, kZW)] = T(0);
        } else {
            T r[kDW];
#pragma unroll
            for (int k = 0; k < kDW; ++k) r[k] = T(0);
            store_rec<T, kDW, 0, kDW>(diag, i, r);
        }
        nis_out[i] = T(NAN);
        return;
    }
    T Pj[6][6];
    {   // P_JJ out of the register image: only the quad rows that hold one of its 21 elements are read
        T P[kPW];
        load_P_rows<T, COMPACT, pose_needs>(st, i, P);
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) Pj[a][b] = Pj[b][a] = P[sidx(innov_state_col(a), innov_state_col(b))];
    }
    Noise<T> nz;
    load_noise<T, PFP>(p, pfp, i, nz);
    const T z[7] = {zr[0], zr[1], zr[2], zr[3], zr[4], zr[5], zr[6]};
    UpdatePrep<T> u;
    ekf_update_prepare<T, DIRECT>(p, nz, x, z, u, [](const T (&)[7]) {});
    T nu[6], Sp[21];
    const T nis = innov_from_prep<T, DIRECT>(u, Pj, nu, Sp);
    if constexpr (GATE) {
        // NaN compares false: a non-finite NIS is never accepted; +Inf only passes an infinite threshold, which accepts finite NIS only
        const bool accepted = isfinite((double)nis) && (double)nis <= chi2_max;
        if (!accepted) zs[word_off<T>(7, i, kZW)] = T(0);
    } else {
        T r[kDW];
#pragma unroll
        for (int k = 0; k < 6; ++k) r[k] = nu[k];
#pragma unroll
        for (int k = 0; k < 21; ++k) r[6 + k] = Sp[k];
        r[27] = T(0);
        store_rec<T, kDW, 0, kDW>(diag, i, r);
    }
    nis_out[i] = nis;
}

}  // namespace qle
