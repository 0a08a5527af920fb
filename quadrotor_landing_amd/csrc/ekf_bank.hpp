// ekf_bank.hpp -- k_bank_fuse: posterior weights and the moment-matched estimate of filter banks on the device (libqle_bank.so,
// include/qle_bank.h).  gfx950.
//
// A handle of B filters is G = B / M banks of M consecutive members (M a power of two in 2..64, B a multiple of M): filters that run
// different noise parameters on the same IMU samples and tag poses.  With the members' unnormalised log-weights l_i (float64: the
// innovation log-likelihood of ekf_score.hpp, or anything else) a bank publishes
//     w_i  = exp(l_i - lmax) / sum_j exp(l_j - lmax)                    over its valid members, lmax their maximum
//     d_i  = x_i (-) x_ref                                               15 words, ref = the lowest-index valid member with l_i == lmax
//     m    = sum w_i d_i
//     xbar = x_ref (+) m                                                 r, v, ab, wb: x_ref + m;  q = norm(q_ref (x) exp(m_th))
//     Pbar = sum w_i (P_i + (d_i - m)(d_i - m)^T)
// the moment-matched Gaussian of the mixture.  The attitude difference is log(norm(q_ref^-1 (x) q_i)), the form of e_th in nees_eval
// (ekf_consistency.hpp) with the w < -0.75 flip of quat_norm, so a member stored as -q is the same attitude.  FIRST ORDER: the member
// covariances are taken as expressed in the fused tangent space (P_i is not transported from member i's tangent space at q_i to the
// one at qbar) -- the usual error-state approximation, exact for members that share an attitude and good while the members' attitudes
// lie within a fraction of a radian of one another, which members of one bank do.
//
// A member is VALID when its mask byte is not 0, it holds a state (filter_uninitialised is false) and l_i is finite.  A bank without a
// valid member is EMPTY: its fused record is all zero (the engine's "not initialised"), best = -1 and every w_i = 0.  An invalid member
// contributes exact zeros to every sum (selects, not products: 0 * NaN is NaN).  A valid member's non-finite words propagate into its own
// bank's record, where k_health flags them, and never into another bank's: no cross-lane operation leaves a bank.
//
// Precision: d_i is formed in the compute dtype T (differences of nearby values: exact or rounded relative to d) and promoted; the
// weights, m, the fused state, every covariance term and every sum are fp64 whatever T is, cast to T once.
//
// Bank sums are a fixed xor-butterfly over the bank's M lanes, offsets 1, 2, ..., M/2: every lane of the bank ends with the same bits,
// and they do not depend on where the bank sits in its tile or in the batch.  No atomics.
//
// The arithmetic is written so that a host compiler accepts it: tests/cpp/bank_harness.cpp runs it on the CPU, with the butterfly
// restated as the same tree over an array, against a numpy restatement with plain sums.  The kernel follows under __HIPCC__.
#pragma once

#include <cmath>
#include <cstdint>

#include "ekf_device.hpp"

namespace qle {

constexpr int kBankMaxMembers = 64;   // a bank never leaves one 64-filter wave tile

__host__ __device__ constexpr bool bank_members_ok(int64_t M) { return M >= 2 && M <= kBankMaxMembers && (M & (M - 1)) == 0; }

// false for NaN and +-Inf (no library call, the same test on host and device)
__host__ __device__ __forceinline__ bool bank_finite(double v) { return v - v == 0.0; }

// asked: mask byte != 0 (or no mask) and inside the batch
template <typename T>
__host__ __device__ __forceinline__ bool bank_member_valid(const T (&x)[16], double logw, bool asked)
{
    return asked && !filter_uninitialised(x) && bank_finite(logw);
}

// w~_i: exp(l_i - lmax) for a valid member, else exactly 0; the member with l_i == lmax gets exactly 1
__host__ __device__ __forceinline__ double bank_weight_raw(bool valid, double logw, double lmax) { return valid ? exp(logw - lmax) : 0.0; }

// d = x (-) xr: plain differences of r, v, ab, wb; log(norm(qr^-1 (x) q)) for the attitude
template <typename T>
__device__ __forceinline__ void bank_diff(const T (&x)[16], const T (&xr)[16], T (&d)[15])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        d[k] = x[k] - xr[k];
        d[3 + k] = x[3 + k] - xr[3 + k];
        d[9 + k] = x[10 + k] - xr[10 + k];
        d[12 + k] = x[13 + k] - xr[13 + k];
    }
    const T qc[4] = {-xr[6], -xr[7], -xr[8], xr[9]}, q[4] = {x[6], x[7], x[8], x[9]};
    T dq[4], dth[3];
    quat_mul(qc, q, dq);
    quat_norm(dq);
    quat_log(dq, dth);
    d[6] = dth[0]; d[7] = dth[1]; d[8] = dth[2];
}

// xbar = x_ref (+) m in fp64, cast once; all zero for an empty bank
template <typename T>
__device__ __forceinline__ void bank_fuse_state(const T (&xr)[16], const double (&m)[15], bool empty, T (&xf)[16])
{
    const double qr[4] = {(double)xr[6], (double)xr[7], (double)xr[8], (double)xr[9]}, mth[3] = {m[6], m[7], m[8]};
    double qe[4], qn[4];
    quat_exp(mth, qe);
    quat_mul(qr, qe, qn);
    quat_norm(qn);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        xf[k] = empty ? T(0) : (T)((double)xr[k] + m[k]);
        xf[3 + k] = empty ? T(0) : (T)((double)xr[3 + k] + m[3 + k]);
        xf[10 + k] = empty ? T(0) : (T)((double)xr[10 + k] + m[9 + k]);
        xf[13 + k] = empty ? T(0) : (T)((double)xr[13 + k] + m[12 + k]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) xf[6 + k] = empty ? T(0) : (T)qn[k];
}

// one member's term of Pbar_ab: w (P_ab + c_a c_b), c = d - m; exactly 0 for an invalid member
__host__ __device__ __forceinline__ double bank_cov_term(bool valid, double w, double P, double ca, double cb)
{
    return valid ? w * (P + ca * cb) : 0.0;
}

// The covariance words of a record, in record order, as (row, column) of P -- the inverse of sidx (full records, 120 words) or of sidx9
// (compact records, 45 words and 3 of padding: row = -1).  A compile-time table.
template <bool COMPACT>
struct BankWords {
    static constexpr int kWords = COMPACT ? 48 : 120;
    signed char a[kWords], b[kWords];
    constexpr BankWords() : a{}, b{}
    {
        for (int w = 0; w < kWords; ++w) a[w] = b[w] = -1;
        const int n = COMPACT ? 9 : 15;
        for (int i = 0; i < n; ++i)
            for (int j = i; j < n; ++j) {
                const int w = COMPACT ? i * 9 - i * (i - 1) / 2 + (j - i) : sidx_formula(i, j);
                a[w] = (signed char)i;
                b[w] = (signed char)j;
            }
    }
};
template <bool COMPACT> constexpr BankWords<COMPACT> kBankWords{};

}  // namespace qle

#if defined(__HIPCC__)
#include "ekf_layout.hpp"

namespace qle {

// ---- the butterflies: N values at once over the M lanes of a bank (M wave-uniform), every lane ends with the result
template <int N>
__device__ __forceinline__ void bank_sum(double (&v)[N], int M)
{
    for (int o = 1; o < M; o <<= 1) {
        double t[N];
#pragma unroll
        for (int k = 0; k < N; ++k) t[k] = __shfl_xor(v[k], o);
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] += t[k];
    }
}
__device__ __forceinline__ double bank_max(double v, int M)
{
    for (int o = 1; o < M; o <<= 1) {
        const double t = __shfl_xor(v, o);
        v = t > v ? t : v;
    }
    return v;
}
__device__ __forceinline__ int bank_min(int v, int M)
{
    for (int o = 1; o < M; o <<= 1) {
        const int t = __shfl_xor(v, o);
        v = t < v ? t : v;
    }
    return v;
}

template <int N, typename F, int... K>
__device__ __forceinline__ void bank_static_for_seq(F&& f, std::integer_sequence<int, K...>) { (..., f(std::integral_constant<int, K>{})); }
template <int N, typename F>
__device__ __forceinline__ void bank_static_for(F&& f) { bank_static_for_seq<N>(f, std::make_integer_sequence<int, N>{}); }

// One lane per member, one wave per workgroup.  Workgroup t < in_tiles reads input tile t; its 64 / M banks are banks
// t * (64 / M) + lane / M, which all lie in output tile t / M at lanes (t % M) * (64 / M) + lane / M: the output tile is a function of
// the workgroup index.  The grid is M * out_tiles workgroups: those past the input (fewer than M) hold no member, read tile in_tiles - 1
// again and write the empty (all zero) records that fill the last output tile, so every record of the workspace is defined.
//
// P is streamed, not resident: the record's covariance quad rows are walked in groups of kBankGroup fp64 terms; a group's rows are
// requested before the butterfly of the group in front of it runs.  Each bank's first lane stores the fused quads.
constexpr int kBankGroup = 20;
template <typename T, bool COMPACT>
__global__ __launch_bounds__(kTile) void k_bank_fuse(const T* __restrict__ st, T* __restrict__ out, const double* __restrict__ logw,
                                                     const uint8_t* __restrict__ mask, double* __restrict__ w_out, int32_t* __restrict__ best,
                                                     int64_t B, int32_t M, int32_t in_tiles)
{
    using Q = typename Quad<T>::type;
    constexpr int VW = Quad<T>::VW;
    constexpr int kRows = BankWords<COMPACT>::kWords / VW;          // covariance quad rows of the record
    constexpr int kGR = kBankGroup / VW;              // quad rows per group
    constexpr int kGroups = (kRows + kGR - 1) / kGR;
    args_early(st, logw, B);
    const int lane = (int)threadIdx.x;
    const int t = (int)blockIdx.x;
    const int64_t i = (int64_t)t * kTile + lane;
    const int64_t row = i < B ? i : B - 1;            // the tensors are not padded: the lanes beyond the end read the last row
    const T* tb = st + (int64_t)(t < in_tiles ? t : in_tiles - 1) * (kSW * kTile);
    const int nb_shift = __builtin_ctz((unsigned)M);  // lane / M
    const int ot = t >> nb_shift;                                                    // t / M
    const int ol = (t & (M - 1)) * (kTile >> nb_shift) + (lane >> nb_shift);         // (t % M) * (64 / M) + lane / M
    T* ob = out + (int64_t)ot * (kSW * kTile);
    const bool leader = (lane & (M - 1)) == 0;
    auto in_quad = [&](int r) { return *reinterpret_cast<const Q*>(tb + (r * kTile + lane) * VW); };
    auto out_quad = [&](int r) { return reinterpret_cast<Q*>(ob + (r * kTile + ol) * VW); };

    T x[kXW];
#pragma unroll
    for (int k = 0; k < kXW / VW; ++k) unpack_quad(in_quad(k), &x[k * VW]);
    Q cur[kGR], nxt[kGR];
    bank_static_for<kGR>([&](auto k) {
        if constexpr (k.value < kRows) cur[k.value] = in_quad(kXW / VW + k.value);
    });
    const double lw = logw[row];
    const bool asked = i < B && (mask ? mask[row] != 0 : true);

    // 1, 2: valid members, weights, the reference member
    const bool valid = bank_member_valid(x, lw, asked);
    const double lmax = bank_max(valid ? lw : -INFINITY, M);
    const int ref = bank_min(valid && lw == lmax ? (lane & (M - 1)) : kBankMaxMembers, M);
    const bool empty = ref == kBankMaxMembers;
    double wsum[1] = {bank_weight_raw(valid, lw, lmax)};
    const double wraw = wsum[0];
    bank_sum<1>(wsum, M);
    const double w = empty ? 0.0 : wraw / wsum[0];
    // 3: differences against the reference member's state, m
    const int src = (lane & ~(M - 1)) + (empty ? 0 : ref);
    T xr[kXW];
#pragma unroll
    for (int k = 0; k < kXW; ++k) xr[k] = __shfl(x[k], src);
    T d[15];
    bank_diff(x, xr, d);
    double c[15], m[15];
#pragma unroll
    for (int k = 0; k < 15; ++k) {
        c[k] = (double)d[k];
        m[k] = valid ? w * c[k] : 0.0;
    }
    bank_sum<15>(m, M);
    // 4: the fused state
    T xf[kXW];
    bank_fuse_state(xr, m, empty, xf);
#pragma unroll
    for (int k = 0; k < 15; ++k) c[k] = valid ? c[k] - m[k] : 0.0;
    if (leader) {
#pragma unroll
        for (int k = 0; k < kXW / VW; ++k) *out_quad(k) = pack_quad(&xf[k * VW]);
    }
    // 5: the covariance, streamed
    bank_static_for<kGroups>([&](auto g) {
        constexpr int r0 = g.value * kGR;
        bank_static_for<kGR>([&](auto k) {
            if constexpr (r0 + kGR + k.value < kRows) nxt[k.value] = in_quad(kXW / VW + r0 + kGR + k.value);
        });
        constexpr int nr = kRows - r0 < kGR ? kRows - r0 : kGR;
        double term[nr * VW];
        bank_static_for<nr>([&](auto k) {
            T p[VW];
            unpack_quad(cur[k.value], p);
            bank_static_for<VW>([&](auto e) {
                constexpr int wd = (r0 + k.value) * VW + e.value;
                constexpr int a = kBankWords<COMPACT>.a[wd], b = kBankWords<COMPACT>.b[wd];
                if constexpr (a >= 0) term[k.value * VW + e.value] = bank_cov_term(valid, w, (double)p[e.value], c[a], c[b]);
                else term[k.value * VW + e.value] = 0.0;   // the padding words of a compact record
            });
        });
        bank_sum<nr * VW>(term, M);
        if (leader) {
            bank_static_for<nr>([&](auto k) {
                T p[VW];
#pragma unroll
                for (int e = 0; e < VW; ++e) p[e] = (T)term[k.value * VW + e];
                *out_quad(kXW / VW + r0 + k.value) = pack_quad(p);
            });
        }
        bank_static_for<kGR>([&](auto k) {
            if constexpr (r0 + kGR + k.value < kRows) cur[k.value] = nxt[k.value];
        });
    });
    if (w_out && i < B) w_out[i] = w;
    if (best && leader && i < B) best[i >> nb_shift] = empty ? -1 : (int32_t)((i & ~(int64_t)(M - 1)) + ref);
}

}  // namespace qle
#endif  // __HIPCC__
