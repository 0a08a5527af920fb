// ekf_imm.hpp -- k_imm_mix and k_imm_update: the mixing step and the mode-probability recursion of an interacting multiple model
// estimator over the banks of ekf_bank.hpp, on the device (libqle_imm.so, include/qle_imm.h).  gfx950.
//
// A bank is M consecutive filters (ekf_bank.hpp: M a power of two in 2..64, so a bank never leaves one 64-filter wave tile).  With the
// members' unnormalised log mode probabilities l_i (float64) and the transition matrix Pi [M][M] (float64, row-major, shared by all
// banks), member j of a bank is re-initialised from the mixture of all members under the mixing weights:
//     mu_i     = exp(l_i - lmax) / sum exp(l_k - lmax)                   the weights of k_bank_fuse; 0 for an invalid member
//     c_j      = sum_i Pi[i][j] mu_i                                     i ascending
//     mu_{i|j} = Pi[i][j] mu_i / c_j
//     d_ij     = x_i (-) x_j                                             bank_diff: member j is its own reference
//     m_j      = sum_i mu_{i|j} d_ij
//     x0_j     = x_j (+) m_j                                             bank_fuse_state
//     P0_j     = sum_i mu_{i|j} (P_i + (d_ij - m_j)(d_ij - m_j)^T)       bank_cov_term
// First order as k_bank_fuse: P_i is not transported between tangent spaces.  d is formed in the compute dtype T; weights, terms and
// sums are fp64, cast to T once.  Every sum over i is a loop in ascending member order.
//
// Member j is MIXED when it is valid (bank_member_valid), c_j is finite and > 0, and some valid i != j has mu_{i|j} > 0; only mixed
// members are stored.  A term takes part where mu_{i|j} > 0, by a select and not by a product (0 * NaN is NaN): a zero of Pi isolates j
// from the non-finite words of i, and no cross-lane operation leaves a bank.
//
// The arithmetic is written so that a host compiler accepts it: tests/cpp/imm_harness.cpp runs it on the CPU, the shuffle loop restated
// as the same ascending loop over an array, against a numpy restatement with plain sums.  The kernels follow under __HIPCC__.
#pragma once

#include "ekf_bank.hpp"

namespace qle {

// one term of c_j; an invalid member has mu = 0 and contributes exactly 0
__host__ __device__ __forceinline__ double imm_pred_term(double pij, double mu_i) { return mu_i > 0.0 ? pij * mu_i : 0.0; }

__host__ __device__ __forceinline__ bool imm_c_ok(double c) { return bank_finite(c) && c > 0.0; }

// mu_{i|j}; 0 for an invalid i, not finite where c_j is no probability (such a j is not mixed)
__host__ __device__ __forceinline__ double imm_mix_weight(double pij, double mu_i, double cj) { return pij * mu_i / cj; }

// m_j += mu_{i|j} d_ij where mu_{i|j} > 0
template <typename T>
__device__ __forceinline__ void imm_mean_step(const T (&xi)[16], const T (&xj)[16], double w, double (&m)[15])
{
    T d[15];
    bank_diff(xi, xj, d);
#pragma unroll
    for (int k = 0; k < 15; ++k) m[k] += w > 0.0 ? w * (double)d[k] : 0.0;
}

// c = d_ij - m_j
template <typename T>
__device__ __forceinline__ void imm_centred(const T (&xi)[16], const T (&xj)[16], const double (&m)[15], double (&c)[15])
{
    T d[15];
    bank_diff(xi, xj, d);
#pragma unroll
    for (int k = 0; k < 15; ++k) c[k] = (double)d[k] - m[k];
}

// ---- the recursion: t_j = logc_j + loglik_j, logmu_j = t_j - logsumexp(t), floored
// ok: mask != 0, inside the batch and logc finite.  A NaN loglik counts as -inf.
__host__ __device__ __forceinline__ double imm_update_term(bool ok, double logc, double loglik) { return ok && loglik == loglik ? logc + loglik : -INFINITY; }
__host__ __device__ __forceinline__ double imm_update_exp(double t, double tmax) { return t > -INFINITY ? exp(t - tmax) : 0.0; }
__host__ __device__ __forceinline__ double imm_update_final(bool ok, double t, double tmax, double esum, double logmu_min)
{
    const double v = t > -INFINITY ? t - (tmax + log(esum)) : -INFINITY;
    return ok ? (v > logmu_min ? v : logmu_min) : -INFINITY;
}

}  // namespace qle

#if defined(__HIPCC__)

namespace qle {

// One lane per member, one wave per workgroup, workgroup t owns tile t.  A lane loads only its own record and stores only its own record;
// the other members' words arrive by __shfl from lane base + i in loops over i whose trip count is M (wave-uniform), so mixing in place
// has no hazard: no lane reads from memory a word that another lane writes.  The lanes of the last tile beyond the batch form whole
// banks without a valid member.
//
// x first (weights, c_j, pass 1 for m_j, the mixed state), then P streamed in the quad-row groups of k_bank_fuse: a group's rows are
// requested before the member loop of the group in front of it runs.  Each group's loop forms c = d_ij - m_j again from the shuffled x_i
// (only the components the group's words need survive), so no 15 x M values are kept.  All arithmetic goes through selects; the only
// divergence is the predicate on the stores.
constexpr int kImmGroup = kBankGroup;
template <typename T, bool COMPACT>
__global__ __launch_bounds__(kTile) void k_imm_mix(T* __restrict__ st, const double* __restrict__ logmu, const double* __restrict__ Pi,
                                                   const uint8_t* __restrict__ mask, double* __restrict__ logc, uint8_t* __restrict__ mixed_out,
                                                   int64_t B, int32_t M)
{
    using Q = typename Quad<T>::type;
    constexpr int VW = Quad<T>::VW;
    constexpr int kRows = BankWords<COMPACT>::kWords / VW;          // covariance quad rows of the record
    constexpr int kGR = kImmGroup / VW;                             // quad rows per group
    constexpr int kGroups = (kRows + kGR - 1) / kGR;
    args_early(st, logmu, B);
    const int lane = (int)threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * kTile + lane;
    const int64_t row = i < B ? i : B - 1;            // the tensors are not padded: the lanes beyond the end read the last row
    T* tb = st + (int64_t)blockIdx.x * (kSW * kTile);
    const int jm = lane & (M - 1), base = lane & ~(M - 1);          // this lane's member index, its bank's first lane
    auto quad = [&](int r) { return reinterpret_cast<Q*>(tb + (r * kTile + lane) * VW); };

    T x[kXW];
#pragma unroll
    for (int k = 0; k < kXW / VW; ++k) unpack_quad(*quad(k), &x[k * VW]);
    Q cur[kGR], nxt[kGR];
    bank_static_for<kGR>([&](auto k) {
        if constexpr (k.value < kRows) cur[k.value] = *quad(kXW / VW + k.value);
    });
    const double lw = logmu[row];
    const bool asked = i < B && (mask ? mask[row] != 0 : true);
    const double* pcol = Pi + jm;                                   // Pi[.][j]

    // the mode probabilities of k_bank_fuse, and the predicted probability c_j
    const bool valid = bank_member_valid(x, lw, asked);
    const double lmax = bank_max(valid ? lw : -INFINITY, M);
    double wsum[1] = {bank_weight_raw(valid, lw, lmax)};
    const double wraw = wsum[0];
    bank_sum<1>(wsum, M);
    const double mu = wsum[0] > 0.0 ? wraw / wsum[0] : 0.0;        // a bank with a valid member has wsum >= 1
    double cj = 0.0;
    for (int k = 0; k < M; ++k) cj += imm_pred_term(pcol[k * M], __shfl(mu, base + k));
    const bool cok = valid && imm_c_ok(cj);

    // pass 1: m_j, and whether anything but j itself takes part
    double m[15];
#pragma unroll
    for (int k = 0; k < 15; ++k) m[k] = 0.0;
    bool other = false;
    for (int k = 0; k < M; ++k) {
        const double w = imm_mix_weight(pcol[k * M], __shfl(mu, base + k), cj);
        T xi[kXW];
#pragma unroll
        for (int e = 0; e < kXW; ++e) xi[e] = __shfl(x[e], base + k);
        other = other || (k != jm && w > 0.0);
        imm_mean_step(xi, x, w, m);
    }
    const bool store = cok && other && i < B;
    T xf[kXW];
    bank_fuse_state(x, m, false, xf);
    if (store) {
#pragma unroll
        for (int k = 0; k < kXW / VW; ++k) *quad(k) = pack_quad(&xf[k * VW]);
    }

    // pass 2: the covariance, streamed
    bank_static_for<kGroups>([&](auto g) {
        constexpr int r0 = g.value * kGR;
        bank_static_for<kGR>([&](auto k) {
            if constexpr (r0 + kGR + k.value < kRows) nxt[k.value] = *quad(kXW / VW + r0 + kGR + k.value);
        });
        constexpr int nr = kRows - r0 < kGR ? kRows - r0 : kGR;
        T own[nr * VW];
        double term[nr * VW];
        bank_static_for<nr>([&](auto k) { unpack_quad(cur[k.value], &own[k.value * VW]); });
#pragma unroll
        for (int e = 0; e < nr * VW; ++e) term[e] = 0.0;
        for (int k = 0; k < M; ++k) {
            const double w = imm_mix_weight(pcol[k * M], __shfl(mu, base + k), cj);
            T xi[kXW];
#pragma unroll
            for (int e = 0; e < kXW; ++e) xi[e] = __shfl(x[e], base + k);
            double c[15];
            imm_centred(xi, x, m, c);
            bank_static_for<nr * VW>([&](auto e) {
                constexpr int wd = r0 * VW + e.value;
                constexpr int a = kBankWords<COMPACT>.a[wd], b = kBankWords<COMPACT>.b[wd];
                if constexpr (a >= 0) term[e.value] += bank_cov_term(w > 0.0, w, (double)__shfl(own[e.value], base + k), c[a], c[b]);
            });
        }
        if (store) {
            bank_static_for<nr>([&](auto k) {
                T p[VW];
                bank_static_for<VW>([&](auto e) {
                    constexpr int wd = (r0 + k.value) * VW + e.value;
                    if constexpr (kBankWords<COMPACT>.a[wd] >= 0) p[e.value] = (T)term[k.value * VW + e.value];
                    else p[e.value] = own[k.value * VW + e.value];   // the padding words of a compact record keep their bits
                });
                *quad(kXW / VW + r0 + k.value) = pack_quad(p);
            });
        }
        bank_static_for<kGR>([&](auto k) {
            if constexpr (r0 + kGR + k.value < kRows) cur[k.value] = nxt[k.value];
        });
    });
    if (i < B) logc[i] = cok ? log(cj) : -INFINITY;
    if (mixed_out && i < B) mixed_out[i] = store ? 1 : 0;
}

// One lane per member; fp64 whatever the handle computes in.
__global__ __launch_bounds__(kTile) void k_imm_update(const double* __restrict__ logc, const double* __restrict__ loglik, const uint8_t* __restrict__ mask,
                                                      double logmu_min, double* __restrict__ logmu, int64_t B, int32_t M)
{
    const int64_t i = (int64_t)blockIdx.x * kTile + (int)threadIdx.x;
    const int64_t row = i < B ? i : B - 1;
    const double lc = logc[row];
    const bool ok = i < B && (mask ? mask[row] != 0 : true) && bank_finite(lc);
    const double t = imm_update_term(ok, lc, loglik[row]);
    const double tmax = bank_max(t, M);
    double e[1] = {imm_update_exp(t, tmax)};
    bank_sum<1>(e, M);
    if (i < B) logmu[i] = imm_update_final(ok, t, tmax, e[0], logmu_min);
}

}  // namespace qle
#endif  // __HIPCC__
