// ekf_budget.hpp -- k_budget, k_budget_reduce: the per-component error budget of a batch against a truth, on the device
// (libqle_budget.so, include/qle_budget.h).  gfx950.
//
// What a Monte-Carlo sweep ends with: per group of filters the count, sum e, sum e e^T and sum P in fp64 -- the bias of every state, the
// sample covariance of the error and the covariance the filters report, averaged over the same ensemble.  k_budget is k_nees
// (ekf_consistency.hpp) with another ending: one lane per filter, one 64-filter tile per wave, one wave per workgroup, the same loads
// (load_rec / load_P_compact, load_truth, load_noise, the mask byte), and the error e of nees_eval (error_state, ekf_device.hpp).  It
// never writes the view.
//
//   words      256 doubles per lane (budget_lane / BudgetWords), 0.0 where the filter is not counted:
//                0            1.0
//                1 + k        e_k, k < 15 (0 for k >= 9 on a handle with 9 states)
//                16 + tri     e_i e_j, i <= j: the product of the two doubles, rounded once and never contracted with a later add
//                136 + tri    P_ij
//              tri(i, j) = 15 i - i (i - 1) / 2 + (j - i), the row-major upper triangle: the public order, not sidx
//   counted    on (mask != 0, a state, i < B), every e_k finite and every covariance word the record holds finite (the w * 0 probe of
//              k_health); status: 0 off, 1 counted, 2 on but not finite
//   tile sum   field f of a tile is the xor-butterfly of wave_sum (ekf_layout.hpp) over the 64 lanes' word f -- by definition.  It is
//              computed as a halving butterfly (reduce-scatter, tile_reduce below) instead of 256 wave_sum calls: at offset 32 a
//              v_permlane32_swap on the two dwords of a pair of fields (A, B) leaves A_l, A_l+32 in the lower half-wave and B_l-32, B_l
//              in the upper, and one v_add_f64 gives each half the pair sum of its field; offset 16 the same with v_permlane16_swap
//              (rows of 16 lanes); offsets 8, 4, 2, 1 move the field a lane gives away by DPP (row_ror:8, row_ror:4 / :12 under bank
//              masks, two quad permutes) and select the one it keeps.  Every add is x_l + x_(l ^ o) in lane l or in lane l ^ o, and fp
//              addition is commutative: each field's tree is exactly wave_sum's.  64 fields per round, four rounds, depth-first: the live
//              partials are a handful of doubles, and each lane ends a round with one field (lane l: field 64 r + l)
//   stores     partials [tiles][256] in field order (coalesced), status [B], err [B][n] in the destination dtype
//
// k_budget_reduce: one workgroup per group of `group_tiles` consecutive tiles, one thread per field, the tiles in ascending order from
// +0.0 (the sum of reduce_tiles<256, 256> on the group's slice) into sums [groups][256].  No atomics anywhere: the result is deterministic to the
// bit and additive over shards that are whole groups.
//
// The per-lane words and the butterfly's recursion are written so that a host compiler accepts them: tests/cpp/budget_harness.cpp runs
// budget_lane on the CPU against numpy and tile_reduce over 64-value arrays (the swaps and the DPP steps as array permutations) against
// the xor-butterfly.  The kernels follow under __HIPCC__.
#pragma once

#include <cmath>
#include <cstdint>

#include "ekf_device.hpp"

namespace qle {

constexpr int kBudgetWords = 256;   // QBG_WORDS of include/qle_budget.h
constexpr int kBudgetErr = 1, kBudgetOuter = 16, kBudgetCov = 136;   // first word of e, of e e^T, of P

// the row-major upper triangle of a 15 x 15 matrix and its inverse
__host__ __device__ constexpr int tri15(int i, int j) { return 15 * i - i * (i - 1) / 2 + (j - i); }
__host__ __device__ constexpr int tri15_row(int t)
{
    int i = 0;
    while (t >= 15 - i) { t -= 15 - i; ++i; }
    return i;
}
__host__ __device__ constexpr int tri15_col(int t) { return tri15_row(t) + (t - tri15(tri15_row(t), tri15_row(t))); }

// a * b rounded once: the product is a value of its own, whatever add follows it
__host__ __device__ __forceinline__ double mul_once(double a, double b)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double p = a * b;
    return p;
}

// The error and the decision of one filter.  x, P (the 15-state register image of the packed covariance), xt and the static biases as
// nees_eval takes them; n_states 15 or 9 (wave-uniform): with 9, e_k = 0 for k >= 9 and the bias blocks of P count as zero (every word
// the record holds still takes part in the decision).  on: mask != 0, a state, inside the batch.
// e: the error as err stores it (whatever `on` says: the caller selects).  Returns counted; then ec and P hold the values the words are
// made of, and zeros otherwise.  COMPACT: the record holds the 9 x 9 pose block only -- the other slots of P are zero on return
// whatever they held, and take no part in the decision.
template <typename T, bool COMPACT>
__device__ __forceinline__ bool budget_lane(const T (&x)[16], T (&P)[120], const T (&xt)[16], const T (&ab_static)[3], const T (&wb_static)[3],
                                            int n_states, bool on, T (&e)[15], T (&ec)[15])
{
    constexpr int NW = COMPACT ? 9 : 15;
    error_state<T>(x, xt, ab_static, wb_static, e);
    const bool nine = n_states == 9;
#pragma unroll
    for (int k = 9; k < 15; ++k) e[k] = nine ? T(0) : e[k];
    T probe = T(0);   // w * 0 is 0 for a finite word and NaN otherwise
#pragma unroll
    for (int k = 0; k < 15; ++k) probe += e[k] * T(0);
#pragma unroll
    for (int a = 0; a < NW; ++a)
#pragma unroll
        for (int b = a; b < NW; ++b) probe += P[sidx(a, b)] * T(0);
    const bool counted = on && probe == T(0);
#pragma unroll
    for (int k = 0; k < 15; ++k) ec[k] = counted ? e[k] : T(0);
#pragma unroll
    for (int a = 0; a < 15; ++a)
#pragma unroll
        for (int b = a; b < 15; ++b) P[sidx(a, b)] = (counted && b < NW && !(nine && b >= 9)) ? P[sidx(a, b)] : T(0);
    return counted;
}

// The 256 words of a lane, each formed where it is asked for (F is a compile-time constant): nothing is held but ec and P.
template <typename T>
struct BudgetWords {
    const T (&ec)[15];
    const T (&P)[120];
    double count;   // 1.0 or 0.0
    template <int F>
    __host__ __device__ __forceinline__ double word() const
    {
        static_assert(F >= 0 && F < kBudgetWords, "256 words");
        if constexpr (F == 0) {
            return count;
        } else if constexpr (F < kBudgetOuter) {
            return (double)ec[F - kBudgetErr];
        } else if constexpr (F < kBudgetCov) {
            constexpr int i = tri15_row(F - kBudgetOuter), j = tri15_col(F - kBudgetOuter);
            return mul_once((double)ec[i], (double)ec[j]);
        } else {
            constexpr int w = sidx(tri15_row(F - kBudgetCov), tri15_col(F - kBudgetCov));   // a constant: the image stays in registers
            return (double)P[w];
        }
    }
};

// ---- the halving butterfly.  Level K of round R holds 2^K fields reduced over the offsets 32 .. 64 >> K; a lane whose bit 64 >> K is
// clear keeps the first half's value, the others the second half's (Ops::combine<O>(a, b): a_l + a_(l ^ O) where bit O of l is clear,
// b_l + b_(l ^ O) where it is set).  A lane therefore ends with the leaf whose position is its own index bit-reversed; the leaves are laid
// out bit-reversed, so that lane l ends with field 64 R + l.
__host__ __device__ constexpr int bitrev6(int v)
{
    int r = 0;
    for (int b = 0; b < 6; ++b) r |= ((v >> b) & 1) << (5 - b);
    return r;
}
template <int K, int J, int R, typename Ops, typename Words>
__host__ __device__ __forceinline__ auto tile_reduce(const Ops& ops, const Words& w)
{
    if constexpr (K == 0) {
        return ops.template leaf<64 * R + bitrev6(J)>(w);
    } else {
        const auto a = tile_reduce<K - 1, J, R>(ops, w);
        const auto b = tile_reduce<K - 1, J + (1 << (K - 1)), R>(ops, w);
        return ops.template combine<(64 >> K)>(a, b);
    }
}

}  // namespace qle

#if defined(__HIPCC__)
#include "ekf_layout.hpp"

namespace qle {

// DPP controls (the dpp_ctrl field of a VOP DPP instruction)
constexpr int kDppQuadXor1 = 0xB1;   // quad_perm:[1,0,3,2]
constexpr int kDppQuadXor2 = 0x4E;   // quad_perm:[2,3,0,1]
constexpr int kDppRowRor = 0x120;    // row_ror:n = 0x120 + n: the row of 16 rotated right, lane l reads lane (l - n) mod 16

// v of lane l ^ O, O = 8, 4, 2 or 1, by DPP moves of the two dwords.  O = 4: row_ror:12 reads l + 4 (= l ^ 4 where bit 2 is clear: banks
// 0 and 2 of a row) and row_ror:4 reads l - 4 (banks 1 and 3); the bank mask keeps the first move's lanes through the second.
template <int O>
__device__ __forceinline__ double lane_xor_dpp(double v)
{
    static_assert(O == 8 || O == 4 || O == 2 || O == 1, "the offsets inside a row of 16 lanes");
    const int lo = __double2loint(v), hi = __double2hiint(v);
    int rl, rh;
    if constexpr (O == 4) {
        rl = __builtin_amdgcn_update_dpp(lo, lo, kDppRowRor + 12, 0xF, 0x5, false);
        rh = __builtin_amdgcn_update_dpp(hi, hi, kDppRowRor + 12, 0xF, 0x5, false);
        rl = __builtin_amdgcn_update_dpp(rl, lo, kDppRowRor + 4, 0xF, 0xA, false);
        rh = __builtin_amdgcn_update_dpp(rh, hi, kDppRowRor + 4, 0xF, 0xA, false);
    } else {
        constexpr int ctrl = O == 8 ? kDppRowRor + 8 : O == 2 ? kDppQuadXor2 : kDppQuadXor1;
        rl = __builtin_amdgcn_update_dpp(lo, lo, ctrl, 0xF, 0xF, false);
        rh = __builtin_amdgcn_update_dpp(hi, hi, ctrl, 0xF, 0xF, false);
    }
    return __hiloint2double(rh, rl);
}

// the butterfly's steps on a wave: a value per lane
template <typename T>
struct WaveOps {
    int lane;
    template <int F>
    __device__ __forceinline__ double leaf(const BudgetWords<T>& w) const { return w.template word<F>(); }
    template <int O>
    __device__ __forceinline__ double combine(double a, double b) const
    {
        if constexpr (O >= 16) {
            // the swap exchanges the upper half (O = 32) / the odd rows (16) of its first operand with the lower half / the even rows of
            // its second: afterwards a holds a_l | b_(l - O) and b holds a_(l + O) | b_l
            const unsigned al = (unsigned)__double2loint(a), ah = (unsigned)__double2hiint(a);
            const unsigned bl = (unsigned)__double2loint(b), bh = (unsigned)__double2hiint(b);
            if constexpr (O == 32) {
                const auto l = __builtin_amdgcn_permlane32_swap(al, bl, false, false);
                const auto h = __builtin_amdgcn_permlane32_swap(ah, bh, false, false);
                return __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
            } else {
                const auto l = __builtin_amdgcn_permlane16_swap(al, bl, false, false);
                const auto h = __builtin_amdgcn_permlane16_swap(ah, bh, false, false);
                return __hiloint2double((int)h[0], (int)l[0]) + __hiloint2double((int)h[1], (int)l[1]);
            }
        } else {
            const bool up = (lane & O) != 0;
            const double keep = up ? b : a, give = up ? a : b;
            return keep + lane_xor_dpp<O>(give);
        }
    }
};

// One lane per filter, one wave per workgroup (a workgroup is one 64-filter tile).  Reads the state, never writes it.
// xt: rows of 16 of float32 / float64 (true_f64), [B] of them (truth_stride = 16) or one for every filter (0); mask [B] or null;
// partials [tiles][256] (fp64); err [B][n_states] of dst dtype and status [B]: either may be null (wave-uniform).
// fp64 holds 240 registers of P: one wave per SIMD, as k_nees<double>; fp32 fits two.
template <typename T, bool PFP, bool COMPACT>
__global__ __launch_bounds__(kTile, sizeof(T) == 8 ? 1 : 2) void k_budget(const T* __restrict__ st, const void* __restrict__ xt, int64_t B,
                                                                          const uint8_t* __restrict__ mask, const T* __restrict__ pfp,
                                                                          double* __restrict__ partials, void* __restrict__ err_out,
                                                                          uint8_t* __restrict__ status, int32_t truth_stride, int32_t n_states,
                                                                          int32_t true_f64, int32_t dst_f64, DevParams<T> p)
{
    args_early(st, xt, B);
    const int64_t i = (int64_t)blockIdx.x * kTile + threadIdx.x;   // the records are allocated for whole tiles: every lane may load
    const int64_t row = i < B ? i : B - 1;                          // the tensors are not: the lanes beyond the end read the last row
    T x[kXW], P[kPW], t[16];
    load_rec<T, kSW, 0, kXW>(st, i, x);
    if constexpr (COMPACT) load_P_compact<T>(st, i, P);
    else load_rec<T, kSW, kXW, kPW>(st, i, P);
    load_truth<T>(xt, truth_stride != 0 ? row : 0, true_f64 != 0, t);
    Noise<T> nz;
    load_noise<T, PFP>(p, pfp, i, nz);
    const bool dead = filter_uninitialised(x);
    if (dead) x[9] = T(1);
    const bool on = !dead && i < B && (mask ? mask[row] != 0 : true);
    T e[15], ec[15];
    const bool counted = budget_lane<T, COMPACT>(x, P, t, nz.ab_static, nz.wb_static, n_states, on, e, ec);
    // the tile sum: every lane takes part (the exchanges need the whole wave), the lanes beyond the end with zeros
    const int lane = (int)threadIdx.x;
    const BudgetWords<T> words{ec, P, counted ? 1.0 : 0.0};
    const WaveOps<T> ops{lane};
    double* out = partials + (int64_t)blockIdx.x * kBudgetWords + lane;
    out[0] = tile_reduce<6, 0, 0>(ops, words);
    out[64] = tile_reduce<6, 0, 1>(ops, words);
    out[128] = tile_reduce<6, 0, 2>(ops, words);
    out[192] = tile_reduce<6, 0, 3>(ops, words);
    if (i >= B) return;
    if (status) status[i] = on ? (counted ? 1 : 2) : 0;
    if (err_out) {
#pragma unroll
        for (int k = 0; k < 15; ++k)
            if (k < n_states) put<T>(err_out, i * n_states + k, on ? e[k] : T(0), dst_f64 != 0);
    }
}

// One workgroup per group: the tiles [g group_tiles, min((g + 1) group_tiles, tiles)) of the partials, one thread per field, in
// ascending order from +0.0 into sums [groups][256] -- the sum reduce_tiles<256, 256> (ekf_layout.hpp) gives on the group's slice, a
// single slice per field.  Written out here because that loop keeps one load in flight per thread: with one group for the batch the
// chain of 1 024 (65 536 filters) or 32 768 (2 097 152) dependent load-add steps of some 0.3 us each was the whole cost of a call
// (profiles/budget.md).  The loads of kReduceAhead tiles are issued together, the adds stay in tile order: the same bits.
constexpr int kReduceAhead = 32;
__global__ __launch_bounds__(kBlock) void k_budget_reduce(const double* __restrict__ partials, int64_t tiles, int64_t group_tiles, double* __restrict__ sums)
{
    static_assert(kBlock == kBudgetWords, "one thread per field");
    const int64_t g = blockIdx.x, t0 = g * group_tiles;
    const int64_t n = tiles - t0 < group_tiles ? tiles - t0 : group_tiles;
    const double* p = partials + t0 * kBudgetWords + threadIdx.x;
    double acc = 0.0;
    int64_t k = 0;
    for (; k + kReduceAhead <= n; k += kReduceAhead) {
        double v[kReduceAhead];
#pragma unroll
        for (int u = 0; u < kReduceAhead; ++u) v[u] = p[(k + u) * kBudgetWords];
#pragma unroll
        for (int u = 0; u < kReduceAhead; ++u) acc += v[u];
    }
    for (; k < n; ++k) acc += p[k * kBudgetWords];
    sums[g * kBudgetWords + threadIdx.x] = acc;
}

}  // namespace qle
#endif  // __HIPCC__
