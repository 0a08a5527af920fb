// ekf_score.hpp -- k_score: innovation scoring for noise sweeps (libqle_score.so, include/qle_score.h).  gfx950.
//
// Which parameter set of a Monte-Carlo sweep is better?  The criterion that needs no truth: each filter's innovation log-likelihood
//     log L = -1/2 sum_t ( NIS_t + log det S_t + 6 ln 2 pi )
// over the run, plus per-component consistency statistics of the innovation.  Everything it is made of is what the gate evaluates
// (pregate_eval, ekf_pregate.hpp): the predict in registers, nu, S = G P G^T + R_k and its L D L^T factor, whose pivots are log det S =
// sum log d_m.  k_score is k_pregate<PREDICT = true> with another ending: instead of deciding, it adds the tick to an accumulator
// record per filter.  It reads the state and the input records and writes neither -- the mask word in particular -- so the tick behind
// it is the plain tick.
//
//   loads      those of k_pregate<PREDICT = true>: x (16), the quad rows of P over pregate_needs, u (6), z (7 + mask word), noise;
//              and the filter's accumulator record, words 0..35 (fp64)
//   evaluate   pregate_eval_pivots: nu, S, NIS, the pivots d_m
//   accumulate score_accumulate, below; fp64 whatever T is
//   stores     the accumulator record, words 0..35, of the filters that are on
// The accumulators are plane-major, acc[kScoreWords][padded batch]: a wave's access to one plane is 512 contiguous bytes.  One lane owns
// one filter: no atomics, a deterministic result.  Words moved per filter, counted in fp32 words as everywhere: the loads of k_pregate
// (full records 150 / 120 in fp32 / fp64, compact records 78 / 76) and 2 x 36 doubles = 144 for the record: 294 / 264 and 222 / 220.
// Per-filter noise adds its 24-word record.
//
// Every lane runs straight-line code up to the stores (k_pregate's rule): a filter that is masked, not initialised or beyond the batch's
// ragged end computes on and selects its own words back.
//
// The batch summary is the two-stage deterministic reduction of the read-only diagnostics: k_score_tiles reduces words 0..29 of a tile's
// filters by xor-shuffles (wave_sum, ekf_layout.hpp) into [tiles][30] partials, k_score_reduce adds the tiles in a fixed order
// (reduce_tiles).
//
// The per-tick arithmetic (score_accumulate) is written so that a host compiler accepts it: tests/cpp/score_harness.cpp runs it on the
// CPU, behind pregate_eval_pivots, over consecutive tag ticks.  The kernels follow under __HIPCC__.
#pragma once

#include <cmath>
#include <cstdint>

#include "ekf_pregate.hpp"

namespace qle {

constexpr int kScoreWords = 40;   // QSC_WORDS: planes of an accumulator array
constexpr int kScoreLive = 36;    // words 0..35 are read and written; 36..39 stay zero
constexpr int kScoreSums = 30;    // QSC_SUMS: words 0..29 are sums (30..35: the previous scored innovation)
// the words of an accumulator record (include/qle_score.h)
enum ScoreWord { kScN = 0, kScNis = 1, kScNis2 = 2, kScLogdet = 3, kScBad = 4, kScPairs = 5, kScNu = 6, kScNu2 = 12, kScSkk = 18, kScLag = 24, kScPrev = 30 };

// One tag tick of one filter into its record a.  on: mask word != 0, the filter holds a state and lies inside the batch.  nis, pd, nu,
// S, d: what pregate_eval_pivots returned.  Scored = on, S positive definite and NIS finite; on but not scored counts in n_bad and
// changes nothing else; not on changes no word (every word is selected, never "plus zero").
template <typename T>
__device__ __forceinline__ void score_accumulate(double (&a)[kScoreLive], bool on, T nis, bool pd, const T (&nu)[6], const T (&S)[6][6], const T (&d)[6])
{
    const double nd = (double)nis;
    const bool scored = on && pd && std::isfinite(nd);
    const bool pair = scored && a[kScN] >= 1.0;   // a previous scored innovation exists
    double logdet = 0.0;
#pragma unroll
    for (int m = 0; m < 6; ++m) logdet += std::log((double)d[m]);
    a[kScN] = scored ? a[kScN] + 1.0 : a[kScN];
    a[kScNis] = scored ? a[kScNis] + nd : a[kScNis];
    a[kScNis2] = scored ? a[kScNis2] + nd * nd : a[kScNis2];
    a[kScLogdet] = scored ? a[kScLogdet] + logdet : a[kScLogdet];
    a[kScBad] = on && !scored ? a[kScBad] + 1.0 : a[kScBad];
    a[kScPairs] = pair ? a[kScPairs] + 1.0 : a[kScPairs];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const double v = (double)nu[k];
        a[kScNu + k] = scored ? a[kScNu + k] + v : a[kScNu + k];
        a[kScNu2 + k] = scored ? a[kScNu2 + k] + v * v : a[kScNu2 + k];
        a[kScSkk + k] = scored ? a[kScSkk + k] + (double)S[k][k] : a[kScSkk + k];
        a[kScLag + k] = pair ? a[kScLag + k] + v * a[kScPrev + k] : a[kScLag + k];
        a[kScPrev + k] = scored ? v : a[kScPrev + k];
    }
}

}  // namespace qle

#if defined(__HIPCC__)
#include "ekf_layout.hpp"

namespace qle {

// One lane per filter, one wave per workgroup (a workgroup is one 64-filter tile).  Reads the state and the tick's records, writes
// neither.  acc [kScoreWords][Bp] doubles, Bp = the padded batch (gridDim.x * kTile): every lane may load its record.
// One wave per SIMD is what the registers are budgeted for: the record is 72 registers next to what k_pregate holds, and bounded to two
// waves every full-record and every fp64 instantiation spilled (up to 612 bytes of scratch per lane); bounded to one, none does, and the
// compact fp32 ones stay below 256 registers and run two waves all the same.
template <typename T, bool DIRECT, bool PFP, bool COMPACT>
__global__ __launch_bounds__(kTile, 1) void k_score(const T* __restrict__ st, const T* __restrict__ us, const T* __restrict__ zs, int64_t B,
                                                    const T* __restrict__ pfp, double* __restrict__ acc, int64_t Bp, DevParams<T> p)
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
    load_noise<T, PFP>(p, pfp, i, nz);
    double a[kScoreLive];
#pragma unroll
    for (int w = 0; w < kScoreLive; ++w) a[w] = acc[(int64_t)w * Bp + i];
    const bool dead = filter_uninitialised(x);
    if (dead) x[9] = T(1);
    const T z[7] = {zr[0], zr[1], zr[2], zr[3], zr[4], zr[5], zr[6]};
    T nu[6], S[6][6], d[6];
    bool pd;
    const T nis = pregate_eval_pivots<T, DIRECT, true>(p, nz, x, P, u, z, nu, S, d, pd);
    const bool on = !dead && zr[7] != T(0) && i < B;
    score_accumulate<T>(a, on, nis, pd, nu, S, d);
    if (!on) return;
#pragma unroll
    for (int w = 0; w < kScoreLive; ++w) acc[(int64_t)w * Bp + i] = a[w];
}

// Batch summary, first stage: one wave per tile; words 0..29 of the tile's filters with mask != 0 (mask [B] or null: all), each by the
// fixed tree of wave_sum, into partials [tiles][kScoreSums].
__global__ __launch_bounds__(kTile) void k_score_tiles(const double* __restrict__ acc, int64_t B, int64_t Bp, const uint8_t* __restrict__ mask,
                                                       double* __restrict__ partials)
{
    const int64_t i = (int64_t)blockIdx.x * kTile + threadIdx.x;   // < Bp: the planes are allocated for whole tiles
    const int64_t row = i < B ? i : B - 1;                          // the mask is not: the lanes beyond the end read the last row
    const bool in = i < B && (mask ? mask[row] != 0 : true);
    const int lane = (int)threadIdx.x;
    double mine = 0.0;
#pragma unroll
    for (int w = 0; w < kScoreSums; ++w) {
        const double v = acc[(int64_t)w * Bp + i];
        const double s = wave_sum(in ? v : 0.0);
        mine = lane == w ? s : mine;
    }
    if (lane < kScoreSums) partials[(int64_t)blockIdx.x * kScoreSums + lane] = mine;
}

// Second stage, one workgroup: the tiles' partials in a fixed order (reduce_tiles, ekf_layout.hpp) into out [kScoreSums].
__global__ __launch_bounds__(kBlock) void k_score_reduce(const double* __restrict__ partials, int64_t tiles, double* __restrict__ out)
{
    reduce_tiles<kScoreSums, 32>(partials, tiles, [&](int f, double tot) { out[f] = tot; });
}

}  // namespace qle
#endif  // __HIPCC__
