// ekf_layout.hpp -- record layout of the batched EKF engine in HBM and the device helpers that move records (gfx950).
//
// Data layout in HBM: "wave tiles".  The batch is cut into tiles of 64
// consecutive filters (one wavefront).  A per-filter record of WT words of
// type T is stored tile by tile; inside a tile it is stored as rows of 16-byte
// quads, row k holding words [k*VW, (k+1)*VW) of the tile's 64 filters
// (VW = 4 for fp32, 2 for fp64):
//     off(word w, filter i) = (i/64)*WT*64 + ((w/VW)*64 + i%64)*VW + w%VW
// Lane l of a wave reads one aligned 16-byte quad per row (global_load_dwordx4),
// a row is 1 KiB contiguous, and the whole record of a wave is one contiguous
// block (state: 144 words -> 36 KiB fp32 / 72 KiB fp64 per tile), so a wave
// touches a handful of DRAM pages / TLB entries instead of one per row.
// A record whose length is not a multiple of VW (fp32 u: 6 words) ends in one
// row of 8-byte halves.
//
// The filter state is ONE record of 144 words: x (16), the packed upper triangle of P (120), and
// the IMU sample that produced it (6 + 2 pad; only written by the multirate EKF, whose history
// entries are exactly these records).  One lane owns one filter; x and P live in VGPRs for the
// whole tick and the state is updated in place.  The multirate filter keeps its history next to it (IMU ring, checkpoints,
// anchors: see k_step_mr); the last 8 words of the record are padding.
#pragma once

#include <type_traits>
#include <utility>

#include "ekf_device.hpp"

namespace qle {

// Cache policy of the stores into the IMU ring of the multirate history (0 cached, 2 non-temporal).  Measured on cfg3mr
// (profiles/r03_tuning.md): cached ring stores make the correcting tick's sample loads cheaper and every predict tick dearer
// (10.1 -> 10.7 us); the whole schedule moves by +0.6 %, inside the box-to-box spread: the ring stays streamed.
constexpr int kRingStorePolicy = 2;
constexpr int kBlock = 256;
constexpr int kTile = 64;   // filters per tile = wavefront size

constexpr int kXW = 16;     // state words
constexpr int kPW = 120;    // packed covariance words
constexpr int kSW = kXW + kPW + 8;  // state record: x, P, 8 words of padding (36 / 72 KiB per tile)
constexpr int kUW = 6;      // IMU words
constexpr int kZW = 8;      // tag pose 7 words + mask word
constexpr int kFW = 24;     // per-filter parameter words
constexpr int kHW = 8;      // IMU sample kept in the multirate history: 6 words + 2 pad

// 16-byte quads as native vectors (global_load/store_dwordx4).  NT selects the cache policy of the hot kernels'
// state accesses: 0 = cached loads and stores (the state lives in the 256 MiB Infinity Cache from tick to tick),
// 1 = non-temporal loads, cached stores, 2 = non-temporal loads and stores.  Every state byte is read once and
// written once per launch; which policy sustains the highest rate depends on the state size (chosen per handle,
// see ekf_capi.hip).  The input records are always read non-temporally.
typedef float qle_f4 __attribute__((ext_vector_type(4)));
typedef double qle_d2 __attribute__((ext_vector_type(2)));
typedef float qle_f2 __attribute__((ext_vector_type(2)));
template <typename T> struct Quad;
template <> struct Quad<float> { using type = qle_f4; static constexpr int VW = 4; };
template <> struct Quad<double> { using type = qle_d2; static constexpr int VW = 2; };

// Which accesses of a hot kernel are non-temporal under policy NT (profiles/r01_tuning.md section 5, sustained rates):
//   IMU / tag records (read once, never again): always non-temporal, so the input stream does not displace the state
//   in the Infinity Cache; state and per-filter parameter records: loads non-temporal for NT >= 1, stores for NT >= 2.
// kCached in place of NT: cached loads whatever the record is -- for a kernel that is not the last reader of an IMU or tag record.
constexpr int kCached = -1;
template <int NT, int WT> struct NtLd { static constexpr int value = NT == kCached ? 0 : (WT == kUW || WT == kZW || NT >= 1) ? 2 : 0; };
template <int NT> struct NtSt { static constexpr int value = NT >= 2 ? 2 : 0; };

template <int NT, typename Q>
__device__ __forceinline__ Q ld_quad(const Q* ptr)
{
    if (NT >= 1) return __builtin_nontemporal_load(ptr);
    return *ptr;
}
template <int NT, typename Q>
__device__ __forceinline__ void st_quad(Q* ptr, Q v)
{
    if (NT >= 1) __builtin_nontemporal_store(v, ptr);
    else *ptr = v;
}
__device__ __forceinline__ void unpack_quad(const qle_f4& v, float* r) { r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w; }
__device__ __forceinline__ void unpack_quad(const qle_d2& v, double* r) { r[0] = v.x; r[1] = v.y; }
__device__ __forceinline__ qle_f4 pack_quad(const float* r) { qle_f4 v = {r[0], r[1], r[2], r[3]}; return v; }
__device__ __forceinline__ qle_d2 pack_quad(const double* r) { qle_d2 v = {r[0], r[1]}; return v; }

// Number of filters a record array must be allocated for (whole tiles).
__host__ __device__ inline int64_t padded_filters(int64_t B) { return (B + kTile - 1) / kTile * kTile; }

// Offset (in words) of word w of filter i in an array of WT-word records.
template <typename T>
__host__ __device__ inline int64_t word_off(int w, int64_t i, int WT)
{
    constexpr int VW = 16 / (int)sizeof(T);
    const int64_t tile = i / kTile;
    const int lane = (int)(i % kTile);
    const int nf = WT / VW;
    const int64_t base = tile * WT * kTile;
    if (w < nf * VW) return base + ((int64_t)(w / VW) * kTile + lane) * VW + (w % VW);
    const int rem = WT - nf * VW;
    return base + (int64_t)nf * VW * kTile + lane * rem + (w - nf * VW);
}

// Tile index of filter i, as a wave-uniform (SGPR) value: the 64 lanes of a wave always belong to one
// tile (blocks are multiples of 64 threads), so the tile base can live in scalar registers and the
// loads/stores use the scalar-base + per-lane-offset addressing form instead of 64-bit VALU adds.
// Block index -> position in the batch (XCD-aware).  Workgroups are dispatched round-robin over the 8 XCDs
// (block b runs on XCD b % 8), so with the identity map every XCD touches every 8th 4-tile group of the state.
// Giving each XCD one contiguous eighth of the batch instead measured +3 % on k_predict at 65 536 filters,
// +3 % at 262 144, +1-2 % at 1 M, -1 % at 131 072 (profiles/r01_tuning.md section 4).  The map is a bijection
// on [0, gridDim.x): the first 8*floor(n/8) blocks are transposed, the ragged rest keeps its index.
// The kernel arguments the first loads depend on, all requested at the kernel's entry.  Left alone the compiler fetches an argument
// where it is first needed and waits there: grid size -> (wait) -> block size, batch size -> (wait) -> record pointers -> (wait) ->
// first load, three scalar-cache misses one after the other in front of every launch's first byte; with this they are one.
// (The per-tick kernels no longer fetch these arguments at all: they are among the 14 dwords the dispatch preloads into SGPRs, see
// k_predict; for them this only pins the order, for k_run_resident -- one launch per run -- it is the single fetch.)
template <typename... A> __device__ __forceinline__ void args_early(A... a)
{
    (..., [](auto v) { asm volatile("" ::"s"(v)); }(a));
}
__device__ __forceinline__ int64_t batch_block(unsigned grid)
{
    const unsigned b = blockIdx.x, n8 = grid & ~7u;
    return b < n8 ? (int64_t)((b & 7u) * (n8 >> 3) + (b >> 3)) : (int64_t)b;
}
__device__ __forceinline__ int64_t batch_block() { return batch_block(gridDim.x); }

__device__ __forceinline__ int64_t wave_tile(int64_t i) { return (int64_t)__builtin_amdgcn_readfirstlane((int)(i >> 6)); }

// Load words [W0, W0+W) of filter i's WT-word record.  W0 and W are whole quads,
// except that the load may end with the record's 8-byte tail row (fp32 only).
template <typename T, int WT, int W0, int W, int NT = 0>
__device__ __forceinline__ void load_rec(const T* __restrict__ base, int64_t i, T (&r)[W])
{
    using Q = typename Quad<T>::type;
    constexpr int VW = Quad<T>::VW;
    constexpr int NFT = WT / VW;       // full quad rows in the record
    constexpr int NF = W / VW;         // full quad rows in this load
    constexpr int REM = W % VW;
    static_assert(W0 % VW == 0, "loads start on a quad row");
    static_assert(REM == 0 || (REM == 2 && W0 + W == WT && W0 / VW + NF == NFT), "only the record's own 8-byte tail may be partial");
    const int64_t tile = wave_tile(i);
    const int lane = (int)(i & 63);
    const T* tb = base + tile * (int64_t)(WT * kTile);
#pragma unroll
    for (int k = 0; k < NF; ++k) {
        Q v = ld_quad<NtLd<NT, WT>::value>(reinterpret_cast<const Q*>(tb + ((W0 / VW + k) * kTile + lane) * VW));
        unpack_quad(v, &r[k * VW]);
    }
    if (REM == 2) {
        qle_f2 v = ld_quad<NtLd<NT, WT>::value>(reinterpret_cast<const qle_f2*>(tb + NFT * VW * kTile + lane * 2));
        r[NF * VW] = v.x;
        r[NF * VW + 1] = v.y;
    }
}

template <typename T, int WT, int W0, int W, int NT = 0>
__device__ __forceinline__ void store_rec(T* __restrict__ base, int64_t i, const T (&r)[W])
{
    using Q = typename Quad<T>::type;
    constexpr int VW = Quad<T>::VW;
    constexpr int NF = W / VW;
    static_assert(W % VW == 0 && W0 % VW == 0, "stored ranges are whole quads");
    const int64_t tile = wave_tile(i);
    const int lane = (int)(i & 63);
    T* tb = base + tile * (int64_t)(WT * kTile);
#pragma unroll
    for (int k = 0; k < NF; ++k) st_quad<NtSt<NT>::value>(reinterpret_cast<Q*>(tb + ((W0 / VW + k) * kTile + lane) * VW), pack_quad(&r[k * VW]));
}

// Compact records: est_bias = false (EKF.cpp:92, num_states = 9) without the multirate history.  The bias blocks of such a filter's P are
// identically zero (no process noise, no coupling: EKF.cpp:405-409), so its record keeps only the 45 words of the 9 x 9 pose block, as
// their own row-major triangle in record words 16..60 (3 words of padding): a tick moves 16 + 48 words per direction instead of 136.
// The arithmetic runs on the same 15-state register image (zeros in the bias blocks), which is what the full-record path computes too.
constexpr int kPWc = 48;
__host__ __device__ constexpr int sidx9(int i, int j) { return i * 9 - i * (i - 1) / 2 + (j - i); }   // i <= j < 9
// record word of P(a, b), a <= b, or -1 when a compact record does not hold it
__host__ __device__ constexpr int p_word(int a, int b, bool compact)
{
    return compact ? (b < 9 ? kXW + sidx9(a, b) : -1) : kXW + sidx(a, b);
}
template <typename T, int NT = 0>
__device__ __forceinline__ void load_P_compact(const T* __restrict__ st, int64_t i, T (&P)[kPW])
{
    T t[kPWc];
    load_rec<T, kSW, kXW, kPWc, NT>(st, i, t);
#pragma unroll
    for (int a = 0; a < 15; ++a)
#pragma unroll
        for (int b = a; b < 15; ++b) P[sidx(a, b)] = b < 9 ? t[sidx9(a, b)] : T(0);
}
template <typename T, int NT = 0>
__device__ __forceinline__ void store_P_compact(T* __restrict__ st, int64_t i, const T (&P)[kPW])
{
    T t[kPWc];
#pragma unroll
    for (int k = 45; k < kPWc; ++k) t[k] = T(0);
#pragma unroll
    for (int a = 0; a < 9; ++a)
#pragma unroll
        for (int b = a; b < 9; ++b) t[sidx9(a, b)] = P[sidx(a, b)];
    store_rec<T, kSW, kXW, kPWc, NT>(st, i, t);
}
// the P part of a state record, either layout (wave-uniform choice)
template <typename T, int NT = 0>
__device__ __forceinline__ void load_P_any(const T* __restrict__ st, int64_t i, T (&P)[kPW], bool compact)
{
    if (compact) load_P_compact<T, NT>(st, i, P);
    else load_rec<T, kSW, kXW, kPW, NT>(st, i, P);
}
template <typename T, int NT = 0>
__device__ __forceinline__ void store_P_any(T* __restrict__ st, int64_t i, const T (&P)[kPW], bool compact)
{
    if (compact) store_P_compact<T, NT>(st, i, P);
    else store_rec<T, kSW, kXW, kPW, NT>(st, i, P);
}


// The covariance words a read-only kernel needs, into the 15-state register image.  NEEDS(a, b), a <= b: does the kernel read P(a, b)?
// Only the 16-byte quad rows that hold a needed word are loaded (whole rows: the image takes every word of a loaded row); the other
// slots are zero -- never read, or the bias blocks a compact record does not hold.
using CovNeeds = bool (*)(int, int);
// the pose block P_JJ, J = r0..2, th0..2: the only columns the measurement Jacobian G touches
__host__ __device__ constexpr bool pose_needs(int a, int b) { return (a < 3 || (a >= 6 && a < 9)) && (b < 3 || (b >= 6 && b < 9)); }
// per quad row (VW words) of the packed covariance: is it loaded?  Per slot of the register image: the loaded covariance word it takes,
// or -1 (zero).  A compile-time table: written as a plain loop over the predicate in the kernel, the selection is not folded and runs
// on the scalar unit (some 20 000 SALU instructions per wave).
template <int VW, bool COMPACT, CovNeeds NEEDS>
struct CovSrc {
    static constexpr int kRows = (COMPACT ? kPWc : kPW) / VW;
    bool row[kRows];
    int w[kPW];
    int words;   // words of the covariance the kernel moves per filter (whole quad rows)
    constexpr CovSrc() : row{}, w{}, words(0)
    {
        for (int a = 0; a < 15; ++a)
            for (int b = a; b < 15; ++b) {
                const int rw = p_word(a, b, COMPACT);
                if (rw >= 0 && NEEDS(a, b)) row[(rw - kXW) / VW] = true;
            }
        for (int k = 0; k < kRows; ++k) words += row[k] ? VW : 0;
        for (int a = 0; a < 15; ++a)
            for (int b = a; b < 15; ++b) {
                const int rw = p_word(a, b, COMPACT);
                w[sidx(a, b)] = (rw >= 0 && row[(rw - kXW) / VW]) ? rw - kXW : -1;
            }
    }
};
template <typename T, bool COMPACT, CovNeeds NEEDS, int... K, int... S>
__device__ __forceinline__ void load_P_rows_seq(const T* __restrict__ tb, int lane, T (&P)[kPW], std::integer_sequence<int, K...>,
                                                std::integer_sequence<int, S...>)
{
    using Q = typename Quad<T>::type;
    constexpr int VW = Quad<T>::VW;
    constexpr CovSrc<VW, COMPACT, NEEDS> src{};
    T w[kPW];
    (..., [&] {
        if constexpr (src.row[K]) unpack_quad(*reinterpret_cast<const Q*>(tb + ((kXW / VW + K) * kTile + lane) * VW), &w[K * VW]);
    }());
    (..., [&] {
        if constexpr (src.w[S] >= 0) P[S] = w[src.w[S]];
        else P[S] = T(0);
    }());
}
template <typename T, bool COMPACT, CovNeeds NEEDS>
__device__ __forceinline__ void load_P_rows(const T* __restrict__ st, int64_t i, T (&P)[kPW])
{
    load_P_rows_seq<T, COMPACT, NEEDS>(st + wave_tile(i) * (int64_t)(kSW * kTile), (int)(i & 63), P,
                                       std::make_integer_sequence<int, CovSrc<Quad<T>::VW, COMPACT, NEEDS>::kRows>{},
                                       std::make_integer_sequence<int, kPW>{});
}

template <typename T, bool PFP>
__device__ __forceinline__ void load_noise(const DevParams<T>& p, const T* __restrict__ pfp, int64_t i, Noise<T>& nz)
{
    if (PFP) {
        T f[kFW];
        load_rec<T, kFW, 0, kFW>(pfp, i, f);
#pragma unroll
        for (int k = 0; k < 12; ++k) nz.Q[k] = f[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) { nz.ab_static[k] = f[12 + k]; nz.wb_static[k] = f[15 + k]; }
#pragma unroll
        for (int k = 0; k < 6; ++k) nz.R[k] = f[18 + k];
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) nz.Q[k] = p.Q[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) { nz.ab_static[k] = p.ab_static[k]; nz.wb_static[k] = p.wb_static[k]; }
#pragma unroll
        for (int k = 0; k < 6; ++k) nz.R[k] = p.R[k];
    }
}

// Load / store a range of whole quad rows [Q0, Q1) of the packed P (record words kXW + 4q ..),
// rows taken in DESCENDING order so that the bias rows (end of the row-major triangle) come first.
template <typename T, int Q0, int Q1, int NT = 0>
__device__ __forceinline__ void load_P_quads_desc(const T* __restrict__ st, int64_t i, T (&P)[kPW])
{
    using Q = typename Quad<T>::type;
    constexpr int VW = Quad<T>::VW;
    const int64_t tile = wave_tile(i);
    const int lane = (int)(i & 63);
    const T* tb = st + tile * (int64_t)(kSW * kTile);
#pragma unroll
    for (int k = Q1 - 1; k >= Q0; --k) {
        Q v = ld_quad<NtLd<NT, kSW>::value>(reinterpret_cast<const Q*>(tb + ((kXW / VW + k) * kTile + lane) * VW));
        unpack_quad(v, &P[k * VW]);
    }
}
template <typename T, int Q0, int Q1, int NT = 0>
__device__ __forceinline__ void store_P_quads_desc(T* __restrict__ st, int64_t i, const T (&P)[kPW])
{
    using Q = typename Quad<T>::type;
    constexpr int VW = Quad<T>::VW;
    const int64_t tile = wave_tile(i);
    const int lane = (int)(i & 63);
    T* tb = st + tile * (int64_t)(kSW * kTile);
#pragma unroll
    for (int k = Q1 - 1; k >= Q0; --k) st_quad<NtSt<NT>::value>(reinterpret_cast<Q*>(tb + ((kXW / VW + k) * kTile + lane) * VW), pack_quad(&P[k * VW]));
}

// NT == 3 ("split", states larger than the Infinity Cache): the workgroups selected by `split` keep their tiles
// cached (policy 0), all others stream (policy 2), so a fixed part of the state that fits the cache stays resident
// from tick to tick.  split >= 0: the first `split` dispatched workgroups (spread over all XCDs by batch_block());
// split < 0: interleaved, workgroups with ((blockIdx.x >> 3) & 63) < -split, i.e. -split/64 of every XCD's share.
__device__ __forceinline__ bool cached_workgroup(int32_t split)
{
    return split >= 0 ? blockIdx.x < (unsigned)split : ((blockIdx.x >> 3) & 63u) < (unsigned)(-split);
}

// f(policy) with the cache policy of this workgroup's state accesses as a std::integral_constant: 0 or 2 under NT == 3, else NT itself.
template <int NT, typename F>
__device__ __forceinline__ void with_policy(int32_t split, F&& f)
{
    if constexpr (NT == 3) {
        if (cached_workgroup(split)) f(std::integral_constant<int, 0>{});
        else f(std::integral_constant<int, 2>{});
    } else {
        f(std::integral_constant<int, NT>{});
    }
}

// one value to an output tensor of either dtype (wave-uniform choice; the plain C++ cast of include/qle_devio.h)
template <typename T>
__device__ __forceinline__ void put(void* dst, int64_t k, T v, bool dst_f64)
{
    if (dst_f64) static_cast<double*>(dst)[k] = (double)v;
    else static_cast<float*>(dst)[k] = (float)v;
}

// row `row` of a truth tensor [rows][16] (the diagnostics against a truth: k_nees, ekf_consistency.hpp; k_budget, ekf_budget.hpp) as
// whole 16-byte pieces, cast to the compute dtype by the plain C cast
template <typename T>
__device__ __forceinline__ void load_truth(const void* __restrict__ xt, int64_t row, bool f64, T (&t)[16])
{
    if (f64) {
        const qle_d2* s = reinterpret_cast<const qle_d2*>(static_cast<const double*>(xt) + row * 16);
#pragma unroll
        for (int k = 0; k < 8; ++k) { const qle_d2 v = s[k]; t[2 * k] = (T)v.x; t[2 * k + 1] = (T)v.y; }
    } else {
        const qle_f4* s = reinterpret_cast<const qle_f4*>(static_cast<const float*>(xt) + row * 16);
#pragma unroll
        for (int k = 0; k < 4; ++k) { const qle_f4 v = s[k]; t[4 * k] = (T)v.x; t[4 * k + 1] = (T)v.y; t[4 * k + 2] = (T)v.z; t[4 * k + 3] = (T)v.w; }
    }
}

// (HIP compilers only: a host compiler that reads this header for the layout arithmetic, tests/cpp/devio_index_harness.cpp, has no
// declaration of __syncthreads.)
#if defined(__HIPCC__)
// The deterministic batch summary of the read-only diagnostics, first stage: a wave's sum by xor-shuffles -- the same value in every
// lane, by a fixed tree (k_nees, ekf_consistency.hpp; k_score_tiles, ekf_score.hpp).
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Second stage: one workgroup of kBlock threads adds the per-tile
// partials [tiles][SUMS] in a fixed order.  Thread t adds field t % PITCH (< SUMS) of the tiles t / PITCH, t / PITCH + kBlock / PITCH,
// ... in ascending order; threads 0..SUMS-1 then add the kBlock / PITCH slices in ascending order and hand the field's total to
// out(field, total).
template <int SUMS, int PITCH, typename Out>
__device__ __forceinline__ void reduce_tiles(const double* __restrict__ partials, int64_t tiles, Out&& out)
{
    static_assert(SUMS <= PITCH && kBlock % PITCH == 0, "a slice holds every field");
    __shared__ double part[kBlock];
    const int f = (int)(threadIdx.x % PITCH), s = (int)(threadIdx.x / PITCH);
    double acc = 0.0;
    if (f < SUMS)
        for (int64_t k = s; k < tiles; k += kBlock / PITCH) acc += partials[k * SUMS + f];
    part[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x < SUMS) {
        double tot = 0.0;
        for (int k = 0; k < kBlock / PITCH; ++k) tot += part[k * PITCH + f];
        out(f, tot);
    }
}
#endif  // __HIPCC__

// Dynamic LDS per wave of the fp64 kernels that keep the two top block-rows of P there (ekf_cov_home.hpp); fp32 launches with none.
constexpr size_t kMrLdsPerWave = (size_t)kTopWords * kTile * sizeof(double);

}  // namespace qle
