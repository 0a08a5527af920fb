// devio_kernels.hpp -- the device-tensor boundary (libqle_devio.so, include/qle_devio.h): AoS tensors in GPU memory <-> the wave-tile
// records the tick kernels read (ekf_layout.hpp), both dtypes on both sides, gfx950.
//
// One wave owns one 64-filter tile, one workgroup is one wave.  The AoS side of a tile is ONE contiguous span (64 x W words) and moves
// as 16-byte pieces, consecutive lanes on consecutive pieces; the tile side moves as the dwordx4 rows of the tick kernels, lane l on
// quad l of a row.  In between the words are transposed through the LDS: a filter's words sit at f * pitch + w with an ODD pitch, so
// that the 64 lanes reading or writing "word w of my filter" fall on distinct banks (fp64: ds_*_b64 in half-waves, 2 * odd * l mod 64
// takes 32 distinct even values), while the pieces touch consecutive LDS words.  The kernels do no arithmetic: a value is converted by
// the plain C++ cast, exactly as the host path converts ((T)double on the way in, (double)T on the way out), so that the results are
// equal bit for bit.  The only sum is the report's bias + static bias, formed in fp64 from the compute-dtype words as k_report_off does.
//
// Ragged batches: the records are allocated for whole tiles (padded_filters), so the tile side may read every lane; the AoS side is
// never touched at or beyond word B * W: a piece that straddles that end moves word by word, a piece beyond it does not move.
//
// Cache policy: the input tensors are read non-temporally (read once), the tick records are written with plain stores (the tick reads
// them next), the state is read with plain cached loads -- the policy that leaves the handle's choice for its state alone (DESIGN.md
// section 3).
//
// The index arithmetic is in plain inline functions at the top (host and device), so that tests/cpp/devio_index_harness.cpp can run
// the same code on the CPU for every (word, filter) of a ragged batch.
#pragma once

#include <type_traits>
#include <utility>

#include "ekf_layout.hpp"

namespace qdv {

using qle::kTile;
using qle::kXW;
using qle::kPW;
using qle::kPWc;
using qle::kSW;
using qle::kUW;
using qle::kZW;
using qle::kFW;

// LDS pitches (words per filter), all odd
constexpr int kPitchU = 7;     // 6 IMU words
constexpr int kPitchZ = 7;     // 7 tag-pose words (the mask word is made in registers)
constexpr int kPitchX = 17;    // 16 state words
constexpr int kPitchP = 121;   // 120 packed covariance words (compact records: 48)
constexpr int kPitchR = 37;    // report: 16 state words + the 21 words of the 6 x 6 pose covariance

// ------------------------------------------------------------------ index arithmetic (host and device)
// Offset, in words from the start of its tile, of word w of lane's WT-word record: off(w, i) of DESIGN.md section 3 without the tile
// base.  The VW words of a quad row are contiguous, which is what lets a lane move them as one 16-byte access.
template <typename T>
__host__ __device__ inline int tile_word(int w, int lane, int WT) { return (int)qle::word_off<T>(w, lane, WT); }
__host__ __device__ inline int64_t tile_base(int64_t tile, int WT) { return tile * WT * kTile; }
// filters of tile `tile` that exist in a batch of B
__host__ __device__ inline int tile_valid(int64_t B, int64_t tile)
{
    const int64_t left = B - tile * kTile;
    return left >= kTile ? kTile : (left > 0 ? (int)left : 0);
}
// The AoS span of a tile in pieces of V words (16 bytes): piece k of a lane starts at this word of the span ...
__host__ __device__ inline int piece_word(int lane, int k, int V) { return (k * kTile + lane) * V; }
// ... and is 2 = whole inside the valid words [0, valid), 1 = across their end (moved word by word), 0 = outside (not moved)
__host__ __device__ inline int piece_kind(int j, int V, int valid) { return j + V <= valid ? 2 : (j < valid ? 1 : 0); }
// AoS word j of a tile's span of W-word rows -> filter of the tile and word of its row; and where that word sits in the LDS
__host__ __device__ inline int aos_filter(int j, int W) { return j / W; }
__host__ __device__ inline int lds_word(int f, int w, int pitch) { return f * pitch + w; }
// Word r = a * n + b of the full n x n covariance -> the record word that holds P(a, b), or -1 where the record holds none (zero)
__host__ __device__ inline int cov_record_word(int r, int n, bool compact)
{
    const int a = r / n, b = r - a * n;
    return a <= b ? qle::p_word(a, b, compact) : qle::p_word(b, a, compact);
}
// The report (NODE.cpp:192-220): rows / columns {0-2, 6-8} of P, kept in the LDS as the 21 words of their upper triangle
__host__ __device__ constexpr int report_sel(int k) { return k < 3 ? k : k + 3; }
__host__ __device__ constexpr int tri6(int a, int b) { return a <= b ? a * 6 - a * (a - 1) / 2 + (b - a) : b * 6 - b * (b - 1) / 2 + (a - b); }
// slot of the report's LDS image that record word rw feeds: 0..15 the state words, 16..36 the pose covariance, -1 none
__host__ __device__ constexpr int report_slot(int rw, bool compact)
{
    if (rw < kXW) return rw;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b)
            if (qle::p_word(report_sel(a), report_sel(b), compact) == rw) return kXW + tri6(a, b);
    return -1;
}
__host__ __device__ constexpr int report_pose_slot(int w) { return w < 3 ? w : w + 3; }   // r (x 0-2), q (x 6-9)
__host__ __device__ constexpr int report_vel_slot(int w) { return 3 + w; }
__host__ __device__ constexpr int report_bias_slot(int w) { return 10 + w; }              // ab (x 10-12), wb (x 13-15)
__host__ __device__ inline int report_cov_slot(int w) { return kXW + tri6(w / 6, w % 6); }

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
// ------------------------------------------------------------------ device helpers
template <typename A, typename B2> struct Narrower { using type = std::conditional_t<(sizeof(A) <= sizeof(B2)), A, B2>; };
template <typename T> struct Vec { using type = typename qle::Quad<T>::type; static constexpr int V = qle::Quad<T>::VW; };

template <typename F, int... K>
__device__ __forceinline__ void static_for(std::integer_sequence<int, K...>, F&& f) { (f(std::integral_constant<int, K>{}), ...); }

// AoS span of a tile (W-word rows of S, nv filters valid) -> LDS image of L, non-temporal 16-byte pieces
template <typename S, typename L, int W, int PITCH>
__device__ __forceinline__ void stage_aos(const S* __restrict__ src, int nv, int lane, L* __restrict__ lds)
{
    using Q = typename Vec<S>::type;
    constexpr int V = Vec<S>::V;
    const int valid = nv * W;
#pragma unroll
    for (int k = 0; k * kTile * V < kTile * W; ++k) {
        const int j = piece_word(lane, k, V);
        if (j >= kTile * W) break;
        const int kind = piece_kind(j, V, valid);
        S r[V];
        if (kind == 2) {
            const Q v = __builtin_nontemporal_load(reinterpret_cast<const Q*>(src + j));
            qle::unpack_quad(v, r);
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) r[e] = (kind == 1 && j + e < valid) ? __builtin_nontemporal_load(src + j + e) : S(0);
        }
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const int f = aos_filter(j + e, W);
            lds[lds_word(f, j + e - f * W, PITCH)] = (L)r[e];
        }
    }
}

// val(f, w) for every word of a tile's AoS span of W-word rows of D -> global memory, 16-byte pieces, nothing at or beyond nv * W
template <typename D, int W, typename F>
__device__ __forceinline__ void emit_aos(D* __restrict__ dst, int nv, int lane, F&& val)
{
    using Q = typename Vec<D>::type;
    constexpr int V = Vec<D>::V;
    const int valid = nv * W;
    for (int k = 0; k * kTile * V < kTile * W; ++k) {
        const int j = piece_word(lane, k, V);
        if (j >= kTile * W) break;
        const int kind = piece_kind(j, V, valid);
        if (kind == 0) continue;
        D r[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const int f = aos_filter(j + e, W);
            r[e] = j + e < valid ? val(f, j + e - f * W) : D(0);
        }
        if (kind == 2) {
            *reinterpret_cast<Q*>(dst + j) = qle::pack_quad(r);
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e)
                if (j + e < valid) dst[j + e] = r[e];
        }
    }
}

// quad row k of a lane's WT-word record (cached load), as VW words
template <typename T, int WT>
__device__ __forceinline__ void load_row(const T* __restrict__ tb, int lane, int k, T* r)
{
    using Q = typename Vec<T>::type;
    qle::unpack_quad(*reinterpret_cast<const Q*>(tb + tile_word<T>(k * Vec<T>::V, lane, WT)), r);
}
template <typename T, int WT>
__device__ __forceinline__ void store_row(T* __restrict__ tb, int lane, int k, const T* r)
{
    using Q = typename Vec<T>::type;
    *reinterpret_cast<Q*>(tb + tile_word<T>(k * Vec<T>::V, lane, WT)) = qle::pack_quad(r);
}

// The record stores of a pack, one definition for k_dv_pack and the many-tick pack of sequence_kernels.hpp.
// A lane's six IMU words -> its IMU record in the tile at tu: the quad rows, and for fp32 the record's 8-byte tail row.
template <typename T>
__device__ __forceinline__ void store_imu_record(T* __restrict__ tu, int lane, const T* r)
{
    constexpr int V = Vec<T>::V;
#pragma unroll
    for (int k = 0; k < kUW / V; ++k) store_row<T, kUW>(tu, lane, k, &r[k * V]);
    if constexpr (kUW % V != 0) {   // fp32: the record's 8-byte tail row
        qle::qle_f2 t = {(float)r[4], (float)r[5]};
        *reinterpret_cast<qle::qle_f2*>(reinterpret_cast<float*>(tu) + tile_word<float>(4, lane, kUW)) = t;
    }
}
// The mask word of filter i, made in registers: mask == nullptr means all set (k_pack_z_off's meaning).
template <typename T>
__device__ __forceinline__ T mask_word(const uint8_t* __restrict__ mask, int64_t i) { return (mask == nullptr || mask[i]) ? T(1) : T(0); }
// A lane's eight tag words (z 7 + mask word) -> its tag record in the tile at tz.
template <typename T>
__device__ __forceinline__ void store_tag_record(T* __restrict__ tz, int lane, const T* r)
{
    constexpr int V = Vec<T>::V;
#pragma unroll
    for (int k = 0; k < kZW / V; ++k) store_row<T, kZW>(tz, lane, k, &r[k * V]);
}

// ------------------------------------------------------------------ kernels
// u [B][6] (+ z [B][7], mask [B]) of S -> the tick's IMU record (+ tag record) of T.  zd == nullptr: no tag record; z == nullptr: identity
// pose; mask == nullptr: all set (k_pack_z_off's meaning).
template <typename T, typename S>
__global__ void __launch_bounds__(kTile) k_dv_pack(const S* __restrict__ u, const S* __restrict__ z, const uint8_t* __restrict__ mask,
                                                  T* __restrict__ ud, T* __restrict__ zd, int64_t B)
{
    __shared__ T lu[kTile * kPitchU];
    __shared__ T lz[kTile * kPitchZ];
    const int lane = (int)threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int nv = tile_valid(B, tile);
    stage_aos<S, T, kUW, kPitchU>(u + tile * (kTile * kUW), nv, lane, lu);
    if (zd && z) stage_aos<S, T, 7, kPitchZ>(z + tile * (kTile * 7), nv, lane, lz);
    __syncthreads();
    if (lane >= nv) return;
    T r[8];
#pragma unroll
    for (int w = 0; w < kUW; ++w) r[w] = lu[lds_word(lane, w, kPitchU)];
    store_imu_record<T>(ud + tile_base(tile, kUW), lane, r);
    if (!zd) return;
#pragma unroll
    for (int w = 0; w < 7; ++w) r[w] = z ? lz[lds_word(lane, w, kPitchZ)] : (w == 6 ? T(1) : T(0));
    r[7] = mask_word<T>(mask, tile * kTile + lane);
    store_tag_record<T>(zd + tile_base(tile, kZW), lane, r);
}

// state records of T -> x [B][16], P [B][N][N] of D (either may be null).  N = 15 or 9; compact only with N = 9.
template <typename T, typename D, int N>
__global__ void __launch_bounds__(kTile) k_dv_state(const T* __restrict__ st, D* __restrict__ x, D* __restrict__ P, int64_t B, int compact)
{
    using L = typename Narrower<T, D>::type;
    __shared__ L lds[kTile * kPitchP];
    __shared__ short tab[N * N];
    constexpr int V = Vec<T>::V;
    const int lane = (int)threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int nv = tile_valid(B, tile);
    const T* tb = st + tile_base(tile, kSW);
    if (x) {
#pragma unroll
        for (int k = 0; k < kXW / V; ++k) {
            T r[V];
            load_row<T, kSW>(tb, lane, k, r);
#pragma unroll
            for (int e = 0; e < V; ++e) lds[lds_word(lane, k * V + e, kPitchX)] = (L)r[e];
        }
        __syncthreads();
        emit_aos<D, kXW>(x + tile * (kTile * kXW), nv, lane, [&](int f, int w) { return (D)lds[lds_word(f, w, kPitchX)]; });
        __syncthreads();
    }
    if (!P) return;
    for (int r = lane; r < N * N; r += kTile) {
        const int rw = cov_record_word(r, N, compact != 0);
        tab[r] = (short)(rw < 0 ? -1 : rw - kXW);
    }
    auto stage = [&](auto nrows) {
#pragma unroll 6
        for (int k = 0; k < decltype(nrows)::value; ++k) {
            T r[V];
            load_row<T, kSW>(tb, lane, kXW / V + k, r);
#pragma unroll
            for (int e = 0; e < V; ++e) lds[lds_word(lane, k * V + e, kPitchP)] = (L)r[e];
        }
    };
    if (N == 9 && compact) stage(std::integral_constant<int, kPWc / V>{});
    else stage(std::integral_constant<int, kPW / V>{});
    __syncthreads();
    emit_aos<D, N * N>(P + tile * (kTile * N * N), nv, lane, [&](int f, int r) {
        const int w = tab[r];
        return w >= 0 ? (D)lds[lds_word(f, w, kPitchP)] : D(0);
    });
}

struct StaticBias { double v[6]; };   // ab_static, wb_static as the compute dtype holds them

// What the node publishes (NODE.cpp:192-220) of D: pose [B][7], pose_cov [B][36], vel [B][3], bias [B][6]; any may be null.
template <typename T, typename D>
__global__ void __launch_bounds__(kTile) k_dv_report(const T* __restrict__ st, const T* __restrict__ pfp, D* __restrict__ pose,
                                                    D* __restrict__ cov, D* __restrict__ vel, D* __restrict__ bias, int64_t B, int compact,
                                                    StaticBias sb)
{
    __shared__ T lds[kTile * kPitchR];
    constexpr int V = Vec<T>::V;
    const int lane = (int)threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int nv = tile_valid(B, tile);
    const T* tb = st + tile_base(tile, kSW);
    auto stage = [&](auto cflag) {
        constexpr bool C = decltype(cflag)::value;
        constexpr int rows = (kXW + (C ? kPWc : kPW)) / V;
        static_for(std::make_integer_sequence<int, rows>{}, [&](auto kc) {
            constexpr int k = decltype(kc)::value;
            constexpr bool any = [] { for (int e = 0; e < V; ++e) if (report_slot(k * V + e, C) >= 0) return true; return false; }();
            if constexpr (any) {
                T r[V];
                load_row<T, kSW>(tb, lane, k, r);
                static_for(std::make_integer_sequence<int, V>{}, [&](auto ec) {
                    constexpr int s = report_slot(k * V + decltype(ec)::value, C);
                    if constexpr (s >= 0) lds[lds_word(lane, s, kPitchR)] = r[decltype(ec)::value];
                });
            }
        });
    };
    if (compact) stage(std::true_type{});
    else stage(std::false_type{});
    __syncthreads();
    if (pose) emit_aos<D, 7>(pose + tile * (kTile * 7), nv, lane, [&](int f, int w) { return (D)lds[lds_word(f, report_pose_slot(w), kPitchR)]; });
    if (cov) emit_aos<D, 36>(cov + tile * (kTile * 36), nv, lane, [&](int f, int w) { return (D)lds[lds_word(f, report_cov_slot(w), kPitchR)]; });
    if (vel) emit_aos<D, 3>(vel + tile * (kTile * 3), nv, lane, [&](int f, int w) { return (D)lds[lds_word(f, report_vel_slot(w), kPitchR)]; });
    if (bias) emit_aos<D, 6>(bias + tile * (kTile * 6), nv, lane, [&](int f, int w) {
        // ab_nom + ab_static, wb_nom + wb_static (NODE.cpp:215-220), summed in fp64 as the host path's report kernel does
        const double s = pfp ? (double)pfp[tile_base(tile, kFW) + tile_word<T>(12 + w, f, kFW)] : sb.v[w];
        return (D)((double)lds[lds_word(f, report_bias_slot(w), kPitchR)] + s);
    });
}
#endif  // device helpers and kernels

}  // namespace qdv
