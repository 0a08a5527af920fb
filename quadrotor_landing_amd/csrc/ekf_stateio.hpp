// ekf_stateio.hpp -- device state I/O (libqle_stateio.so, include/qle_stateio.h): AoS tensors in GPU memory -> state records, and state
// records -> state records of another view, gfx950.  The kernels compute nothing but the symmetric part of a covariance; everything
// else is moved or cast.
//
// k_si_copy: one lane per DESTINATION filter, one wave per 64-filter tile.  A record is record_words words = ROWS 16-byte quads (fp32
// 34 / 16 compact, fp64 68 / 32), and a quad is moved as it is -- the kernel does not know the dtype beyond the row count, which is
// what makes the copy bitwise.  Lane l of a wave stores quad l of a row (1 KiB contiguous per row, the tick kernels' access); it loads
// quad (index % 64) of the same row of tile index / 64, so with the identity index the loads are the same 1 KiB rows and with a
// permutation each is a 16-byte access of its own.  The loads of up to kCopyBatch rows are requested before the first of their stores
// (136 registers); an fp64 record goes in two such halves, which keeps every instantiation out of scratch.  Plain cached loads and
// stores: a restore's destination is read by the next tick, and for a snapshot non-temporal stores, with or without non-temporal
// loads, measured within 2 % of the plain ones at 2 097 152 filters and ahead of them nowhere consistently (profiles/stateio.md).
//
// k_si_pack: the inverse of k_dv_state (devio_kernels.hpp), one wave per tile.  The AoS span of a tile moves as 16-byte pieces,
// consecutive lanes on consecutive pieces, into the LDS; each lane then reads the words of its own filter (x: pitch 17; P: pitch n * n,
// odd for n = 15 and 9, so the span lands in the LDS as it is), forms its record rows and stores them as quads.  A tile's fp64
// 15 x 15 covariances (115 KiB) go through the LDS in two passes of 32 filters.
//
// The index arithmetic and the packing arithmetic are plain inline functions at the top (host and device), so that
// tests/cpp/stateio_harness.cpp runs the same code on the CPU for every word of a ragged batch.
#pragma once

#include "devio_kernels.hpp"

namespace qsi {

using qdv::kTile;
using qdv::kXW;
using qdv::kPW;
using qdv::kPWc;
using qdv::kSW;
using qdv::kFW;
using qdv::kPitchX;

// ------------------------------------------------------------------ index and packing arithmetic (host and device)
constexpr int kQuadBytes = 16;
constexpr int kCopyBatch = 34;   // quad rows whose loads are in flight before the first store: one fp32 record, half an fp64 record

// 16-byte quads of `words` words of `wsz` bytes, per filter
__host__ __device__ constexpr int quads_of(int words, int wsz) { return words * wsz / kQuadBytes; }
// Quad index, in an array of records of `recq` quads per filter, of quad row k of filter i: off(k * VW, i) / VW of the layout.
__host__ __device__ inline int64_t quad_at(int64_t i, int k, int recq) { return (i / kTile) * ((int64_t)recq * kTile) + (int64_t)k * kTile + i % kTile; }

// Which source filter destination filter i takes, or -1 when it is not written: beyond the batch, masked out, or an index outside
// the source batch.
__host__ __device__ inline int64_t copy_source(int64_t i, int64_t dst_batch, const int32_t* index, const uint8_t* mask, int64_t src_batch)
{
    if (i >= dst_batch) return -1;
    if (mask != nullptr && mask[i] == 0) return -1;
    const int64_t j = index != nullptr ? (int64_t)index[i] : i;
    return (j >= 0 && j < src_batch) ? j : -1;
}

// (a, b), a <= b, of the covariance word at record word kXW + idx, or (-1, -1) for a padding word (compact: idx 45..47).
struct CovAB { int a, b; };
__host__ __device__ constexpr CovAB cov_ab(int idx, bool compact)
{
    for (int a = 0; a < 15; ++a)
        for (int b = a; b < 15; ++b)
            if (qle::p_word(a, b, compact) == kXW + idx) return CovAB{a, b};
    return CovAB{-1, -1};
}
// covariance words a pack writes per filter: whole quad rows of either dtype
__host__ __device__ constexpr int cov_words(bool compact) { return compact ? kPWc : kPW; }

// A state word and a covariance word as qle_set_state forms them from the host's doubles: (T)double, and (T) of the symmetric part
// formed in double (k_pack_off, k_pack_P_off); 0 where the record has a word for a state the n-state filter does not estimate.
template <typename T, typename S>
__host__ __device__ inline T pack_x_word(S v) { return (T)(double)v; }
template <typename T, typename S>
__host__ __device__ inline T pack_cov_word(const S* m, int a, int b, int n)
{
    if (a < 0 || a >= n || b >= n) return T(0);
    const double v = 0.5 * ((double)m[a * n + b] + (double)m[b * n + a]);
    return (T)v;
}

// filters of a tile whose n x n covariances of S go through the LDS in one pass (<= 60 KiB)
template <typename S>
__host__ __device__ constexpr int pass_filters(int n) { return (int64_t)kTile * n * n * (int64_t)sizeof(S) <= 60 * 1024 ? kTile : kTile / 2; }

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
// ------------------------------------------------------------------ kernels
typedef unsigned int qsi_u4 __attribute__((ext_vector_type(4)));

// rows [K0, K0 + N) of a record: every load, then every store
template <int K0, int N>
__device__ __forceinline__ void copy_rows(const qsi_u4* __restrict__ s, qsi_u4* __restrict__ d)
{
    qsi_u4 r[N];
#pragma unroll
    for (int k = 0; k < N; ++k) r[k] = s[(K0 + k) * kTile];
    asm volatile("" ::: "memory");   // left alone the scheduler interleaves the stores with the loads, some ten rows in flight
#pragma unroll
    for (int k = 0; k < N; ++k) d[(K0 + k) * kTile] = r[k];
}
template <int ROWS>
__device__ __forceinline__ void copy_record(const qsi_u4* __restrict__ s, qsi_u4* __restrict__ d)
{
    constexpr int H = ROWS <= kCopyBatch ? ROWS : ROWS / 2;
    static_assert(H <= kCopyBatch && (H == ROWS || 2 * H == ROWS), "a record goes in one batch of loads or in two halves");
    copy_rows<0, H>(s, d);
    if constexpr (H != ROWS) copy_rows<H, ROWS - H>(s, d);
}

// dst filter i <- src filter index[i] (nullptr: i), ROWS quads of a record of RECQ quads; the parameter record (PARQ quads) with it
// when both pointers are given.  written: nullptr, or one byte per destination filter.
template <int ROWS, int RECQ, int PARQ>
__global__ void __launch_bounds__(kTile) k_si_copy(const qsi_u4* __restrict__ src, qsi_u4* __restrict__ dst, const int32_t* __restrict__ index,
                                                  const uint8_t* __restrict__ mask, int64_t src_batch, int64_t dst_batch,
                                                  const qsi_u4* __restrict__ src_par, qsi_u4* __restrict__ dst_par, uint8_t* __restrict__ written)
{
    const int64_t i = (int64_t)blockIdx.x * kTile + threadIdx.x;
    const int64_t j = copy_source(i, dst_batch, index, mask, src_batch);
    if (i < dst_batch && written) written[i] = j >= 0 ? 1 : 0;
    if (j < 0) return;
    copy_record<ROWS>(src + quad_at(j, 0, RECQ), dst + quad_at(i, 0, RECQ));
    if (src_par && dst_par) copy_record<PARQ>(src_par + quad_at(j, 0, PARQ), dst_par + quad_at(i, 0, PARQ));
}

// `span` words of S at src, of which the first `valid` exist -> lds[0, span), 16-byte non-temporal pieces; a piece across the end of
// the valid words moves word by word, one beyond it does not move (stage_aos of devio_kernels.hpp with the identity map into the LDS).
template <typename S>
__device__ __forceinline__ void stage_span(const S* __restrict__ src, int valid, int span, int lane, S* __restrict__ lds)
{
    using Q = typename qdv::Vec<S>::type;
    constexpr int V = qdv::Vec<S>::V;
    for (int k = 0; qdv::piece_word(0, k, V) < span; ++k) {
        const int j = qdv::piece_word(lane, k, V);
        if (j >= span) break;
        const int kind = qdv::piece_kind(j, V, valid);
        if (kind == 2) {
            const Q v = __builtin_nontemporal_load(reinterpret_cast<const Q*>(src + j));
            qle::unpack_quad(v, lds + j);
        } else if (kind == 1) {
#pragma unroll
            for (int e = 0; e < V; ++e)
                if (j + e < valid) lds[j + e] = __builtin_nontemporal_load(src + j + e);
        }
    }
}

// x [B][16], P [B][N][N] of S (either may be null) -> the state records of T.  N = 15 or 9; COMPACT only with N = 9.
template <typename T, typename S, int N, bool COMPACT>
__global__ void __launch_bounds__(kTile) k_si_pack(const S* __restrict__ x, const S* __restrict__ P, const uint8_t* __restrict__ mask,
                                                  T* __restrict__ st, int64_t B)
{
    static_assert(N == 15 || (N == 9), "15 or 9 states");
    static_assert(!COMPACT || N == 9, "compact records hold the 9 x 9 pose block");
    constexpr int NN = N * N;
    constexpr int FPB = pass_filters<S>(N);
    constexpr int V = qdv::Vec<T>::V;
    constexpr int kLds = FPB * NN > kTile * kPitchX ? FPB * NN : kTile * kPitchX;
    static_assert((FPB * NN * sizeof(S)) % kQuadBytes == 0, "a pass starts on a 16-byte piece");
    __shared__ S lds[kLds];
    const int lane = (int)threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int nv = qdv::tile_valid(B, tile);
    const bool on = lane < nv && (mask == nullptr || mask[tile * kTile + lane] != 0);
    T* tb = st + qdv::tile_base(tile, kSW);
    if (x) {
        qdv::stage_aos<S, S, kXW, kPitchX>(x + tile * (kTile * kXW), nv, lane, lds);
        __syncthreads();
        if (on) {
#pragma unroll
            for (int k = 0; k < kXW / V; ++k) {
                T r[V];
#pragma unroll
                for (int e = 0; e < V; ++e) r[e] = pack_x_word<T, S>(lds[qdv::lds_word(lane, k * V + e, kPitchX)]);
                qdv::store_row<T, kSW>(tb, lane, k, r);
            }
        }
        __syncthreads();
    }
    if (!P) return;
    for (int f0 = 0; f0 < nv; f0 += FPB) {   // nv is the same in every lane: the barriers below are reached by all or none
        const int nvp = nv - f0 < FPB ? nv - f0 : FPB;
        stage_span<S>(P + (tile * kTile + f0) * NN, nvp * NN, FPB * NN, lane, lds);
        __syncthreads();
        if (on && lane >= f0 && lane < f0 + FPB) {
            const S* m = lds + (lane - f0) * NN;
            qdv::static_for(std::make_integer_sequence<int, cov_words(COMPACT) / V>{}, [&](auto kc) {
                constexpr int k = decltype(kc)::value;
                T r[V];
                qdv::static_for(std::make_integer_sequence<int, V>{}, [&](auto ec) {
                    constexpr int e = decltype(ec)::value;
                    constexpr CovAB ab = cov_ab(k * V + e, COMPACT);
                    r[e] = pack_cov_word<T, S>(m, ab.a, ab.b, N);
                });
                qdv::store_row<T, kSW>(tb, lane, kXW / V + k, r);
            });
        }
        __syncthreads();
    }
}
#endif  // kernels

}  // namespace qsi
