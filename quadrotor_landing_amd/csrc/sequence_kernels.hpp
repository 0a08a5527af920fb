// sequence_kernels.hpp -- k_sq_pack: the job of k_dv_pack (devio_kernels.hpp) for up to kSeqChunk ticks in ONE launch
// (libqle_sequence.so, include/qle_sequence.h), gfx950.
//
// Geometry: blockIdx.x is the 64-filter tile, blockIdx.y the tick inside the chunk, one wave per workgroup.  A workgroup moves
// 64 x 6 IMU words (and 64 x 7 tag-pose words plus 64 mask bytes when its tick has a tag slot) from the contiguous source tensors
// u_seq [n][B][6], z_seq [m][B][7], mask_seq [m][B] into the tick's records: 13 words and a byte in, 14 words out per filter and tick
// at most.  The transposition goes through the LDS with the odd pitches of devio_kernels.hpp; the record stores are the helpers
// k_dv_pack calls (store_imu_record, mask_word, store_tag_record), so the two kernels write a record the same way by construction.
//
// Where the records of a tick live is not derived from a pitch: the host asks qle_inputs_get_device_view tick by tick and hands the
// pointers over BY VALUE, kSeqChunk x (u, z, zsrc) in one argument struct behind the scalars and source pointers (which stay inside
// the 14 preloaded argument dwords).  No table is copied to the device.
//
// Alignment.  Tick k's slab of u_seq starts k * B * 6 words into the tensor, which for a ragged B is no 16-byte boundary (B = 2391,
// fp32: u slabs of odd ticks are off by 8 bytes, z slabs by 4 or 12; fp64: z slabs of odd k * B by 8).  A tile's span inherits that,
// since 64 x W words are whole 16-byte pieces.  stage_aos_head takes the number of words in front of the span's first 16-byte boundary
// -- wave-uniform, computed from the span's address -- and walks the span as piece 0 = those head words, pieces 1.. = the aligned
// 16-byte pieces behind them.  The head piece and a piece across the end of the valid words move word by word, the others as one
// non-temporal 16-byte load; no word at or beyond nv * W of the span is touched.  The walk's index arithmetic is in plain inline
// functions (host and device) of the kind of piece_word / piece_kind, in sequence_index.hpp: a header without dependencies, so that
// any host compiler can run it (tests/cpp/sequence_harness.cpp, g++ with ASan and UBSan).
#pragma once

#include "devio_kernels.hpp"
#include "sequence_index.hpp"
#include "sequence_plan.hpp"

namespace qsq {

using qdv::kTile;
using qdv::kUW;
using qdv::kZW;
using qdv::kPitchU;
using qdv::kPitchZ;

#if defined(__HIP_DEVICE_COMPILE__) || defined(__HIPCC__)
using qdv::Vec;

// One tick of a chunk: its IMU records, its tag records (nullptr: no tag slot) and the slab of z_seq / mask_seq that fills them (-1: none)
template <typename T>
struct SeqEntry {
    T* u;
    T* z;
    int32_t zsrc;
    int32_t reserved;
};
template <typename T>
struct SeqChunk {
    SeqEntry<T> e[kSeqChunk];
};

// AoS span of a tile (W-word rows of S, nv filters valid) that starts `head` words in front of a 16-byte boundary -> LDS image of L.
// stage_aos (devio_kernels.hpp) for a span that is only element-aligned.  Words at or beyond nv * W are neither read nor written to
// the LDS: the lanes that would read them there (lane >= nv) leave the kernel before they do.
template <typename S, typename L, int W, int PITCH>
__device__ __forceinline__ void stage_aos_head(const S* __restrict__ src, int head, int nv, int lane, L* __restrict__ lds)
{
    using Q = typename Vec<S>::type;
    constexpr int V = Vec<S>::V;
    constexpr int NP = seq_pieces(kTile * W, V);
    const int valid = nv * W;
#pragma unroll
    for (int k = 0; k * kTile < NP; ++k) {
        const int p = k * kTile + lane;
        const int j = seq_piece_word(p, V, head);
        const int len = seq_piece_len(p, V, head);
        const int kind = seq_piece_kind(j, len, V, valid);
        S r[V];
        if (kind == 2) {
            const Q v = __builtin_nontemporal_load(reinterpret_cast<const Q*>(src + j));
            qle::unpack_quad(v, r);
        } else {
#pragma unroll
            for (int e = 0; e < V; ++e) r[e] = (kind == 1 && seq_word_moved(j, e, len, valid)) ? __builtin_nontemporal_load(src + j + e) : S(0);
        }
#pragma unroll
        for (int e = 0; e < V; ++e) {
            if (kind != 0 && seq_word_moved(j, e, len, valid)) {
                const int f = qdv::aos_filter(j + e, W);
                lds[qdv::lds_word(f, j + e - f * W, PITCH)] = (L)r[e];
            }
        }
    }
}

// ------------------------------------------------------------------ kernel
// Slabs k0 .. k0 + gridDim.y - 1 of u_seq (+ the slabs of z_seq / mask_seq the entries name) of S -> the records of T of the chunk's
// ticks.  mask_seq == nullptr: all set.  The grid is (tiles, entries in use): every entry the kernel reads is filled.
template <typename T, typename S>
__global__ void __launch_bounds__(kTile) k_sq_pack(const S* __restrict__ u_seq, const S* __restrict__ z_seq, const uint8_t* __restrict__ mask_seq,
                                                  int64_t B, int64_t k0, SeqChunk<T> chunk)
{
    __shared__ T lu[kTile * kPitchU];
    __shared__ T lz[kTile * kPitchZ];
    const int lane = (int)threadIdx.x;
    const int64_t tile = blockIdx.x;
    const int y = (int)blockIdx.y;
    const int nv = qdv::tile_valid(B, tile);
    T* const ud = chunk.e[y].u;
    T* const zd = chunk.e[y].z;
    const int64_t zsrc = chunk.e[y].zsrc;
    const bool tag = zd != nullptr && zsrc >= 0;
    const S* us = u_seq + ((k0 + y) * B + tile * kTile) * kUW;
    stage_aos_head<S, T, kUW, kPitchU>(us, seq_head_words((uint64_t)us, (int)sizeof(S)), nv, lane, lu);
    if (tag) {
        const S* zs = z_seq + (zsrc * B + tile * kTile) * 7;
        stage_aos_head<S, T, 7, kPitchZ>(zs, seq_head_words((uint64_t)zs, (int)sizeof(S)), nv, lane, lz);
    }
    __syncthreads();
    if (lane >= nv) return;
    T r[8];
#pragma unroll
    for (int w = 0; w < kUW; ++w) r[w] = lu[qdv::lds_word(lane, w, kPitchU)];
    qdv::store_imu_record<T>(ud + qdv::tile_base(tile, kUW), lane, r);
    if (!tag) return;
#pragma unroll
    for (int w = 0; w < 7; ++w) r[w] = lz[qdv::lds_word(lane, w, kPitchZ)];
    r[7] = qdv::mask_word<T>(mask_seq ? mask_seq + zsrc * B : nullptr, tile * kTile + lane);
    qdv::store_tag_record<T>(zd + qdv::tile_base(tile, kZW), lane, r);
}
#endif  // device helpers and kernel

}  // namespace qsq
