// sequence_index.hpp -- the index arithmetic of stage_aos_head (sequence_kernels.hpp): how a tile's AoS span that is only
// element-aligned is walked in pieces.  Plain inline functions for host and device, the counterparts of piece_word / piece_kind of
// devio_kernels.hpp for a span with `head` words in front of its first 16-byte boundary.  The header depends on nothing, so that a
// host compiler without the HIP headers can run the very code the kernel runs (tests/cpp/sequence_harness.cpp).
#pragma once

#include <cstdint>

#if !defined(__HIPCC__) && !defined(__host__)   // a host compiler without the HIP headers: the decorators mean nothing
#define __host__
#define __device__
#endif

namespace qsq {

// words of elem_bytes in front of the first 16-byte boundary at or behind addr (addr is a multiple of elem_bytes)
__host__ __device__ inline int seq_head_words(uint64_t addr, int elem_bytes) { return (int)(((16u - (unsigned)(addr & 15u)) & 15u) / (unsigned)elem_bytes); }
// pieces a span of `words` words is walked in: the head piece and the 16-byte pieces (a span is whole pieces: 64 x W words)
__host__ __device__ constexpr int seq_pieces(int words, int V) { return words / V + 1; }
// piece p of a span whose first 16-byte boundary is `head` words in (0 <= head < V) starts at this word of the span ...
__host__ __device__ inline int seq_piece_word(int p, int V, int head) { return p == 0 ? 0 : head + (p - 1) * V; }
// ... and has this many words: piece 0 is the head itself (empty when the span is aligned)
__host__ __device__ inline int seq_piece_len(int p, int V, int head) { return p == 0 ? head : V; }
// 2 = a whole aligned piece inside the valid words [0, valid), 1 = the head piece or a piece across their end (moved word by word:
// word j + e for e < len and j + e < valid), 0 = nothing to move
__host__ __device__ inline int seq_piece_kind(int j, int len, int V, int valid) { return (len == V && j + V <= valid) ? 2 : ((len > 0 && j < valid) ? 1 : 0); }
// is word e of such a piece moved
__host__ __device__ inline bool seq_word_moved(int j, int e, int len, int valid) { return e < len && j + e < valid; }

}  // namespace qsq
