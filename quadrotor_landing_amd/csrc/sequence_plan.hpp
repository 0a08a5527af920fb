// sequence_plan.hpp -- the host-side plan of a many-tick pack (libqle_sequence.so, include/qle_sequence.h).  Host code only, no HIP:
// tests/cpp/sequence_harness.cpp runs it on the CPU.
//
// qsq_pack fills ticks [t0, t0 + n) of a sequence from u_seq [n][B][6], z_seq [m][B][7] and mask_seq [m][B], m being the number of
// those ticks that have a tag slot, in tick order.  One launch of k_sq_pack (sequence_kernels.hpp) packs a chunk of at most kSeqChunk
// consecutive ticks: entry y of chunk c is tick t0 + c * kSeqChunk + y, whose IMU slab is slab k = c * kSeqChunk + y of u_seq and
// whose tag slab is slab zsrc of z_seq / mask_seq, or none (zsrc = -1).
#pragma once

#include <cstdint>
#include <vector>

namespace qsq {

constexpr int kSeqChunk = 32;   // ticks one launch packs: blockIdx.y, and the entries of the argument struct

struct PlanEntry {
    int64_t tick;    // tick of the sequence this entry fills
    int32_t zsrc;    // index of its tag pose in z_seq / mask_seq, -1 = the tick has no tag slot
};
struct PlanChunk {
    int64_t k0;      // index in u_seq of entry 0's slab
    int32_t count;   // entries in use, 1 .. kSeqChunk
    PlanEntry e[kSeqChunk];
};

inline int64_t plan_chunks(int64_t n) { return n <= 0 ? 0 : (n + kSeqChunk - 1) / kSeqChunk; }

// has_tag(t): does tick t of the sequence have a tag slot.  *m receives the number of tag slots in the range.
template <typename HasTag>
inline std::vector<PlanChunk> sequence_plan(int64_t t0, int64_t n, HasTag&& has_tag, int64_t* m)
{
    std::vector<PlanChunk> plan((size_t)plan_chunks(n));
    int64_t slots = 0;
    for (int64_t k = 0; k < n; ++k) {
        PlanChunk& c = plan[(size_t)(k / kSeqChunk)];
        const int y = (int)(k % kSeqChunk);
        if (y == 0) { c.k0 = k; c.count = 0; }
        c.e[y].tick = t0 + k;
        c.e[y].zsrc = has_tag(t0 + k) ? (int32_t)slots++ : -1;
        c.count = y + 1;
    }
    if (m) *m = slots;
    return plan;
}

}  // namespace qsq
