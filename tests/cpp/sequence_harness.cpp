// sequence_harness.cpp -- host build of the index arithmetic of quadrotor_landing_amd/csrc/sequence_kernels.hpp and of the pack plan
// of sequence_plan.hpp (TEST ONLY).
//
// Both headers are free of HIP and are compiled unmodified by g++.  The
// program walks every lane and piece of a span exactly as stage_aos_head does (same seq_piece_word / seq_piece_len / seq_piece_kind /
// seq_word_moved calls) on heap arrays of exactly valid * W words, so that a sanitizer build (-fsanitize=address,undefined,
// tests/test_sequence_cpu.py) faults on any access outside the valid words, and writes what it saw to a file of int64 that the test
// checks against its own statement of what a staging routine owes.  The plan is written out entry by entry the same way.
//
// usage: sequence_harness out.bin
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../quadrotor_landing_amd/csrc/sequence_index.hpp"
#include "../../quadrotor_landing_amd/csrc/sequence_plan.hpp"

constexpr int kTile = 64;                 // filters of a tile
constexpr int kPitchU = 7, kPitchZ = 7;   // the LDS pitches of the two images (devio_kernels.hpp)

using namespace qsq;

static std::vector<int64_t> out;
static void put(int64_t v) { out.push_back(v); }

// the walk of stage_aos_head over a span of nv valid W-word rows that starts `head` words in front of a 16-byte boundary
static void walk(int W, int V, int head, int nv, int pitch)
{
    const int valid = nv * W;
    int64_t* cnt = new int64_t[(size_t)valid]();   // exactly the valid words: the sanitizer guards both ends
    int64_t* fw = new int64_t[(size_t)valid]();
    int64_t vec = 0, scalar = 0, lo = INT64_MAX, hi = -1, lds_max = -1, misaligned = 0;
    const int NP = seq_pieces(kTile * W, V);
    for (int lane = 0; lane < kTile; ++lane)
        for (int k = 0; k * kTile < NP; ++k) {
            const int p = k * kTile + lane;
            const int j = seq_piece_word(p, V, head);
            const int len = seq_piece_len(p, V, head);
            const int kind = seq_piece_kind(j, len, V, valid);
            if (kind == 0) continue;
            if (kind == 2) {
                ++vec;
                if ((j - head) % V != 0 || j < head) ++misaligned;   // a 16-byte access must start on the boundary grid
            }
            for (int e = 0; e < V; ++e) {
                if (kind == 1 && !seq_word_moved(j, e, len, valid)) continue;
                if (kind == 1) ++scalar;
                const int q = j + e;
                if (q < lo) lo = q;
                if (q > hi) hi = q;
                const int f = q / W, w = q - f * W;
                cnt[q] += 1;
                fw[q] = (int64_t)f * 1000 + w;
                const int l = f * pitch + w;
                if (l > lds_max) lds_max = l;
            }
        }
    for (int q = 0; q < valid; ++q) put(cnt[q]);
    for (int q = 0; q < valid; ++q) put(fw[q]);
    put(vec); put(scalar); put(valid ? lo : 0); put(hi); put(lds_max); put(misaligned);
    delete[] cnt;
    delete[] fw;
}

int main(int argc, char** argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s out.bin\n", argv[0]); return 2; }
    // 1. head words of an address, fp32 then fp64 elements
    for (uint64_t a = 0; a < 32; a += 4) put(seq_head_words(0x7f0000001000ull + a, 4));
    for (uint64_t a = 0; a < 32; a += 8) put(seq_head_words(0x7f0000001000ull + a, 8));
    // 2. the staging walks: source width V words per 16 bytes, every head, W = 6 (IMU) and 7 (tag pose), valid filters
    const int nvs[5] = {0, 1, 23, 63, 64};
    for (int V = 4; V >= 2; V -= 2)
        for (int head = 0; head < V; ++head)
            for (int W = 6; W <= 7; ++W)
                for (int nv : nvs) walk(W, V, head, nv, W == 6 ? kPitchU : kPitchZ);
    // 3. the plan: n, t0, tag pattern (0 none, 1 all, 2 the ticks of the list)
    const int64_t ns[5] = {1, 31, 32, 33, 70}, t0s[2] = {0, 5}, tagged[7] = {0, 3, 31, 32, 33, 64, 69};
    for (int64_t n : ns)
        for (int64_t t0 : t0s)
            for (int pat = 0; pat < 3; ++pat) {
                int64_t m = -1;
                const std::vector<PlanChunk> plan = sequence_plan(t0, n, [&](int64_t t) {
                    if (pat < 2) return pat == 1;
                    for (int64_t g : tagged) if (g == t) return true;
                    return false;
                }, &m);
                put((int64_t)plan.size()); put(plan_chunks(n)); put(m);
                for (const PlanChunk& c : plan) {
                    put(c.k0); put(c.count);
                    for (int y = 0; y < c.count; ++y) { put(c.e[y].tick); put(c.e[y].zsrc); }
                }
            }
    put(kSeqChunk);
    FILE* f = std::fopen(argv[1], "wb");
    if (!f) return 3;
    std::fwrite(out.data(), sizeof(int64_t), out.size(), f);
    std::fclose(f);
    std::printf("%zu\n", out.size());
    return 0;
}
