// bank_lanes.hpp -- what bank_harness.cpp and imm_harness.cpp share on top of harness_io.hpp: the kernels' xor-butterfly restated as the
// same tree over an array of a bank's M lanes, and the move between a row-major 15 x 15 covariance and the record words of BankWords
// (quadrotor_landing_amd/csrc/ekf_bank.hpp, which both product headers under test are built on).  TEST ONLY.
#pragma once
#include <cstdlib>
#include <cstring>

#include "../../quadrotor_landing_amd/csrc/ekf_bank.hpp"
#include "harness_io.hpp"

// the butterfly of bank_sum / bank_max / bank_min over an array v[lane][n]: stage o = 1, 2, ..., M/2 replaces v[l] by op(v[l], v[l ^ o])
// in every lane, and every lane must end with the same bits
template <typename V, typename Op>
static void tree(std::vector<V>& v, int n, int M, Op op)
{
    std::vector<V> t(v.size());
    for (int o = 1; o < M; o <<= 1) {
        t = v;
        for (int l = 0; l < M; ++l)
            for (int k = 0; k < n; ++k) v[l * n + k] = op(t[l * n + k], t[(l ^ o) * n + k]);
    }
    for (int l = 1; l < M; ++l)
        if (std::memcmp(&v[l * n], &v[0], n * sizeof(V)) != 0) { std::fprintf(stderr, "the lanes of a bank disagree\n"); std::exit(7); }
}
static double add(double a, double b) { return a + b; }
static double larger(double a, double b) { return b > a ? b : a; }

// the record words of one filter from its covariance P[15][15]; a padding word is 0
template <bool COMPACT, typename T>
static void words_from_P(const double* P, T* Pw)
{
    constexpr qle::BankWords<COMPACT> words{};
    for (int wd = 0; wd < words.kWords; ++wd) Pw[wd] = words.a[wd] < 0 ? T(0) : (T)P[words.a[wd] * 15 + words.b[wd]];
}

// ... and back: P[15][15] = 0, then value(wd) in both triangles for every word that is not padding
template <bool COMPACT, typename Value>
static void P_from_words(double* P, Value value)
{
    constexpr qle::BankWords<COMPACT> words{};
    for (int k = 0; k < 225; ++k) P[k] = 0.0;
    for (int wd = 0; wd < words.kWords; ++wd)
        if (words.a[wd] >= 0) P[words.a[wd] * 15 + words.b[wd]] = P[words.b[wd] * 15 + words.a[wd]] = value(wd);
}
