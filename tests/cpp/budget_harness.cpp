// budget_harness.cpp -- the host-compilable parts of k_budget (quadrotor_landing_amd/csrc/ekf_budget.hpp) compiled for the host,
// unmodified, and run on a batch read from a file (tests/test_budget_cpu.py writes it and checks the result).  TEST ONLY; the product
// has no CPU path.
//
//   budget_harness <in> <out>
// in  (doubles): B, fp64, compact, n_states, mode, then
//   mode 0 (the lane): per filter x[16], P[15][15], x_true[16], ab_static[3], wb_static[3], on
//                      out per filter: the 256 words (budget_lane + BudgetWords), counted, e[15] of error_state, e[15] of nees_eval
//   mode 1 (the tile sum): B tiles of words[64][256]; out per tile: 256 fields -- tile_reduce, the recursion k_budget runs, over
//                      64-value arrays: v_permlane32_swap, v_permlane16_swap and the DPP moves as the array permutations they are
// A compact run is handed NaN in every covariance word a compact record does not hold: they must not matter.
#include <cmath>
#include <utility>

#include "../../quadrotor_landing_amd/csrc/ekf_budget.hpp"
#include "../../quadrotor_landing_amd/csrc/ekf_consistency.hpp"
#include "harness_io.hpp"

using namespace qle;

static const int kHdr = 5, kPer = 16 + 225 + 16 + 6 + 1, kOut = 256 + 1 + 15 + 15;

template <typename T, int... F>
static void all_words(const BudgetWords<T>& w, double* o, std::integer_sequence<int, F...>)
{
    (..., (o[F] = w.template word<F>()));
}

template <typename T, bool COMPACT>
static void run_lane(const double* h, const double* d, double* out)
{
    const int64_t B = (int64_t)h[0];
    const int n_states = (int)h[3];
    for (int64_t i = 0; i < B; ++i) {
        const double* f = d + i * kPer;
        T x[16], P[120], Pn[120], xt[16], ab[3], wb[3], e[15], ec[15], en[15];
        for (int k = 0; k < 16; ++k) { x[k] = (T)f[k]; xt[k] = (T)f[241 + k]; }
        for (int a = 0; a < 15; ++a)
            for (int b = a; b < 15; ++b) Pn[sidx(a, b)] = P[sidx(a, b)] = COMPACT && b >= 9 ? (T)NAN : (T)f[16 + a * 15 + b];
        for (int k = 0; k < 3; ++k) { ab[k] = (T)f[257 + k]; wb[k] = (T)f[260 + k]; }
        const bool dead = filter_uninitialised(x);   // as k_budget: a filter without a state computes on with a unit quaternion, off
        if (dead) x[9] = T(1);
        const bool counted = budget_lane<T, COMPACT>(x, P, xt, ab, wb, n_states, !dead && f[263] != 0, e, ec);
        const BudgetWords<T> words{ec, P, counted ? 1.0 : 0.0};
        double* o = out + i * kOut;
        all_words<T>(words, o, std::make_integer_sequence<int, kBudgetWords>{});
        o[256] = counted ? 1.0 : 0.0;
        bool pd;
        (void)nees_eval<T, COMPACT>(x, Pn, xt, ab, wb, COMPACT || n_states == 9 ? 7u : kNeesAllBlocks, en, pd);
        error_state<T>(x, xt, ab, wb, e);   // as it leaves the function: the select of a 9-state handle is budget_lane's
        for (int k = 0; k < 15; ++k) { o[257 + k] = (double)e[k]; o[272 + k] = (double)en[k]; }
    }
}

// ---- the butterfly over arrays: a value per lane
struct Lanes { double v[64]; };
struct NoWords {};
struct ArrayOps {
    const double* w;   // [64][256]
    template <int F>
    Lanes leaf(const NoWords&) const
    {
        Lanes r;
        for (int l = 0; l < 64; ++l) r.v[l] = w[l * 256 + F];
        return r;
    }
    template <int O>
    Lanes combine(Lanes a, Lanes b) const
    {
        Lanes r;
        if (O == 32) {          // v_permlane32_swap a, b: lanes 32..63 of a <-> lanes 0..31 of b
            for (int l = 0; l < 32; ++l) std::swap(a.v[32 + l], b.v[l]);
            for (int l = 0; l < 64; ++l) r.v[l] = a.v[l] + b.v[l];
        } else if (O == 16) {   // v_permlane16_swap a, b: the odd rows of a <-> the even rows of b
            for (int l = 0; l < 16; ++l) { std::swap(a.v[16 + l], b.v[l]); std::swap(a.v[48 + l], b.v[32 + l]); }
            for (int l = 0; l < 64; ++l) r.v[l] = a.v[l] + b.v[l];
        } else {
            Lanes keep, give, got;
            for (int l = 0; l < 64; ++l) { const bool up = (l & O) != 0; keep.v[l] = up ? b.v[l] : a.v[l]; give.v[l] = up ? a.v[l] : b.v[l]; }
            static const int q2[4] = {2, 3, 0, 1}, q1[4] = {1, 0, 3, 2};
            for (int l = 0; l < 64; ++l) {
                const int row = l & ~15, in = l & 15, bank = in >> 2;
                int src;
                if (O == 8) src = row | ((in - 8) & 15);                                     // row_ror:8: lane l reads lane (l - 8) mod 16
                else if (O == 4) src = row | ((in - ((bank & 1) == 0 ? 12 : 4)) & 15);       // row_ror:12 in banks 0, 2; row_ror:4 in banks 1, 3
                else src = (l & ~3) | (O == 2 ? q2[l & 3] : q1[l & 3]);                      // quad_perm
                got.v[l] = give.v[src];
            }
            for (int l = 0; l < 64; ++l) r.v[l] = keep.v[l] + got.v[l];
        }
        return r;
    }
};

static void run_tiles(const double* h, const double* d, double* out)
{
    for (int64_t t = 0; t < (int64_t)h[0]; ++t) {
        const ArrayOps ops{d + t * 64 * 256};
        const Lanes r[4] = {tile_reduce<6, 0, 0>(ops, NoWords{}), tile_reduce<6, 0, 1>(ops, NoWords{}), tile_reduce<6, 0, 2>(ops, NoWords{}),
                            tile_reduce<6, 0, 3>(ops, NoWords{})};
        for (int k = 0; k < 4; ++k)
            for (int l = 0; l < 64; ++l) out[t * 256 + 64 * k + l] = r[k].v[l];   // lane l ends round k with field 64 k + l, and stores it there
    }
}

int main(int argc, char** argv)
{
    const auto tiles = [](const double* h) { return h[4] != 0; };
    return harness_main(
        argc, argv, kHdr, no_check, [&](const double* h) { return (size_t)h[0] * (tiles(h) ? 64 * 256 : kPer); },
        [&](const double* h) { return (size_t)h[0] * (tiles(h) ? 256 : kOut); },
        [&](const double* h, const double* d, double* out) {
            if (tiles(h)) return run_tiles(h, d, out);
            by_dtype(h[1] != 0, [&](auto t) { by_flags(h[2] != 0, [&](auto compact) { run_lane<decltype(t), decltype(compact)::value>(h, d, out); }); });
        });
}
