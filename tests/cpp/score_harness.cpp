// score_harness.cpp -- the arithmetic of k_score (quadrotor_landing_amd/csrc/ekf_score.hpp: score_accumulate behind pregate_eval_pivots of
// ekf_pregate.hpp) compiled for the host, unmodified, and run over consecutive tag ticks read from a file (tests/test_score_cpu.py writes
// it and checks the accumulators against the dense oracle, numpy's slogdet and plain fp64 sums).  TEST ONLY; the product has no CPU path.
//
//   score_harness <in> <out>
// in  (doubles): B, direct, ticks, use_pfp, fp64, then dT, dTw, bias_on, small_ang_tol, g[3], q_vc[4], C_vc[9], r_v_cv[3], Q[12], R[6],
//                ab_static[3], wb_static[3], then per tick, per filter: x[16], P[15][15], u[6], z[7], pfp[24], on -- the state BEFORE the tick
// out (doubles): per filter the accumulator record, 40 words (include/qle_score.h)
#include <cmath>

#include "../../quadrotor_landing_amd/csrc/ekf_score.hpp"
#include "harness_io.hpp"

using namespace qle;

static const int kHdr = 5 + 4 + 3 + 4 + 9 + 3 + 12 + 6 + 3 + 3, kPer = 16 + 225 + 6 + 7 + 24 + 1;

template <typename T, bool DIRECT>
static void run(const double* h, const double* data, double* out)
{
    const int64_t B = (int64_t)h[0];
    const int ticks = (int)h[2];
    const bool use_pfp = h[3] != 0;
    const double* q = h + 5;
    const DevParams<T> p = decode_params<T>(q, 0);
    for (int64_t i = 0; i < B; ++i) {
        double a[kScoreLive] = {};
        for (int t = 0; t < ticks; ++t) {
            const double* f = data + ((int64_t)t * B + i) * kPer;
            T x[16], Po[120], u[6], z[7], nu[6], S[6][6], d[6];
            for (int k = 0; k < 16; ++k) x[k] = (T)f[k];
            for (int r = 0; r < 15; ++r)
                for (int c = r; c < 15; ++c) Po[sidx(r, c)] = pregate_needs(r, c) ? (T)(0.5 * (f[16 + r * 15 + c] + f[16 + c * 15 + r])) : (T)NAN;   // a word the kernel does not load must not matter
            for (int k = 0; k < 6; ++k) u[k] = (T)f[241 + k];
            for (int k = 0; k < 7; ++k) z[k] = (T)f[247 + k];
            const Noise<T> nz = noise_from(p, f + 254, use_pfp);
            bool pd;
            const T nis = pregate_eval_pivots<T, DIRECT, true>(p, nz, x, Po, u, z, nu, S, d, pd);
            score_accumulate<T>(a, f[278] != 0, nis, pd, nu, S, d);
        }
        double* o = out + i * kScoreWords;
        for (int w = 0; w < kScoreWords; ++w) o[w] = w < kScoreLive ? a[w] : 0.0;
    }
}

int main(int argc, char** argv)
{
    const auto check = [](const double* h) { return h[0] < 1 || h[2] < 1 ? 4 : 0; };
    return harness_main(argc, argv, kHdr, check, [](const double* h) { return (size_t)((int64_t)h[0] * (int64_t)h[2]) * kPer; }, per_filter(kScoreWords),
                        [](const double* h, const double* d, double* out) {
                            by_dtype(h[4] != 0, [&](auto t) { by_flags(h[1] != 0, [&](auto direct) { run<decltype(t), decltype(direct)::value>(h, d, out); }); });
                        });
}
