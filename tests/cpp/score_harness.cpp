// score_harness.cpp -- the arithmetic of k_score (quadrotor_landing_amd/csrc/ekf_score.hpp: score_accumulate behind pregate_eval_pivots of
// ekf_pregate.hpp) compiled for the host, unmodified, and run over consecutive tag ticks read from a file (tests/test_score_cpu.py writes
// it and checks the accumulators against the dense oracle, numpy's slogdet and plain fp64 sums).  TEST ONLY; the product has no CPU path.
//
//   score_harness <in> <out>
// in  (doubles): B, direct, ticks, use_pfp, fp64, then dT, dTw, bias_on, small_ang_tol, g[3], q_vc[4], C_vc[9], r_v_cv[3], Q[12], R[6],
//                ab_static[3], wb_static[3], then per tick, per filter: x[16], P[15][15], u[6], z[7], pfp[24], on -- the state BEFORE the tick
// out (doubles): per filter the accumulator record, 40 words (include/qle_score.h)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../quadrotor_landing_amd/csrc/ekf_score.hpp"

using namespace qle;

static const int kHdr = 5 + 4 + 3 + 4 + 9 + 3 + 12 + 6 + 3 + 3, kPer = 16 + 225 + 6 + 7 + 24 + 1;

template <typename T, bool DIRECT>
static void run(const double* h, const double* data, int64_t B, int ticks, bool use_pfp, double* out)
{
    DevParams<T> p;
    const double* q = h + 5;
    p.dT = (T)q[0]; p.dTw = (T)q[1]; p.bias_on = (T)q[2]; p.small_ang_tol = (T)q[3]; q += 4;
    for (int k = 0; k < 3; ++k) p.g[k] = (T)*q++;
    for (int k = 0; k < 4; ++k) p.q_vc[k] = (T)*q++;
    for (int k = 0; k < 9; ++k) p.C_vc[k] = (T)*q++;
    for (int k = 0; k < 3; ++k) p.r_v_cv[k] = (T)*q++;
    for (int k = 0; k < 12; ++k) p.Q[k] = (T)*q++;
    for (int k = 0; k < 6; ++k) p.R[k] = (T)*q++;
    for (int k = 0; k < 3; ++k) p.ab_static[k] = (T)*q++;
    for (int k = 0; k < 3; ++k) p.wb_static[k] = (T)*q++;
    p.compact = 0;
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
            const double* pf = f + 254;
            Noise<T> nz;
            for (int k = 0; k < 12; ++k) nz.Q[k] = use_pfp ? (T)pf[k] : p.Q[k];
            for (int k = 0; k < 3; ++k) { nz.ab_static[k] = use_pfp ? (T)pf[12 + k] : p.ab_static[k]; nz.wb_static[k] = use_pfp ? (T)pf[15 + k] : p.wb_static[k]; }
            for (int k = 0; k < 6; ++k) nz.R[k] = use_pfp ? (T)pf[18 + k] : p.R[k];
            bool pd;
            const T nis = pregate_eval_pivots<T, DIRECT, true>(p, nz, x, Po, u, z, nu, S, d, pd);
            score_accumulate<T>(a, f[278] != 0, nis, pd, nu, S, d);
        }
        double* o = out + i * kScoreWords;
        for (int w = 0; w < kScoreWords; ++w) o[w] = w < kScoreLive ? a[w] : 0.0;
    }
}

template <typename T>
static void run_t(const double* h, const double* d, int64_t B, double* out)
{
    const int ticks = (int)h[2];
    const bool pfp = h[3] != 0;
    if (h[1] != 0) run<T, true>(h, d, B, ticks, pfp, out);
    else run<T, false>(h, d, B, ticks, pfp, out);
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* fi = std::fopen(argv[1], "rb");
    if (!fi) return 3;
    std::vector<double> h(kHdr);
    if (std::fread(h.data(), sizeof(double), kHdr, fi) != (size_t)kHdr) return 4;
    const int64_t B = (int64_t)h[0], ticks = (int64_t)h[2];
    if (B < 1 || ticks < 1) return 4;
    std::vector<double> d((size_t)(B * ticks) * kPer), out((size_t)B * kScoreWords);
    if (std::fread(d.data(), sizeof(double), d.size(), fi) != d.size()) return 5;
    std::fclose(fi);
    if (h[4] != 0) run_t<double>(h.data(), d.data(), B, out.data());
    else run_t<float>(h.data(), d.data(), B, out.data());
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo || std::fwrite(out.data(), sizeof(double), out.size(), fo) != out.size()) return 6;
    std::fclose(fo);
    std::printf("%lld\n", (long long)B);
    return 0;
}
