// lookahead_harness.cpp -- the per-filter body of k_lookahead (quadrotor_landing_amd/csrc/ekf_lookahead.hpp: lookahead_filter) compiled for
// the host, unmodified, and run on a batch read from a file (tests/test_lookahead_cpu.py writes it and checks the result against h
// applications of the dense oracle's predict).  TEST ONLY; the product has no CPU path.
//
//   lookahead_harness <in> <out>
// in  (doubles): B, fp64, compact, use_pfp, h, sigma_r_max, sigma_theta_max, then dT, dTw, bias_on, small_ang_tol, g[3], q_vc[4], C_vc[9],
//                r_v_cv[3], Q[12], R[6], ab_static[3], wb_static[3], then per filter x[16], P[15][15], u[6], pfp[24], asked
// out (doubles): per filter x[16], P[15][15], ticks_to_limit
// compact: the record holds the 9 x 9 pose block only -- the bias blocks of the input are not read (the kernel's load puts zeros into the
// register image) and come back as NaN (the kernel's store has no word for them).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../quadrotor_landing_amd/csrc/ekf_lookahead.hpp"

using namespace qle;

static const int kHdr = 7 + 4 + 3 + 4 + 9 + 3 + 12 + 6 + 3 + 3, kPer = 16 + 225 + 6 + 24 + 1, kOut = 16 + 225 + 1;

template <typename T>
static void run(const double* h, const double* d, int64_t B, double* out)
{
    const bool compact = h[2] != 0, use_pfp = h[3] != 0;
    const int32_t horizon = (int32_t)h[4];
    CoastLimits lim;
    lim.r2 = h[5] * h[5];      // the squares formed in double, as lookahead_capi.hip forms them
    lim.th2 = h[6] * h[6];
    DevParams<T> p;
    const double* q = h + 7;
    p.dT = (T)q[0]; p.dTw = (T)q[1]; p.bias_on = (T)q[2]; p.small_ang_tol = (T)q[3]; q += 4;
    for (int k = 0; k < 3; ++k) p.g[k] = (T)*q++;
    for (int k = 0; k < 4; ++k) p.q_vc[k] = (T)*q++;
    for (int k = 0; k < 9; ++k) p.C_vc[k] = (T)*q++;
    for (int k = 0; k < 3; ++k) p.r_v_cv[k] = (T)*q++;
    for (int k = 0; k < 12; ++k) p.Q[k] = (T)*q++;
    for (int k = 0; k < 6; ++k) p.R[k] = (T)*q++;
    for (int k = 0; k < 3; ++k) p.ab_static[k] = (T)*q++;
    for (int k = 0; k < 3; ++k) p.wb_static[k] = (T)*q++;
    p.compact = compact ? 1 : 0;
    for (int64_t i = 0; i < B; ++i) {
        const double* f = d + i * kPer;
        T x[16], P[120], u[6];
        for (int k = 0; k < 16; ++k) x[k] = (T)f[k];
        for (int a = 0; a < 15; ++a)
            for (int b = a; b < 15; ++b) P[sidx(a, b)] = (compact && b >= 9) ? T(0) : (T)f[16 + a * 15 + b];
        for (int k = 0; k < 6; ++k) u[k] = (T)f[241 + k];
        const double* pf = f + 247;
        Noise<T> nz;
        for (int k = 0; k < 12; ++k) nz.Q[k] = use_pfp ? (T)pf[k] : p.Q[k];
        for (int k = 0; k < 3; ++k) { nz.ab_static[k] = use_pfp ? (T)pf[12 + k] : p.ab_static[k]; nz.wb_static[k] = use_pfp ? (T)pf[15 + k] : p.wb_static[k]; }
        for (int k = 0; k < 6; ++k) nz.R[k] = use_pfp ? (T)pf[18 + k] : p.R[k];
        int32_t ticks = 12345;
        lookahead_filter<T>(p, nz, x, P, u, horizon, lim, f[271] != 0, ticks);
        double* o = out + i * kOut;
        for (int k = 0; k < 16; ++k) o[k] = (double)x[k];
        for (int a = 0; a < 15; ++a)
            for (int b = 0; b < 15; ++b) {
                const int lo = a < b ? a : b, hi = a < b ? b : a;
                o[16 + a * 15 + b] = (compact && hi >= 9) ? NAN : (double)P[sidx(lo, hi)];
            }
        o[241] = (double)ticks;
    }
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* fi = std::fopen(argv[1], "rb");
    if (!fi) return 3;
    std::vector<double> h(kHdr);
    if (std::fread(h.data(), sizeof(double), kHdr, fi) != (size_t)kHdr) return 4;
    const int64_t B = (int64_t)h[0];
    if (B <= 0 || h[4] < 0 || h[4] > kMaxHorizon) return 7;
    std::vector<double> d((size_t)B * kPer), out((size_t)B * kOut);
    if (std::fread(d.data(), sizeof(double), d.size(), fi) != d.size()) return 5;
    std::fclose(fi);
    if (h[1] != 0) run<double>(h.data(), d.data(), B, out.data());
    else run<float>(h.data(), d.data(), B, out.data());
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo || std::fwrite(out.data(), sizeof(double), out.size(), fo) != out.size()) return 6;
    std::fclose(fo);
    std::printf("%lld\n", (long long)B);
    return 0;
}
