// pregate_harness.cpp -- the arithmetic of k_pregate (quadrotor_landing_amd/csrc/ekf_pregate.hpp: pregate_eval) compiled for the host,
// unmodified, and run on a batch read from a file (tests/test_gate_cpu.py writes it and checks the result against the dense oracle).
// TEST ONLY; the product has no CPU path.
//
//   pregate_harness <in> <out>
// in  (doubles): B, direct, predict, use_pfp, fp64, then dT, dTw, bias_on, small_ang_tol, g[3], q_vc[4], C_vc[9], r_v_cv[3], Q[12], R[6],
//                ab_static[3], wb_static[3], then per filter x[16], P[15][15], u[6], z[7], pfp[24]
// out (doubles): per filter nis, nu[6], S[36]
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../quadrotor_landing_amd/csrc/ekf_pregate.hpp"

using namespace qle;

static const int kHdr = 5 + 4 + 3 + 4 + 9 + 3 + 12 + 6 + 3 + 3, kPer = 16 + 225 + 6 + 7 + 24, kOut = 1 + 6 + 36;

template <typename T, bool DIRECT, bool PREDICT>
static void run(const double* h, const double* d, int64_t B, bool use_pfp, double* out)
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
        const double* f = d + i * kPer;
        T x[16], Po[120], u[6], z[7], nu[6], S[6][6];
        for (int k = 0; k < 16; ++k) x[k] = (T)f[k];
        for (int a = 0; a < 15; ++a)
            for (int b = a; b < 15; ++b) Po[sidx(a, b)] = pregate_needs(a, b) || !PREDICT ? (T)(0.5 * (f[16 + a * 15 + b] + f[16 + b * 15 + a])) : (T)NAN;   // a word the kernel does not load must not matter
        for (int k = 0; k < 6; ++k) u[k] = (T)f[241 + k];
        for (int k = 0; k < 7; ++k) z[k] = (T)f[247 + k];
        const double* pf = f + 254;
        Noise<T> nz;
        for (int k = 0; k < 12; ++k) nz.Q[k] = use_pfp ? (T)pf[k] : p.Q[k];
        for (int k = 0; k < 3; ++k) { nz.ab_static[k] = use_pfp ? (T)pf[12 + k] : p.ab_static[k]; nz.wb_static[k] = use_pfp ? (T)pf[15 + k] : p.wb_static[k]; }
        for (int k = 0; k < 6; ++k) nz.R[k] = use_pfp ? (T)pf[18 + k] : p.R[k];
        const T nis = pregate_eval<T, DIRECT, PREDICT>(p, nz, x, Po, u, z, nu, S);
        double* o = out + i * kOut;
        o[0] = (double)nis;
        for (int k = 0; k < 6; ++k) o[1 + k] = (double)nu[k];
        for (int a = 0; a < 6; ++a)
            for (int b = 0; b < 6; ++b) o[7 + 6 * a + b] = (double)S[a][b];
    }
}

template <typename T>
static void run_t(const double* h, const double* d, int64_t B, double* out)
{
    const bool direct = h[1] != 0, predict = h[2] != 0, pfp = h[3] != 0;
    if (direct && predict) run<T, true, true>(h, d, B, pfp, out);
    else if (direct) run<T, true, false>(h, d, B, pfp, out);
    else if (predict) run<T, false, true>(h, d, B, pfp, out);
    else run<T, false, false>(h, d, B, pfp, out);
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* fi = std::fopen(argv[1], "rb");
    if (!fi) return 3;
    std::vector<double> h(kHdr);
    if (std::fread(h.data(), sizeof(double), kHdr, fi) != (size_t)kHdr) return 4;
    const int64_t B = (int64_t)h[0];
    std::vector<double> d((size_t)B * kPer), out((size_t)B * kOut);
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
