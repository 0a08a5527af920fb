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

#include "../../quadrotor_landing_amd/csrc/ekf_lookahead.hpp"
#include "harness_io.hpp"

using namespace qle;

static const int kHdr = 7 + 4 + 3 + 4 + 9 + 3 + 12 + 6 + 3 + 3, kPer = 16 + 225 + 6 + 24 + 1, kOut = 16 + 225 + 1;

template <typename T>
static void run(const double* h, const double* d, double* out)
{
    const int64_t B = (int64_t)h[0];
    const bool compact = h[2] != 0, use_pfp = h[3] != 0;
    const int32_t horizon = (int32_t)h[4];
    CoastLimits lim;
    lim.r2 = h[5] * h[5];      // the squares formed in double, as lookahead_capi.hip forms them
    lim.th2 = h[6] * h[6];
    const double* q = h + 7;
    const DevParams<T> p = decode_params<T>(q, compact ? 1 : 0);
    for (int64_t i = 0; i < B; ++i) {
        const double* f = d + i * kPer;
        T x[16], P[120], u[6];
        for (int k = 0; k < 16; ++k) x[k] = (T)f[k];
        for (int a = 0; a < 15; ++a)
            for (int b = a; b < 15; ++b) P[sidx(a, b)] = (compact && b >= 9) ? T(0) : (T)f[16 + a * 15 + b];
        for (int k = 0; k < 6; ++k) u[k] = (T)f[241 + k];
        const Noise<T> nz = noise_from(p, f + 247, use_pfp);
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
    const auto check = [](const double* h) { return h[0] < 1 || h[4] < 0 || h[4] > kMaxHorizon ? 7 : 0; };
    return harness_main(argc, argv, kHdr, check, per_filter(kPer), per_filter(kOut),
                        [](const double* h, const double* d, double* out) { by_dtype(h[1] != 0, [&](auto t) { run<decltype(t)>(h, d, out); }); });
}
