// health_harness.cpp -- the per-filter classification of k_health (quadrotor_landing_amd/csrc/ekf_health.hpp: health_classify) compiled
// for the host, unmodified, and run on a batch read from a file (tests/test_health_cpu.py writes it and checks the status bytes against
// a numpy restatement).  TEST ONLY; the product has no CPU path.
//
//   health_harness <in> <out>
// in  (doubles): B, fp64, compact, n, sigma_r_max, sigma_v_max, sigma_theta_max, qnorm_tol, select, then per filter x[16], P[15][15]
// out (doubles): per filter status (what the kernel stores: 0 for a filter without state), no_state
// A compact run is handed NaN in every covariance word a compact record does not hold: they must not matter.
#include <cmath>

#include "../../quadrotor_landing_amd/csrc/ekf_health.hpp"
#include "harness_io.hpp"

using namespace qle;

static const int kHdr = 9, kPer = 16 + 225, kOut = 2;

template <typename T, bool COMPACT, int N>
static void run(const double* h, const double* d, double* out)
{
    const int64_t B = (int64_t)h[0];
    HealthLimits lim;
    lim.r2 = h[4] * h[4]; lim.v2 = h[5] * h[5]; lim.th2 = h[6] * h[6];
    lim.qnorm_tol = h[7];
    lim.select = (uint32_t)h[8];
    for (int64_t i = 0; i < B; ++i) {
        const double* f = d + i * kPer;
        T x[16], P[120];
        for (int k = 0; k < 16; ++k) x[k] = (T)f[k];
        for (int a = 0; a < 15; ++a)
            for (int b = a; b < 15; ++b) P[sidx(a, b)] = COMPACT && b >= 9 ? (T)NAN : (T)f[16 + a * 15 + b];
        bool no_state;
        const uint32_t s = health_classify<T, COMPACT, N>(x, P, T(0), lim, no_state);
        out[i * kOut] = no_state ? 0.0 : (double)s;
        out[i * kOut + 1] = no_state ? 1.0 : 0.0;
    }
}

int main(int argc, char** argv)
{
    const auto check = [](const double* h) {
        const int n = (int)h[3];
        return n != 15 && n != 9 ? 7 : h[2] != 0 && n != 9 ? 8 : 0;
    };
    return harness_main(argc, argv, kHdr, check, per_filter(kPer), per_filter(kOut), [](const double* h, const double* d, double* out) {
        by_dtype(h[1] != 0, [&](auto t) {
            by_flags(h[2] != 0, h[3] == 15, [&](auto compact, auto fifteen) {   // check(): a compact record has 9 states
                constexpr bool c = decltype(compact)::value;
                run<decltype(t), c, decltype(fifteen)::value && !c ? 15 : 9>(h, d, out);
            });
        });
    });
}
