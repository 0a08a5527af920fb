// consistency_harness.cpp -- the arithmetic of k_nees (quadrotor_landing_amd/csrc/ekf_consistency.hpp: nees_eval) compiled for the host,
// unmodified, and run on a batch read from a file (tests/test_consistency_cpu.py writes it and checks the result against numpy's dense
// solve).  TEST ONLY; the product has no CPU path.
//
//   consistency_harness <in> <out>
// in  (doubles): B, fp64, compact, blocks, then per filter x[16], P[15][15], x_true[16], ab_static[3], wb_static[3]
// out (doubles): per filter nees, pd, err[15]
// A compact run is handed NaN in every covariance word a compact record does not hold: they must not matter.
#include <cmath>

#include "../../quadrotor_landing_amd/csrc/ekf_consistency.hpp"
#include "harness_io.hpp"

using namespace qle;

static const int kHdr = 4, kPer = 16 + 225 + 16 + 6, kOut = 2 + 15;

template <typename T, bool COMPACT>
static void run(const double* h, const double* d, double* out)
{
    const int64_t B = (int64_t)h[0];
    const uint32_t blocks = (uint32_t)h[3];
    for (int64_t i = 0; i < B; ++i) {
        const double* f = d + i * kPer;
        T x[16], P[120], xt[16], ab[3], wb[3], e[15];
        for (int k = 0; k < 16; ++k) { x[k] = (T)f[k]; xt[k] = (T)f[241 + k]; }
        for (int a = 0; a < 15; ++a)
            for (int b = a; b < 15; ++b) P[sidx(a, b)] = COMPACT && b >= 9 ? (T)NAN : (T)f[16 + a * 15 + b];
        for (int k = 0; k < 3; ++k) { ab[k] = (T)f[257 + k]; wb[k] = (T)f[260 + k]; }
        bool pd;
        const T nees = nees_eval<T, COMPACT>(x, P, xt, ab, wb, blocks, e, pd);
        double* o = out + i * kOut;
        o[0] = (double)nees;
        o[1] = pd ? 1.0 : 0.0;
        for (int k = 0; k < 15; ++k) o[2 + k] = (double)e[k];
    }
}

int main(int argc, char** argv)
{
    return harness_main(argc, argv, kHdr, no_check, per_filter(kPer), per_filter(kOut), [](const double* h, const double* d, double* out) {
        by_dtype(h[1] != 0, [&](auto t) { by_flags(h[2] != 0, [&](auto compact) { run<decltype(t), decltype(compact)::value>(h, d, out); }); });
    });
}
