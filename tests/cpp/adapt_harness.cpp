// adapt_harness.cpp -- the arithmetic of k_adapt_observe and k_adapt_apply (quadrotor_landing_amd/csrc/ekf_adapt.hpp: noise_columns,
// adapt_sample, adapt_accumulate and adapt_apply_one behind pregate_eval_pivots of ekf_pregate.hpp) compiled for the host, unmodified, and
// run over consecutive tag ticks read from a file, with an apply after every window-th tick (tests/test_adapt_cpu.py writes it and checks
// the accumulators against the dense oracle, numpy.linalg.solve and plain fp64 sums, and every apply against the formula in numpy).
// TEST ONLY; the product has no CPU path.
//
//   adapt_harness <in> <out>
// in  (doubles): B, direct, ticks, fp64, window, gain, n_min, chi2_max, R_lo[6], R_hi[6], then dT, dTw, bias_on, small_ang_tol, g[3],
//                q_vc[4], C_vc[9], r_v_cv[3], Q[12], R[6], ab_static[3], wb_static[3], then
//                ticks >= 1: per tick, per filter: x[16], P[15][15], u[6], z[7], pfp[24], on -- the state BEFORE the tick; Q and the
//                            static biases of every tick's pfp are used, R of the first tick's only (the harness carries R on)
//                ticks == 0: per filter x[16], R[6]
// out (doubles): ticks >= 1: per filter the accumulator record (24 words, include/qle_adapt.h), R[6] after the run, then per apply
//                            (ticks / window of them): the record before it (24), R before (6), R after (6), applied (1)
//                ticks == 0: per filter R_k of quad::update_noise as a full 6 x 6, then N of noise_columns (6 x 6, row-major)
#include <cmath>

#include "../../quadrotor_landing_amd/csrc/ekf_adapt.hpp"
#include "harness_io.hpp"

using namespace qle;

static const int kCfg = 20, kHdr = kCfg + 4 + 3 + 4 + 9 + 3 + 12 + 6 + 3 + 3, kPer = 16 + 225 + 6 + 7 + 24 + 1, kPerApply = 24 + 6 + 6 + 1;

static size_t out_words(const double* h)
{
    const int ticks = (int)h[2], window = (int)h[4];
    return ticks == 0 ? 72 : (size_t)(kAdaptWords + 6 + (ticks / window) * kPerApply);
}

template <typename T, bool DIRECT>
static void run_noise(const double* h, const double* data, double* out)
{
    const int64_t B = (int64_t)h[0];
    const double* q = h + kCfg;
    const DevParams<T> p = decode_params<T>(q, 0);
    for (int64_t i = 0; i < B; ++i) {
        const double* f = data + i * 22;
        T x[16], Gx[9], Rk[quad::kRkWords], N[6][6];
        quad::NoiseV<T> nz{};
        for (int k = 0; k < 16; ++k) x[k] = (T)f[k];
        for (int k = 0; k < 6; ++k) nz.R[k] = (T)f[16 + k];
        quad::update_noise<quad::ScalarQ<T>, T, DIRECT>(p, nz, x, Gx, Rk);
        noise_columns<T, DIRECT>(p, x, N);
        double* o = out + i * 72;
        for (int a = 0; a < 6; ++a)
            for (int b = 0; b < 6; ++b) {
                o[a * 6 + b] = (double)Rk[a <= b ? quad::rk_idx(a, b) : quad::rk_idx(b, a)];
                o[36 + a * 6 + b] = (double)N[a][b];
            }
    }
}

template <typename T, bool DIRECT>
static void run(const double* h, const double* data, double* out)
{
    const int64_t B = (int64_t)h[0];
    const int ticks = (int)h[2], window = (int)h[4];
    if (ticks == 0) return run_noise<T, DIRECT>(h, data, out);
    AdaptApplyCfg cfg;
    cfg.gain = h[5];
    cfg.n_min = h[6];
    const double chi2_max = h[7];
    for (int k = 0; k < 6; ++k) { cfg.lo[k] = h[8 + k]; cfg.hi[k] = h[14 + k]; }
    const double* q = h + kCfg;
    const DevParams<T> p = decode_params<T>(q, 0);
    const size_t per_out = out_words(h);
    for (int64_t i = 0; i < B; ++i) {
        double a[kAdaptLive] = {};
        double* o = out + i * per_out;
        double* oa = o + kAdaptWords + 6;
        T R[6];
        for (int k = 0; k < 6; ++k) R[k] = (T)(data + i * kPer)[254 + 18 + k];
        for (int t = 0; t < ticks; ++t) {
            const double* f = data + ((int64_t)t * B + i) * kPer;
            T x[16], Po[120], u[6], z[7], nu[6], S[6][6], d[6];
            for (int k = 0; k < 16; ++k) x[k] = (T)f[k];
            for (int r = 0; r < 15; ++r)
                for (int c = r; c < 15; ++c) Po[sidx(r, c)] = pregate_needs(r, c) ? (T)(0.5 * (f[16 + r * 15 + c] + f[16 + c * 15 + r])) : (T)NAN;   // a word the kernel does not load must not matter
            for (int k = 0; k < 6; ++k) u[k] = (T)f[241 + k];
            for (int k = 0; k < 7; ++k) z[k] = (T)f[247 + k];
            Noise<T> nz = noise_from(p, f + 254, true);
            for (int k = 0; k < 6; ++k) nz.R[k] = R[k];
            bool pd0, pd;
            pregate_eval_pivots<T, DIRECT, true>(p, nz, x, Po, u, z, nu, S, d, pd0);
            T N[6][6], ak[6], ck[6], rhat[6];
            noise_columns<T, DIRECT>(p, x, N);
            const T nis = adapt_sample<T>(S, nu, N, nz.R, ak, ck, rhat, pd);
            adapt_accumulate<T>(a, f[278] != 0, nis, pd, ak, ck, rhat, chi2_max);
            if ((t + 1) % window == 0) {   // what k_adapt_apply does with adapt_apply_one
                for (int w = 0; w < kAdaptWords; ++w) oa[w] = w < kAdaptLive ? a[w] : 0.0;
                for (int k = 0; k < 6; ++k) oa[24 + k] = (double)R[k];
                const double sum[6] = {a[2], a[3], a[4], a[5], a[6], a[7]};
                T Rn[6];
                const bool ok = adapt_apply_one<T>(cfg, a[kAdN], sum, R, Rn);
                if (ok) {
                    for (int k = 0; k < 6; ++k) R[k] = Rn[k];
                    a[kAdN] = 0.0;
                    for (int w = kAdRhat; w < kAdTotal; ++w) a[w] = 0.0;
                    a[kAdWindows] += 1.0;
                }
                for (int k = 0; k < 6; ++k) oa[30 + k] = (double)R[k];
                oa[36] = ok ? 1.0 : 0.0;
                oa += kPerApply;
            }
        }
        for (int w = 0; w < kAdaptWords; ++w) o[w] = w < kAdaptLive ? a[w] : 0.0;
        for (int k = 0; k < 6; ++k) o[kAdaptWords + k] = (double)R[k];
    }
}

int main(int argc, char** argv)
{
    const auto check = [](const double* h) { return h[0] < 1 || h[2] < 0 || h[4] < 1 ? 4 : 0; };
    return harness_main(argc, argv, kHdr, check,
                        [](const double* h) { return h[2] == 0 ? (size_t)h[0] * 22 : (size_t)((int64_t)h[0] * (int64_t)h[2]) * kPer; },
                        [](const double* h) { return (size_t)h[0] * out_words(h); },
                        [](const double* h, const double* d, double* out) {
                            by_dtype(h[3] != 0, [&](auto t) { by_flags(h[1] != 0, [&](auto direct) { run<decltype(t), decltype(direct)::value>(h, d, out); }); });
                        });
}
