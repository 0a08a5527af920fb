// imm_harness.cpp -- the arithmetic of k_imm_mix and k_imm_update (quadrotor_landing_amd/csrc/ekf_imm.hpp: imm_pred_term, imm_c_ok,
// imm_mix_weight, imm_mean_step, imm_centred, imm_update_*, over bank_member_valid, bank_weight_raw, bank_diff, bank_fuse_state,
// bank_cov_term and the word table of ekf_bank.hpp) compiled for the host, unmodified, and run on a batch read from a file
// (tests/test_imm_cpu.py writes it and checks the result against the numpy restatement of tests/imm_util.py).  The kernel's shuffle loops
// over the members are restated here as the same ascending loops over an array of the bank's M lanes; its butterflies (the weights, the
// sums of the recursion) as the same tree over an array, the one tests/cpp/bank_harness.cpp uses (tests/cpp/bank_lanes.hpp).  TEST ONLY;
// the product has no CPU path.
//
//   imm_harness mix <in> <out>
// in  (doubles): B, fp64, compact, M, then Pi[M][M], then per filter x[16], P[15][15], logmu, mask
// out (doubles): per filter logc, mixed, x[16], P[15][15]  (an unmixed filter: its own words)
// A compact run is handed NaN in every covariance word a compact record does not hold: they must not matter (they come back 0).
//
//   imm_harness update <in> <out>
// in  (doubles): B, M, logmu_min, then per filter logc, loglik, mask
// out (doubles): per filter logmu
#include <cmath>

#include "../../quadrotor_landing_amd/csrc/ekf_imm.hpp"
#include "bank_lanes.hpp"

using namespace qle;

static const int kPer = 16 + 225 + 2, kOut = 2 + 16 + 225;

template <typename T, bool COMPACT>
static void mix(const double* Pi, const double* in, int64_t B, int M, double* out)
{
    constexpr BankWords<COMPACT> words{};
    constexpr int W = BankWords<COMPACT>::kWords;
    for (int64_t g = 0; g < B / M; ++g) {
        std::vector<T> x(M * 16), Pw((size_t)M * W);
        std::vector<double> lw(M), lm(M), ws(M), wraw(M), mu(M);
        std::vector<char> valid(M);
        for (int l = 0; l < M; ++l) {
            const double* f = in + (g * M + l) * kPer;
            T xl[16];
            for (int k = 0; k < 16; ++k) x[l * 16 + k] = xl[k] = (T)f[k];
            words_from_P<COMPACT>(f + 16, &Pw[(size_t)l * W]);
            lw[l] = f[241];
            valid[l] = bank_member_valid(xl, lw[l], f[242] != 0.0);
            lm[l] = valid[l] ? lw[l] : -INFINITY;
        }
        tree(lm, 1, M, larger);
        for (int l = 0; l < M; ++l) ws[l] = wraw[l] = bank_weight_raw(valid[l], lw[l], lm[0]);
        tree(ws, 1, M, add);
        for (int l = 0; l < M; ++l) mu[l] = ws[0] > 0.0 ? wraw[l] / ws[0] : 0.0;
        for (int j = 0; j < M; ++j) {
            T xj[16], xi[16];
            for (int k = 0; k < 16; ++k) xj[k] = x[j * 16 + k];
            double cj = 0.0;
            for (int k = 0; k < M; ++k) cj += imm_pred_term(Pi[k * M + j], mu[k]);
            const bool cok = valid[j] && imm_c_ok(cj);
            double m[15] = {};
            bool other = false;
            for (int k = 0; k < M; ++k) {
                const double w = imm_mix_weight(Pi[k * M + j], mu[k], cj);
                for (int e = 0; e < 16; ++e) xi[e] = x[k * 16 + e];
                other = other || (k != j && w > 0.0);
                imm_mean_step(xi, xj, w, m);
            }
            const bool store = cok && other;
            T xf[16];
            bank_fuse_state(xj, m, false, xf);
            std::vector<double> term(W, 0.0);
            for (int k = 0; k < M; ++k) {
                const double w = imm_mix_weight(Pi[k * M + j], mu[k], cj);
                for (int e = 0; e < 16; ++e) xi[e] = x[k * 16 + e];
                double c[15];
                imm_centred(xi, xj, m, c);
                for (int wd = 0; wd < W; ++wd)
                    if (words.a[wd] >= 0) term[wd] += bank_cov_term(w > 0.0, w, (double)Pw[(size_t)k * W + wd], c[words.a[wd]], c[words.b[wd]]);
            }
            double* o = out + (g * M + j) * kOut;
            o[0] = cok ? log(cj) : -INFINITY;
            o[1] = store ? 1.0 : 0.0;
            for (int k = 0; k < 16; ++k) o[2 + k] = (double)(store ? xf[k] : xj[k]);
            P_from_words<COMPACT>(o + 18, [&](int wd) { return store ? (double)(T)term[wd] : (double)Pw[(size_t)j * W + wd]; });
        }
    }
}

static void update(const double* in, int64_t B, int M, double logmu_min, double* out)
{
    for (int64_t g = 0; g < B / M; ++g) {
        std::vector<double> t(M), tm(M), e(M);
        std::vector<char> ok(M);
        for (int l = 0; l < M; ++l) {
            const double* f = in + (g * M + l) * 3;
            ok[l] = f[2] != 0.0 && bank_finite(f[0]);
            tm[l] = t[l] = imm_update_term(ok[l], f[0], f[1]);
        }
        tree(tm, 1, M, larger);
        for (int l = 0; l < M; ++l) e[l] = imm_update_exp(t[l], tm[0]);
        tree(e, 1, M, add);
        for (int l = 0; l < M; ++l) out[g * M + l] = imm_update_final(ok[l], t[l], tm[0], e[0], logmu_min);
    }
}

// B in h[0] and M in h[m]: a power of two in 2..64 that divides the batch
static int check_bank(const double* h, int m) { return !bank_members_ok((int)h[m]) || (int64_t)h[0] <= 0 || (int64_t)h[0] % (int)h[m] != 0 ? 9 : 0; }

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    if (std::strcmp(argv[1], "mix") == 0)
        return harness_main(argc - 1, argv + 1, 4, [](const double* h) { return check_bank(h, 3); },
                            [](const double* h) { return (size_t)h[3] * (size_t)h[3] + (size_t)h[0] * kPer; }, per_filter(kOut),
                            [](const double* h, const double* d, double* out) {
                                const int M = (int)h[3];
                                by_dtype(h[1] != 0, [&](auto t) {
                                    by_flags(h[2] != 0, [&](auto compact) { mix<decltype(t), decltype(compact)::value>(d, d + M * M, (int64_t)h[0], M, out); });
                                });
                            });
    if (std::strcmp(argv[1], "update") == 0)
        return harness_main(argc - 1, argv + 1, 3, [](const double* h) { return check_bank(h, 1); }, per_filter(3), per_filter(1),
                            [](const double* h, const double* d, double* out) { update(d, (int64_t)h[0], (int)h[1], h[2], out); });
    return 2;
}
