// imm_harness.cpp -- the arithmetic of k_imm_mix and k_imm_update (quadrotor_landing_amd/csrc/ekf_imm.hpp: imm_pred_term, imm_c_ok,
// imm_mix_weight, imm_mean_step, imm_centred, imm_update_*, over bank_member_valid, bank_weight_raw, bank_diff, bank_fuse_state,
// bank_cov_term and the word table of ekf_bank.hpp) compiled for the host, unmodified, and run on a batch read from a file
// (tests/test_imm_cpu.py writes it and checks the result against the numpy restatement of tests/imm_util.py).  The kernel's shuffle loops
// over the members are restated here as the same ascending loops over an array of the bank's M lanes; its butterflies (the weights, the
// sums of the recursion) as the same tree over an array, as tests/cpp/bank_harness.cpp does.  TEST ONLY; the product has no CPU path.
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
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../quadrotor_landing_amd/csrc/ekf_imm.hpp"

using namespace qle;

static const int kPer = 16 + 225 + 2, kOut = 2 + 16 + 225;

// the butterfly of bank_sum / bank_max over an array: v[lane]
template <typename Op>
static void tree(std::vector<double>& v, int M, Op op)
{
    std::vector<double> t(v.size());
    for (int o = 1; o < M; o <<= 1) {
        t = v;
        for (int l = 0; l < M; ++l) v[l] = op(t[l], t[l ^ o]);
    }
    for (int l = 1; l < M; ++l)
        if (std::memcmp(&v[l], &v[0], sizeof(double)) != 0) { std::fprintf(stderr, "the lanes of a bank disagree\n"); std::exit(7); }
}
static double add(double a, double b) { return a + b; }
static double larger(double a, double b) { return b > a ? b : a; }

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
            for (int wd = 0; wd < W; ++wd) Pw[(size_t)l * W + wd] = words.a[wd] < 0 ? T(0) : (T)f[16 + words.a[wd] * 15 + words.b[wd]];
            lw[l] = f[241];
            valid[l] = bank_member_valid(xl, lw[l], f[242] != 0.0);
            lm[l] = valid[l] ? lw[l] : -INFINITY;
        }
        tree(lm, M, larger);
        for (int l = 0; l < M; ++l) ws[l] = wraw[l] = bank_weight_raw(valid[l], lw[l], lm[0]);
        tree(ws, M, add);
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
            for (int k = 0; k < 225; ++k) o[18 + k] = 0.0;
            for (int wd = 0; wd < W; ++wd) {
                if (words.a[wd] < 0) continue;
                const double v = store ? (double)(T)term[wd] : (double)Pw[(size_t)j * W + wd];
                o[18 + words.a[wd] * 15 + words.b[wd]] = o[18 + words.b[wd] * 15 + words.a[wd]] = v;
            }
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
        tree(tm, M, larger);
        for (int l = 0; l < M; ++l) e[l] = imm_update_exp(t[l], tm[0]);
        tree(e, M, add);
        for (int l = 0; l < M; ++l) out[g * M + l] = imm_update_final(ok[l], t[l], tm[0], e[0], logmu_min);
    }
}

static bool read_all(const char* path, std::vector<double>& d)
{
    FILE* fi = std::fopen(path, "rb");
    if (!fi) return false;
    std::fseek(fi, 0, SEEK_END);
    const long n = std::ftell(fi);
    std::fseek(fi, 0, SEEK_SET);
    d.resize((size_t)n / sizeof(double));
    const bool ok = std::fread(d.data(), sizeof(double), d.size(), fi) == d.size();
    std::fclose(fi);
    return ok;
}

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    std::vector<double> d, out;
    if (!read_all(argv[2], d) || d.size() < 4) return 3;
    int64_t B;
    if (std::strcmp(argv[1], "mix") == 0) {
        B = (int64_t)d[0];
        const int M = (int)d[3];
        if (!bank_members_ok(M) || B <= 0 || B % M != 0 || d.size() != 4 + (size_t)M * M + (size_t)B * kPer) return 9;
        const bool f64 = d[1] != 0, compact = d[2] != 0;
        const double* Pi = d.data() + 4;
        const double* in = Pi + M * M;
        out.resize((size_t)B * kOut);
        if (f64 && compact) mix<double, true>(Pi, in, B, M, out.data());
        else if (f64) mix<double, false>(Pi, in, B, M, out.data());
        else if (compact) mix<float, true>(Pi, in, B, M, out.data());
        else mix<float, false>(Pi, in, B, M, out.data());
    } else if (std::strcmp(argv[1], "update") == 0) {
        B = (int64_t)d[0];
        const int M = (int)d[1];
        if (!bank_members_ok(M) || B <= 0 || B % M != 0 || d.size() != 3 + (size_t)B * 3) return 9;
        out.resize((size_t)B);
        update(d.data() + 3, B, M, d[2], out.data());
    } else {
        return 2;
    }
    FILE* fo = std::fopen(argv[3], "wb");
    if (!fo || std::fwrite(out.data(), sizeof(double), out.size(), fo) != out.size()) return 6;
    std::fclose(fo);
    std::printf("%lld\n", (long long)B);
    return 0;
}
