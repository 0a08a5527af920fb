// bank_harness.cpp -- the arithmetic of k_bank_fuse (quadrotor_landing_amd/csrc/ekf_bank.hpp: bank_member_valid, bank_weight_raw,
// bank_diff, bank_fuse_state, bank_cov_term and the word table BankWords) compiled for the host, unmodified, and run on a batch read
// from a file (tests/test_bank_cpu.py writes it and checks the result against the numpy restatement of tests/bank_util.py).  The
// kernel's xor-butterflies are restated here as the same tree over an array of the bank's M lanes: stage o = 1, 2, ..., M/2 replaces
// v[l] by v[l] + v[l ^ o] in every lane, and every lane must end with the same bits (checked).  TEST ONLY; the product has no CPU path.
//
//   bank_harness <in> <out>
// in  (doubles): B, fp64, compact, M, then per filter x[16], P[15][15], logw, mask
// out (doubles): per filter w; then per bank best, x[16], P[15][15]
// A compact run is handed NaN in every covariance word a compact record does not hold: they must not matter (they come back 0).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../quadrotor_landing_amd/csrc/ekf_bank.hpp"

using namespace qle;

static const int kHdr = 4, kPer = 16 + 225 + 2, kBankOut = 1 + 16 + 225;

// the butterfly of bank_sum / bank_max / bank_min over an array: v[lane][k]
template <typename V, typename Op>
static void tree(std::vector<V>& v, int n, int M, Op op)
{
    std::vector<V> t(v.size());
    for (int o = 1; o < M; o <<= 1) {
        t = v;
        for (int l = 0; l < M; ++l)
            for (int k = 0; k < n; ++k) v[l * n + k] = op(t[l * n + k], t[(l ^ o) * n + k]);
    }
    for (int l = 1; l < M; ++l)
        if (std::memcmp(&v[l * n], &v[0], n * sizeof(V)) != 0) { std::fprintf(stderr, "the lanes of a bank disagree\n"); std::exit(7); }
}

template <typename T, bool COMPACT>
static void run(const double* in, int64_t B, int M, double* w_out, double* bank_out)
{
    constexpr BankWords<COMPACT> words{};
    constexpr int W = BankWords<COMPACT>::kWords;
    const auto add = [](double a, double b) { return a + b; };
    for (int64_t g = 0; g < B / M; ++g) {
        std::vector<T> x(M * 16), Pw((size_t)M * W);
        std::vector<double> lw(M), lm(M), ws(M), m(M * 15), c(M * 15), term((size_t)M * W);
        std::vector<int> ref(M);
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
        tree(lm, 1, M, [](double a, double b) { return b > a ? b : a; });
        for (int l = 0; l < M; ++l) ref[l] = valid[l] && lw[l] == lm[0] ? l : kBankMaxMembers;
        tree(ref, 1, M, [](int a, int b) { return b < a ? b : a; });
        const bool empty = ref[0] == kBankMaxMembers;
        std::vector<double> wraw(M);
        for (int l = 0; l < M; ++l) ws[l] = wraw[l] = bank_weight_raw(valid[l], lw[l], lm[0]);
        tree(ws, 1, M, add);
        T xr[16];
        for (int k = 0; k < 16; ++k) xr[k] = x[(empty ? 0 : ref[0]) * 16 + k];
        std::vector<double> w(M);
        for (int l = 0; l < M; ++l) {
            w[l] = empty ? 0.0 : wraw[l] / ws[0];
            w_out[g * M + l] = w[l];
            T xl[16], d[15];
            for (int k = 0; k < 16; ++k) xl[k] = x[l * 16 + k];
            bank_diff(xl, xr, d);
            for (int k = 0; k < 15; ++k) {
                c[l * 15 + k] = (double)d[k];
                m[l * 15 + k] = valid[l] ? w[l] * c[l * 15 + k] : 0.0;
            }
        }
        tree(m, 15, M, add);
        double mm[15];
        for (int k = 0; k < 15; ++k) mm[k] = m[k];
        T xf[16];
        bank_fuse_state(xr, mm, empty, xf);
        for (int l = 0; l < M; ++l)
            for (int k = 0; k < 15; ++k) c[l * 15 + k] = valid[l] ? c[l * 15 + k] - mm[k] : 0.0;
        for (int l = 0; l < M; ++l)
            for (int wd = 0; wd < W; ++wd)
                term[(size_t)l * W + wd] = words.a[wd] < 0 ? 0.0
                                                           : bank_cov_term(valid[l], w[l], (double)Pw[(size_t)l * W + wd], c[l * 15 + words.a[wd]], c[l * 15 + words.b[wd]]);
        tree(term, W, M, add);
        double* o = bank_out + g * kBankOut;
        o[0] = empty ? -1.0 : (double)(g * M + ref[0]);
        for (int k = 0; k < 16; ++k) o[1 + k] = (double)xf[k];
        for (int k = 0; k < 225; ++k) o[17 + k] = 0.0;
        for (int wd = 0; wd < W; ++wd) {
            if (words.a[wd] < 0) {
                if (term[wd] != 0.0) { std::fprintf(stderr, "a padding word is not zero\n"); std::exit(8); }
                continue;
            }
            const double v = (double)(T)term[wd];
            o[17 + words.a[wd] * 15 + words.b[wd]] = o[17 + words.b[wd] * 15 + words.a[wd]] = v;
        }
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
    const int M = (int)h[3];
    if (!bank_members_ok(M) || B <= 0 || B % M != 0) return 9;
    std::vector<double> d((size_t)B * kPer), out((size_t)B + (size_t)(B / M) * kBankOut);
    if (std::fread(d.data(), sizeof(double), d.size(), fi) != d.size()) return 5;
    std::fclose(fi);
    const bool f64 = h[1] != 0, compact = h[2] != 0;
    double* w = out.data();
    double* bank = out.data() + B;
    if (f64 && compact) run<double, true>(d.data(), B, M, w, bank);
    else if (f64) run<double, false>(d.data(), B, M, w, bank);
    else if (compact) run<float, true>(d.data(), B, M, w, bank);
    else run<float, false>(d.data(), B, M, w, bank);
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo || std::fwrite(out.data(), sizeof(double), out.size(), fo) != out.size()) return 6;
    std::fclose(fo);
    std::printf("%lld\n", (long long)B);
    return 0;
}
