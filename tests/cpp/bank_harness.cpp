// bank_harness.cpp -- the arithmetic of k_bank_fuse (quadrotor_landing_amd/csrc/ekf_bank.hpp: bank_member_valid, bank_weight_raw,
// bank_diff, bank_fuse_state, bank_cov_term and the word table BankWords) compiled for the host, unmodified, and run on a batch read
// from a file (tests/test_bank_cpu.py writes it and checks the result against the numpy restatement of tests/bank_util.py).  The
// kernel's xor-butterflies are restated as the same tree over an array of the bank's M lanes (tests/cpp/bank_lanes.hpp): stage
// o = 1, 2, ..., M/2 replaces v[l] by v[l] + v[l ^ o] in every lane, and every lane must end with the same bits (checked).  TEST ONLY;
// the product has no CPU path.
//
//   bank_harness <in> <out>
// in  (doubles): B, fp64, compact, M, then per filter x[16], P[15][15], logw, mask
// out (doubles): per filter w; then per bank best, x[16], P[15][15]
// A compact run is handed NaN in every covariance word a compact record does not hold: they must not matter (they come back 0).
#include <cmath>

#include "bank_lanes.hpp"

using namespace qle;

static const int kHdr = 4, kPer = 16 + 225 + 2, kBankOut = 1 + 16 + 225;

template <typename T, bool COMPACT>
static void run(const double* in, int64_t B, int M, double* w_out, double* bank_out)
{
    constexpr BankWords<COMPACT> words{};
    constexpr int W = BankWords<COMPACT>::kWords;
    for (int64_t g = 0; g < B / M; ++g) {
        std::vector<T> x(M * 16), Pw((size_t)M * W);
        std::vector<double> lw(M), lm(M), ws(M), m(M * 15), c(M * 15), term((size_t)M * W);
        std::vector<int> ref(M);
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
        for (int wd = 0; wd < W; ++wd)
            if (words.a[wd] < 0 && term[wd] != 0.0) { std::fprintf(stderr, "a padding word is not zero\n"); std::exit(8); }
        double* o = bank_out + g * kBankOut;
        o[0] = empty ? -1.0 : (double)(g * M + ref[0]);
        for (int k = 0; k < 16; ++k) o[1 + k] = (double)xf[k];
        P_from_words<COMPACT>(o + 17, [&](int wd) { return (double)(T)term[wd]; });
    }
}

int main(int argc, char** argv)
{
    const auto check = [](const double* h) { return !bank_members_ok((int)h[3]) || (int64_t)h[0] <= 0 || (int64_t)h[0] % (int)h[3] != 0 ? 9 : 0; };
    const auto out_size = [](const double* h) { return (size_t)h[0] + (size_t)((int64_t)h[0] / (int)h[3]) * kBankOut; };
    return harness_main(argc, argv, kHdr, check, per_filter(kPer), out_size, [](const double* h, const double* d, double* out) {
        const int64_t B = (int64_t)h[0];
        by_dtype(h[1] != 0, [&](auto t) {
            by_flags(h[2] != 0, [&](auto compact) { run<decltype(t), decltype(compact)::value>(d, B, (int)h[3], out, out + B); });
        });
    });
}
