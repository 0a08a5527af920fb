// harness_io.hpp -- what the file-protocol harnesses of tests/cpp share (pregate, consistency, health, lookahead, score, bank, imm): the
// file reading and writing with its exit statuses, the decode of the shared filter parameters, the per-filter noise, and the dispatch
// from run-time header words to template arguments.  It includes ekf_device.hpp alone, the header every one of the seven product
// headers under test starts from; what is particular to the banks is in bank_lanes.hpp.  TEST ONLY.
#pragma once
#include <cstdint>
#include <cstdio>
#include <type_traits>
#include <vector>

#include "../../quadrotor_landing_amd/csrc/ekf_device.hpp"

// <program> <in> <out>: reads kHdr doubles h, refuses with check(h) when that is not 0 (a harness's own statuses 7, 8, 9), reads
// payload_size(h) doubles d to the end of the file, calls run(h, d, out) on out_size(h) doubles, writes them and prints h[0], the batch.
// Exit status: 2 usage, 3 open, 4 header, 5 payload, 6 write.
template <typename Check, typename PayloadSize, typename OutSize, typename Run>
static int harness_main(int argc, char** argv, int kHdr, Check check, PayloadSize payload_size, OutSize out_size, Run run)
{
    if (argc != 3) return 2;
    FILE* fi = std::fopen(argv[1], "rb");
    if (!fi) return 3;
    std::vector<double> h(kHdr);
    if (std::fread(h.data(), sizeof(double), h.size(), fi) != h.size()) return 4;
    if (const int refused = check(h.data())) return refused;
    std::vector<double> d(payload_size(h.data())), out(out_size(h.data()));
    if (std::fread(d.data(), sizeof(double), d.size(), fi) != d.size() || std::fgetc(fi) != EOF) return 5;
    std::fclose(fi);
    run(h.data(), d.data(), out.data());
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo || std::fwrite(out.data(), sizeof(double), out.size(), fo) != out.size()) return 6;
    std::fclose(fo);
    std::printf("%lld\n", (long long)h[0]);
    return 0;
}
static int no_check(const double*) { return 0; }
static auto per_filter(int words) { return [words](const double* h) { return (size_t)h[0] * words; }; }   // a size: h[0] x words

// dT, dTw, bias_on, small_ang_tol, g[3], q_vc[4], C_vc[9], r_v_cv[3], Q[12], R[6], ab_static[3], wb_static[3]: the 47 doubles, in this
// order, that params_header of tests/host_harness.py writes.  q is left behind the last of them.
template <typename T>
static qle::DevParams<T> decode_params(const double*& q, int compact)
{
    qle::DevParams<T> p;
    const auto take = [&q](T* dst, int n) { for (int k = 0; k < n; ++k) dst[k] = (T)*q++; };
    take(&p.dT, 1); take(&p.dTw, 1); take(&p.bias_on, 1); take(&p.small_ang_tol, 1);
    take(p.g, 3); take(p.q_vc, 4); take(p.C_vc, 9); take(p.r_v_cv, 3); take(p.Q, 12); take(p.R, 6); take(p.ab_static, 3); take(p.wb_static, 3);
    p.compact = compact;
    return p;
}

// the noise a filter's tick uses: its own 24 words pfp (Q[12], ab_static[3], wb_static[3], R[6]) or the shared ones of p
template <typename T>
static qle::Noise<T> noise_from(const qle::DevParams<T>& p, const double* pfp, bool use_pfp)
{
    qle::Noise<T> nz;
    for (int k = 0; k < 12; ++k) nz.Q[k] = use_pfp ? (T)pfp[k] : p.Q[k];
    for (int k = 0; k < 3; ++k) { nz.ab_static[k] = use_pfp ? (T)pfp[12 + k] : p.ab_static[k]; nz.wb_static[k] = use_pfp ? (T)pfp[15 + k] : p.wb_static[k]; }
    for (int k = 0; k < 6; ++k) nz.R[k] = use_pfp ? (T)pfp[18 + k] : p.R[k];
    return nz;
}

// f(T()) with T = double or float; f(A) or f(A, B) with std::true_type / std::false_type for one or two booleans: inside f,
// decltype(A)::value is a template argument
template <typename F>
static void by_dtype(bool f64, F f)
{
    if (f64) f(double());
    else f(float());
}
template <typename F>
static void by_flags(bool a, F f)
{
    if (a) f(std::true_type());
    else f(std::false_type());
}
template <typename F>
static void by_flags(bool a, bool b, F f)
{
    by_flags(a, [&](auto A) { by_flags(b, [&](auto B) { f(A, B); }); });
}
