// ekf_helper_kernels.hpp -- the cold kernels of the C ABI (ekf_capi.hip): fill and rebase of the per-filter counters, layout conversion
// between host rows and device tiles, seeding, reporting.  None of them is on the tick path.
#pragma once

#include "ekf_layout.hpp"

namespace qle {

template <typename I>   // a template only so that every translation unit may include this header
__global__ void k_fill_i32(I* __restrict__ dst, I v, int64_t B)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) dst[i] = v;
}

// Shift the tick origin: subtract `shift` from every filter's last-correction index so that the
// 32-bit tick arithmetic never wraps in a long-running service.  "Never / long ago" saturates.
template <typename I>
__global__ void k_rebase_ticks(I* __restrict__ last_corr, I shift, int64_t B)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    // saturate far in the past: such a filter has not corrected / has no history entry for longer than any
    // rate limit or ring capacity, which is all the consumers of these indices distinguish
    const int64_t v = (int64_t)last_corr[i] - shift;
    last_corr[i] = (int32_t)(v < -(int64_t)(1 << 30) ? -(int64_t)(1 << 30) : v);
}

// upds_since_correction (EKF.hpp:128) per filter from the implicit counter: ticks since the filter's last correction,
// 0 for a filter that is not initialised yet (the reference never advances it, EKF.cpp:129-130).
template <typename T>
__global__ void k_upds_since(const T* __restrict__ st, const int32_t* __restrict__ last_corr, int32_t tick, int32_t* __restrict__ out, int64_t B)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    bool init = false;
    for (int w = 6; w < 10; ++w) init |= st[word_off<T>(w, i, kSW)] != T(0);
    out[i] = init ? tick - 1 - last_corr[i] : 0;
}

// ------------------------------------------------ layout conversion kernels
// Host-facing AoS fp64 <-> device tiles, one chunk [i0, i0+n) of the batch per
// launch (the AoS side is a staging buffer holding only that chunk).  W words
// of the host row go to words [w0, w0+W) of the WT-word device record.
// Not on the hot path.
template <typename T>
__global__ void k_pack_off(const double* __restrict__ aos, int stride, int W, T* __restrict__ dst, int WT, int w0, int64_t i0, int64_t n)
{
    const int64_t li = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (li >= n) return;
    for (int w = 0; w < W; ++w) dst[word_off<T>(w0 + w, i0 + li, WT)] = (T)aos[li * stride + w];
}
template <typename T>
__global__ void k_unpack_off(const T* __restrict__ src, int stride, int W, double* __restrict__ aos, int WT, int w0, int64_t i0, int64_t n)
{
    const int64_t li = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (li >= n) return;
    for (int w = 0; w < W; ++w) aos[li * stride + w] = (double)src[word_off<T>(w0 + w, i0 + li, WT)];
}
// z (7) + mask -> 8-word record; z == nullptr writes an identity pose, mask == nullptr means "all".
template <typename T>
__global__ void k_pack_z_off(const double* __restrict__ z, const uint8_t* __restrict__ mask, T* __restrict__ dst, int64_t i0, int64_t n)
{
    const int64_t li = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (li >= n) return;
    for (int w = 0; w < 7; ++w) dst[word_off<T>(w, i0 + li, kZW)] = z ? (T)z[li * 7 + w] : (w == 6 ? T(1) : T(0));
    dst[word_off<T>(7, i0 + li, kZW)] = (mask == nullptr || mask[li]) ? T(1) : T(0);
}
template <typename T>
__global__ void k_unpack_z_off(const T* __restrict__ src, double* __restrict__ z, uint8_t* __restrict__ mask, int64_t i0, int64_t n)
{
    const int64_t li = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (li >= n) return;
    for (int w = 0; w < 7; ++w) z[li * 7 + w] = (double)src[word_off<T>(w, i0 + li, kZW)];
    mask[li] = src[word_off<T>(7, i0 + li, kZW)] != T(0) ? 1 : 0;
}
// Full n x n row-major covariance -> packed symmetric part (P + P^T)/2 of the state record.
template <typename T>
__global__ void k_pack_P_off(const double* __restrict__ Pf, int n, T* __restrict__ st, int64_t i0, int64_t m, int compact)
{
    const int64_t li = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (li >= m) return;
    const double* Pi = Pf + li * n * n;
    for (int a = 0; a < 15; ++a)
        for (int b = a; b < 15; ++b) {
            double v = (a < n && b < n) ? 0.5 * (Pi[a * n + b] + Pi[b * n + a]) : 0.0;
            const int w = p_word(a, b, compact != 0);
            if (w >= 0) st[word_off<T>(w, i0 + li, kSW)] = (T)v;
        }
}
template <typename T>
__global__ void k_unpack_P_off(const T* __restrict__ st, int n, double* __restrict__ Pf, int64_t i0, int64_t m, int compact)
{
    const int64_t li = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (li >= m) return;
    double* Pi = Pf + li * n * n;
    for (int a = 0; a < n; ++a)
        for (int b = 0; b < n; ++b) {
            const int w = a <= b ? p_word(a, b, compact != 0) : p_word(b, a, compact != 0);
            Pi[a * n + b] = w >= 0 ? (double)st[word_off<T>(w, i0 + li, kSW)] : 0.0;
        }
}

// The covariance part of every record from one layout to the other (a handle re-configured with the other est_bias, qle_set_params).
template <typename T>
__global__ void k_relayout_P(T* __restrict__ st, int from_compact, int to_compact, int64_t B)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    T P[kPW];
    load_P_any<T>(st, i, P, from_compact != 0);
    store_P_any<T>(st, i, P, to_compact != 0);
}

// initialize_state, EKF.cpp:305-344, one filter per lane, for the filters whose tag record's mask word is set
// (the node seeds a filter on ITS first detection, NODE.cpp:169-174).  A filter that was not initialised before starts
// its counters here: upds_since_correction = 0 (EKF.cpp:77), i.e. last_corr = tick - 1.  Every seeded filter restarts
// its multirate history with the single entry "state now" (EKF.cpp:337-339).
template <typename T>
__global__ void k_seed(DevParams<T> p, const T* __restrict__ zs, T* __restrict__ st, T cov0, T cov1, T cov2, T cov3, T cov4,
                       int reinit_bias, int32_t tick, int32_t* __restrict__ last_corr, int32_t* __restrict__ hist_first,
                       T* __restrict__ anchor, int64_t B)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    T zr[kZW], x[kXW], P[kPW];
    load_rec<T, kZW, 0, kZW>(zs, i, zr);
    if (zr[7] == T(0)) return;
    load_rec<T, kSW, 0, kXW>(st, i, x);
    const bool fresh = filter_uninitialised(x);
    T qct[4] = {zr[3], zr[4], zr[5], zr[6]}, t[4], qn[4], C[9], pv[3];
    quat_mul(p.q_vc, qct, t);                       // EKF.cpp:310
    qn[0] = -t[0]; qn[1] = -t[1]; qn[2] = -t[2]; qn[3] = t[3];
    quat_norm(qn);                                  // EKF.cpp:311
    quat_to_rot(qn, C);
#pragma unroll
    for (int k = 0; k < 3; ++k) pv[k] = (p.C_vc[3 * k] * zr[0] + p.C_vc[3 * k + 1] * zr[1] + p.C_vc[3 * k + 2] * zr[2]) + p.r_v_cv[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        x[k] = -(C[3 * k] * pv[0] + C[3 * k + 1] * pv[1] + C[3 * k + 2] * pv[2]);  // EKF.cpp:313
        x[3 + k] = T(0);                                                        // EKF.cpp:315
        if (reinit_bias) { x[10 + k] = T(0); x[13 + k] = T(0); }                // EKF.cpp:317-321
        x[10 + k] *= p.bias_on; x[13 + k] *= p.bias_on;
    }
    x[6] = qn[0]; x[7] = qn[1]; x[8] = qn[2]; x[9] = qn[3];
#pragma unroll
    for (int k = 0; k < kPW; ++k) P[k] = T(0);
#pragma unroll
    for (int k = 0; k < 3; ++k) {                                               // EKF.cpp:323
        P[sidx(k, k)] = cov0; P[sidx(3 + k, 3 + k)] = cov1; P[sidx(6 + k, 6 + k)] = cov2;
        P[sidx(9 + k, 9 + k)] = cov3; P[sidx(12 + k, 12 + k)] = cov4;
    }
    store_rec<T, kSW, 0, kXW>(st, i, x);
    store_P_any<T>(st, i, P, p.compact != 0);
    if (fresh && last_corr) last_corr[i] = tick - 1;
    if (hist_first) {   // multirate: the history is the single entry "state now" (EKF.cpp:337-339)
        hist_first[i] = tick - 1;
        store_rec<T, kSW, 0, kXW>(anchor, i, x);
        store_rec<T, kSW, kXW, kPW>(anchor, i, P);
    }
}

// What the node publishes after a tick (NODE.cpp:192-220), AoS fp64, one chunk.
template <typename T>
__global__ void k_report_off(DevParams<T> p, const T* __restrict__ st, const T* __restrict__ pfp, double* __restrict__ pose,
                             double* __restrict__ pose_cov, double* __restrict__ vel, double* __restrict__ bias, int64_t i0, int64_t n)
{
    const int64_t li = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (li >= n) return;
    const int64_t i = i0 + li;
    auto X = [&](int w) { return (double)st[word_off<T>(w, i, kSW)]; };
    for (int k = 0; k < 3; ++k) pose[li * 7 + k] = X(k);
    for (int k = 0; k < 4; ++k) pose[li * 7 + 3 + k] = X(6 + k);
    {  // rows/cols {0-2, 6-8}, row-major (NODE.cpp:203-210)
        const int sel[6] = {0, 1, 2, 6, 7, 8};
        for (int a = 0; a < 6; ++a)
            for (int b = 0; b < 6; ++b)
                pose_cov[li * 36 + a * 6 + b] = X(sel[a] <= sel[b] ? p_word(sel[a], sel[b], p.compact != 0) : p_word(sel[b], sel[a], p.compact != 0));
    }
    for (int k = 0; k < 3; ++k) vel[li * 3 + k] = X(3 + k);
    for (int k = 0; k < 3; ++k) {  // ab_nom + ab_static, wb_nom + wb_static (NODE.cpp:215-220)
        double as = pfp ? (double)pfp[word_off<T>(12 + k, i, kFW)] : (double)p.ab_static[k];
        double ws = pfp ? (double)pfp[word_off<T>(15 + k, i, kFW)] : (double)p.wb_static[k];
        bias[li * 6 + k] = X(10 + k) + as;
        bias[li * 6 + 3 + k] = X(13 + k) + ws;
    }
}

template <typename T>
__global__ void k_count_nonfinite(const T* __restrict__ st, unsigned long long* __restrict__ out, int64_t B, int record_words)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    bool bad = false;
    for (int w = 0; w < record_words; ++w) bad |= !isfinite((double)st[word_off<T>(w, i, kSW)]);   // the words a tick reads (64 in compact records)
    if (bad) atomicAdd(out, 1ULL);
}

}  // namespace qle
