// ekf_multirate.hpp -- the multirate tick that carries tag poses: k_step_mr and its history addressing (gfx950).
#pragma once

#include "ekf_cov_home.hpp"
#include "ekf_gate.hpp"
#include "ekf_layout.hpp"
#include "ekf_stamps.hpp"

namespace qle {

// ------------------------------------------------------------ multirate EKF
// filter_update with multirate_ekf = true (EKF.cpp:196-236, 251-264): a tag pose that was taken `step` ticks ago is fused
// into the state the filter held THEN, and the predictions since are replayed with the stored IMU samples.
//
// History.  The reference keeps per-filter vectors x_hist / u_hist / P_hist (EKF.hpp:62-64) with one entry per tick; only
// the entry `step` ticks back (at most step_max) and its successors are ever read again, and after a correction the history
// starts at the corrected entry (the trim of EKF.cpp:214-219).  "State after tick t" is a pure function of an earlier state of
// the same chain and the IMU samples in between, so the engine stores
//   cur      the state after the newest tick, in place (one record array, cache-resident exactly like the single-rate filter);
//   u ring   the IMU sample of every tick, slot t % Cu (8 words per filter and tick);
//   ckpt     a copy of the state after every k-th tick, slot (t/k) % Nc (Cu = k Nc >= step_max + k + 1);
//   anchor   per filter the corrected entry of its last correction (tick hist_first[i]) -- the start of its history;
//   extra    one more checkpoint slot (index Nc) that the host places where it expects the NEXT measurement's entry: tag poses come at
//            a regular cadence with a near-constant latency, so after a correcting tick n the next entry will be about
//            n + (ticks between the last two correcting ticks) - (nominal step delay); the predict launch of that tick copies the state
//            there as well.  A filter whose entry is at or just after it starts from it and replays nothing (or a tick or two) instead of
//            (k-1)/2 ticks from the grid; a filter it does not fit (another phase, an early pose) never looks at it;
// and rebuilds the entry a measurement belongs to by replaying at most k-1 predictions from the newest checkpoint in
// (hist_first, mt], or from the anchor.  The replay towards "now" rewrites the checkpoints it passes, so every checkpoint
// newer than hist_first always holds the current chain.  Same arithmetic on the same stored samples as the reference's
// rewritten history entries, hence the same values; a predict-only tick costs 8 + 136/k extra words instead of a second copy
// of the state, and the history of 65 536 fp32 filters at 400 Hz with a 200 ms window is 0.75 GB instead of 6 GB.
__host__ __device__ inline int32_t floor_div(int32_t a, int32_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
template <typename T>
__device__ __forceinline__ T* mr_u_slot(T* uring, const MrParams& m, int32_t tick)
{
    int32_t s = tick % m.Cu;
    if (s < 0) s += m.Cu;
    return uring + (int64_t)s * m.u_words;
}
template <typename T>
__device__ __forceinline__ T* mr_ck_slot(T* ckpt, const MrParams& m, int32_t tick)   // tick is a multiple of k, >= 0
{
    return ckpt + (int64_t)((tick / m.k) % m.Nc) * m.slot_words;
}

__device__ __forceinline__ int32_t wave_max_i32(int32_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int32_t o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return __builtin_amdgcn_readfirstlane(v);
}
// Minimum of a value over the 64 lanes of the wave, as a wave-uniform (SGPR) value.  Every lane must be active.
__device__ __forceinline__ int32_t wave_min_i32(int32_t v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int32_t o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return __builtin_amdgcn_readfirstlane(v);
}

// The stored IMU sample of tick ts (wave-uniform) into dst: from the ring, or -- the current tick's own -- from the input record; a tick
// beyond the current one has none.
template <typename T>
__device__ __forceinline__ void mr_request_sample(const MrParams& m, T* uring, const T* __restrict__ us, int64_t i, int32_t ts, T (&dst)[kUW])
{
    if (ts < m.tick) {
        T ur[kHW];
        load_rec<T, kHW, 0, kHW>(mr_u_slot(uring, m, ts), i, ur);
#pragma unroll
        for (int k = 0; k < kUW; ++k) dst[k] = ur[k];
    } else if (ts == m.tick) {
        T uc[kUW];
        load_rec<T, kUW, 0, kUW>(us, i, uc);
#pragma unroll
        for (int k = 0; k < kUW; ++k) dst[k] = uc[k];
    }
}

// A multirate tick that carries tag poses.  Lanes that correct: load the newest checkpoint at or before the entry the
// measurement belongs to (or the anchor), replay up to that entry, fuse the measurement there (the corrected entry becomes the
// anchor), replay the predictions up to n-1 from the stored IMU samples -- rewriting the checkpoints on the way -- then predict
// tick n.  Lanes that do not: plain predict of `cur`.
//
// The covariance stays in registers for the whole chain (12-35 predictions), so the kernel is bound by the number of instructions per
// replayed tick, not by bytes (profiles/r02_tuning.md section 10): the chain runs on the register-block form of ekf_packed.hpp
// (packed fp32 FMAs, no libm call per tick), and the loop counter is WAVE-UNIFORM -- the wave walks from the earliest entry any of its
// lanes starts from, a lane joins at its own entry -- so that the history addresses (IMU ring slot, checkpoint slot) are scalar and
// the "is this the current tick" selects are scalar branches.  One predict call site serves the replay and the current tick.
template <typename T, bool DIRECT, bool PFP>
__global__ __launch_bounds__(kBlock) void k_step_mr(T* cur, const T* __restrict__ us, const T* __restrict__ zs, int64_t B, int32_t grid_x, int32_t block_x,
                                                    int32_t* __restrict__ hist_first, T* uring,   // (argument order: see k_predict; the first loads need these 14 dwords)
                                                    T* ckpt, T* anchor, const T* __restrict__ pfp,
                                                    const double* __restrict__ stamp, T* __restrict__ aux_accel, T* __restrict__ aux_obs,
                                                    int32_t* __restrict__ last_corr, uint8_t* __restrict__ flags,
                                                    double* __restrict__ delay_out, DevParams<T> p, GateParams gp, MrParams m)
{
    args_early(cur, us, zs, B, grid_x, block_x, hist_first, uring, ckpt, anchor);
    const int64_t i = batch_block((unsigned)grid_x) * block_x + threadIdx.x;
    if ((i & ~(int64_t)63) >= B) return;             // the whole wave lies beyond the batch (wave-uniform)
    // from here on all 64 lanes stay active (the record arrays are allocated in whole tiles; a lane beyond B sees a zeroed,
    // i.e. not initialised, filter and never touches the per-filter scalar arrays)
    T x[kXW], u[kUW], accel[3] = {T(0), T(0), T(0)};
    QLE_STAMP(0, (T)(i & 63));
    load_rec<T, kUW, 0, kUW>(us, i, u);
    Noise<T> nz;
    load_noise<T, PFP>(p, pfp, i, nz);
    T zr[kZW];
    load_rec<T, kZW, 0, kZW>(zs, i, zr);
    load_rec<T, kSW, 0, kXW>(cur, i, x);
    // the per-filter history indices are requested with the records above, not after them (they depend on nothing but i)
    const int32_t first_i = i < B ? hist_first[i] : 0;
    const int32_t lastc_i = (m.gate && i < B) ? last_corr[i] : 0;
    QLE_STAMP(1, x[9] + zr[7] + u[5]);
    const bool valid = i < B && !filter_uninitialised(x);   // EKF.cpp:129-130
    bool corr = valid && zr[7] != T(0);
    if (m.gate && valid) {  // EKF.cpp:147-186
        const bool consume = corr && (!gp.limit || (gp.tick - lastc_i) >= gp.upd_per_meas);
        bool ok = consume;
        if (consume && gp.corner_enbl) {
            const double zd[7] = {(double)zr[0], (double)zr[1], (double)zr[2], (double)zr[3], (double)zr[4], (double)zr[5], (double)zr[6]};
            ok = corner_gate(gp, zd);
        }
        corr = ok;
        if (ok) last_corr[i] = gp.tick;
        flags[i] = (uint8_t)((ok ? 1 : 0) | (consume ? 2 : 0));
    }
    int32_t start = m.tick - 1, mt = 0;    // entry the chain starts from; tick the measurement belongs to (if corr)
    const T* sp = cur;
    if (corr) {
        // EKF.cpp:199-201: delay -> step delay -> history entry the measurement belongs to
        int32_t step = m.fixed_step;
        if (m.dynamic) {
            const double age = stamp ? (m.t_curr - stamp[i]) : m.uniform_age;
            const double dcur = fmin(age + m.offset, m.delay_max);
            delay_out[i] = dcur;
            step = (int32_t)(dcur / m.dT + 0.5);
            if (step < 1) step = 1;
        }
        const int32_t first = first_i;
        const int32_t len = m.tick - first;    // entries first .. n-1
        int32_t ind = len - step;
        if (ind < 0) ind = 0;
        mt = first + ind;
        const int32_t c0 = floor_div(mt, m.k) * m.k;   // newest checkpoint tick <= mt
        if (c0 > first) { start = c0; sp = mr_ck_slot(ckpt, m, c0); }
        else { start = first; sp = anchor; }
        // the extra checkpoint, written where the host expected this measurement's entry (a regular cadence: no pre-replay at all)
        if (m.e_tick > start && m.e_tick <= mt) { start = m.e_tick; sp = ckpt + (int64_t)m.Nc * m.slot_words; }
        hist_first[i] = mt;                    // EKF.cpp:214-219
    }
    const int32_t t_lo = wave_min_i32(valid ? start : 0x7fffffff);
    if (t_lo == 0x7fffffff) return;            // no initialised filter in this wave (wave-uniform)
    QLE_STAMP(2, (T)start);
    // The correction of one lane at the entry its measurement belongs to (EKF.cpp:202-211): fuse, then the corrected entry is the anchor.
    auto emit = [&](const T (&o)[7]) {                    // EKF.cpp:209
        if (aux_accel) {
#pragma unroll
            for (int k = 0; k < 7; ++k) aux_obs[i * 7 + k] = o[k];
        }
    };
    auto new_anchor = [&](auto&& store_cov_to) {          // EKF.cpp:210-211: the history now starts here
        store_rec<T, kSW, 0, kXW, 2>(anchor, i, x);
        store_cov_to(anchor, i);
    };
    MrChain<T> S;
    S.init();
    auto correct_chain = [&]() {
        T z[7];
        if constexpr (sizeof(T) == 8) {   // fp64: the tag pose is read again here instead of occupying 16 registers through the pre-replay
            T zq[kZW];
            load_rec<T, kZW, 0, kZW>(zs, i, zq);
#pragma unroll
            for (int k = 0; k < 7; ++k) z[k] = zq[k];
        } else {
#pragma unroll
            for (int k = 0; k < 7; ++k) z[k] = zr[k];
        }
        if constexpr (sizeof(T) == 8 && PFP) load_noise<T, PFP>(p, pfp, i, nz);
        S.template correct<DIRECT>(p, nz, x, z, emit, new_anchor);
    };
    // fp32, regular cadence: every lane's chain starts AT its measurement's entry (the extra checkpoint).  The correction then runs on the
    // loaded triangle directly -- its scalar chains (innovation, R_k) under the tail of the 36 MB load, no pack / unpack round trip through
    // the register blocks in front of it -- and the loop below finds nothing left to correct (wave-uniform choice).
    // The IMU sample of the next replayed tick is requested one tick ahead (wave-uniform slot addresses), the first in front of the
    // correction: one step of arithmetic (~1.8 us) covers the latency of the ring, which was streamed to HBM.  Deeper queues (the idea: a
    // sample requested behind the 36 / 72 MB of anchor stores is not delivered before they have drained) measured no gain at 2 / 3 / 4
    // ticks ahead (profiles/r04_tuning.md section 8), and requesting the whole window up front (LDS-DMA, profiles/r03_tuning.md) made the
    // prologue 15 000 cycles longer.
    // A sample index beyond the current tick has no request; the current tick's own sample comes from `us` (it is asked for again here so
    // that it is not carried in registers through the whole replay).
    T un0[kUW];
    auto request_sample = [&](int32_t ts, T (&dst)[kUW]) { mr_request_sample<T>(m, uring, us, i, ts, dst); };   // ts is wave-uniform
    request_sample(t_lo + 1, un0);
    bool early = false;
    if (sp != cur) load_rec<T, kSW, 0, kXW>(sp, i, x);
    if constexpr (sizeof(T) == 4) {
        T P[kPW];
        load_rec<T, kSW, kXW, kPW>(sp, i, P);
        early = __ballot(valid && !(corr && start == mt)) == 0;
        if (early && corr) {
            QLE_STAMP(5, x[0]);
            const T z[7] = {zr[0], zr[1], zr[2], zr[3], zr[4], zr[5], zr[6]};
            ekf_update_emit<T, DIRECT>(p, nz, x, P, z, emit);
            new_anchor([&](T* __restrict__ dst, int64_t ii) { store_rec<T, kSW, kXW, kPW, 2>(dst, ii, P); });
            QLE_STAMP(6, x[0]);
        }
        S.from_flat(P);
        QLE_STAMP(3, P[0] + P[119] + x[0]);
    } else {
        S.load_cov(sp, i);
        QLE_STAMP(3, S.probe() + x[0]);
    }
    // The chain.  Two copies of the loop: the first runs up to the last entry any lane of the wave corrects at (wave-uniform t_cmax) with
    // the correction inside; the second takes the rest -- after that tick nothing of the correction (the tag pose, R, its temporaries) is
    // live across the replayed ticks, which is what the 256-VGPR kernel is short of.  On a regular cadence (`early`) the first has nothing to do.
    int32_t t = t_lo;                          // wave-uniform
    int dbg_j = 0;
    (void)dbg_j;
    auto chain = [&](auto corr_in_loop, int32_t t_stop) {
    for (;;) {
        if constexpr (decltype(corr_in_loop)::value) {
            if (corr && t == mt) {                            // the entry the measurement belongs to
                QLE_STAMP(5, x[0]);
                correct_chain();
                QLE_STAMP(6, x[0]);
            }
        }
        if (t == t_stop) break;
        ++t;                                                  // EKF.cpp:222-226, then :249
        const bool now = t == m.tick;                         // wave-uniform
        T u6[kUW];
#pragma unroll
        for (int k = 0; k < kUW; ++k) u6[k] = un0[k];
        QLE_STAMP(8 + 2 * dbg_j, u6[0] + u6[5]);
        request_sample(t + 1, un0);
        if (valid && t > start) {
            if constexpr (sizeof(T) == 8 && PFP) load_noise<T, PFP>(p, pfp, i, nz);   // fp64: 24 values read again (L2) rather than 48 registers held through the loop
            S.predict(p, nz, x, u6, accel);
            QLE_STAMP(9 + 2 * dbg_j, x[0] + x[9] + S.probe());
            const bool extra = t == m.e_tick;                 // wave-uniform
            const bool ck = (t % m.k == 0 || extra) && (now || (corr && t > mt));   // checkpoints of the rewritten part of the chain
            if constexpr (sizeof(T) == 4) {
                if (now || ck) {
                    S.template with_flat<false>([&](const T (&P)[kPW]) {
                        if (now) {
                            store_rec<T, kSW, 0, kXW>(cur, i, x);
                            store_rec<T, kSW, kXW, kPW>(cur, i, P);
                        }
                        if (ck) {
                            T* ckp = extra ? ckpt + (int64_t)m.Nc * m.slot_words : mr_ck_slot(ckpt, m, t);
                            store_rec<T, kSW, 0, kXW, 2>(ckp, i, x);
                            store_rec<T, kSW, kXW, kPW, 2>(ckp, i, P);
                        }
                    });
                }
            } else {
                if (now) {
                    store_rec<T, kSW, 0, kXW>(cur, i, x);
                    S.template store_cov<0>(cur, i);
                }
                if (ck) {
                    T* ckp = extra ? ckpt + (int64_t)m.Nc * m.slot_words : mr_ck_slot(ckpt, m, t);
                    store_rec<T, kSW, 0, kXW, 2>(ckp, i, x);
                    S.template store_cov<2>(ckp, i);
                }
            }
            if (now) {
                const T uk[kHW] = {u6[0], u6[1], u6[2], u6[3], u6[4], u6[5], T(0), T(0)};
                store_rec<T, kHW, 0, kHW, kRingStorePolicy>(mr_u_slot(uring, m, t), i, uk);   // EKF.cpp:254-256
            }
        }
#ifdef QLE_MR_STAMPS
        ++dbg_j;
#endif
    }
    };
    {
        const int32_t t_cmax = early ? (int32_t)0x80000000 : wave_max_i32(corr ? mt : (int32_t)0x80000000);
        if (t_cmax >= t_lo) chain(std::true_type{}, t_cmax);       // mt >= start >= t_lo for every correcting lane
        chain(std::false_type{}, m.tick);
    }
    QLE_STAMP(7, x[0]);
    if (aux_accel && valid) {
#pragma unroll
        for (int k = 0; k < 3; ++k) aux_accel[i * 3 + k] = accel[k];
    }
}

}  // namespace qle
