// ekf_kernels.hpp -- the one-lane-per-filter tick kernels of the batched EKF engine (gfx950): k_predict, k_step, k_update and the
// on-chip-resident k_run_resident.  One lane owns one filter; x and P live in VGPRs for the whole tick and the state record
// (ekf_layout.hpp) is updated in place.
#pragma once

#include "ekf_cov_home.hpp"
#include "ekf_fused.hpp"
#include "ekf_gate.hpp"
#include "ekf_layout.hpp"

namespace qle {

// Minimum waves per SIMD the predict kernel is compiled for (register budget 512/waves).
// Measured on MI355X (profiles/r01_sweep.md): forcing two waves for fp32 costs 16 spilled VGPRs
// (68 B/lane of scratch traffic) and is slower at every batch size, so it is one for both dtypes.
constexpr int kPredictWaves = 1;

// ------------------------------------------------------------- hot kernels
// Predict tick: reads x16 + P120 + u6, writes x16 + P120 (278 words/filter).
// Packed P (sidx in ekf_device.hpp): the words of block-row r come first, then v, th, ab, wb.
// Loads are issued bottom-up and each block-row of the new P is stored as soon as it is final
// (ekf_predict_levels), so the stores overlap the loads of the rows above inside the one wave a
// SIMD holds at B = 65 536.
// `src` is the state at tick n-1, `dst` the state at tick n: the same array (in place: every load of a lane is issued
// before its first store).  MR (multirate filter): the tick also appends to the history -- the IMU sample goes to its slot
// of the IMU ring (hist_u, EKF.cpp:254-256) and on checkpoint ticks the new state is copied to its checkpoint slot
// (hist_ck != nullptr, wave-uniform); see k_step_mr for the history scheme.
template <typename T, bool PFP, int NT, bool MR, bool COMPACT = false, bool LF = false>
__device__ __forceinline__ void predict_tick(const DevParams<T>& p, const T* src, T* dst, const T* __restrict__ us,
                                             const T* __restrict__ pfp, T* __restrict__ aux_accel, T* __restrict__ hist_u,
                                             T* __restrict__ hist_ck, bool ck_cached, int64_t i)
{
    T x[kXW], P[kPW], u[kUW], accel[3];
    load_rec<T, kUW, 0, kUW, NT>(us, i, u);
    load_rec<T, kSW, 0, kXW, NT>(src, i, x);
    Noise<T> nz;
    load_noise<T, PFP>(p, pfp, i, nz);
    constexpr int VW = Quad<T>::VW;
    constexpr int NQ = kPW / VW;
    if constexpr (COMPACT) load_P_compact<T, NT>(src, i, P);
    else load_P_quads_desc<T, 0, NQ, NT>(src, i, P);
    // Every load of the tick is requested before the first instruction that needs one of them: left alone the scheduler issued ten of
    // the 36 record loads, waited for x and u, ran the first dozen instructions of the nominal predict (they feed the wave-uniform
    // branch of the half-angle series that ends the block) and only then requested the other 26 quads of the covariance -- one memory
    // round trip later.  LF is chosen per launch (tu_predict.hip): +1 % where every SIMD holds ONE wave (65 536 filters: 9.39 -> 9.30 us),
    // nothing below, and -3 % with two waves per SIMD (131 072: 20.8 -> 21.4 us), where the staggered requests are the gentler pattern
    // for the caches (profiles/r04_tuning.md section 10).
    // (nothing is scheduled across the barrier: the loads in front of it are all issued before the arithmetic behind it starts)
    if constexpr (LF) __builtin_amdgcn_sched_barrier(0);
    // A filter that is not initialised is left untouched.  No early exit: the compiler would sink the covariance loads below such a
    // branch and every wave would wait for x before it even issues them (+1 us per tick at 65 536 filters, profiles/r02_tuning.md).
    // Instead the lane computes on (with a unit quaternion, so that its arithmetic stays finite) and only its stores are masked.
    const bool dead = filter_uninitialised(x);
    if (dead) x[9] = T(1);
    T Pn[kPW];
    // a quad is final once every word in it is: first quad that holds only block-rows >= ab / th / v (ekf_device.hpp)
    constexpr int q_ab = level_first_word(3, VW) / VW, q_th = level_first_word(2, VW) / VW, q_v = level_first_word(1, VW) / VW;
    // the words that are final after `level` (-1: the nominal state) into the record array `to` under cache policy `nt`
    auto store_level = [&](T* to, auto nt, int level) {
        constexpr int POL = decltype(nt)::value;
        if (level == -1) store_rec<T, kSW, 0, kXW, POL>(to, i, x);
        else if (level == 0) store_P_quads_desc<T, q_ab, NQ, POL>(to, i, Pn);
        else if (level == 1) store_P_quads_desc<T, q_th, q_ab, POL>(to, i, Pn);
        else if (level == 2) store_P_quads_desc<T, q_v, q_th, POL>(to, i, Pn);
        else store_P_quads_desc<T, 0, q_v, POL>(to, i, Pn);
    };
    ekf_predict_levels<T>(p, nz, x, P, u, accel, Pn, [&](int level) {
        if (dead) return;
        if (COMPACT && level != -1) { if (level == 3) store_P_compact<T, NT>(dst, i, Pn); }
        else store_level(dst, std::integral_constant<int, NT>{}, level);
        if (MR && hist_ck) {
            // checkpoint copy of the same words: a grid checkpoint is streamed past the caches (it is rarely read again); the extra
            // checkpoint at the expected entry of the next tag pose is read back a dozen ticks later and is written CACHED, so that it
            // waits in the Infinity Cache next to the state (wave-uniform choice)
            if (ck_cached) store_level(hist_ck, std::integral_constant<int, 0>{}, level);
            else store_level(hist_ck, std::integral_constant<int, 2>{}, level);
        }
    });
    if (dead) return;
    if (MR) {
        const T uk[kHW] = {u[0], u[1], u[2], u[3], u[4], u[5], T(0), T(0)};
        store_rec<T, kHW, 0, kHW, kRingStorePolicy>(hist_u, i, uk);
    }
    if (aux_accel) {  // optional side output (wave-uniform), AoS [B][3] in the compute dtype
#pragma unroll
        for (int k = 0; k < 3; ++k) aux_accel[i * 3 + k] = accel[k];
    }
}

template <typename T, bool PFP, int NT, bool MR, bool COMPACT = false, bool LF = false>
__global__ __launch_bounds__(kBlock, kPredictWaves) void k_predict(const T* src, T* dst, const T* __restrict__ us, int64_t B, int64_t i0,
                                                       int32_t grid_x, int32_t block_x, int32_t split, int32_t ck_cached,
                                                       const T* __restrict__ pfp, T* __restrict__ aux_accel, T* __restrict__ hist_u,
                                                       T* __restrict__ hist_ck, DevParams<T> p)
{
    // Argument order: what the first loads depend on comes first, 14 dwords of it, so that the wave finds them in its SGPRs when it starts
    // (the translation units are built with -amdgpu-kernarg-preload-count; grid and block size are passed explicitly because the
    // hidden arguments are not among the preloaded ones) instead of fetching them from the kernel-argument segment -- a memory round
    // trip in front of every launch's first load.  The parameter block, needed when the first data arrive, comes last.
    args_early(src, dst, us, B, i0, grid_x, block_x);
    const int64_t i = i0 + batch_block((unsigned)grid_x) * block_x + threadIdx.x;   // i0: first filter of this launch (the launchers pass 0)
    if (i >= B) return;
    with_policy<NT>(split, [&](auto nt) {
        predict_tick<T, PFP, decltype(nt)::value, MR, COMPACT, LF>(p, src, dst, us, pfp, aux_accel, hist_u, hist_ck, ck_cached != 0, i);
    });
}

// The nominal state of a lane in / out of its column of an LDS array (step_tick: fp64 keeps x there during the covariance sweep).
template <typename T, bool ON, bool LOAD>
struct LdsPark {
    static constexpr bool parked = ON;
    T (*slot)[ON ? kBlock : 1];
    __device__ __forceinline__ void operator()(T (&xx)[kXW]) const
    {
        if constexpr (ON) {
#pragma unroll
            for (int k = 0; k < kXW; ++k) {
                if (LOAD) xx[k] = slot[k][threadIdx.x];
                else slot[k][threadIdx.x] = xx[k];
            }
        }
    }
};

// Fused tick (filter_update single-rate branch, EKF.cpp:238-249,265-290): predict, then correct where the record's mask word is
// non-zero, as one straight-line schedule (ekf_step_fused, ekf_fused.hpp).
// Reads x16 + P120 + u6 + z7 (+mask), writes x16 + P120 (285 words/filter).
template <typename T, bool DIRECT, bool PFP, bool GATE, int NT, bool COMPACT = false>
__device__ __forceinline__ void step_tick(const DevParams<T>& p, const GateParams& gp, T* st, const T* __restrict__ us,
                                          const T* __restrict__ zs, const T* __restrict__ pfp,
                                          T* __restrict__ aux_accel, T* __restrict__ aux_obs,
                                          int32_t* __restrict__ last_corr, uint8_t* __restrict__ flags, int64_t i)
{
    using Q = typename Quad<T>::type;
    constexpr int VW = Quad<T>::VW;
    T x[kXW], Po[kPW], u[kUW], zr[kZW];
    load_rec<T, kUW, 0, kUW, NT>(us, i, u);
    load_rec<T, kZW, 0, kZW, NT>(zs, i, zr);
    load_rec<T, kSW, 0, kXW, NT>(st, i, x);
    load_P_any<T, NT>(st, i, Po, COMPACT);   // ascending: the fused schedule starts with rows r
    const bool dead = filter_uninitialised(x);   // left untouched; no early exit (see predict_tick)
    if (dead) x[9] = T(1);
    bool corr = !dead && zr[7] != T(0);
    if (GATE) {  // the mask word means "measurement_ready"; decide here (EKF.cpp:147-186)
        const bool consume = corr && (!gp.limit || (gp.tick - last_corr[i]) >= gp.upd_per_meas);
        bool ok = consume;
        if (consume && gp.corner_enbl) {
            const double zd[7] = {(double)zr[0], (double)zr[1], (double)zr[2], (double)zr[3], (double)zr[4], (double)zr[5], (double)zr[6]};
            ok = corner_gate(gp, zd);
        }
        corr = ok;
        if (ok) last_corr[i] = gp.tick;
        flags[i] = (uint8_t)((ok ? 1 : 0) | (consume ? 2 : 0));
    }
    Noise<T> nz;
    load_noise<T, PFP>(p, pfp, i, nz);
    const T z[7] = {zr[0], zr[1], zr[2], zr[3], zr[4], zr[5], zr[6]};
    T* tb = st + wave_tile(i) * (int64_t)(kSW * kTile);
    const int lane = (int)(i & 63);
    T Pc[kPWc];   // compact records only: written group by group in the final sweep (every pose-block word is in one), never otherwise
    auto tag_pose = [&](T (&zz)[7]) {
        if constexpr (sizeof(T) == 8) {   // fp64: read again where the innovation needs it (an L2 hit) instead of 14 registers held through the sweep
            T zq[kZW];
            load_rec<T, kZW, 0, kZW, NT>(zs, i, zq);
#pragma unroll
            for (int k = 0; k < 7; ++k) zz[k] = zq[k];
        } else {
#pragma unroll
            for (int k = 0; k < 7; ++k) zz[k] = z[k];
        }
    };
    // fp64, conventional orientation method: the nominal state (16 values) waits out the covariance sweep in the LDS (32 KiB per workgroup)
    // and r and q are read back from there for each block-row's Gx -- with that the kernel needs no scratch (was 140-250 B per lane)
    constexpr bool kPark = sizeof(T) == 8 && !DIRECT;   // the direct method fits without (256 + 215 registers) and is 1.7 us faster so (28.5 vs 26.8 us)
    __shared__ T parked[kPark ? kXW : 1][kPark ? kBlock : 1];
    const LdsPark<T, kPark, false> park{parked};
    const LdsPark<T, kPark, true> unpark{parked};
    ekf_step_fused_z<T, DIRECT>(p, nz, x, Po, u, tag_pose, corr, !dead,
        [&](const T (&accel)[3]) {
            if (aux_accel && !dead) {   // optional side outputs (wave-uniform), written as soon as they exist
#pragma unroll
                for (int k = 0; k < 3; ++k) aux_accel[i * 3 + k] = accel[k];
            }
        },
        [&](const T (&obs)[7]) {
            if (aux_accel) {
#pragma unroll
                for (int k = 0; k < 7; ++k) aux_obs[i * 7 + k] = obs[k];
            }
        },
        [&]() { store_rec<T, kSW, 0, kXW, NT>(st, i, x); },
        [&](auto qc, const T* w4) {   // q4 = index of a 4-word group of P; one 16-byte quad in fp32, two in fp64
            constexpr int q4 = decltype(qc)::value;
            if constexpr (COMPACT) {   // compact records: the words of the pose block are collected and stored once, below
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (word_col(4 * q4 + k) < 9) Pc[sidx9(word_row(4 * q4 + k), word_col(4 * q4 + k))] = w4[k];
                return;
            }
#pragma unroll
            for (int h = 4 / VW - 1; h >= 0; --h) {
                const int qr = kXW / VW + q4 * (4 / VW) + h;
                st_quad<NtSt<NT>::value>(reinterpret_cast<Q*>(tb + (qr * kTile + lane) * VW), pack_quad(w4 + h * VW));
            }
        }, park, unpark);
    if (COMPACT && !dead) {
#pragma unroll
        for (int k = 45; k < kPWc; ++k) Pc[k] = T(0);
        store_rec<T, kSW, kXW, kPWc, NT>(st, i, Pc);
    }
}

template <typename T, bool DIRECT, bool PFP, bool GATE, int NT, bool COMPACT = false>
__global__ __launch_bounds__(kBlock, sizeof(T) == 8 ? 1 : 2) void k_step(T* st, const T* __restrict__ us, const T* __restrict__ zs, int64_t B, int64_t i0,
                                                 int32_t grid_x, int32_t block_x, int32_t split,   // (argument order: see k_predict)
                                                 const T* __restrict__ pfp, T* __restrict__ aux_accel, T* __restrict__ aux_obs,
                                                 int32_t* __restrict__ last_corr, uint8_t* __restrict__ flags, DevParams<T> p, GateParams gp)
{
    args_early(st, us, zs, B, i0, grid_x, block_x);
    const int64_t i = i0 + batch_block((unsigned)grid_x) * block_x + threadIdx.x;
    if (i >= B) return;
    with_policy<NT>(split, [&](auto nt) {
        step_tick<T, DIRECT, PFP, GATE, decltype(nt)::value, COMPACT>(p, gp, st, us, zs, pfp, aux_accel, aux_obs, last_corr, flags, i);
    });
}

// On-chip-resident multi-tick kernel: x and P stay in registers for n ticks of the single-rate
// filter (predict every tick, correct where the tick has a tag record whose mask word is set).
// Per tick only the 6-word IMU record (and the 8-word tag record on measurement ticks) is read;
// the next tick's IMU record is loaded before the current tick's arithmetic.
template <typename T, bool DIRECT, bool PFP, bool COMPACT = false>
__global__ __launch_bounds__(kBlock) void k_run_resident(DevParams<T> p, T* st, const T* __restrict__ us, const T* __restrict__ zs,
                                                         const int32_t* __restrict__ slot, int64_t pitch_u, int64_t pitch_z, int64_t T_seq,
                                                         int64_t t0, int64_t n, const T* __restrict__ pfp, int64_t B)
{
    args_early(st, us, zs, slot, B, gridDim.x, blockDim.x);
    const int64_t i = batch_block() * blockDim.x + threadIdx.x;
    if (i >= B) return;
    T x[kXW], u[kUW], un[kUW], accel[3];
    load_rec<T, kSW, 0, kXW>(st, i, x);
    // fp64: the covariance split between the LDS and registers (ekf_split.hpp; launched with kMrLdsPerWave of dynamic LDS per wave) -- the flat
    // triangle with the sequential update next to it spilled 0.8-1.2 KB per lane here as it did in k_step_mr; fp32: the flat triangle
    constexpr bool kSplit = sizeof(T) == 8;
    MrChain<T, !kSplit> S;      // (fp32 instantiates the block form's type only to keep one declaration; it is not used there)
    T P[kSplit ? 1 : kPW];
    if constexpr (kSplit) {
        S.init();
        T Pf[kPW];
        load_P_any<T>(st, i, Pf, COMPACT);
        S.from_flat(Pf);
    } else {
        load_P_any<T>(st, i, P, COMPACT);
    }
    if (filter_uninitialised(x)) return;
    Noise<T> nz;
    load_noise<T, PFP>(p, pfp, i, nz);
    int64_t t = t0 % T_seq;
    load_rec<T, kUW, 0, kUW>(us + t * pitch_u, i, u);
    for (int64_t k = 0; k < n; ++k) {
        const int64_t tn = (t + 1 == T_seq) ? 0 : t + 1;
        if (k + 1 < n) load_rec<T, kUW, 0, kUW>(us + tn * pitch_u, i, un);
        const int32_t s = slot[t];  // wave-uniform
        T zr[kZW];
        if (s >= 0) load_rec<T, kZW, 0, kZW>(zs + (int64_t)s * pitch_z, i, zr);
        if constexpr (kSplit) {
            if constexpr (PFP) load_noise<T, PFP>(p, pfp, i, nz);   // read again per tick (L2) rather than 48 registers held through the loop
            S.predict(p, nz, x, u, accel);
        } else {
            ekf_predict<T>(p, nz, x, P, u, accel);
        }
        if (s >= 0 && zr[7] != T(0)) {
            const T z[7] = {zr[0], zr[1], zr[2], zr[3], zr[4], zr[5], zr[6]};
            if constexpr (kSplit) ekf_update_split<T, DIRECT>(p, nz, x, S.top, S.lo, z, [](const T (&)[7]) {});
            else ekf_update_emit<T, DIRECT>(p, nz, x, P, z, [](const T (&)[7]) {});
        }
#pragma unroll
        for (int c = 0; c < kUW; ++c) u[c] = un[c];
        t = tn;
    }
    store_rec<T, kSW, 0, kXW>(st, i, x);
    if constexpr (kSplit) S.template with_flat<false>([&](const T (&Pf)[kPW]) { store_P_any<T>(st, i, Pf, COMPACT); });
    else store_P_any<T>(st, i, P, COMPACT);
}

// Stand-alone correction (correction_step, EKF.cpp:417-502) where mask != 0.
template <typename T, bool DIRECT, bool PFP, bool COMPACT = false>
__global__ __launch_bounds__(kBlock) void k_update(T* __restrict__ st, const T* __restrict__ zs, int64_t B, int32_t grid_x, int32_t block_x,   // (argument order: see k_predict)
                                                   const T* __restrict__ pfp, T* __restrict__ aux_obs, DevParams<T> p)
{
    args_early(st, zs, B, grid_x, block_x);
    const int64_t i = batch_block((unsigned)grid_x) * block_x + threadIdx.x;
    if (i >= B) return;
    T zr[kZW];
    load_rec<T, kZW, 0, kZW>(zs, i, zr);
    if (zr[7] == T(0)) return;
    T x[kXW];
    load_rec<T, kSW, 0, kXW>(st, i, x);
    Noise<T> nz;
    T z[7] = {zr[0], zr[1], zr[2], zr[3], zr[4], zr[5], zr[6]};
    T obs[7];
    if constexpr (sizeof(T) == 8) {   // fp64: the split covariance and the batch-form correction (no scratch; see k_run_resident)
        MrChain<T, false> S;
        S.init();
        if constexpr (COMPACT) {
            T Pf[kPW];
            load_P_compact<T>(st, i, Pf);
            S.from_flat(Pf);
        } else {
            S.load_cov(st, i);
        }
        if (filter_uninitialised(x)) return;
        load_noise<T, PFP>(p, pfp, i, nz);
        ekf_update_split<T, DIRECT>(p, nz, x, S.top, S.lo, z, [&](const T (&o)[7]) {
#pragma unroll
            for (int k = 0; k < 7; ++k) obs[k] = o[k];
        });
        store_rec<T, kSW, 0, kXW>(st, i, x);
        if constexpr (COMPACT) S.template with_flat<false>([&](const T (&Pf)[kPW]) { store_P_compact<T>(st, i, Pf); });
        else S.template store_cov<0>(st, i);
    } else {
        T P[kPW];
        load_P_any<T>(st, i, P, COMPACT);
        if (filter_uninitialised(x)) return;
        load_noise<T, PFP>(p, pfp, i, nz);
        ekf_update<T, DIRECT>(p, nz, x, P, z, obs);
        store_rec<T, kSW, 0, kXW>(st, i, x);
        store_P_any<T>(st, i, P, COMPACT);
    }
    if (aux_obs) {
#pragma unroll
        for (int k = 0; k < 7; ++k) aux_obs[i * 7 + k] = obs[k];
    }
}

}  // namespace qle
