// ekf_cov_home.hpp -- where a lane keeps its covariance between the ticks of a kernel that holds it on chip (k_step_mr, fp64 k_update,
// fp64 k_run_resident): MrChain.
#pragma once

#include "ekf_fused.hpp"   // static_for
#include "ekf_layout.hpp"
#include "ekf_packed.hpp"
#include "ekf_split.hpp"

namespace qle {

// The covariance of a replayed chain as it is held between the ticks of the loop.  fp32: the register blocks of ekf_packed.hpp (two FMAs per
// instruction), the correction on the unpacked triangle.  fp64: SPLIT (ekf_split.hpp) -- the packed triangle alone is 240 of a wave's 512
// registers and with the correction's gain vectors next to it the kernel spilled 1.2-1.5 KB per lane (240 us per launch); the two top
// block-rows (75 of the 120 values) live in the wave's 37.5 KiB window of the LDS instead, the three bottom ones in registers, and predict
// and correction stream the top rows through registers a 3 x 3 block at a time: no scratch.
extern __shared__ unsigned char qle_dyn_lds[];
template <typename T, bool BLOCKS = (sizeof(T) == 4)> struct MrChain;
template <typename T> struct MrChain<T, true> {
    PackedCov<T> S;
    __device__ __forceinline__ void init() {}
    __device__ __forceinline__ void from_flat(const T (&P)[kPW]) { cov_pack<T>(P, S); }
    __device__ __forceinline__ void load_cov(const T* __restrict__ src, int64_t i)
    {
        T P[kPW];
        load_rec<T, kSW, kXW, kPW>(src, i, P);
        from_flat(P);
    }
    template <int NT> __device__ __forceinline__ void store_cov(T* __restrict__ dst, int64_t i)
    {
        with_flat<false>([&](const T (&P)[kPW]) { store_rec<T, kSW, kXW, kPW, NT>(dst, i, P); });
    }
    // f(P) on the packed triangle; MODIFIES: f changes P
    template <bool MODIFIES, typename F> __device__ __forceinline__ void with_flat(F&& f)
    {
        T P[kPW];
        cov_unpack<T>(S, P);
        f(P);
        if (MODIFIES) cov_pack<T>(P, S);
    }
    __device__ __forceinline__ void predict(const DevParams<T>& p, const Noise<T>& nz, T (&x)[kXW], const T (&u)[kUW], T (&accel)[3])
    {
        ekf_predict_packed<T>(p, nz, x, S, u, accel);
    }
    // correction_step at the entry the measurement belongs to; done(P): the corrected triangle (the new anchor)
    template <bool DIRECT, typename Emit, typename Done>
    __device__ __forceinline__ void correct(const DevParams<T>& p, const Noise<T>& nz, T (&x)[kXW], const T (&z)[7], Emit&& emit, Done&& done)
    {
        with_flat<true>([&](T (&P)[kPW]) {
            ekf_update_emit<T, DIRECT>(p, nz, x, P, z, emit);
            done([&](T* __restrict__ dst, int64_t i) { store_rec<T, kSW, kXW, kPW, 2>(dst, i, P); });
        });
    }
    __device__ __forceinline__ T probe() const { return S.blk(2, 2).d + S.blk(0, 1).c.x; }   // values a predict forms last (diagnostic stamps)
};
template <typename T> struct MrChain<T, false> {
    T lo[kLoWords];
    LdsTop<T> top;
    __device__ __forceinline__ void init()
    {
        top.p = reinterpret_cast<T*>(qle_dyn_lds) + (size_t)(threadIdx.x >> 6) * (kTopWords * kTile) + (threadIdx.x & 63);
    }
    // Record words [W0, W0 + W) of the packed triangle <-> their homes.  The record is moved in two parts with a fence between them
    // (the first 84 words hold block-rows r and v, which go to the LDS): all 120 words at once would be 240 registers in flight next to
    // everything else the kernel holds at that point.
    template <int W0, int W> __device__ __forceinline__ void load_part(const T* __restrict__ src, int64_t i)
    {
        T t[W];
        load_rec<T, kSW, kXW + W0, W>(src, i, t);
        static_for<W0, W0 + W>([&](auto wc) {   // a compile-time loop: every index must be a constant (no array may reach scratch)
            constexpr int w = decltype(wc)::value, hw = split_word(word_row(w), word_col(w));
            if constexpr (word_row(w) < 6) top.st(hw, t[w - W0]);
            else lo[hw] = t[w - W0];
        });
    }
    template <int NT, int W0, int W> __device__ __forceinline__ void store_part(T* __restrict__ dst, int64_t i)
    {
        T t[W];
        static_for<W0, W0 + W>([&](auto wc) {
            constexpr int w = decltype(wc)::value, hw = split_word(word_row(w), word_col(w));
            if constexpr (word_row(w) < 6) t[w - W0] = top.ld(hw);
            else t[w - W0] = lo[hw];
        });
        store_rec<T, kSW, kXW + W0, W, NT>(dst, i, t);
    }
    // the whole triangle at once (callers with little else live: k_run_resident, compact records)
    __device__ __forceinline__ void from_flat(const T (&Pf)[kPW]) { split_from_flat<T>(Pf, top, lo); }
    template <bool MODIFIES, typename F> __device__ __forceinline__ void with_flat(F&& f)
    {
        T P[kPW];
        split_to_flat<T>(top, lo, P);
        f(P);
        if (MODIFIES) split_from_flat<T>(P, top, lo);
    }
    static constexpr int kTopPart = 84;   // words 0..83: block-rows r, v and the first words of row th (sidx order, ekf_device.hpp)
    __device__ __forceinline__ void load_cov(const T* __restrict__ src, int64_t i)
    {
        load_part<0, kTopPart>(src, i);
        QLE_PHASE_FENCE();
        load_part<kTopPart, kPW - kTopPart>(src, i);
        QLE_PHASE_FENCE();
    }
    template <int NT> __device__ __forceinline__ void store_cov(T* __restrict__ dst, int64_t i)
    {
        QLE_PHASE_FENCE();
        store_part<NT, 0, kTopPart>(dst, i);
        QLE_PHASE_FENCE();
        store_part<NT, kTopPart, kPW - kTopPart>(dst, i);
        QLE_PHASE_FENCE();
    }
    __device__ __forceinline__ void predict(const DevParams<T>& p, const Noise<T>& nz, T (&x)[kXW], const T (&u)[kUW], T (&accel)[3])
    {
        ekf_predict_split<T>(p, nz, x, top, lo, u, accel);
    }
    template <bool DIRECT, typename Emit, typename Done>
    __device__ __forceinline__ void correct(const DevParams<T>& p, const Noise<T>& nz, T (&x)[kXW], const T (&z)[7], Emit&& emit, Done&& done)
    {
        ekf_update_split<T, DIRECT>(p, nz, x, top, lo, z, emit);
        done([&](T* __restrict__ dst, int64_t i) { store_cov<2>(dst, i); });
    }
    __device__ __forceinline__ T probe() const { return lo[L_TT] + top.ld(T_RV); }
};

}  // namespace qle
