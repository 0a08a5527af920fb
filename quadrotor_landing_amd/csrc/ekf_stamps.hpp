// ekf_stamps.hpp -- s_memtime stamps of the diagnostic build (make dbg, -DQLE_MR_STAMPS); they expand to nothing in the product.
#pragma once

namespace qle {

// Per-wave timeline of k_step_mr (diagnostic build only: make dbg, -DQLE_MR_STAMPS; profiles/r03_scripts/mr_timeline.py reads it back
// through qle_debug_clocks).  Lane 0 of every wave writes s_memtime at the marked points; each stamp takes a value of the phase before it
// as an input so that it cannot move.  Slots: 0 entry, 1 inputs and x arrived, 2 chain start decided, 3 chain state arrived, 4 first
// IMU sample arrived, 5 / 6 correction begin / end, 7 end; 8 + 2 j / 9 + 2 j: IMU sample of loop iteration j ready / its predict done.
#ifdef QLE_MR_STAMPS
constexpr int kDbgSlots = 128, kDbgWaves = 4096;
static __device__ unsigned long long qle_dbg_clock[kDbgWaves * kDbgSlots];
#define QLE_STAMP(k, dep)                                                                                                  \
    do {                                                                                                                   \
        unsigned long long t_;                                                                                             \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) : "v"(dep) : "memory");                              \
        if ((i & 63) == 0 && (i >> 6) < kDbgWaves && (k) < kDbgSlots) qle_dbg_clock[(i >> 6) * kDbgSlots + (k)] = t_;       \
    } while (0)
// the same for a kernel that names its wave and its writing lane itself (kw_tick: one workgroup per tile)
#define QLE_STAMPW(wave, writer, k, dep)                                                                                   \
    do {                                                                                                                   \
        unsigned long long t_;                                                                                             \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) : "v"(dep) : "memory");                              \
        if ((writer) && (wave) < kDbgWaves && (k) < kDbgSlots) qle_dbg_clock[(wave) * kDbgSlots + (k)] = t_;                \
    } while (0)
#else
#define QLE_STAMP(k, dep) do { } while (0)
#define QLE_STAMPW(wave, writer, k, dep) do { } while (0)
#endif

}  // namespace qle
