// Per-phase cycle counters of the kernels (debug builds, -DRVC_CONV_TIMING; the product library carries none of this).  Private to csrc/.
//
// Device side: a kernel owns one PhaseTimer<clock>.  With the macro it keeps eight sums and a running time stamp in registers and adds the
// sums to the translation unit's table once, at flush(); without the macro it is an empty type whose members do nothing, so a kernel
// needs no conditional of its own.  The clock is the kernel's choice (recorded profiles stay comparable): PhaseClock::cycle is
// __builtin_readcyclecounter() (s_memtime: shader clock), PhaseClock::clock64 is clock64(), PhaseClock::wall is wall_clock64() (100 MHz).
// What slots [1] .. [7] mean is the kernel's business (a comment at its timer says so); [0] counts tiles or workgroups, [6] is the total.
//
// Host side: device globals cannot be shared across translation units without relocatable device code, so every translation unit that
// includes this header has its own table.  One line at file scope, RVC_PHASE_TABLE_REGISTER;, adds the unit's reader to the list that
// conv_timing_read() (conv_mfma.hip) walks: rvc_debug_conv_timing is the sum over all tables.  Nothing registers in a product build.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>

namespace rvc {

enum class PhaseClock { cycle, clock64, wall };
using PhaseTableReader = void (*)(unsigned long long* out8, bool reset);
std::vector<PhaseTableReader>& phase_table_readers();        // conv_mfma.hip

#ifdef RVC_CONV_TIMING
static __device__ unsigned long long g_phase_table[8];
static void phase_table_read(unsigned long long* out8, bool reset) {
  (void)hipDeviceSynchronize();
  (void)hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_phase_table), sizeof(unsigned long long) * 8);
  if (reset) { unsigned long long z[8] = {0}; (void)hipMemcpyToSymbol(HIP_SYMBOL(g_phase_table), z, sizeof(z)); }
}
#define RVC_PHASE_TABLE_REGISTER static const bool phase_table_registered = (rvc::phase_table_readers().push_back(&rvc::phase_table_read), true)

template <PhaseClock C> struct PhaseTimer {
  long long sum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  long long begin, last;
  __device__ __forceinline__ static long long now() {
    if constexpr (C == PhaseClock::cycle) return (long long)__builtin_readcyclecounter();
    else if constexpr (C == PhaseClock::clock64) return (long long)clock64();
    else return (long long)wall_clock64();
  }
  __device__ __forceinline__ PhaseTimer() : begin(now()), last(begin) {}
  // slot i += time since the last mark, and mark; returns the new mark (for a later since())
  __device__ __forceinline__ long long lap(int i) { const long long t = now(); sum[i] += t - last; last = t; return t; }
  __device__ __forceinline__ void mark() { last = now(); }
  __device__ __forceinline__ void add(int i, long long dt) { sum[i] += dt; }
  // slot i += time since an earlier mark; the running mark stays
  __device__ __forceinline__ void since(int i, long long t0) { sum[i] += now() - t0; }
  // slot i += the time f() takes; the running mark stays (f's time is ALSO inside the phase that surrounds it)
  template <class F> __device__ __forceinline__ void span(int i, F&& f) { const long long t0 = now(); f(); sum[i] += now() - t0; }
  // at the end: [6] += time since construction (or the last flush), thread 0 adds the eight sums to the table.  The sums restart, so a
  // kernel with an early exit flushes unconditionally in front of it and again at its end, each interval counted once
  __device__ __forceinline__ void flush() {
    const long long t = now();
    sum[6] += t - begin; begin = t;
    if (threadIdx.x == 0) for (int i = 0; i < 8; ++i) atomicAdd(&g_phase_table[i], (unsigned long long)sum[i]);
    for (int i = 0; i < 8; ++i) sum[i] = 0;
  }
};
#else
#define RVC_PHASE_TABLE_REGISTER static_assert(true, "")
template <PhaseClock C> struct PhaseTimer {
  __device__ __forceinline__ long long lap(int) { return 0; }
  __device__ __forceinline__ void mark() {}
  __device__ __forceinline__ void add(int, long long) {}
  __device__ __forceinline__ void since(int, long long) {}
  template <class F> __device__ __forceinline__ void span(int, F&& f) { f(); }
  __device__ __forceinline__ void flush() {}
};
#endif

}  // namespace rvc
