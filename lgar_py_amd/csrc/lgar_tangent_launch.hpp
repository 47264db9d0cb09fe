// lgar_tangent_launch.hpp -- what the translation units of the tangent kernels (lgar_tangent_nl.hip, lgar_tangent_forced_nl.hip)
// share on the host side: the occupancy rule of their kernels, one launch, one call's chain of launches.
#pragma once
#include <hip/hip_runtime.h>

#include "lgar_host.hpp"
#include "lgar_tangent_body.hpp"

namespace lgar {

// Waves per SIMD the register allocator is held to.  The 8-front fp32 kernel needs 259 registers on its own -- three too many
// for two waves -- and a single resident wave gets an issue slot only every ~7 cycles: held to 256, it
// runs two waves per SIMD (backward pass of the 100 000-column ensemble 61.6 -> 44.7 ms).  The fp64 kernels stay at one wave:
// their dual-number front table alone is 40 KB of LDS per wave.
#ifndef LGAR_TAN_F32_WAVES
#define LGAR_TAN_F32_WAVES 2
#endif
template <typename R, int CAP> struct TangentOccupancy {
  static constexpr int waves = (ScalarKind<R>::f32 && CAP == LGAR_CAP_SMALL) ? LGAR_TAN_F32_WAVES : 1;
};

// One launch of `kernel` on its argument block (TArgs, TWArgs or TFArgs).
template <typename K, typename A> static void launch_one(K kernel, A &a, unsigned nblocks, unsigned *ticket, hipStream_t st) {
  targs(a).ticket = ticket;
  unsigned grid = nblocks;
  if (ticket != nullptr) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      cus = 256;
    // resident one-wave workgroups per CU for THIS kernel (registers and LDS decide: 4 for the fp64 dual-number kernels --
    // 256 VGPRs + ~180 AGPRs, one wave per SIMD -- 8 for the fp32 ones)
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, WAVE, 0) != hipSuccess || per_cu <= 0) per_cu = 4;
    const unsigned slots = (unsigned)cus * (unsigned)per_cu;
    grid = nblocks < slots ? nblocks : slots;
  }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(WAVE), 0, st, a);
}

// One call on the argument block `a`: the work counters cleared, then the plan (lgar_plan.hpp), one launch per kernel of it.  `kernel(cap, mode)`: the
// family's kernel for that capacity and mode.
template <typename A, typename Pick>
static int launch_chain(A a, const LgarDims *dims, int nl, hipStream_t st, unsigned *tickets, Pick kernel) {
  if (tickets != nullptr && hipMemsetAsync(tickets, 0, LGAR_NTICKETS * sizeof(unsigned), st) != hipSuccess) return LGAR_E_LAUNCH;
  const TangentPlan plan = tangent_plan(dims, nl);
  return tangent_chain(a, plan, tickets, [&](auto cap, auto mode, unsigned *tk) {
    launch_one(kernel(cap, mode), a, plan.blocks, tk, st);
    return launch_status();
  });
}

}  // namespace lgar
