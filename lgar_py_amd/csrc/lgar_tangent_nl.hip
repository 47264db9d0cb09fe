// lgar_tangent_nl.hip -- the forward-mode tangent kernels for ONE soil-layer count (compiled with -DLGAR_NL=<n>), both
// families: lgar_tangent_kernel (lgar_forward_tangent, from a fresh state) and lgar_tangent_window_kernel
// (lgar_forward_tangent_window, from a carried state); see lgar_tangent_body.hpp.  One occupancy rule, one wave loop
// (lgar_tangent_wave.hpp), one launch, one walk of the plan (tangent_chain).
#include <hip/hip_runtime.h>

#include "lgar_host.hpp"
#include "lgar_launch.hpp"
#include "lgar_tangent_body.hpp"

#ifndef LGAR_NL
#error "compile with -DLGAR_NL=<number of soil layers>"
#endif

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

template <typename R, int NL, int CAP, int MODE>
__global__ __launch_bounds__(WAVE, (TangentOccupancy<R, CAP>::waves)) void lgar_tangent_kernel(TArgs<R> a) {
#define LGAR_TANGENT_WINDOW 0
#include "lgar_tangent_wave.hpp"
#undef LGAR_TANGENT_WINDOW
}

template <typename R, int NL, int CAP, int MODE>
__global__ __launch_bounds__(WAVE, (TangentOccupancy<R, CAP>::waves)) void lgar_tangent_window_kernel(TWArgs<R> a) {
#define LGAR_TANGENT_WINDOW 1
#include "lgar_tangent_wave.hpp"
#undef LGAR_TANGENT_WINDOW
}

// One launch of `kernel` on its argument block (TArgs or TWArgs).
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

template <int NL>
int launch_tangent_nl(const LgarDims *dims, const LgarParams *params, const LgarParams *direction, const LgarForcing *forcing,
                      const void *w_runoff, const void *w_perc, void *grad_out, void *tangent_runoff, int32_t *status,
                      int dtype, hipStream_t st, unsigned *tickets) {
  auto typed = [&](auto r) {
    using R = decltype(r);
    return launch_chain(make_targs<R>(dims, params, direction, forcing, w_runoff, w_perc, grad_out, tangent_runoff, status), dims, NL,
                        st, tickets, [](auto cap, auto mode) { return lgar_tangent_kernel<R, NL, decltype(cap)::value, decltype(mode)::value>; });
  };
  if (dtype == LGAR_F64) return typed(double());
  if (dtype == LGAR_F32) return typed(float());
  return LGAR_E_ARG;
}

template <int NL>
int launch_tangent_window_nl(const LgarDims *dims, const LgarParams *params, const LgarParams *direction, const LgarForcing *forcing,
                             const void *w_runoff, const void *w_perc, const LgarTangentWindow *window, void *grad_out,
                             void *tangent_runoff, int32_t *status, int dtype, hipStream_t st, unsigned *tickets) {
  auto typed = [&](auto r) {
    using R = decltype(r);
    return launch_chain(make_twargs<R>(dims, params, direction, forcing, w_runoff, w_perc, window, grad_out, tangent_runoff, status),
                        dims, NL, st, tickets,
                        [](auto cap, auto mode) { return lgar_tangent_window_kernel<R, NL, decltype(cap)::value, decltype(mode)::value>; });
  };
  if (dtype == LGAR_F64) return typed(double());
  if (dtype == LGAR_F32) return typed(float());
  return LGAR_E_ARG;
}

#if defined(LGAR_MEASURE) && defined(LGAR_CLOCKS)
// measurement builds: the cycle attribution of this translation unit's kernels (lgar_measure.hpp LGAR_POINT_CLK)
extern "C" int lgar_debug_clocks_tangent(unsigned long long *out, int reset) {
  unsigned long long z[64] = {0};
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(lgar_dbg_clk), sizeof(z)) != hipSuccess) return -1;
  if (reset && hipMemcpyToSymbol(HIP_SYMBOL(lgar_dbg_clk), z, sizeof(z)) != hipSuccess) return -1;
  return 0;
}
#endif

template int launch_tangent_nl<LGAR_NL>(const LgarDims *, const LgarParams *, const LgarParams *, const LgarForcing *,
                                        const void *, const void *, void *, void *, int32_t *, int, hipStream_t, unsigned *);
template int launch_tangent_window_nl<LGAR_NL>(const LgarDims *, const LgarParams *, const LgarParams *, const LgarForcing *,
                                               const void *, const void *, const LgarTangentWindow *, void *, void *, int32_t *,
                                               int, hipStream_t, unsigned *);

}  // namespace lgar
