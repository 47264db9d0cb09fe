// lgar_tangent_nl.hip -- the forward-mode tangent kernels for ONE soil-layer count (compiled with -DLGAR_NL=<n>), both
// families: lgar_tangent_kernel (lgar_forward_tangent, from a fresh state) and lgar_tangent_window_kernel
// (lgar_forward_tangent_window, from a carried state); see lgar_tangent_body.hpp.  One occupancy rule and one launch
// (lgar_tangent_launch.hpp, shared with lgar_tangent_forced_nl.hip), one wave loop (lgar_tangent_wave.hpp), one walk of the plan
// (tangent_chain).
#include <hip/hip_runtime.h>

#include "lgar_host.hpp"
#include "lgar_launch.hpp"
#include "lgar_tangent_body.hpp"
#include "lgar_tangent_launch.hpp"

#ifndef LGAR_NL
#error "compile with -DLGAR_NL=<number of soil layers>"
#endif

namespace lgar {

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
