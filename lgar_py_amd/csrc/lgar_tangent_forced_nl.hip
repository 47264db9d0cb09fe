// lgar_tangent_forced_nl.hip -- the tangent kernels that take a forcing direction, for ONE soil-layer count (compiled with
// -DLGAR_NL=<n>): lgar_tangent_forced_kernel (lgar_forward_tangent_forced).  The window family's lane with dual-number forcing
// (tangent_lane<..., WINDOW = true, FORCED = true>, lgar_tangent_body.hpp); the wave loop, the occupancy rule, the launch and
// the walk of the plan are the other two families' (lgar_tangent_wave.hpp, lgar_tangent_launch.hpp, tangent_chain).  A unit of
// its own: the kernels of lgar_tangent_nl.hip stay, instruction for instruction, what they were.
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
__global__ __launch_bounds__(WAVE, (TangentOccupancy<R, CAP>::waves)) void lgar_tangent_forced_kernel(TFArgs<R> a) {
#define LGAR_TANGENT_WINDOW 2
#include "lgar_tangent_wave.hpp"
#undef LGAR_TANGENT_WINDOW
}

template <int NL>
int launch_tangent_forced_nl(const LgarDims *dims, const LgarParams *params, const LgarParams *direction, const LgarForcing *forcing,
                             const LgarForcing *dforcing, const void *w_runoff, const void *w_perc, const LgarTangentWindow *window,
                             void *grad_out, void *tangent_runoff, int32_t *status, int dtype, hipStream_t st, unsigned *tickets) {
  auto typed = [&](auto r) {
    using R = decltype(r);
    return launch_chain(make_tfargs<R>(dims, params, direction, forcing, dforcing, w_runoff, w_perc, window, grad_out, tangent_runoff,
                                       status),
                        dims, NL, st, tickets,
                        [](auto cap, auto mode) { return lgar_tangent_forced_kernel<R, NL, decltype(cap)::value, decltype(mode)::value>; });
  };
  if (dtype == LGAR_F64) return typed(double());
  if (dtype == LGAR_F32) return typed(float());
  return LGAR_E_ARG;
}

template int launch_tangent_forced_nl<LGAR_NL>(const LgarDims *, const LgarParams *, const LgarParams *, const LgarForcing *,
                                               const LgarForcing *, const void *, const void *, const LgarTangentWindow *, void *,
                                               void *, int32_t *, int, hipStream_t, unsigned *);

}  // namespace lgar
