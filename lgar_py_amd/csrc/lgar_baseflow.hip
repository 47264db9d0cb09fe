// lgar_baseflow.hip -- the catchment-baseflow kernels and their C-ABI entry points (lgar_catchment_baseflow /
// lgar_catchment_baseflow_grad, include/lgar.h; lgar_baseflow.hpp holds the per-catchment walk, the adjoint step, gw_exp and the
// refusals).
//
// One launch per call, on the caller's stream.  Lane p owns catchment p and walks all rows: 64 lanes are 64 catchments, their
// loads and stores 512-byte row segments.  Workgroups of 256 lanes; the grid is capped and the lanes stride over the
// catchments, so any B launches.  Every decision of the walk is a select, so the lanes of a wave stay together.  No LDS.
#include <hip/hip_runtime.h>

#include "lgar_baseflow.hpp"
#include "lgar_host.hpp"

namespace lgar {

#define LGAR_GW_GRID_CAP 2048  // workgroups of four waves: eight waves per SIMD of 256 CUs

__global__ __launch_bounds__(256) void lgar_baseflow_kernel(GwArgs a) {
  for (long long b = (long long)blockIdx.x * 256 + threadIdx.x; b < a.B; b += (long long)gridDim.x * 256) gw_walk(a, b);
}

template <bool GP> __global__ __launch_bounds__(256) void lgar_baseflow_grad_kernel(GwGradArgs a) {
  for (long long b = (long long)blockIdx.x * 256 + threadIdx.x; b < a.B; b += (long long)gridDim.x * 256) gw_walk_back<GP>(a, b);
}

static dim3 gw_grid(long long B) {
  const long long blocks = (B + 255) / 256;
  return dim3((unsigned)(blocks < LGAR_GW_GRID_CAP ? blocks : LGAR_GW_GRID_CAP));
}

int launch_baseflow(const GwArgs &a, hipStream_t stream) {
  hipLaunchKernelGGL(lgar_baseflow_kernel, gw_grid(a.B), dim3(256), 0, stream, a);
  return launch_status();
}

int launch_baseflow_grad(const GwGradArgs &a, hipStream_t stream) {
  if (a.gpar) hipLaunchKernelGGL(lgar_baseflow_grad_kernel<true>, gw_grid(a.B), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(lgar_baseflow_grad_kernel<false>, gw_grid(a.B), dim3(256), 0, stream, a);
  return launch_status();
}

}  // namespace lgar

// The C-ABI entry points live here, not with the other wrappers in lgar_kernels.hip: the forward translation units stay
// byte-identical.
extern "C" {

int32_t lgar_catchment_baseflow(const double *r, int32_t n_rows, int32_t n_catchments, const double *par, double dt_h,
                                const double *state_in, double *state_out, double *q, double *s, void *stream) {
  const int rc = lgar::gw_check(r, n_rows, n_catchments, par, dt_h, state_out, q);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::GwArgs a;
  a.r = r, a.par = par, a.state_in = state_in, a.q = q, a.s = s, a.state_out = state_out;
  a.dt_h = dt_h, a.T = n_rows, a.B = n_catchments;
  return lgar::launch_baseflow(a, (hipStream_t)stream);
}

int32_t lgar_catchment_baseflow_grad(const double *gq, const double *gs, const double *r, const double *s, int32_t n_rows,
                                     int32_t n_catchments, const double *par, double dt_h, const double *state_in, double *gr,
                                     double *gpar, double *gstate, void *stream) {
  const int rc = lgar::gw_grad_check(gq, r, s, n_rows, n_catchments, par, dt_h, gr, gpar, gstate);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::GwGradArgs a;
  a.gq = gq, a.gs = gs, a.r = r, a.s = s, a.par = par, a.state_in = state_in, a.gr = gr, a.gpar = gpar, a.gstate = gstate;
  a.dt_h = dt_h, a.T = n_rows, a.B = n_catchments;
  return lgar::launch_baseflow_grad(a, (hipStream_t)stream);
}

}  // extern "C"
