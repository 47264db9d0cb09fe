// lgar_snow.hip -- the catchment-snowpack kernels and their C-ABI entry points (lgar_catchment_snow / lgar_catchment_snow_grad,
// include/lgar.h; lgar_snow.hpp holds the per-cell walk, the adjoint walk and the refusals).
//
// One launch per call, on the caller's stream.  Lane p owns forcing cell p and walks all rows: 64 lanes are 64 cells, their loads
// and stores 512-byte row segments.  Workgroups of 256 lanes; the grid is capped and the lanes stride over the cells, so any B
// launches.  Every decision of the walk is a select, so the lanes of a wave stay together.  No LDS, no atomics.
#include <hip/hip_runtime.h>

#include "lgar_snow.hpp"
#include "lgar_host.hpp"

namespace lgar {

#define LGAR_SN_GRID_CAP 2048  // workgroups of four waves: eight waves per SIMD of 256 CUs

__global__ __launch_bounds__(256) void lgar_snow_kernel(SnArgs a) {
  for (long long b = (long long)blockIdx.x * 256 + threadIdx.x; b < a.B; b += (long long)gridDim.x * 256) sn_walk(a, b);
}

template <bool GP> __global__ __launch_bounds__(256) void lgar_snow_grad_kernel(SnGradArgs a) {
  for (long long b = (long long)blockIdx.x * 256 + threadIdx.x; b < a.B; b += (long long)gridDim.x * 256) sn_walk_back<GP>(a, b);
}

// one lane per (cell, direction): lane i = k * B + b
__global__ __launch_bounds__(256) void lgar_snow_tangent_kernel(SnTanArgs a) {
  const long long n = a.B * a.D;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) sn_walk_tangent(a, i % a.B, i / a.B);
}

static dim3 sn_grid(long long B) {
  const long long blocks = (B + 255) / 256;
  return dim3((unsigned)(blocks < LGAR_SN_GRID_CAP ? blocks : LGAR_SN_GRID_CAP));
}

int launch_snow(const SnArgs &a, hipStream_t stream) {
  hipLaunchKernelGGL(lgar_snow_kernel, sn_grid(a.B), dim3(256), 0, stream, a);
  return launch_status();
}

int launch_snow_tangent(const SnTanArgs &a, hipStream_t stream) {
  hipLaunchKernelGGL(lgar_snow_tangent_kernel, sn_grid(a.B * a.D), dim3(256), 0, stream, a);
  return launch_status();
}

int launch_snow_grad(const SnGradArgs &a, hipStream_t stream) {
  if (a.gpar) hipLaunchKernelGGL(lgar_snow_grad_kernel<true>, sn_grid(a.B), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(lgar_snow_grad_kernel<false>, sn_grid(a.B), dim3(256), 0, stream, a);
  return launch_status();
}

}  // namespace lgar

// The C-ABI entry points live here, not with the other wrappers in lgar_kernels.hip: every other translation unit stays
// byte-identical.
extern "C" {

int32_t lgar_catchment_snow(const double *p, const double *ta, int32_t n_rows, int32_t n_cells, const double *par, double dt_h,
                            const double *state_in, double *state_out, double *w, double *ice, double *liq, void *stream) {
  const int rc = lgar::sn_check(p, ta, n_rows, n_cells, par, dt_h, state_out, w, ice, liq);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::SnArgs a;
  a.p = p, a.ta = ta, a.par = par, a.state_in = state_in, a.w = w, a.ice = ice, a.liq = liq, a.state_out = state_out;
  a.dt_h = dt_h, a.T = n_rows, a.B = n_cells;
  return lgar::launch_snow(a, (hipStream_t)stream);
}

int32_t lgar_catchment_snow_grad(const double *gw, const double *gice, const double *gliq, const double *p, const double *ta,
                                 const double *ice, const double *liq, int32_t n_rows, int32_t n_cells, const double *par,
                                 double dt_h, const double *state_in, double *gp, double *gta, double *gpar, double *gstate,
                                 void *stream) {
  const int rc = lgar::sn_grad_check(gw, p, ta, ice, liq, n_rows, n_cells, par, dt_h, gp, gpar, gstate);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::SnGradArgs a;
  a.gw = gw, a.gice = gice, a.gliq = gliq, a.p = p, a.ta = ta, a.ice = ice, a.liq = liq, a.par = par, a.state_in = state_in;
  a.gp = gp, a.gta = gta, a.gpar = gpar, a.gstate = gstate;
  a.dt_h = dt_h, a.T = n_rows, a.B = n_cells;
  return lgar::launch_snow_grad(a, (hipStream_t)stream);
}

int32_t lgar_catchment_snow_tangent(const double *p, const double *ta, int32_t n_rows, int32_t n_cells, const double *par, double dt_h,
                                    const double *state_in, int32_t n_dirs, const double *dp, const double *dta, const double *dpar,
                                    const double *dstate_in, double *dw, int32_t ld, int32_t k0, double *dice, double *dliq,
                                    double *dstate_out, void *stream) {
  const int rc = lgar::sn_tangent_check(p, ta, n_rows, n_cells, par, dt_h, n_dirs, dw, ld, k0, dice, dliq, dstate_out);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::SnTanArgs a;
  a.p = p, a.ta = ta, a.par = par, a.state_in = state_in, a.dp = dp, a.dta = dta, a.dpar = dpar, a.dstate_in = dstate_in;
  a.dw = dw, a.dice = dice, a.dliq = dliq, a.dstate_out = dstate_out;
  a.dt_h = dt_h, a.T = n_rows, a.B = n_cells, a.D = n_dirs, a.ld = ld, a.k0 = k0;
  return lgar::launch_snow_tangent(a, (hipStream_t)stream);
}

}  // extern "C"
