// lgar_canopy.hip -- the catchment-canopy kernels and their C-ABI entry points (lgar_catchment_canopy / lgar_catchment_canopy_grad /
// lgar_catchment_canopy_tangent, include/lgar.h; lgar_canopy.hpp holds the per-cell walk, the adjoint walk, the tangent walk and
// the refusals).
//
// One launch per call, on the caller's stream.  Lane p owns forcing cell p (the tangent: cell p % B along direction p / B) and
// walks all rows: 64 lanes are 64 cells, their loads and stores 512-byte row segments.  Workgroups of 256 lanes; the grid is
// capped and the lanes stride, so any B launches.  Every decision of the walk is a select, so the lanes of a wave stay together.
// No LDS, no atomics.
#include <hip/hip_runtime.h>

#include "lgar_canopy.hpp"
#include "lgar_host.hpp"

namespace lgar {

#define LGAR_CN_GRID_CAP 2048  // workgroups of four waves: eight waves per SIMD of 256 CUs

__global__ __launch_bounds__(256) void lgar_canopy_kernel(CnArgs a) {
  for (long long b = (long long)blockIdx.x * 256 + threadIdx.x; b < a.B; b += (long long)gridDim.x * 256) cn_walk(a, b);
}

template <bool GP> __global__ __launch_bounds__(256) void lgar_canopy_grad_kernel(CnGradArgs a) {
  for (long long b = (long long)blockIdx.x * 256 + threadIdx.x; b < a.B; b += (long long)gridDim.x * 256) cn_walk_back<GP>(a, b);
}

// one lane per (cell, direction): lane i = k * B + b
__global__ __launch_bounds__(256) void lgar_canopy_tangent_kernel(CnTanArgs a) {
  const long long n = a.B * a.D;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) cn_walk_tangent(a, i % a.B, i / a.B);
}

static dim3 cn_grid(long long lanes) {
  const long long blocks = (lanes + 255) / 256;
  return dim3((unsigned)(blocks < LGAR_CN_GRID_CAP ? blocks : LGAR_CN_GRID_CAP));
}

int launch_canopy(const CnArgs &a, hipStream_t stream) {
  hipLaunchKernelGGL(lgar_canopy_kernel, cn_grid(a.B), dim3(256), 0, stream, a);
  return launch_status();
}

int launch_canopy_grad(const CnGradArgs &a, hipStream_t stream) {
  if (a.gpar) hipLaunchKernelGGL(lgar_canopy_grad_kernel<true>, cn_grid(a.B), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL(lgar_canopy_grad_kernel<false>, cn_grid(a.B), dim3(256), 0, stream, a);
  return launch_status();
}

int launch_canopy_tangent(const CnTanArgs &a, hipStream_t stream) {
  hipLaunchKernelGGL(lgar_canopy_tangent_kernel, cn_grid(a.B * a.D), dim3(256), 0, stream, a);
  return launch_status();
}

}  // namespace lgar

// The C-ABI entry points live here, not with the other wrappers in lgar_kernels.hip: every other translation unit stays
// byte-identical.
extern "C" {

int32_t lgar_catchment_canopy(const double *p, const double *e, const double *lai, int32_t n_rows, int32_t n_cells, const double *par,
                              double dt_h, const double *state_in, double *state_out, double *w, double *pet_out, double *store,
                              double *evap, void *stream) {
  const int rc = lgar::cn_check(p, e, n_rows, n_cells, par, dt_h, state_out, w, pet_out, store, evap);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::CnArgs a;
  a.p = p, a.e = e, a.lai = lai, a.par = par, a.state_in = state_in;
  a.w = w, a.pet = pet_out, a.store = store, a.evap = evap, a.state_out = state_out;
  a.dt_h = dt_h, a.T = n_rows, a.B = n_cells;
  return lgar::launch_canopy(a, (hipStream_t)stream);
}

int32_t lgar_catchment_canopy_grad(const double *gw, const double *gpet, const double *gstore, const double *gevap, const double *p,
                                   const double *e, const double *lai, const double *store, int32_t n_rows, int32_t n_cells,
                                   const double *par, double dt_h, const double *state_in, double *gp, double *ge, double *glai,
                                   double *gpar, double *gstate, void *stream) {
  const int rc = lgar::cn_grad_check(gw, gpet, p, e, store, n_rows, n_cells, par, dt_h, gp, ge, gpar, gstate);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::CnGradArgs a;
  a.gw = gw, a.gpet = gpet, a.gstore = gstore, a.gevap = gevap, a.p = p, a.e = e, a.lai = lai, a.store = store, a.par = par;
  a.state_in = state_in, a.gp = gp, a.ge = ge, a.glai = glai, a.gpar = gpar, a.gstate = gstate;
  a.dt_h = dt_h, a.T = n_rows, a.B = n_cells;
  return lgar::launch_canopy_grad(a, (hipStream_t)stream);
}

int32_t lgar_catchment_canopy_tangent(const double *p, const double *e, const double *lai, int32_t n_rows, int32_t n_cells,
                                      const double *par, double dt_h, const double *state_in, int32_t n_dirs, const double *dp,
                                      const double *de, const double *dlai, const double *dpar, const double *dstate_in, double *dw,
                                      double *dpet, int32_t ld, int32_t k0, double *dstore, double *devap, double *dstate_out,
                                      void *stream) {
  const int rc = lgar::cn_tangent_check(p, e, n_rows, n_cells, par, dt_h, n_dirs, dw, ld, k0, dstore, devap, dstate_out);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::CnTanArgs a;
  a.p = p, a.e = e, a.lai = lai, a.par = par, a.state_in = state_in;
  a.dp = dp, a.de = de, a.dlai = dlai, a.dpar = dpar, a.dstate_in = dstate_in;
  a.dw = dw, a.dpet = dpet, a.dstore = dstore, a.devap = devap, a.dstate_out = dstate_out;
  a.dt_h = dt_h, a.T = n_rows, a.B = n_cells, a.D = n_dirs, a.ld = ld, a.k0 = k0;
  return lgar::launch_canopy_tangent(a, (hipStream_t)stream);
}

}  // extern "C"
