// lgar_network_mc.hip -- the Muskingum-Cunge network kernels and their C-ABI entry points (lgar_network_route_mc /
// lgar_network_route_mc_grad, include/lgar.h; lgar_network_mc.hpp holds the row, mc_ln, the per-reach walks and the refusals).
//
// The launch shape is lgar_network.hip's: one launch per non-empty level on the caller's stream (ascending for the forward,
// descending for the adjoint), lane p of a level owns reach order[p] and walks all rows, workgroups of 256 lanes, the grid capped
// and the rest by stride.  level_ptr is read HERE, on the host, to size the launches.  A row is a dependent chain of a logarithm,
// an exponential and four divisions: the walk is bound by that latency, not by its loads.
#include <hip/hip_runtime.h>

#include "lgar_host.hpp"
#include "lgar_network_mc.hpp"

namespace lgar {

#define LGAR_NET_GRID_CAP 4096  // workgroups of four waves, as lgar_network.hip

__global__ __launch_bounds__(256) void lgar_network_mc_kernel(McArgs a, long long p0, long long p1) {
  for (long long p = p0 + (long long)blockIdx.x * 256 + threadIdx.x; p < p1; p += (long long)gridDim.x * 256)
    mc_walk(a, net_reach(a.order, p, a.B));
}

template <bool GP> __global__ __launch_bounds__(256) void lgar_network_mc_grad_kernel(McGradArgs a, long long p0, long long p1) {
  for (long long p = p0 + (long long)blockIdx.x * 256 + threadIdx.x; p < p1; p += (long long)gridDim.x * 256)
    mc_walk_back<GP>(a, net_reach(a.order, p, a.B));
}

static dim3 mc_level_grid(long long width) {
  const long long blocks = (width + 255) / 256;
  return dim3((unsigned)(blocks < LGAR_NET_GRID_CAP ? blocks : LGAR_NET_GRID_CAP));
}

int launch_network_mc(const McArgs &a, const int32_t *level_ptr, int n_levels, hipStream_t stream) {
  for (int l = 0; l < n_levels; l++) {
    const long long p0 = level_ptr[l], p1 = level_ptr[l + 1];
    if (p1 > p0) hipLaunchKernelGGL(lgar_network_mc_kernel, mc_level_grid(p1 - p0), dim3(256), 0, stream, a, p0, p1);
  }
  return launch_status();
}

int launch_network_mc_grad(const McGradArgs &a, const int32_t *level_ptr, int n_levels, hipStream_t stream) {
  for (int l = n_levels - 1; l >= 0; l--) {
    const long long p0 = level_ptr[l], p1 = level_ptr[l + 1];
    if (p1 <= p0) continue;
    if (a.gpar) hipLaunchKernelGGL(lgar_network_mc_grad_kernel<true>, mc_level_grid(p1 - p0), dim3(256), 0, stream, a, p0, p1);
    else hipLaunchKernelGGL(lgar_network_mc_grad_kernel<false>, mc_level_grid(p1 - p0), dim3(256), 0, stream, a, p0, p1);
  }
  return launch_status();
}

}  // namespace lgar

// The C-ABI entry points live here: every other translation unit stays byte-identical.
extern "C" {

int32_t lgar_network_route_mc(const double *x, int32_t n_rows, int32_t n_catchments, const double *par, double dt_h, double rmin,
                              double rmax, const int32_t *up_ptr, const int32_t *up_idx, int32_t n_edges, const int32_t *order,
                              const int32_t *level_ptr, int32_t n_levels, const double *state_in, double *state_out, double *y,
                              void *stream) {
  const int rc = lgar::mc_route_check(x, n_rows, n_catchments, par, dt_h, rmin, rmax, up_ptr, up_idx, n_edges, order, level_ptr, n_levels,
                                      state_out, y);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::McArgs a;
  a.x = x, a.par = par, a.state_in = state_in, a.y = y, a.state_out = state_out;
  a.order = order, a.up_ptr = up_ptr, a.up_idx = up_idx;
  a.dt_h = dt_h, a.rmin = rmin, a.rmax = rmax;
  a.T = n_rows, a.B = n_catchments, a.E = n_edges;
  return lgar::launch_network_mc(a, level_ptr, n_levels, (hipStream_t)stream);
}

int32_t lgar_network_route_mc_grad(const double *gy, int32_t n_rows, int32_t n_catchments, const double *par, double dt_h, double rmin,
                                   double rmax, const int32_t *down, const int32_t *order, const int32_t *level_ptr, int32_t n_levels,
                                   double *gx, const double *x, const double *y, const int32_t *up_ptr, const int32_t *up_idx,
                                   int32_t n_edges, const double *state_in, double *gpar, double *gstate, void *stream) {
  const int rc = lgar::mc_grad_check(gy, n_rows, n_catchments, par, dt_h, rmin, rmax, down, order, level_ptr, n_levels, gx, x, y, up_ptr,
                                     up_idx, n_edges, gpar, gstate);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::McGradArgs a;
  a.gy = gy, a.x = x, a.y = y, a.par = par, a.state_in = state_in, a.gx = gx, a.gpar = gpar, a.gstate = gstate;
  a.order = order, a.down = down, a.up_ptr = up_ptr, a.up_idx = up_idx;
  a.dt_h = dt_h, a.rmin = rmin, a.rmax = rmax;
  a.T = n_rows, a.B = n_catchments, a.E = n_edges;
  return lgar::launch_network_mc_grad(a, level_ptr, n_levels, (hipStream_t)stream);
}

}  // extern "C"
