// lgar_network_pool.hip -- the kernels of the network with reaches and level-pool reservoirs and their C-ABI entry points
// (lgar_network_route_pool / lgar_network_route_pool_grad, include/lgar.h; lgar_network_pool.hpp holds the pool row, the per-pool
// walks and the refusals, lgar_network_mc.hpp the reach walks).
//
// The launch shape is lgar_network_mc.hip's, with the level cut in two: positions [level_ptr[l], pool_ptr[l]) of `order` are
// reaches and get the reach kernel (mc_walk / mc_walk_back as they are), positions [pool_ptr[l], level_ptr[l + 1]) are pools and
// get the pool kernel; an empty segment launches nothing.  So no wave ever holds both kinds.  Both launches of a level go to the
// caller's stream one after the other (either order: the nodes of a level do not read each other), the levels ascending for the
// forward and descending for the adjoint; lane p owns node order[p] and walks all rows, workgroups of 256 lanes, the grid capped
// and the rest by stride.  level_ptr and pool_ptr are read HERE, on the host.  A pool row is a dependent chain of a logarithm, an
// exponential and up to four divisions: the walk is bound by that latency, not by its loads.
#include <hip/hip_runtime.h>

#include "lgar_host.hpp"
#include "lgar_network_pool.hpp"

namespace lgar {

#define LGAR_NET_GRID_CAP 4096  // workgroups of four waves, as lgar_network.hip

__global__ __launch_bounds__(256) void lgar_network_pool_reach_kernel(McArgs a, long long p0, long long p1) {
  for (long long p = p0 + (long long)blockIdx.x * 256 + threadIdx.x; p < p1; p += (long long)gridDim.x * 256)
    mc_walk(a, net_reach(a.order, p, a.B));
}

__global__ __launch_bounds__(256) void lgar_network_pool_kernel(PoolArgs a, long long p0, long long p1) {
  for (long long p = p0 + (long long)blockIdx.x * 256 + threadIdx.x; p < p1; p += (long long)gridDim.x * 256)
    pool_walk(a, net_reach(a.mc.order, p, a.mc.B));
}

template <bool GP> __global__ __launch_bounds__(256) void lgar_network_pool_reach_grad_kernel(McGradArgs a, long long p0, long long p1) {
  for (long long p = p0 + (long long)blockIdx.x * 256 + threadIdx.x; p < p1; p += (long long)gridDim.x * 256)
    mc_walk_back<GP>(a, net_reach(a.order, p, a.B));
}

template <bool GP> __global__ __launch_bounds__(256) void lgar_network_pool_grad_kernel(PoolGradArgs a, long long p0, long long p1) {
  for (long long p = p0 + (long long)blockIdx.x * 256 + threadIdx.x; p < p1; p += (long long)gridDim.x * 256)
    pool_walk_back<GP>(a, net_reach(a.mc.order, p, a.mc.B));
}

static dim3 pool_level_grid(long long width) {
  const long long blocks = (width + 255) / 256;
  return dim3((unsigned)(blocks < LGAR_NET_GRID_CAP ? blocks : LGAR_NET_GRID_CAP));
}

int launch_network_pool(const PoolArgs &a, const int32_t *level_ptr, const int32_t *pool_ptr, int n_levels, hipStream_t stream) {
  for (int l = 0; l < n_levels; l++) {
    const long long p0 = level_ptr[l], pm = pool_ptr[l], p1 = level_ptr[l + 1];
    if (pm > p0) hipLaunchKernelGGL(lgar_network_pool_reach_kernel, pool_level_grid(pm - p0), dim3(256), 0, stream, a.mc, p0, pm);
    if (p1 > pm) hipLaunchKernelGGL(lgar_network_pool_kernel, pool_level_grid(p1 - pm), dim3(256), 0, stream, a, pm, p1);
  }
  return launch_status();
}

int launch_network_pool_grad(const PoolGradArgs &a, const int32_t *level_ptr, const int32_t *pool_ptr, int n_levels, hipStream_t stream) {
  for (int l = n_levels - 1; l >= 0; l--) {
    const long long p0 = level_ptr[l], pm = pool_ptr[l], p1 = level_ptr[l + 1];
    if (pm > p0) {
      if (a.mc.gpar) hipLaunchKernelGGL(lgar_network_pool_reach_grad_kernel<true>, pool_level_grid(pm - p0), dim3(256), 0, stream, a.mc, p0, pm);
      else hipLaunchKernelGGL(lgar_network_pool_reach_grad_kernel<false>, pool_level_grid(pm - p0), dim3(256), 0, stream, a.mc, p0, pm);
    }
    if (p1 > pm) {
      if (a.gpool) hipLaunchKernelGGL(lgar_network_pool_grad_kernel<true>, pool_level_grid(p1 - pm), dim3(256), 0, stream, a, pm, p1);
      else hipLaunchKernelGGL(lgar_network_pool_grad_kernel<false>, pool_level_grid(p1 - pm), dim3(256), 0, stream, a, pm, p1);
    }
  }
  return launch_status();
}

}  // namespace lgar

// The C-ABI entry points live here: every other translation unit stays byte-identical.
extern "C" {

int32_t lgar_network_route_pool(const double *x, int32_t n_rows, int32_t n_catchments, const double *par_mc, const double *par_pool,
                                int32_t n_pools, double dt_h, double rmin, double rmax, double prmin, double prmax,
                                const int32_t *up_ptr, const int32_t *up_idx, int32_t n_edges, const int32_t *order,
                                const int32_t *level_ptr, const int32_t *pool_ptr, int32_t n_levels, const int32_t *pool_slot,
                                const double *state_in, double *state_out, double *y, double *storage, void *stream) {
  const int rc = lgar::pool_route_check(x, n_rows, n_catchments, par_mc, par_pool, n_pools, dt_h, rmin, rmax, prmin, prmax, up_ptr, up_idx,
                                        n_edges, order, level_ptr, pool_ptr, n_levels, pool_slot, state_out, y);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::PoolArgs a;
  a.mc.x = x, a.mc.par = par_mc, a.mc.state_in = state_in, a.mc.y = y, a.mc.state_out = state_out;
  a.mc.order = order, a.mc.up_ptr = up_ptr, a.mc.up_idx = up_idx;
  a.mc.dt_h = dt_h, a.mc.rmin = rmin, a.mc.rmax = rmax;
  a.mc.T = n_rows, a.mc.B = n_catchments, a.mc.E = n_edges;
  a.par_pool = par_pool, a.pool_slot = pool_slot, a.storage = storage;
  a.prmin = prmin, a.prmax = prmax, a.P = n_pools;
  return lgar::launch_network_pool(a, level_ptr, pool_ptr, n_levels, (hipStream_t)stream);
}

int32_t lgar_network_route_pool_grad(const double *gy, int32_t n_rows, int32_t n_catchments, const double *par_mc, const double *par_pool,
                                     int32_t n_pools, double dt_h, double rmin, double rmax, double prmin, double prmax,
                                     const int32_t *down, const int32_t *order, const int32_t *level_ptr, const int32_t *pool_ptr,
                                     int32_t n_levels, const int32_t *pool_slot, double *gx, const double *x, const double *y,
                                     const double *storage, const int32_t *up_ptr, const int32_t *up_idx, int32_t n_edges,
                                     const double *state_in, double *gpar_mc, double *gpool, double *gstate, void *stream) {
  const int rc = lgar::pool_grad_check(gy, n_rows, n_catchments, par_mc, par_pool, n_pools, dt_h, rmin, rmax, prmin, prmax, down, order,
                                       level_ptr, pool_ptr, n_levels, pool_slot, gx, x, y, storage, up_ptr, up_idx, n_edges, gpar_mc, gpool,
                                       gstate);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::PoolGradArgs a;
  a.mc.gy = gy, a.mc.x = x, a.mc.y = y, a.mc.par = par_mc, a.mc.state_in = state_in, a.mc.gx = gx, a.mc.gpar = gpar_mc, a.mc.gstate = gstate;
  a.mc.order = order, a.mc.down = down, a.mc.up_ptr = up_ptr, a.mc.up_idx = up_idx;
  a.mc.dt_h = dt_h, a.mc.rmin = rmin, a.mc.rmax = rmax;
  a.mc.T = n_rows, a.mc.B = n_catchments, a.mc.E = n_edges;
  a.par_pool = par_pool, a.storage = storage, a.pool_slot = pool_slot, a.gpool = gpool;
  a.prmin = prmin, a.prmax = prmax, a.P = n_pools;
  return lgar::launch_network_pool_grad(a, level_ptr, pool_ptr, n_levels, (hipStream_t)stream);
}

}  // extern "C"
