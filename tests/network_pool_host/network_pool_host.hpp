// TEST INFRASTRUCTURE ONLY -- the reach-and-pool network entry points of include/lgar.h with the host in the GPU's place.
//
// The per-node walks the kernels run (lgar_py_amd/csrc/lgar_network_pool.hpp, and lgar_network_mc.hpp's for the reaches) are plain
// C++; with -DLGAR_DEVSIM they compile for the host, one lane after the other, one level after the other, a level's reaches before
// its pools.  The refusals of the C-ABI wrappers are that header's own functions (pool_route_check / pool_grad_check), so this
// file only puts the argument blocks together: one function per entry point, with the argument list of include/lgar.h minus the
// stream, and the release law cq rc^m over arrays.  Compiled on its own it is libnetworkpoolhost.so, which SimCatchmentNetworkPool
// (tests/network_pool_host) puts behind the product's calling surface next to the other two network libraries;
// network_pool_host.cpp is the stand-alone program around it, which also runs under AddressSanitizer + UBSan.  Never built or
// used by the product.
#ifndef LGAR_TESTS_NETWORK_POOL_HOST_HPP
#define LGAR_TESTS_NETWORK_POOL_HOST_HPP
#define LGAR_DEVSIM 1
#include <stddef.h>
#include <stdint.h>

#include "../../lgar_py_amd/csrc/lgar_network_pool.hpp"

extern "C" {

int32_t networkpoolhost_network_route_pool(const double *x, int32_t n_rows, int32_t n_catchments, const double *par_mc, const double *par_pool,
                                           int32_t n_pools, double dt_h, double rmin, double rmax, double prmin, double prmax,
                                           const int32_t *up_ptr, const int32_t *up_idx, int32_t n_edges, const int32_t *order,
                                           const int32_t *level_ptr, const int32_t *pool_ptr, int32_t n_levels, const int32_t *pool_slot,
                                           const double *state_in, double *state_out, double *y, double *storage) {
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
  lgar::pool_route_all(a, level_ptr, pool_ptr, n_levels);
  return 0;
}

int32_t networkpoolhost_network_route_pool_grad(const double *gy, int32_t n_rows, int32_t n_catchments, const double *par_mc,
                                                const double *par_pool, int32_t n_pools, double dt_h, double rmin, double rmax, double prmin,
                                                double prmax, const int32_t *down, const int32_t *order, const int32_t *level_ptr,
                                                const int32_t *pool_ptr, int32_t n_levels, const int32_t *pool_slot, double *gx,
                                                const double *x, const double *y, const double *storage, const int32_t *up_ptr,
                                                const int32_t *up_idx, int32_t n_edges, const double *state_in, double *gpar_mc,
                                                double *gpool, double *gstate) {
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
  lgar::pool_grad_all(a, level_ptr, pool_ptr, n_levels);
  return 0;
}

// Ql of pool_row for cq = 1 (the release law rc^m as the row forms it) from rc = a / sref with s0 = 0, sref = 1
void networkpoolhost_release(const double *rc, const double *m, int32_t n, double prmin, double prmax, double *out) {
  for (int32_t i = 0; i < n; i++) out[i] = lgar::pool_row(rc[i], 0.0, 1.0, m[i], 0.0, 1.0, 1.0, 1.0, prmin, prmax).Ql;
}

}  // extern "C"
#endif
