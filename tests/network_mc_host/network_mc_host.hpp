// TEST INFRASTRUCTURE ONLY -- the Muskingum-Cunge network entry points of include/lgar.h with the host in the GPU's place.
//
// The per-reach walks the kernels run (lgar_py_amd/csrc/lgar_network_mc.hpp) are plain C++; with -DLGAR_DEVSIM they compile for
// the host, one lane after the other, one level after the other.  The refusals of the C-ABI wrappers are that header's own
// functions (mc_route_check / mc_grad_check), so this file only puts the argument blocks together: one function per entry point,
// with the argument list of include/lgar.h minus the stream, and mc_ln over an array.  Compiled on its own it is
// libnetworkmchost.so, which SimCatchmentNetworkMC (tests/network_mc_host) puts behind the product's calling surface next to
// libnetworkhost.so; network_mc_host.cpp is the stand-alone program around it, which also runs under AddressSanitizer + UBSan.
// Never built or used by the product.
#ifndef LGAR_TESTS_NETWORK_MC_HOST_HPP
#define LGAR_TESTS_NETWORK_MC_HOST_HPP
#define LGAR_DEVSIM 1
#include <stddef.h>
#include <stdint.h>

#include "../../lgar_py_amd/csrc/lgar_network_mc.hpp"

extern "C" {

int32_t networkmchost_network_route_mc(const double *x, int32_t n_rows, int32_t n_catchments, const double *par, double dt_h, double rmin,
                                       double rmax, const int32_t *up_ptr, const int32_t *up_idx, int32_t n_edges, const int32_t *order,
                                       const int32_t *level_ptr, int32_t n_levels, const double *state_in, double *state_out, double *y) {
  const int rc = lgar::mc_route_check(x, n_rows, n_catchments, par, dt_h, rmin, rmax, up_ptr, up_idx, n_edges, order, level_ptr, n_levels,
                                      state_out, y);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::McArgs a;
  a.x = x, a.par = par, a.state_in = state_in, a.y = y, a.state_out = state_out;
  a.order = order, a.up_ptr = up_ptr, a.up_idx = up_idx;
  a.dt_h = dt_h, a.rmin = rmin, a.rmax = rmax;
  a.T = n_rows, a.B = n_catchments, a.E = n_edges;
  lgar::mc_route_all(a, level_ptr, n_levels);
  return 0;
}

int32_t networkmchost_network_route_mc_grad(const double *gy, int32_t n_rows, int32_t n_catchments, const double *par, double dt_h,
                                            double rmin, double rmax, const int32_t *down, const int32_t *order, const int32_t *level_ptr,
                                            int32_t n_levels, double *gx, const double *x, const double *y, const int32_t *up_ptr,
                                            const int32_t *up_idx, int32_t n_edges, const double *state_in, double *gpar, double *gstate) {
  const int rc = lgar::mc_grad_check(gy, n_rows, n_catchments, par, dt_h, rmin, rmax, down, order, level_ptr, n_levels, gx, x, y, up_ptr,
                                     up_idx, n_edges, gpar, gstate);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::McGradArgs a;
  a.gy = gy, a.x = x, a.y = y, a.par = par, a.state_in = state_in, a.gx = gx, a.gpar = gpar, a.gstate = gstate;
  a.order = order, a.down = down, a.up_ptr = up_ptr, a.up_idx = up_idx;
  a.dt_h = dt_h, a.rmin = rmin, a.rmax = rmax;
  a.T = n_rows, a.B = n_catchments, a.E = n_edges;
  lgar::mc_grad_all(a, level_ptr, n_levels);
  return 0;
}

void networkmchost_mc_ln(const double *x, int32_t n, double *out) {
  for (int32_t i = 0; i < n; i++) out[i] = lgar::mc_ln(x[i]);
}

}  // extern "C"
#endif
