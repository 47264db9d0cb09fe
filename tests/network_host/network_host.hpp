// TEST INFRASTRUCTURE ONLY -- the catchment-network entry points of include/lgar.h with the host in the GPU's place.
//
// The per-reach walks the kernels run (lgar_py_amd/csrc/lgar_network.hpp) are plain C++; with -DLGAR_DEVSIM they compile for the
// host, one lane after the other, one level after the other.  The refusals of the C-ABI wrappers are that header's own
// functions (net_route_check / net_grad_check), so this file only puts the argument blocks together: one function per entry
// point, with the argument list of include/lgar.h minus the stream.  Compiled on its own it is libnetworkhost.so, which
// SimCatchmentNetwork (tests/network_host) puts behind the product's calling surface; network_host.cpp is the stand-alone
// program around it, which also runs under AddressSanitizer + UBSan.  Never built or used by the product.
#ifndef LGAR_TESTS_NETWORK_HOST_HPP
#define LGAR_TESTS_NETWORK_HOST_HPP
#define LGAR_DEVSIM 1
#include <stddef.h>
#include <stdint.h>

#include "../../lgar_py_amd/csrc/lgar_network.hpp"

extern "C" {

int32_t networkhost_network_route(const double *x, int32_t n_rows, int32_t n_catchments, const double *coef, const int32_t *up_ptr,
                                  const int32_t *up_idx, int32_t n_edges, const int32_t *order, const int32_t *level_ptr,
                                  int32_t n_levels, const double *state_in, double *state_out, double *y) {
  const int rc = lgar::net_route_check(x, n_rows, n_catchments, coef, up_ptr, up_idx, n_edges, order, level_ptr, n_levels, state_out, y);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::NetArgs a;
  a.x = x, a.coef = coef, a.state_in = state_in, a.y = y, a.state_out = state_out;
  a.order = order, a.up_ptr = up_ptr, a.up_idx = up_idx;
  a.T = n_rows, a.B = n_catchments, a.E = n_edges;
  lgar::net_route_all(a, level_ptr, n_levels);
  return 0;
}

int32_t networkhost_network_route_grad(const double *gy, int32_t n_rows, int32_t n_catchments, const double *coef, const int32_t *down,
                                       const int32_t *order, const int32_t *level_ptr, int32_t n_levels, double *gx, const double *x,
                                       const double *y, const int32_t *up_ptr, const int32_t *up_idx, int32_t n_edges,
                                       const double *state_in, double *gc) {
  const int rc = lgar::net_grad_check(gy, n_rows, n_catchments, coef, down, order, level_ptr, n_levels, gx, x, y, up_ptr, up_idx, n_edges, gc);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::NetGradArgs a;
  a.gy = gy, a.coef = coef, a.x = x, a.y = y, a.state_in = state_in, a.gx = gx, a.gc = gc;
  a.order = order, a.down = down, a.up_ptr = up_ptr, a.up_idx = up_idx;
  a.T = n_rows, a.B = n_catchments, a.E = n_edges;
  lgar::net_grad_all(a, level_ptr, n_levels);
  return 0;
}

}  // extern "C"
#endif
