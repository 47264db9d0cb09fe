// TEST INFRASTRUCTURE ONLY -- the catchment-baseflow entry points of include/lgar.h with the host in the GPU's place.
//
// The per-catchment walks the kernels run (lgar_py_amd/csrc/lgar_baseflow.hpp) are plain C++; with -DLGAR_DEVSIM they compile
// for the host, one lane after the other.  The refusals of the C-ABI wrappers are that header's own functions (gw_check /
// gw_grad_check), so this file only puts the argument blocks together: one function per entry point, with the argument list of
// include/lgar.h minus the stream, and gw_exp on an array.  Compiled on its own it is libbaseflowhost.so, which
// SimCatchmentBaseflow (tests/baseflow_host) puts behind the product's calling surface; baseflow_host.cpp is the stand-alone
// program around it, which also runs under AddressSanitizer + UBSan.  Never built or used by the product.
#ifndef LGAR_TESTS_BASEFLOW_HOST_HPP
#define LGAR_TESTS_BASEFLOW_HOST_HPP
#define LGAR_DEVSIM 1
#include <stddef.h>
#include <stdint.h>

#include "../../lgar_py_amd/csrc/lgar_baseflow.hpp"

extern "C" {

int32_t baseflowhost_catchment_baseflow(const double *r, int32_t n_rows, int32_t n_catchments, const double *par, double dt_h,
                                        const double *state_in, double *state_out, double *q, double *s) {
  const int rc = lgar::gw_check(r, n_rows, n_catchments, par, dt_h, state_out, q);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::GwArgs a;
  a.r = r, a.par = par, a.state_in = state_in, a.q = q, a.s = s, a.state_out = state_out;
  a.dt_h = dt_h, a.T = n_rows, a.B = n_catchments;
  lgar::gw_all(a);
  return 0;
}

int32_t baseflowhost_catchment_baseflow_grad(const double *gq, const double *gs, const double *r, const double *s, int32_t n_rows,
                                             int32_t n_catchments, const double *par, double dt_h, const double *state_in, double *gr,
                                             double *gpar, double *gstate) {
  const int rc = lgar::gw_grad_check(gq, r, s, n_rows, n_catchments, par, dt_h, gr, gpar, gstate);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::GwGradArgs a;
  a.gq = gq, a.gs = gs, a.r = r, a.s = s, a.par = par, a.state_in = state_in, a.gr = gr, a.gpar = gpar, a.gstate = gstate;
  a.dt_h = dt_h, a.T = n_rows, a.B = n_catchments;
  lgar::gw_grad_all(a);
  return 0;
}

// out[i] = gw_exp(z[i])
void baseflowhost_gw_exp(const double *z, int32_t n, double *out) {
  for (int32_t i = 0; i < n; i++) out[i] = lgar::gw_exp(z[i]);
}

}  // extern "C"
#endif
