// TEST INFRASTRUCTURE ONLY -- the catchment-snowpack entry points of include/lgar.h with the host in the GPU's place.
//
// The per-cell walks the kernels run (lgar_py_amd/csrc/lgar_snow.hpp) are plain C++; with -DLGAR_DEVSIM they compile for the
// host, one lane after the other.  The refusals of the C-ABI wrappers are that header's own functions (sn_check /
// sn_grad_check), so this file only puts the argument blocks together: one function per entry point, with the argument list of
// include/lgar.h minus the stream.  Compiled on its own it is libsnowhost.so, which SimCatchmentSnow (tests/snow_host) puts
// behind the product's calling surface; snow_host.cpp is the stand-alone program around it, which also runs under
// AddressSanitizer + UBSan.  Never built or used by the product.
#ifndef LGAR_TESTS_SNOW_HOST_HPP
#define LGAR_TESTS_SNOW_HOST_HPP
#define LGAR_DEVSIM 1
#include <stddef.h>
#include <stdint.h>

#include "../../lgar_py_amd/csrc/lgar_snow.hpp"

extern "C" {

int32_t snowhost_catchment_snow(const double *p, const double *ta, int32_t n_rows, int32_t n_cells, const double *par, double dt_h,
                                const double *state_in, double *state_out, double *w, double *ice, double *liq) {
  const int rc = lgar::sn_check(p, ta, n_rows, n_cells, par, dt_h, state_out, w, ice, liq);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::SnArgs a;
  a.p = p, a.ta = ta, a.par = par, a.state_in = state_in, a.w = w, a.ice = ice, a.liq = liq, a.state_out = state_out;
  a.dt_h = dt_h, a.T = n_rows, a.B = n_cells;
  lgar::sn_all(a);
  return 0;
}

int32_t snowhost_catchment_snow_grad(const double *gw, const double *gice, const double *gliq, const double *p, const double *ta,
                                     const double *ice, const double *liq, int32_t n_rows, int32_t n_cells, const double *par,
                                     double dt_h, const double *state_in, double *gp, double *gta, double *gpar, double *gstate) {
  const int rc = lgar::sn_grad_check(gw, p, ta, ice, liq, n_rows, n_cells, par, dt_h, gp, gpar, gstate);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::SnGradArgs a;
  a.gw = gw, a.gice = gice, a.gliq = gliq, a.p = p, a.ta = ta, a.ice = ice, a.liq = liq, a.par = par, a.state_in = state_in;
  a.gp = gp, a.gta = gta, a.gpar = gpar, a.gstate = gstate;
  a.dt_h = dt_h, a.T = n_rows, a.B = n_cells;
  lgar::sn_grad_all(a);
  return 0;
}

}  // extern "C"
#endif
