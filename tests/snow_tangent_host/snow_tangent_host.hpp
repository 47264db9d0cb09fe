// TEST INFRASTRUCTURE ONLY -- lgar_catchment_snow_tangent of include/lgar.h with the host in the GPU's place: the per-lane walk the
// kernel runs (lgar_py_amd/csrc/lgar_snow.hpp, sn_walk_tangent) compiled with -DLGAR_DEVSIM, one lane after the other, behind the
// header's own refusals (sn_tangent_check).  The argument list is include/lgar.h's minus the stream.  libsnowtanhost.so is this
// header as a library; snow_tangent_host.cpp is the stand-alone program around it, which also runs under AddressSanitizer +
// UBSan.  Never built or used by the product.
#ifndef LGAR_TESTS_SNOW_TANGENT_HOST_HPP
#define LGAR_TESTS_SNOW_TANGENT_HOST_HPP
#define LGAR_DEVSIM 1
#include <stddef.h>
#include <stdint.h>

#include "../../lgar_py_amd/csrc/lgar_snow.hpp"

extern "C" {

int32_t snowtanhost_catchment_snow_tangent(const double *p, const double *ta, int32_t n_rows, int32_t n_cells, const double *par,
                                           double dt_h, const double *state_in, int32_t n_dirs, const double *dp, const double *dta,
                                           const double *dpar, const double *dstate_in, double *dw, int32_t ld, int32_t k0, double *dice,
                                           double *dliq, double *dstate_out) {
  const int rc = lgar::sn_tangent_check(p, ta, n_rows, n_cells, par, dt_h, n_dirs, dw, ld, k0, dice, dliq, dstate_out);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::SnTanArgs a;
  a.p = p, a.ta = ta, a.par = par, a.state_in = state_in, a.dp = dp, a.dta = dta, a.dpar = dpar, a.dstate_in = dstate_in;
  a.dw = dw, a.dice = dice, a.dliq = dliq, a.dstate_out = dstate_out;
  a.dt_h = dt_h, a.T = n_rows, a.B = n_cells, a.D = n_dirs, a.ld = ld, a.k0 = k0;
  lgar::sn_tangent_all(a);
  return 0;
}

}  // extern "C"
#endif
