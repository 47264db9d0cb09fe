// TEST INFRASTRUCTURE ONLY -- the catchment-canopy entry points of include/lgar.h with the host in the GPU's place.
//
// The per-cell walks the kernels run (lgar_py_amd/csrc/lgar_canopy.hpp) are plain C++; with -DLGAR_DEVSIM they compile for the
// host, one lane after the other.  The refusals of the C-ABI wrappers are that header's own functions (cn_check / cn_grad_check /
// cn_tangent_check), so this file only puts the argument blocks together: one function per entry point, with the argument list of
// include/lgar.h minus the stream.  Compiled on its own it is libcanopyhost.so, which SimCatchmentCanopy (tests/canopy_host) puts
// behind the product's calling surface; canopy_host.cpp is the stand-alone program around it, which also runs under
// AddressSanitizer + UBSan.  Never built or used by the product.
#ifndef LGAR_TESTS_CANOPY_HOST_HPP
#define LGAR_TESTS_CANOPY_HOST_HPP
#define LGAR_DEVSIM 1
#include <stddef.h>
#include <stdint.h>

#include "../../lgar_py_amd/csrc/lgar_canopy.hpp"

extern "C" {

int32_t canopyhost_catchment_canopy(const double *p, const double *e, const double *lai, int32_t n_rows, int32_t n_cells,
                                    const double *par, double dt_h, const double *state_in, double *state_out, double *w,
                                    double *pet_out, double *store, double *evap) {
  const int rc = lgar::cn_check(p, e, n_rows, n_cells, par, dt_h, state_out, w, pet_out, store, evap);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::CnArgs a;
  a.p = p, a.e = e, a.lai = lai, a.par = par, a.state_in = state_in;
  a.w = w, a.pet = pet_out, a.store = store, a.evap = evap, a.state_out = state_out;
  a.dt_h = dt_h, a.T = n_rows, a.B = n_cells;
  lgar::cn_all(a);
  return 0;
}

int32_t canopyhost_catchment_canopy_grad(const double *gw, const double *gpet, const double *gstore, const double *gevap,
                                         const double *p, const double *e, const double *lai, const double *store, int32_t n_rows,
                                         int32_t n_cells, const double *par, double dt_h, const double *state_in, double *gp,
                                         double *ge, double *glai, double *gpar, double *gstate) {
  const int rc = lgar::cn_grad_check(gw, gpet, p, e, store, n_rows, n_cells, par, dt_h, gp, ge, gpar, gstate);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::CnGradArgs a;
  a.gw = gw, a.gpet = gpet, a.gstore = gstore, a.gevap = gevap, a.p = p, a.e = e, a.lai = lai, a.store = store, a.par = par;
  a.state_in = state_in, a.gp = gp, a.ge = ge, a.glai = glai, a.gpar = gpar, a.gstate = gstate;
  a.dt_h = dt_h, a.T = n_rows, a.B = n_cells;
  lgar::cn_grad_all(a);
  return 0;
}

int32_t canopyhost_catchment_canopy_tangent(const double *p, const double *e, const double *lai, int32_t n_rows, int32_t n_cells,
                                            const double *par, double dt_h, const double *state_in, int32_t n_dirs, const double *dp,
                                            const double *de, const double *dlai, const double *dpar, const double *dstate_in,
                                            double *dw, double *dpet, int32_t ld, int32_t k0, double *dstore, double *devap,
                                            double *dstate_out) {
  const int rc = lgar::cn_tangent_check(p, e, n_rows, n_cells, par, dt_h, n_dirs, dw, ld, k0, dstore, devap, dstate_out);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::CnTanArgs a;
  a.p = p, a.e = e, a.lai = lai, a.par = par, a.state_in = state_in;
  a.dp = dp, a.de = de, a.dlai = dlai, a.dpar = dpar, a.dstate_in = dstate_in;
  a.dw = dw, a.dpet = dpet, a.dstore = dstore, a.devap = devap, a.dstate_out = dstate_out;
  a.dt_h = dt_h, a.T = n_rows, a.B = n_cells, a.D = n_dirs, a.ld = ld, a.k0 = k0;
  lgar::cn_tangent_all(a);
  return 0;
}

}  // extern "C"
#endif
