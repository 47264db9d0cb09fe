// TEST INFRASTRUCTURE ONLY -- the host build of the soil-moisture tangent (lgar_py_amd/csrc/lgar_moisture_tangent.hpp).
//
// The per-column function the kernel runs is plain C++; with -DLGAR_DEVSIM it compiles for the host, one lane after the other.
// This header holds what lgar_moisture_tangent.hip puts around it -- the refusals (moist_tangent_check, shared with the library),
// the early-out of a job without lanes, the dispatch over the compiled bin capacities and the lane loop -- with the argument
// list of include/lgar.h minus the stream.  Compiled on its own it is libmthost.so, which MoistureTangentSimEngine puts behind the
// product's calling surface; moisture_tangent_host.cpp is the stand-alone program around it, which also runs under
// AddressSanitizer + UBSan.  Never built or used by the product.
#ifndef LGAR_TESTS_MOISTURE_TANGENT_HOST_HPP
#define LGAR_TESTS_MOISTURE_TANGENT_HOST_HPP
#define LGAR_DEVSIM 1
#include <stddef.h>
#include <stdint.h>

#include "../../lgar_py_amd/csrc/lgar_moisture_tangent.hpp"

namespace mthost {

template <typename R>
void typed(const LgarDims *d, const LgarParams *p, const LgarState *s, const LgarState *ds, const double *edges, int nb, int what,
           void *out, const double *cot, int group, void *grad) {
  const R *depth = (const R *)s->depth, *theta = (const R *)s->theta, *dd = (const R *)ds->depth, *dth = (const R *)ds->theta;
  const R *thick = (const R *)p->thickness;
  const size_t n = (size_t)d->n_columns, g = (size_t)group;
  const int L = d->n_layers, F = d->front_slots > 0 ? d->front_slots : LGAR_FMAX;
  R *o = (R *)out, *gr = (R *)grad;
  for (size_t c = 0; c < n; c++) {
    // the kernel's dispatch (lgar_moisture_tangent.hip): layer bins, or the smallest compiled bin capacity that fits
    if (!edges)
      lgar::moist_tangent_column<R, 8, true>(depth, theta, s->flags, s->n_fronts, dd, dth, thick, nullptr, n, c, L, F, nb, what, o, cot, g, gr);
    else if (nb <= 8)
      lgar::moist_tangent_column<R, 8, false>(depth, theta, s->flags, s->n_fronts, dd, dth, thick, edges, n, c, L, F, nb, what, o, cot, g, gr);
    else if (nb <= 16)
      lgar::moist_tangent_column<R, 16, false>(depth, theta, s->flags, s->n_fronts, dd, dth, thick, edges, n, c, L, F, nb, what, o, cot, g, gr);
    else
      lgar::moist_tangent_column<R, LGAR_MOIST_BINS, false>(depth, theta, s->flags, s->n_fronts, dd, dth, thick, edges, n, c, L, F, nb, what, o,
                                                            cot, g, gr);
  }
}

}  // namespace mthost

extern "C" int32_t mthost_soil_moisture_tangent(const LgarDims *dims, const LgarParams *params, const LgarState *state,
                                                const LgarState *dstate, const double *edges, int32_t n_bins, int32_t what, void *out,
                                                const double *cot, int32_t group, void *grad, int32_t dtype) {
  const int rc = lgar::moist_tangent_check(dims, params, state, dstate, edges, n_bins, what, out, cot, group, grad, dtype);
  if (rc) return rc;
  if (dims->n_columns == 0) return 0;
  if (dtype == LGAR_F64) mthost::typed<double>(dims, params, state, dstate, edges, n_bins, what, out, cot, group, grad);
  else mthost::typed<float>(dims, params, state, dstate, edges, n_bins, what, out, cot, group, grad);
  return 0;
}
#endif
