// lgar_moisture_tangent.hip -- the soil-moisture tangent kernel (lgar_soil_moisture_tangent, include/lgar.h): the derivative of the
// depth bins along a tangent state's direction, one lane per lane-column (lgar_moisture_tangent.hpp holds the per-column function
// and the definition).
//
// Memory-bound like the value kernel: a wave reads each front row of its 64 lanes once (depth, theta, the flag byte and the two
// tangent rows, lane-contiguous, up to its largest n_fronts), n_fronts and the thicknesses; the bins are accumulated in registers,
// so traffic does not grow with the bin count.  It writes n_bins lane-contiguous rows (out), or reads n_bins rows of the cotangent
// and updates one row (grad), or both.  No LDS, no atomics; compiled for bin capacities 8, 16 and LGAR_MOIST_BINS.
#include <hip/hip_runtime.h>

#include "lgar_host.hpp"
#include "lgar_moisture_tangent.hpp"

#ifndef LGAR_NO_TANGENT
namespace lgar {

template <typename R> struct MoistTangentArgs {
  const R *depth, *theta, *ddepth, *dtheta, *thickness;
  const uint8_t *flags;
  const int32_t *n_fronts;
  const double *edges, *cot;
  R *out, *grad;
  long long N, group;
  int n_layers, front_slots, n_bins, what;
};

template <typename R, int NB, bool LAYER_BINS>
__global__ __launch_bounds__(256) void lgar_moisture_tangent_kernel(MoistTangentArgs<R> a) {
  const size_t c = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (c >= (size_t)a.N) return;
  moist_tangent_column<R, NB, LAYER_BINS>(a.depth, a.theta, a.flags, a.n_fronts, a.ddepth, a.dtheta, a.thickness, a.edges, (size_t)a.N, c,
                                          a.n_layers, a.front_slots, a.n_bins, a.what, a.out, a.cot, (size_t)a.group, a.grad);
}

template <typename R>
static int launch_typed(const LgarDims *dims, const LgarParams *params, const LgarState *state, const LgarState *dstate,
                        const double *edges, int n_bins, int what, void *out, const double *cot, int group, void *grad,
                        hipStream_t stream) {
  MoistTangentArgs<R> a;
  a.depth = (const R *)state->depth;
  a.theta = (const R *)state->theta;
  a.ddepth = (const R *)dstate->depth;
  a.dtheta = (const R *)dstate->theta;
  a.thickness = (const R *)params->thickness;
  a.flags = state->flags;
  a.n_fronts = state->n_fronts;
  a.edges = edges;
  a.cot = cot;
  a.out = (R *)out;
  a.grad = (R *)grad;
  a.N = dims->n_columns;
  a.group = group;
  a.n_layers = dims->n_layers;
  a.front_slots = front_slots(dims);
  a.n_bins = n_bins;
  a.what = what;
  const dim3 grid((unsigned)(((size_t)dims->n_columns + 255u) / 256u)), block(256);
  if (edges == nullptr) hipLaunchKernelGGL((lgar_moisture_tangent_kernel<R, 8, true>), grid, block, 0, stream, a);
  else if (n_bins <= 8) hipLaunchKernelGGL((lgar_moisture_tangent_kernel<R, 8, false>), grid, block, 0, stream, a);
  else if (n_bins <= 16) hipLaunchKernelGGL((lgar_moisture_tangent_kernel<R, 16, false>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((lgar_moisture_tangent_kernel<R, LGAR_MOIST_BINS, false>), grid, block, 0, stream, a);
  return launch_status();
}

int launch_soil_moisture_tangent(const LgarDims *dims, const LgarParams *params, const LgarState *state, const LgarState *dstate,
                                 const double *edges, int n_bins, int what, void *out, const double *cot, int group, void *grad,
                                 int dtype, hipStream_t stream) {
  static_assert(LGAR_LMAX <= 8 && LGAR_MOIST_BINS >= 16, "bin capacities of the kernel");
  if (dtype == LGAR_F64) return launch_typed<double>(dims, params, state, dstate, edges, n_bins, what, out, cot, group, grad, stream);
  if (dtype == LGAR_F32) return launch_typed<float>(dims, params, state, dstate, edges, n_bins, what, out, cot, group, grad, stream);
  return LGAR_E_ARG;
}

}  // namespace lgar

extern "C" int32_t lgar_soil_moisture_tangent(const LgarDims *dims, const LgarParams *params, const LgarState *state,
                                              const LgarState *dstate, const double *edges, int32_t n_bins, int32_t what, void *out,
                                              const double *cot, int32_t group, void *grad, int32_t dtype, void *stream) {
  using namespace lgar;
  if (!dims) return LGAR_E_ARG;
  LgarDims d = *dims;  // what lgar_soil_moisture refuses of the dims, but for a job of no lanes
  if (d.n_columns == 0) d.n_columns = 1, d.forcing_group = 0, d.tangent_share = 0;
  int rc = check_dims(&d);
  if (rc) return rc;
  rc = moist_tangent_check(dims, params, state, dstate, edges, n_bins, what, out, cot, group, grad, dtype);
  if (rc) return rc;
  if (dims->n_columns == 0) return 0;
  return launch_soil_moisture_tangent(dims, params, state, dstate, edges, n_bins, what, out, cot, group, grad, dtype, (hipStream_t)stream);
}
#endif
