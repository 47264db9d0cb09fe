// lgar_moisture.hip -- the soil-moisture kernel (lgar_soil_moisture, include/lgar.h): depth-binned water content from the
// front table, one lane per column (lgar_moisture.hpp holds the per-column function and the definition).
//
// Memory-bound by construction: a wave reads each front row of its 64 columns once (up to its largest n_fronts; depth, theta
// and the flag byte, lane-contiguous), n_fronts and the thicknesses, and writes n_bins lane-contiguous rows; the bins are
// accumulated in registers, so traffic does not grow with the bin count.  The kernel is compiled for bin capacities 8, 16 and
// LGAR_MOIST_BINS (the accumulators of the unused bins cost registers, nothing else).
#include <hip/hip_runtime.h>

#include "lgar_host.hpp"
#include "lgar_moisture.hpp"

namespace lgar {

template <typename R> struct MoistArgs {
  const R *depth, *theta, *thickness;
  const uint8_t *flags;
  const int32_t *n_fronts;
  const double *edges;
  R *out;
  long long N;
  int n_layers, front_slots, n_bins, what;
};

template <typename R, int NB, bool LAYER_BINS> __global__ __launch_bounds__(256) void lgar_moisture_kernel(MoistArgs<R> a) {
  const size_t c = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (c >= (size_t)a.N) return;
  moist_column<R, NB, LAYER_BINS>(a.depth, a.theta, a.flags, a.n_fronts, a.thickness, a.edges, (size_t)a.N, c, a.n_layers,
                                  a.front_slots, a.n_bins, a.what, a.out);
}

template <typename R>
static int launch_typed(const LgarDims *dims, const LgarParams *params, const LgarState *state, const double *edges, int n_bins,
                        int what, void *out, hipStream_t stream) {
  MoistArgs<R> a;
  a.depth = (const R *)state->depth;
  a.theta = (const R *)state->theta;
  a.thickness = (const R *)params->thickness;
  a.flags = state->flags;
  a.n_fronts = state->n_fronts;
  a.edges = edges;
  a.out = (R *)out;
  a.N = dims->n_columns;
  a.n_layers = dims->n_layers;
  a.front_slots = front_slots(dims);
  a.n_bins = n_bins;
  a.what = what;
  const dim3 grid((unsigned)(((size_t)dims->n_columns + 255u) / 256u)), block(256);
  if (edges == nullptr) hipLaunchKernelGGL((lgar_moisture_kernel<R, 8, true>), grid, block, 0, stream, a);
  else if (n_bins <= 8) hipLaunchKernelGGL((lgar_moisture_kernel<R, 8, false>), grid, block, 0, stream, a);
  else if (n_bins <= 16) hipLaunchKernelGGL((lgar_moisture_kernel<R, 16, false>), grid, block, 0, stream, a);
  else hipLaunchKernelGGL((lgar_moisture_kernel<R, LGAR_MOIST_BINS, false>), grid, block, 0, stream, a);
  return launch_status();
}

// one lane per column; rows are lane-contiguous.  The adds are the forward kernels' own (tot = tot + acc, in R, step by step)
template <typename R> struct ReplayArgs {
  const R *series[7];
  R *running;
  long long N;
  int n_rows;
};

template <typename R> __global__ __launch_bounds__(256) void lgar_totals_replay_kernel(ReplayArgs<R> a) {
  const size_t c = (size_t)blockIdx.x * 256u + threadIdx.x;
  const size_t N = (size_t)a.N;
  if (c >= N) return;
#pragma unroll
  for (int j = 0; j < 7; j++) {
    if (a.series[j] == nullptr) continue;
    R r = a.running[(size_t)j * N + c];
    for (int t = 0; t < a.n_rows; t++) r = r + a.series[j][(size_t)t * N + c];
    a.running[(size_t)j * N + c] = r;
  }
}

template <typename R>
static int replay_typed(const LgarDims *dims, const LgarStepOut *stored, int n_rows, void *running, hipStream_t stream) {
  ReplayArgs<R> a;
  for (int j = 0; j < 7; j++) a.series[j] = (const R *)stored->series[j];
  a.running = (R *)running;
  a.N = dims->n_columns;
  a.n_rows = n_rows;
  hipLaunchKernelGGL(lgar_totals_replay_kernel<R>, dim3((unsigned)(((size_t)dims->n_columns + 255u) / 256u)), dim3(256), 0, stream, a);
  return launch_status();
}

int launch_totals_replay(const LgarDims *dims, const LgarStepOut *stored, int n_rows, void *running, int dtype, hipStream_t stream) {
  if (dtype == LGAR_F64) return replay_typed<double>(dims, stored, n_rows, running, stream);
  if (dtype == LGAR_F32) return replay_typed<float>(dims, stored, n_rows, running, stream);
  return LGAR_E_ARG;
}

int launch_soil_moisture(const LgarDims *dims, const LgarParams *params, const LgarState *state, const double *edges,
                         int n_bins, int what, void *out, int dtype, hipStream_t stream) {
  static_assert(LGAR_LMAX <= 8 && LGAR_MOIST_BINS >= 16, "bin capacities of the kernel");
  if (n_bins < 1 || n_bins > LGAR_MOIST_BINS) return LGAR_E_ARG;
  if (dtype == LGAR_F64) return launch_typed<double>(dims, params, state, edges, n_bins, what, out, stream);
  if (dtype == LGAR_F32) return launch_typed<float>(dims, params, state, edges, n_bins, what, out, stream);
  return LGAR_E_ARG;
}

}  // namespace lgar
