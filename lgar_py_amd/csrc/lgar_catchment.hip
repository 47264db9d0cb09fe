// lgar_catchment.hip -- the catchment kernels (lgar_catchment_sums / lgar_catchment_spread, include/lgar.h;
// lgar_catchment.hpp holds the per-lane accumulation, the combine order and the definition).
//
// Sums: ONE wave per (row, catchment), which owns out[row][catchment] and writes it: no atomics, nothing to zero -- in jobs of
// many catchments one wave per (four rows, catchment), which reads column, status and weight once for its four rows (the same
// bits: each row has its own partials).  Waves are numbered row-major (catchment fastest), so the waves in flight together
// read neighbouring stretches of one row.  Without
// `order` a wave's loads are lane-contiguous (256 B per load instruction in fp32); with it they gather.  A lane keeps up to 16
// loads in flight.  The grid is capped and the waves stride over the (row, catchment) pairs, so any rows x catchments launches.
// Spread: element-wise, one lane per column, rows lane-contiguous; a lane reads its column's catchment, weight and status once
// and walks the rows.
#include <hip/hip_runtime.h>

#include "lgar_catchment.hpp"
#include "lgar_host.hpp"

namespace lgar {

template <typename R> struct CatchSumArgs {
  const R *series, *weights;
  const int32_t *status, *order, *offsets;
  double *out;
  long long n_columns, n_order, n_rows, n_catchments;
};

// NR: rows a wave carries its catchment through (row groups of NR; the last one may be ragged)
template <typename R, int NR> __global__ __launch_bounds__(256) void lgar_catchment_sums_kernel(CatchSumArgs<R> a) {
  const int lane = (int)(threadIdx.x & 63u);
  const long long waves = (long long)gridDim.x * 4;
  const long long groups = (a.n_rows + NR - 1) / NR;
  const long long total = groups * a.n_catchments;
  for (long long w = (long long)blockIdx.x * 4 + (long long)(threadIdx.x >> 6); w < total; w += waves) {
    const long long tg = w / a.n_catchments, b = w - tg * a.n_catchments;
    const long long t0 = tg * NR;
    const int rows = (int)(a.n_rows - t0 < NR ? a.n_rows - t0 : NR);
    const R *row = a.series ? a.series + (size_t)t0 * (size_t)a.n_columns : nullptr;
    const CatchRow<R> r = catch_row<R>(row, rows, a.weights, a.status, a.order, a.n_order, a.n_columns);
    long long lo, n;
    catch_range(a.offsets, b, r.len, lo, n);
    double q[NR];
    catch_lane<R, NR>(r, lo, n, lane, q);
#pragma unroll
    for (int i = 0; i < NR; i++) {
      const double v = catch_butterfly(q[i]);
      if (lane == 0 && i < rows) a.out[(size_t)(t0 + i) * (size_t)a.n_catchments + (size_t)b] = v;
    }
  }
}

template <typename R> struct CatchSpreadArgs {
  const double *grad;
  const R *weights;
  const int32_t *status, *catchment_of;
  R *out;
  long long n_columns, n_rows, n_catchments;
};

template <typename R> __global__ __launch_bounds__(256) void lgar_catchment_spread_kernel(CatchSpreadArgs<R> a) {
  const size_t c = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (c >= (size_t)a.n_columns) return;
  const int32_t cat = a.catchment_of[c];
  const int32_t st = a.status ? a.status[c] : 0;
  const double w = a.weights ? (double)a.weights[c] : 1.0;
  for (long long t = blockIdx.y; t < a.n_rows; t += gridDim.y)
    a.out[(size_t)t * (size_t)a.n_columns + c] = catch_spread<R>(a.grad + (size_t)t * (size_t)a.n_catchments, a.n_catchments, cat, st, w);
}

template <typename R>
static void sums_typed(const void *series, long long n_rows, int n_columns, const int32_t *offsets, int n_catchments,
                       const int32_t *order, int n_order, const void *weights, const int32_t *status, double *out,
                       hipStream_t stream) {
  CatchSumArgs<R> a;
  a.series = (const R *)series;
  a.weights = (const R *)weights;
  a.status = status;
  a.order = order;
  a.offsets = offsets;
  a.out = out;
  a.n_columns = n_columns;
  a.n_order = n_order;
  a.n_rows = n_rows;
  a.n_catchments = n_catchments;
  // A wave carries its catchment through four rows at a time (column, status and weight read once for the four) when that
  // still leaves every wave slot of the chip several waves; a job of few catchments keeps one wave per (row, catchment).
  // Four waves per workgroup; the grid is capped at four times the chip's wave slots at 8 waves per SIMD (the rest by stride).
  const long long cap = (long long)wave_slots(8);
  const bool four = ((n_rows + 3) / 4) * (long long)n_catchments >= 4 * cap;
  const long long blocks = ((four ? (n_rows + 3) / 4 : n_rows) * (long long)n_catchments + 3) / 4;
  const dim3 grid((unsigned)(blocks < cap ? blocks : cap));
  if (four) hipLaunchKernelGGL((lgar_catchment_sums_kernel<R, 4>), grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((lgar_catchment_sums_kernel<R, 1>), grid, dim3(256), 0, stream, a);
}

int launch_catchment_sums(const void *series, int n_rows, int n_columns, const int32_t *offsets, int n_catchments,
                          const int32_t *order, int n_order, const void *weights, const int32_t *status, double *out,
                          double *weight_sums, int dtype, hipStream_t stream) {
  if (dtype != LGAR_F32 && dtype != LGAR_F64) return LGAR_E_ARG;
  if (n_catchments == 0) return 0;
  if (n_rows > 0) {
    if (dtype == LGAR_F64) sums_typed<double>(series, n_rows, n_columns, offsets, n_catchments, order, n_order, weights, status, out, stream);
    else sums_typed<float>(series, n_rows, n_columns, offsets, n_catchments, order, n_order, weights, status, out, stream);
  }
  if (weight_sums) {  // the same pass over one row of ones: the terms are the weights themselves
    if (dtype == LGAR_F64) sums_typed<double>(nullptr, 1, n_columns, offsets, n_catchments, order, n_order, weights, status, weight_sums, stream);
    else sums_typed<float>(nullptr, 1, n_columns, offsets, n_catchments, order, n_order, weights, status, weight_sums, stream);
  }
  return launch_status();
}

template <typename R>
static void spread_typed(const double *grad, int n_rows, int n_catchments, const int32_t *catchment_of, int n_columns,
                         const void *weights, const int32_t *status, void *out, hipStream_t stream) {
  CatchSpreadArgs<R> a;
  a.grad = grad;
  a.weights = (const R *)weights;
  a.status = status;
  a.catchment_of = catchment_of;
  a.out = (R *)out;
  a.n_columns = n_columns;
  a.n_rows = n_rows;
  a.n_catchments = n_catchments;
  const dim3 grid((unsigned)(((size_t)n_columns + 255u) / 256u), (unsigned)(n_rows < 1024 ? n_rows : 1024));
  hipLaunchKernelGGL(lgar_catchment_spread_kernel<R>, grid, dim3(256), 0, stream, a);
}

int launch_catchment_spread(const double *grad, int n_rows, int n_catchments, const int32_t *catchment_of, int n_columns,
                            const void *weights, const int32_t *status, void *out, int dtype, hipStream_t stream) {
  if (dtype != LGAR_F32 && dtype != LGAR_F64) return LGAR_E_ARG;
  if (n_rows == 0 || n_columns == 0) return 0;
  if (dtype == LGAR_F64) spread_typed<double>(grad, n_rows, n_catchments, catchment_of, n_columns, weights, status, out, stream);
  else spread_typed<float>(grad, n_rows, n_catchments, catchment_of, n_columns, weights, status, out, stream);
  return launch_status();
}

}  // namespace lgar
