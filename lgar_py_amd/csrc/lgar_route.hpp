// lgar_route.hpp -- catchment routing: one unit hydrograph per catchment over the [T][B] matrix of catchment sums, its adjoint
// and the gradient with respect to the ordinates (lgar_catchment_route / lgar_catchment_route_grad, include/lgar.h has the full
// statement).
//
// All arrays are fp64, catchment fastest.  The definition is the reference's queue recurrence (lgar/giuh.py:8-20 without its
// skip test); what is computed here is the equivalent fold with no dependence between rows: output row r of catchment b
//
//     acc = queue_in[r][b] if r < K (and there is a queue), else +0.0
//     acc = acc + g[k][b] * x[r - k][b]   for k = min(r, K - 1) down to max(0, r - T + 1)       (oldest term first)
//
// is y[r][b] for r < T and queue_out[r - T][b] for the virtual rows r = T .. T + K - 1 (the hand-over: what the rows of the
// NEXT call still owe to the rows of this one).  One rounded product and one rounded add per term (the library is built with
// -ffp-contract=off), the chain in the order of the recurrence: the same bits.  The result for catchment b reads column b only.
//
// Reverse (the adjoint with respect to x) is the same fold under t -> T - 1 - t on input and output: the caller hands in x and
// y through a negative row stride.
//
// Ordinate gradient: g_out[k][b] = sum_{t = k}^{T - 1} gy[t][b] * x[t - k][b] from +0.0 in increasing t.  One lane carries
// LGAR_ROUTE_KG consecutive k of one catchment up the rows: gy[t] is read once for all of them and x through a window of
// registers that slides one row per step (one new x load per step), each k with its own accumulator.
//
// Like lgar_catchment.hpp this header also compiles for the host with -DLGAR_DEVSIM: tests/route_host runs the same text
// against the numpy statement of the recurrence.
#pragma once
#ifndef LGAR_DEVSIM
#include <hip/hip_runtime.h>
#define LGAR_ROUTE_FN __device__ __forceinline__
#define LGAR_ROUTE_HD __host__ __device__ __forceinline__  // what the launch code needs as well
#else
#define LGAR_ROUTE_FN inline
#define LGAR_ROUTE_HD inline
#endif
#include <stddef.h>
#include <stdint.h>

#include "../../include/lgar.h"

namespace lgar {

#define LGAR_ROUTE_LANES 64
#define LGAR_ROUTE_KG 4  // ordinates one lane of the gradient kernel carries

// One routing call.  x and y are addressed through a signed row stride: row j of the fold is x[j * x_stride] (forward: x,
// +B; reverse: the last row, -B), likewise y.  g_stride: B for per-catchment ordinates (g[k * B + b]), 1 for shared ones
// (g[k]); g_col: 1 / 0, whether b offsets g at all.
struct RouteArgs {
  const double *x, *g, *q_in;
  double *y, *q_out;
  long long T, B;
  long long x_stride, y_stride, g_stride, g_col;
  int K;
};

LGAR_ROUTE_HD RouteArgs route_args(const double *x, long long T, long long B, const double *g, int K, bool per_catchment,
                                   const double *q_in, double *q_out, double *y, bool reverse) {
  RouteArgs a;
  const long long last = T > 0 ? (T - 1) * B : 0;
  a.x = reverse ? x + last : x;
  a.y = reverse ? y + last : y;
  a.x_stride = a.y_stride = reverse ? -B : B;
  a.g = g;
  a.g_stride = per_catchment ? B : 1;
  a.g_col = per_catchment ? 1 : 0;
  a.q_in = q_in;
  a.q_out = q_out;
  a.T = T;
  a.B = B;
  a.K = K;
  return a;
}

// rows the call writes: the T rows of y and, with a queue_out, the K virtual rows behind them
LGAR_ROUTE_HD long long route_rows(const RouteArgs &a) { return a.T + (a.q_out ? a.K : 0); }

// The fold of output row r (0 <= r < T + K) of catchment b.  xat(j): x of fold row j, 0 <= j < T, of this catchment.
template <typename XAt> LGAR_ROUTE_FN double route_fold(const RouteArgs &a, long long r, long long b, XAt xat) {
  double acc = (a.q_in && r < a.K) ? a.q_in[r * a.B + b] : 0.0;
  const long long hi = r < a.K - 1 ? r : a.K - 1;
  const long long lo = r >= a.T ? r - a.T + 1 : 0;
  const double *g = a.g + b * a.g_col;
  for (long long k = hi; k >= lo; k--) acc = acc + g[k * a.g_stride] * xat(r - k);
  return acc;
}

// ... with x read from memory: K cached reads per output
LGAR_ROUTE_FN double route_fold(const RouteArgs &a, long long r, long long b) {
  return route_fold(a, r, b, [&a, b](long long j) { return a.x[j * a.x_stride + b]; });
}

// The hand-over: row r < T is y's, the virtual row T + i is queue_out[i]
LGAR_ROUTE_FN void route_store(const RouteArgs &a, long long r, long long b, double v) {
  if (r < a.T) a.y[r * a.y_stride + b] = v;
  else a.q_out[(r - a.T) * a.B + b] = v;
}

// Ordinate gradient of catchment b for k = k0 .. k0 + KG - 1 (acc[j] belongs to k0 + j; a k >= K costs nothing but the adds
// and its accumulator is dropped by the caller).  w[j] holds x[t - k0 - j]: rows before 0 do not exist and add NOTHING.
template <int KG>
LGAR_ROUTE_FN void route_grad_lane(const double *x, const double *gy, long long T, long long B, long long b, long long k0,
                                   double (&acc)[KG]) {
  double w[KG];
#pragma unroll
  for (int j = 0; j < KG; j++) acc[j] = w[j] = 0.0;
  for (long long t = k0; t < T; t++) {
#pragma unroll
    for (int j = KG - 1; j > 0; j--) w[j] = w[j - 1];
    w[0] = x[(t - k0) * B + b];
    const double gyt = gy[t * B + b];
#pragma unroll
    for (int j = 0; j < KG; j++) acc[j] = t - k0 - j >= 0 ? acc[j] + gyt * w[j] : acc[j];
  }
}

#ifdef LGAR_DEVSIM
// the kernels' work, one lane at a time
inline void route_all(const RouteArgs &a) {
  const long long rows = route_rows(a);
  for (long long r = 0; r < rows; r++)
    for (long long b = 0; b < a.B; b++) route_store(a, r, b, route_fold(a, r, b));
}

inline void route_grad_all(const double *x, const double *gy, long long T, long long B, int K, double *g_out) {
  for (long long k0 = 0; k0 < K; k0 += LGAR_ROUTE_KG)
    for (long long b = 0; b < B; b++) {
      double acc[LGAR_ROUTE_KG];
      route_grad_lane<LGAR_ROUTE_KG>(x, gy, T, B, b, k0, acc);
      for (int j = 0; j < LGAR_ROUTE_KG && k0 + j < K; j++) g_out[(k0 + j) * B + b] = acc[j];
    }
}
#else
// host-side launches (lgar_route.hip); arguments already checked by the C-ABI wrappers there.  0 / LGAR_E_*.
int launch_catchment_route(const double *x, int n_rows, int n_catchments, const double *ordinates, int n_ordinates,
                           int per_catchment, const double *queue_in, double *queue_out, double *y, int reverse,
                           hipStream_t stream);
int launch_catchment_route_grad(const double *x, const double *gy, int n_rows, int n_catchments, int n_ordinates, double *g_out,
                                hipStream_t stream);
#endif

}  // namespace lgar
