// TEST INFRASTRUCTURE ONLY -- the post-processing entry points of include/lgar.h with the host in the GPU's place.
//
// The per-column, per-lane and per-output functions the kernels run (lgar_py_amd/csrc/lgar_moisture.hpp, lgar_catchment.hpp,
// lgar_route.hpp) are plain C++; with -DLGAR_DEVSIM they compile for the host, one lane after the other.  This header holds
// what the .hip files put around them -- the argument refusals of the C-ABI wrappers, the launchers' early-outs, the kernels'
// dispatch and lane loops -- once: one function per entry point, with the argument list of include/lgar.h minus the stream.
// Compiled on its own it is libposthost.so, which the device-code simulator (tests/devsim) puts behind the product's calling
// surface; post_host.cpp is the stand-alone program around it, which also runs under AddressSanitizer + UBSan.  Never built or
// used by the product.
#ifndef LGAR_TESTS_POST_HOST_HPP
#define LGAR_TESTS_POST_HOST_HPP
#define LGAR_DEVSIM 1
#include <stddef.h>
#include <stdint.h>

#include "../../lgar_py_amd/csrc/lgar_catchment.hpp"
#include "../../lgar_py_amd/csrc/lgar_moisture.hpp"
#include "../../lgar_py_amd/csrc/lgar_route.hpp"

namespace post_host {

inline bool is_dtype(int32_t dtype) { return dtype == LGAR_F32 || dtype == LGAR_F64; }
inline int front_slots(const LgarDims *d) { return d->front_slots > 0 ? d->front_slots : LGAR_FMAX; }

template <typename R>
void moisture_typed(const LgarDims *d, const LgarParams *p, const LgarState *s, const double *edges, int nb, int what, void *out) {
  const R *depth = (const R *)s->depth, *theta = (const R *)s->theta, *thick = (const R *)p->thickness;
  const size_t n = (size_t)d->n_columns;
  const int L = d->n_layers, F = front_slots(d);
  for (size_t c = 0; c < n; c++) {
    // the kernel's dispatch (lgar_moisture.hip): layer bins, or the smallest compiled bin capacity that fits
    if (!edges)
      lgar::moist_column<R, 8, true>(depth, theta, s->flags, s->n_fronts, thick, nullptr, n, c, L, F, nb, what, (R *)out);
    else if (nb <= 8)
      lgar::moist_column<R, 8, false>(depth, theta, s->flags, s->n_fronts, thick, edges, n, c, L, F, nb, what, (R *)out);
    else if (nb <= 16)
      lgar::moist_column<R, 16, false>(depth, theta, s->flags, s->n_fronts, thick, edges, n, c, L, F, nb, what, (R *)out);
    else
      lgar::moist_column<R, LGAR_MOIST_BINS, false>(depth, theta, s->flags, s->n_fronts, thick, edges, n, c, L, F, nb, what, (R *)out);
  }
}

// lgar_totals_replay_kernel (lgar_moisture.hip), one lane per column: the forward kernels' own adds (tot = tot + acc, in R)
template <typename R> void replay_typed(const LgarDims *d, const LgarStepOut *stored, int n_rows, void *running) {
  const size_t N = (size_t)d->n_columns;
  for (size_t c = 0; c < N; c++)
    for (int j = 0; j < 7; j++) {
      const R *series = (const R *)stored->series[j];
      if (series == nullptr) continue;
      R r = ((R *)running)[(size_t)j * N + c];
      for (int t = 0; t < n_rows; t++) r = r + series[(size_t)t * N + c];
      ((R *)running)[(size_t)j * N + c] = r;
    }
}

// rows_per_wave 1: one wave per (row, catchment); 4: the kernel's row groups of four (the last one ragged)
template <typename R>
void sums_typed(const void *series, size_t T, size_t N, const int32_t *offsets, size_t B, const int32_t *order, long long n_order,
                const void *weights, const int32_t *status, double *out, size_t NR) {
  for (size_t t = 0; t < T; t += NR) {
    const int rows = (int)(T - t < NR ? T - t : NR);
    const R *row = series ? (const R *)series + t * N : nullptr;
    const lgar::CatchRow<R> a = lgar::catch_row<R>(row, rows, (const R *)weights, status, order, n_order, (long long)N);
    for (size_t b = 0; b < B; b++) {
      double q[4];
      if (NR == 4) lgar::catch_sum<R, 4>(a, offsets, (long long)b, q);
      else lgar::catch_sum<R, 1>(a, offsets, (long long)b, q);
      for (int r = 0; r < rows; r++) out[(t + r) * B + b] = q[r];
    }
  }
}

template <typename R>
void spread_typed(const double *grad, size_t T, size_t B, const int32_t *cat, size_t N, const void *weights, const int32_t *st, void *out) {
  const R *w = (const R *)weights;
  for (size_t t = 0; t < T; t++)
    for (size_t c = 0; c < N; c++)
      ((R *)out)[t * N + c] = lgar::catch_spread<R>(grad + t * B, (long long)B, cat[c], st ? st[c] : 0, w ? (double)w[c] : 1.0);
}

}  // namespace post_host

extern "C" {

// (without lgar_soil_moisture's `weights` / `basin`: that reduction's summation order lives in a .hip file and has no host form)
int32_t posthost_soil_moisture(const LgarDims *dims, const LgarParams *params, const LgarState *state, const double *edges,
                               int32_t n_bins, int32_t what, void *out, int32_t dtype) {
  // what lgar_soil_moisture itself refuses (lgar_kernels.hip): the function is only ever called inside these bounds
  if (!dims || dims->n_layers < LGAR_LMIN || dims->n_layers > LGAR_LMAX || dims->front_slots < 0 || dims->front_slots > LGAR_FMAX ||
      dims->n_columns < 1 || n_bins < 1 || n_bins > LGAR_MOIST_BINS || (!edges && n_bins != dims->n_layers) ||
      (what != 0 && what != 1) || !post_host::is_dtype(dtype))
    return LGAR_E_ARG;
  if (!params || !params->thickness || !state || !state->depth || !state->theta || !state->flags || !state->n_fronts || !out)
    return LGAR_E_ARG;
  if (dtype == LGAR_F64) post_host::moisture_typed<double>(dims, params, state, edges, n_bins, what, out);
  else post_host::moisture_typed<float>(dims, params, state, edges, n_bins, what, out);
  return 0;
}

int32_t posthost_totals_replay(const LgarDims *dims, const LgarStepOut *stored, int32_t n_rows, void *running, int32_t dtype) {
  if (!dims || dims->n_columns < 1 || !stored || !running || n_rows < 0 || !post_host::is_dtype(dtype)) return LGAR_E_ARG;
  if (n_rows == 0) return 0;
  if (dtype == LGAR_F64) post_host::replay_typed<double>(dims, stored, n_rows, running);
  else post_host::replay_typed<float>(dims, stored, n_rows, running);
  return 0;
}

// rows_per_wave (1 or 4) is the test's choice of the kernel the library picks by job size: the same bits either way
int32_t posthost_catchment_sums(const void *series, int32_t n_rows, int32_t n_columns, const int32_t *offsets, int32_t n_catchments,
                                const int32_t *order, int32_t n_order, const void *weights, const int32_t *status, double *out,
                                double *weight_sums, int32_t dtype, int32_t rows_per_wave) {
  // what the C-ABI wrapper itself refuses (lgar_kernels.hip)
  if (n_rows < 0 || n_columns < 0 || n_catchments < 0 || !offsets || (order && n_order < 0)) return LGAR_E_ARG;
  if (n_rows > 0 && n_catchments > 0 && (!out || (!series && n_columns > 0))) return LGAR_E_ARG;
  if (!post_host::is_dtype(dtype) || (rows_per_wave != 1 && rows_per_wave != 4)) return LGAR_E_ARG;
  if (n_catchments == 0) return 0;
  const size_t T = (size_t)n_rows, N = (size_t)n_columns, B = (size_t)n_catchments, NR = (size_t)rows_per_wave;
  if (n_rows > 0) {
    if (dtype == LGAR_F64) post_host::sums_typed<double>(series, T, N, offsets, B, order, n_order, weights, status, out, NR);
    else post_host::sums_typed<float>(series, T, N, offsets, B, order, n_order, weights, status, out, NR);
  }
  if (weight_sums) {  // the same pass over one row of ones: the terms are the weights themselves
    if (dtype == LGAR_F64) post_host::sums_typed<double>(nullptr, 1, N, offsets, B, order, n_order, weights, status, weight_sums, 1);
    else post_host::sums_typed<float>(nullptr, 1, N, offsets, B, order, n_order, weights, status, weight_sums, 1);
  }
  return 0;
}

int32_t posthost_catchment_spread(const double *grad, int32_t n_rows, int32_t n_catchments, const int32_t *catchment_of,
                                  int32_t n_columns, const void *weights, const int32_t *status, void *out, int32_t dtype) {
  if (n_rows < 0 || n_columns < 0 || n_catchments < 0) return LGAR_E_ARG;
  if (n_rows > 0 && n_columns > 0 && (!catchment_of || !out || (n_catchments > 0 && !grad))) return LGAR_E_ARG;
  if (!post_host::is_dtype(dtype)) return LGAR_E_ARG;
  if (n_rows == 0 || n_columns == 0) return 0;
  const size_t T = (size_t)n_rows, N = (size_t)n_columns, B = (size_t)n_catchments;
  if (dtype == LGAR_F64) post_host::spread_typed<double>(grad, T, B, catchment_of, N, weights, status, out);
  else post_host::spread_typed<float>(grad, T, B, catchment_of, N, weights, status, out);
  return 0;
}

int32_t posthost_catchment_route(const double *x, int32_t n_rows, int32_t n_catchments, const double *ordinates, int32_t n_ordinates,
                                 int32_t per_catchment, const double *queue_in, double *queue_out, double *y, int32_t reverse) {
  // what the C-ABI wrappers themselves refuse (lgar_route.hip)
  if (n_rows < 0 || n_catchments < 0 || n_ordinates < 1 || n_ordinates > LGAR_ROUTE_KMAX || !ordinates) return LGAR_E_ARG;
  if (n_rows > 0 && n_catchments > 0 && (!x || !y)) return LGAR_E_ARG;
  if (reverse && (queue_in || queue_out)) return LGAR_E_ARG;
  if (n_catchments == 0) return 0;
  lgar::route_all(lgar::route_args(x, n_rows, n_catchments, ordinates, n_ordinates, per_catchment != 0, queue_in, queue_out, y, reverse != 0));
  return 0;
}

int32_t posthost_catchment_route_grad(const double *x, const double *gy, int32_t n_rows, int32_t n_catchments, int32_t n_ordinates,
                                      double *g_out) {
  if (n_rows < 0 || n_catchments < 0 || n_ordinates < 1 || n_ordinates > LGAR_ROUTE_KMAX) return LGAR_E_ARG;
  if (n_catchments > 0 && (!g_out || (n_rows > 0 && (!x || !gy)))) return LGAR_E_ARG;
  if (n_catchments == 0) return 0;
  lgar::route_grad_all(x, gy, n_rows, n_catchments, n_ordinates, g_out);
  return 0;
}

}  // extern "C"
#endif
