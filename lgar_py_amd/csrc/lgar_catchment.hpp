// lgar_catchment.hpp -- catchment sums: one row of a stored [rows][n_columns] series summed per catchment, and the adjoint.
//
// The catchment map is CSR (include/lgar.h has the full statement): offsets int32[B + 1], order int32[offsets[B]] or NULL
// (NULL: catchment b is the contiguous columns offsets[b] .. offsets[b + 1] - 1).  For row t and catchment b with the members
// c_0 .. c_{n-1} in map order
//
//     x_i = (double)w[c_i] * (double)series[t][c_i]                 (w = 1 without weights; exact for fp32 inputs)
//     member i has NO term when its column is outside [0, n_columns) or status[c_i] has a fault bit
//     s_p = the terms with i mod 256 == p, added in increasing i from +0.0          (256 partials, plain fp64 adds)
//     q_l = (s_l + s_{l+64}) + (s_{l+128} + s_{l+192}),  l = 0 .. 63
//     for off = 32, 16, 8, 4, 2, 1:  q_l <- q_l + q_{l xor off}   (all l at once)
//     out[t][b] = q_0
//
// which is what ONE wavefront does when lane l owns the partials l, l + 64, l + 128, l + 192: four independent accumulators per
// lane, the pair sums lane-local, the butterfly over the lanes.  (A wave may carry the same catchment through several rows at
// once -- column, status and weight are then read once for all of them -- with one such set of accumulators per row.)  The result is a pure function of the catchment's own members:
// their values, weights and order -- not of B, of the other catchments, of where the members sit in the launch, or of the run.
// The library is built with -ffp-contract=off: the multiply and the adds round separately.
//
// Memory safety before meaning (as in lgar_moisture.hpp): offsets are clamped into [0, len] (len = the length of `order`, or
// n_columns without it), a catchment whose clamped end is not beyond its start is empty, and a member outside [0, n_columns)
// is skipped, so a corrupt map cannot index out of bounds.
//
// Like lgar_moisture.hpp this header also compiles for the host with -DLGAR_DEVSIM (the 64 lanes one after the other, the
// butterfly over an array): tests/catchment_host runs the same text against the numpy statement of the definition.
#pragma once
#ifndef LGAR_DEVSIM
#include <hip/hip_runtime.h>
#define LGAR_CATCH_FN __device__ __forceinline__
#else
#define LGAR_CATCH_FN inline
#endif
#include <stddef.h>
#include <stdint.h>

#include "../../include/lgar.h"

namespace lgar {

#define LGAR_CATCH_LANES 64
#define LGAR_CATCH_PARTIALS 256  // four per lane

// What the sums of one catchment over `rows` consecutive rows read.  row: the first of the series rows ([n_columns] each, R,
// row_stride elements apart) or NULL = every value is 1 (the sum of the weights).
template <typename R> struct CatchRow {
  const R *row;
  const R *weights;       // [n_columns] or NULL = 1
  const int32_t *status;  // [n_columns] or NULL = no column is skipped for its status
  const int32_t *order;   // [len] or NULL = member at map position p is column p
  long long n_columns;
  long long len;          // length of `order`; n_columns without it
  long long row_stride;
  int rows;               // rows behind `row` (>= 1): a wave that carries more re-reads the last one and drops the result
};

// (a job without columns has no members at all: catch_term may then read column 0 unconditionally)
template <typename R>
LGAR_CATCH_FN CatchRow<R> catch_row(const R *row, int rows, const R *weights, const int32_t *status, const int32_t *order,
                                    long long n_order, long long n_columns) {
  CatchRow<R> a;
  a.row = row;
  a.weights = weights;
  a.status = status;
  a.order = order;
  a.n_columns = n_columns;
  a.len = n_columns <= 0 ? 0 : (order ? (n_order < 0 ? 0 : n_order) : n_columns);
  a.row_stride = n_columns;
  a.rows = rows < 1 ? 1 : rows;
  return a;
}

LGAR_CATCH_FN long long catch_clamp(long long x, long long hi) { return x < 0 ? 0 : (x > hi ? hi : x); }

// Members of catchment b: map positions lo .. lo + n - 1 (clamped as the header comment says).
LGAR_CATCH_FN void catch_range(const int32_t *offsets, long long b, long long len, long long &lo, long long &n) {
  lo = catch_clamp((long long)offsets[b], len);
  const long long hi = catch_clamp((long long)offsets[b + 1], len);
  n = hi > lo ? hi - lo : 0;
}

// The terms of the member at map position `pos` (< len) in NR rows: false = the member is skipped.  Column, status and weight
// are read once for all the rows.  The loads are unconditional (a skipped member reads column 0, or its own flagged values,
// and drops them), so a lane keeps all the loads of a block in flight.
template <typename R, int NR> LGAR_CATCH_FN bool catch_term(const CatchRow<R> &a, long long pos, double (&x)[NR]) {
  const long long c = a.order ? (long long)a.order[pos] : pos;
  const bool inside = c >= 0 && c < a.n_columns;
  const size_t at = inside ? (size_t)c : (size_t)0;
  const int32_t st = a.status ? a.status[at] : 0;
  const double w = a.weights ? (double)a.weights[at] : 1.0;
#pragma unroll
  for (int r = 0; r < NR; r++) {
    const long long rr = r < a.rows ? r : a.rows - 1;
    const double v = a.row ? (double)a.row[(size_t)rr * (size_t)a.row_stride + at] : 1.0;
    x[r] = w * v;
  }
  return inside && (st & LGAR_ST_FAULT_MASK) == 0;
}

// U slices of 64 members from member `base` (a multiple of 256) on: this lane's are base + lane + 64 u, which belongs to the
// lane's partial u mod 4 (of every row).  All loads first, then the adds in increasing member order.
template <typename R, int NR, int U, bool GUARD>
LGAR_CATCH_FN void catch_block(const CatchRow<R> &a, long long lo, long long base, long long n, int lane, double (&s)[NR][4]) {
  static_assert(U % 4 == 0, "a block is whole groups of 256 members");
  double x[U][NR];
  bool ok[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const long long i = base + lane + 64 * u;
#pragma unroll
    for (int r = 0; r < NR; r++) x[u][r] = 0.0;
    ok[u] = false;
    if (!GUARD || i < n) ok[u] = catch_term<R, NR>(a, lo + i, x[u]);
  }
#pragma unroll
  for (int u = 0; u < U; u++)
#pragma unroll
    for (int r = 0; r < NR; r++) s[r][u & 3] = ok[u] ? s[r][u & 3] + x[u][r] : s[r][u & 3];
}

// One lane's four partials per row over the n members from map position lo on, then its pair sums q[row].  One row at a time a
// lane keeps 16 value loads in flight, four rows at a time 4 x 4 (and reads column, status and weight once for the four).
template <typename R, int NR> LGAR_CATCH_FN void catch_lane(const CatchRow<R> &a, long long lo, long long n, int lane, double (&q)[NR]) {
  constexpr int U = NR == 1 ? 16 : 4;
  double s[NR][4];
#pragma unroll
  for (int r = 0; r < NR; r++) s[r][0] = s[r][1] = s[r][2] = s[r][3] = 0.0;
  long long base = 0;
  for (; base + 64 * U <= n; base += 64 * U) catch_block<R, NR, U, false>(a, lo, base, n, lane, s);
  for (; base < n; base += 256) catch_block<R, NR, 4, true>(a, lo, base, n, lane, s);
#pragma unroll
  for (int r = 0; r < NR; r++) q[r] = (s[r][0] + s[r][1]) + (s[r][2] + s[r][3]);
}

#ifndef LGAR_DEVSIM
// q_l <- q_l + q_{l xor off}, off = 32 .. 1: every lane ends with the same bits (an fp64 add commutes)
LGAR_CATCH_FN double catch_butterfly(double q) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) q = q + __shfl_xor(q, off);
  return q;
}
#else
inline double catch_butterfly(double (&q)[LGAR_CATCH_LANES]) {
  for (int off = 32; off > 0; off >>= 1) {
    double r[LGAR_CATCH_LANES];
    for (int l = 0; l < LGAR_CATCH_LANES; l++) r[l] = q[l] + q[l ^ off];
    for (int l = 0; l < LGAR_CATCH_LANES; l++) q[l] = r[l];
  }
  return q[0];
}

// the wave of lgar_catchment_sums_kernel, one lane at a time: out[r] = the sum of catchment b in row r of a.rows (<= NR) rows
template <typename R, int NR> inline void catch_sum(const CatchRow<R> &a, const int32_t *offsets, long long b, double *out) {
  long long lo, n;
  catch_range(offsets, b, a.len, lo, n);
  double q[NR][LGAR_CATCH_LANES];
  for (int l = 0; l < LGAR_CATCH_LANES; l++) {
    double ql[NR];
    catch_lane<R, NR>(a, lo, n, l, ql);
    for (int r = 0; r < NR; r++) q[r][l] = ql[r];
  }
  for (int r = 0; r < NR && r < a.rows; r++) out[r] = catch_butterfly(q[r]);
}
#endif

// Spread, the adjoint: the tangent weight of column c in a row whose [B] gradient is grad_row.  0 for a column of no catchment
// (catchment_of[c] outside [0, B)) or with a fault bit; else grad_row[catchment_of[c]] * (double)w[c], rounded once to R.
template <typename R>
LGAR_CATCH_FN R catch_spread(const double *grad_row, long long n_catchments, int32_t catchment, int32_t status, double w) {
  const bool live = catchment >= 0 && (long long)catchment < n_catchments && (status & LGAR_ST_FAULT_MASK) == 0;
  if (!live) return R(0);
  return (R)(grad_row[catchment] * w);
}

#ifndef LGAR_DEVSIM
// host-side launches (lgar_catchment.hip); arguments already checked by the C-ABI wrappers (lgar_kernels.hip).  0 / LGAR_E_*.
int launch_catchment_sums(const void *series, int n_rows, int n_columns, const int32_t *offsets, int n_catchments,
                          const int32_t *order, int n_order, const void *weights, const int32_t *status, double *out,
                          double *weight_sums, int dtype, hipStream_t stream);
int launch_catchment_spread(const double *grad, int n_rows, int n_catchments, const int32_t *catchment_of, int n_columns,
                            const void *weights, const int32_t *status, void *out, int dtype, hipStream_t stream);
#endif

}  // namespace lgar
