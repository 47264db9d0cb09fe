// lgar_score.hpp -- catchment scores: per-catchment moments of a [T][B] simulation against [To][B] observations with gaps, and
// their adjoint (lgar_catchment_moments / lgar_catchment_moments_grad, include/lgar.h has the full statement; DESIGN.md
// section 13).
//
// All arrays are fp64, catchment fastest.  A pair (j, b) is valid iff obs[j][b] is finite; the aggregated simulation is
//
//     s[j][b] = (((0.0 + sim[j r][b]) + sim[j r + 1][b]) + ...) / (double)r                          r = window
//
// and every sum over j is THE GATED FOLD: the rows are cut into blocks of LGAR_SCORE_BLOCK = 64 observation rows, a block partial
// starts at +0.0 and adds the terms of its valid rows in increasing j (an invalid row adds no term at all), the result starts at
// +0.0 and adds the block partials in increasing k.  Plain fp64 adds and products (the library is built with -ffp-contract=off).
// The block size belongs to the definition, not to the launch: the result for catchment b reads column b only.
//
// Two passes: the first folds (1, o, s) into n and the means mo, ms; the second folds the four centred terms.  A block partial
// is one lane's work (score_block_first / score_block_centred), the fold of the partials another's (score_fold); both passes
// keep their partials in the caller's workspace, ws[(k * LGAR_SCORE_WSROWS + term) * B + b].  The gradient is elementwise
// (score_grad_element).
//
// Like lgar_route.hpp this header also compiles for the host with -DLGAR_DEVSIM: tests/score_host runs the same text against
// the numpy statement of the definition.
#pragma once
#ifndef LGAR_DEVSIM
#include <hip/hip_runtime.h>
#define LGAR_SCORE_FN __device__ __forceinline__
#define LGAR_SCORE_HD __host__ __device__ __forceinline__  // what the launch code needs as well
#else
#define LGAR_SCORE_FN inline
#define LGAR_SCORE_HD inline
#endif
#include <stddef.h>
#include <stdint.h>

#include "../../include/lgar.h"

namespace lgar {

#define LGAR_SCORE_LANES 64
#define LGAR_SCORE_WSROWS 4  // partials a block keeps per catchment: (n, o, s) in the first pass, the four centred sums in the second

// One scoring call: sim[To * r][B], obs[To][B].
struct ScoreArgs {
  const double *sim, *obs;
  long long To, B, r;
};

LGAR_SCORE_HD long long score_blocks(long long To) { return (To + LGAR_SCORE_BLOCK - 1) / LGAR_SCORE_BLOCK; }

// bytes of workspace a call needs
LGAR_SCORE_HD long long score_workspace_bytes(long long To, long long B) {
  return score_blocks(To) * LGAR_SCORE_WSROWS * B * (long long)sizeof(double);
}

// finite: neither NaN nor an infinity (a comparison with NaN is false)
LGAR_SCORE_FN bool score_valid(double o) { return __builtin_fabs(o) <= 1.7976931348623157e308; }

// the aggregated simulation of observation row j.  ONE: window = 1, the same bits without the loop ((0.0 + x) / 1.0).  Otherwise
// the window's rows are loaded LGAR_SCORE_AGG at a time ahead of the adds that wait for them (six divides the usual ratios of
// two time steps -- 2, 3, 6, 12, 24 -- or leaves little over; a chunk that reaches past the window re-reads its last row and
// adds nothing for it).
#define LGAR_SCORE_AGG 6
template <bool ONE> LGAR_SCORE_FN double score_agg(const ScoreArgs &a, long long j, long long b) {
  if (ONE) return (0.0 + a.sim[j * a.B + b]) / 1.0;
  const double *p = a.sim + (j * a.r) * a.B + b;
  double acc = 0.0;
  for (long long i = 0; i < a.r; i += LGAR_SCORE_AGG) {
    double x[LGAR_SCORE_AGG];
#pragma unroll
    for (int u = 0; u < LGAR_SCORE_AGG; u++) x[u] = p[(i + u < a.r ? i + u : a.r - 1) * a.B];
#pragma unroll
    for (int u = 0; u < LGAR_SCORE_AGG; u++) acc = i + u < a.r ? acc + x[u] : acc;
  }
  return acc / (double)a.r;
}

LGAR_SCORE_FN double score_agg(const ScoreArgs &a, long long j, long long b) {
  return a.r == 1 ? score_agg<true>(a, j, b) : score_agg<false>(a, j, b);
}

// The rows of block k of catchment b in increasing j: row(o, s, valid) for each, valid = whether the row adds its terms at all.
// The rows are taken in chunks whose loads are all issued before the first of them is used (a chunk that reaches past the
// block re-reads its last row: every load stays inside the arrays), and `row` selects, it does not branch: a load that sits
// behind a branch on another load's value waits for it, and a block is a chain of such waits.  window = 1 (ONE): eight rows
// of obs and sim are in flight at a time; otherwise two rows of obs and six of a window's rows of sim (score_agg).
template <bool ONE, typename Row> LGAR_SCORE_FN void score_block_rows(const ScoreArgs &a, long long k, long long b, Row row) {
  constexpr int CH = ONE ? 8 : 2;
  const long long j0 = k * LGAR_SCORE_BLOCK, j1 = j0 + LGAR_SCORE_BLOCK < a.To ? j0 + LGAR_SCORE_BLOCK : a.To;
  for (long long j = j0; j < j1; j += CH) {
    double o[CH], s[CH];
#pragma unroll
    for (int u = 0; u < CH; u++) o[u] = a.obs[(j + u < j1 ? j + u : j1 - 1) * a.B + b];
#pragma unroll
    for (int u = 0; u < CH; u++) s[u] = score_agg<ONE>(a, j + u < j1 ? j + u : j1 - 1, b);
#pragma unroll
    for (int u = 0; u < CH; u++) row(o[u], s[u], j + u < j1 && score_valid(o[u]));
  }
}

// First pass, block k of catchment b: part = (number of valid rows, sum of o, sum of s) over the valid rows in increasing j
LGAR_SCORE_FN void score_block_first(const ScoreArgs &a, long long k, long long b, double (&part)[3]) {
  double n = 0.0, so = 0.0, ss = 0.0;
  auto row = [&](double o, double s, bool valid) {
    n = valid ? n + 1.0 : n;
    so = valid ? so + o : so;
    ss = valid ? ss + s : ss;
  };
  if (a.r == 1) score_block_rows<true>(a, k, b, row);
  else score_block_rows<false>(a, k, b, row);
  part[0] = n, part[1] = so, part[2] = ss;
}

// Second pass: part = the sums of (o - mo)^2, (s - ms)^2, (o - mo)(s - ms), (s - o)^2 over the valid rows of the block
LGAR_SCORE_FN void score_block_centred(const ScoreArgs &a, long long k, long long b, double mo, double ms, double (&part)[4]) {
  double soo = 0.0, sss = 0.0, sos = 0.0, see = 0.0;
  auto row = [&](double o, double s, bool valid) {
    const double d_o = o - mo, d_s = s - ms, e = s - o;
    soo = valid ? soo + d_o * d_o : soo;
    sss = valid ? sss + d_s * d_s : sss;
    sos = valid ? sos + d_o * d_s : sos;
    see = valid ? see + e * e : see;
  };
  if (a.r == 1) score_block_rows<true>(a, k, b, row);
  else score_block_rows<false>(a, k, b, row);
  part[0] = soo, part[1] = sss, part[2] = sos, part[3] = see;
}

// a block's partials go to / come from the workspace
template <int N> LGAR_SCORE_FN void score_store(double *ws, long long k, long long B, long long b, const double (&part)[N]) {
#pragma unroll
  for (int t = 0; t < N; t++) ws[(k * LGAR_SCORE_WSROWS + t) * B + b] = part[t];
}

// The fold of the block partials of catchment b, every term from +0.0 in increasing k.  The N terms go up the blocks together
// and four blocks' loads are in flight at a time: the adds of a term form one chain, the loads wait for nothing.
template <int N> LGAR_SCORE_FN void score_fold(const double *ws, long long n_blocks, long long B, long long b, double (&acc)[N]) {
#pragma unroll
  for (int t = 0; t < N; t++) acc[t] = 0.0;
#pragma unroll 4
  for (long long k = 0; k < n_blocks; k++) {
#pragma unroll
    for (int t = 0; t < N; t++) acc[t] = acc[t] + ws[(k * LGAR_SCORE_WSROWS + t) * B + b];
  }
}

// after the first pass: rows 0 .. 2 of the moments (n, mo, ms; n = 0 gives NaN means: an IEEE 0 / 0)
LGAR_SCORE_FN void score_means(const double *ws, long long n_blocks, long long B, long long b, double *moments) {
  double acc[3];
  score_fold<3>(ws, n_blocks, B, b, acc);
  moments[0 * B + b] = acc[0];
  moments[1 * B + b] = acc[1] / acc[0];
  moments[2 * B + b] = acc[2] / acc[0];
}

// after the second pass: rows 3 .. 6
LGAR_SCORE_FN void score_centred(const double *ws, long long n_blocks, long long B, long long b, double *moments) {
  double acc[4];
  score_fold<4>(ws, n_blocks, B, b, acc);
#pragma unroll
  for (int t = 0; t < 4; t++) moments[(3 + t) * B + b] = acc[t];
}

// The gradient of observation row j of catchment b with respect to each of its r simulation rows: 0 on an invalid row, else
//     g = ((c0 / n + (2 c1)(s - ms)) + c2 (o - mo)) + (2 c3)(s - o),     g / (double)r
// coef: [4][B], d F / d (ms, sss, sos, see)
LGAR_SCORE_FN double score_grad_element(const ScoreArgs &a, const double *moments, const double *coef, long long j, long long b) {
  const double o = a.obs[j * a.B + b];
  if (!score_valid(o)) return 0.0;
  const double n = moments[b], mo = moments[a.B + b], ms = moments[2 * a.B + b];
  const double c0 = coef[b], c1 = coef[a.B + b], c2 = coef[2 * a.B + b], c3 = coef[3 * a.B + b];
  const double s = score_agg(a, j, b);
  const double g = ((c0 / n + (2.0 * c1) * (s - ms)) + c2 * (o - mo)) + (2.0 * c3) * (s - o);
  return g / (double)a.r;
}

LGAR_SCORE_FN void score_grad_store(const ScoreArgs &a, long long j, long long b, double v, double *grad_sim) {
  double *p = grad_sim + (j * a.r) * a.B + b;
  for (long long i = 0; i < a.r; i++) p[i * a.B] = v;
}

#ifdef LGAR_DEVSIM
// the kernels' work, one lane at a time
inline void score_moments_all(const ScoreArgs &a, double *moments, double *ws) {
  const long long nb = score_blocks(a.To);
  for (long long k = 0; k < nb; k++)
    for (long long b = 0; b < a.B; b++) {
      double part[3];
      score_block_first(a, k, b, part);
      score_store<3>(ws, k, a.B, b, part);
    }
  for (long long b = 0; b < a.B; b++) score_means(ws, nb, a.B, b, moments);
  for (long long k = 0; k < nb; k++)
    for (long long b = 0; b < a.B; b++) {
      double part[4];
      score_block_centred(a, k, b, moments[a.B + b], moments[2 * a.B + b], part);
      score_store<4>(ws, k, a.B, b, part);
    }
  for (long long b = 0; b < a.B; b++) score_centred(ws, nb, a.B, b, moments);
}

inline void score_grad_all(const ScoreArgs &a, const double *moments, const double *coef, double *grad_sim) {
  for (long long j = 0; j < a.To; j++)
    for (long long b = 0; b < a.B; b++) score_grad_store(a, j, b, score_grad_element(a, moments, coef, j, b), grad_sim);
}
#else
// host-side launches (lgar_score.hip); arguments already checked by the C-ABI wrappers there.  0 / LGAR_E_*.
int launch_catchment_moments(const double *sim, const double *obs, int n_obs_rows, int n_catchments, int window, double *moments,
                             double *workspace, hipStream_t stream);
int launch_catchment_moments_grad(const double *sim, const double *obs, int n_obs_rows, int n_catchments, int window,
                                  const double *moments, const double *coef, double *grad_sim, hipStream_t stream);
#endif

}  // namespace lgar
