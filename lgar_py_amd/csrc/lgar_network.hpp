// lgar_network.hpp -- catchment network: linear Muskingum channel routing over the reach graph of the catchments, its adjoint and
// the gradient with respect to the coefficients (lgar_network_route / lgar_network_route_grad, include/lgar.h has the full
// statement).
//
// All floating-point arrays are fp64, catchment fastest: the lateral inflow x[T][B], the discharge y[T][B], coef[3][B] = c0, c1,
// c2 of every reach.  The topology is int32: down[B] (-1: an outlet), the CSR lists up_ptr[B + 1] / up_idx[E] of the direct
// upstream catchments in ascending index, order[B] = the catchments sorted by (level, index).  One reach b, for t = 0 .. T - 1:
//
//     I = x[t][b];  I = I + y[t][up_idx[e]]  for e = up_ptr[b] .. up_ptr[b + 1] - 1     (ascending e, one rounded add each)
//     O = (c0 I + c1 Iprev) + c2 Oprev;   y[t][b] = O;   Iprev = I;   Oprev = O
//
// A reach is one lane's work: it walks all rows (net_walk), the rows in chunks of LGAR_NET_CHUNK whose loads -- the chunk's rows
// of x, then the same rows of y of one upstream reach after the other -- are all issued before the first of them is used (a
// chunk that reaches past the rows re-reads its last row: every load stays inside the arrays).  The recurrence itself is serial,
// so the bits are the definition's whatever the chunk is.  The reaches of a level are independent of each other and read only
// y of lower levels: the caller runs the levels one after the other.  The adjoint (net_walk_back) is the same walk downward
// over the levels in descending order; with the coefficient gradient wanted it re-forms I[t] by the forward's own fold
// (net_inflow: the same bits) and adds the terms of c1 and c2 of row t + 1 while it is at row t, where I[t] and y[t] are at hand:
// every accumulator still receives its terms in decreasing t.
//
// Every index read from device memory is clamped into its array (net_clamp: order, up_idx and down to [0, B - 1], up_ptr to
// [0, E]): a corrupt topology gives wrong numbers, never an access out of bounds.  Offsets are 64-bit.
//
// Like lgar_route.hpp and lgar_score.hpp this header also compiles for the host with -DLGAR_DEVSIM: tests/network_host runs the
// same text against the numpy statement of the definition.
#pragma once
#ifndef LGAR_DEVSIM
#include <hip/hip_runtime.h>
#define LGAR_NET_FN __device__ __forceinline__
#else
#define LGAR_NET_FN inline
#endif
#include <stddef.h>
#include <stdint.h>

#include "../../include/lgar.h"

namespace lgar {

#define LGAR_NET_CHUNK 8  // rows of a reach whose loads are in flight together

// One forward call.  state_in / state_out: [2][B] = Iprev, Oprev (NULL: zeros / not wanted).  E: entries of up_idx.
struct NetArgs {
  const double *x, *coef, *state_in;
  double *y, *state_out;
  const int32_t *order, *up_ptr, *up_idx;
  long long T, B, E;
};

// One adjoint call.  gc == NULL: the coefficient gradient is not wanted, and x, y, state_in, up_ptr, up_idx are not read.
struct NetGradArgs {
  const double *gy, *coef, *x, *y, *state_in;
  double *gx, *gc;
  const int32_t *order, *down, *up_ptr, *up_idx;
  long long T, B, E;
};

LGAR_NET_FN long long net_clamp(long long v, long long hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the reach of position p of `order`
LGAR_NET_FN long long net_reach(const int32_t *order, long long p, long long B) { return net_clamp(order[p], B - 1); }

// row u of a chunk that starts at t0 and runs upward (DIR = +1) or downward (DIR = -1), kept inside 0 .. T - 1
template <int DIR> LGAR_NET_FN long long net_row(long long t0, int u, long long T) {
  return DIR > 0 ? (t0 + u < T ? t0 + u : T - 1) : (t0 - u > 0 ? t0 - u : 0);
}

// The inflows of the CH rows of a chunk of reach b: I = x[t][b], then + y[t][up] for the entries e0 .. e1 - 1 in ascending e.
// The chunk's loads of x go out first, then one upstream reach's CH rows of y at a time.
template <int CH, int DIR>
LGAR_NET_FN void net_inflow(const double *x, const double *y, const int32_t *up_idx, long long T, long long B, long long b, long long e0,
                            long long e1, long long t0, double (&I)[CH]) {
#pragma unroll
  for (int u = 0; u < CH; u++) I[u] = x[net_row<DIR>(t0, u, T) * B + b];
  for (long long e = e0; e < e1; e++) {
    const double *yu = y + net_clamp(up_idx[e], B - 1);
    double v[CH];
#pragma unroll
    for (int u = 0; u < CH; u++) v[u] = yu[net_row<DIR>(t0, u, T) * B];
#pragma unroll
    for (int u = 0; u < CH; u++) I[u] = I[u] + v[u];
  }
}

// The forward walk of reach b over all rows.
LGAR_NET_FN void net_walk(const NetArgs &a, long long b) {
  constexpr int CH = LGAR_NET_CHUNK;
  double Iprev = a.state_in ? a.state_in[b] : 0.0, Oprev = a.state_in ? a.state_in[a.B + b] : 0.0;
  if (a.T > 0) {
    const double c0 = a.coef[b], c1 = a.coef[a.B + b], c2 = a.coef[2 * a.B + b];
    const long long e0 = net_clamp(a.up_ptr[b], a.E), e1 = net_clamp(a.up_ptr[b + 1], a.E);
    for (long long t0 = 0; t0 < a.T; t0 += CH) {
      double I[CH];
      net_inflow<CH, 1>(a.x, a.y, a.up_idx, a.T, a.B, b, e0, e1, t0, I);
#pragma unroll
      for (int u = 0; u < CH; u++)
        if (t0 + u < a.T) {
          const double O = (c0 * I[u] + c1 * Iprev) + c2 * Oprev;
          a.y[(t0 + u) * a.B + b] = O;
          Iprev = I[u];
          Oprev = O;
        }
    }
  }
  if (a.state_out) {
    a.state_out[b] = Iprev;
    a.state_out[a.B + b] = Oprev;
  }
}

// The adjoint walk of reach b, rows T - 1 down to 0:
//     a = gy[t][b] (+ gx[t][down[b]]);  lam = a + c2 lam_next;  gx[t][b] = c0 lam + c1 lam_next
// GC: also gc0 += lam I[t], gc1 += lam I[t - 1], gc2 += lam y[t - 1][b], each from +0.0 in decreasing t.  At row t the walk holds
// I[t] and y[t][b], which are what the terms of row t + 1 of gc1 and gc2 need, and lam_next is that row's lam: they are added
// here, and the terms of row 0 (I[-1], y[-1]: state_in, or zeros) after the last row.  The first row walked adds no such term.
template <bool GC> LGAR_NET_FN void net_walk_back(const NetGradArgs &a, long long b) {
  constexpr int CH = LGAR_NET_CHUNK;
  double lam_next = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
  if (a.T > 0) {
    const double c0 = a.coef[b], c1 = a.coef[a.B + b], c2 = a.coef[2 * a.B + b];
    const long long d_raw = a.down[b];
    const bool has = d_raw >= 0;
    const double *gd = a.gx + net_clamp(d_raw, a.B - 1);
    long long e0 = 0, e1 = 0;
    if (GC) e0 = net_clamp(a.up_ptr[b], a.E), e1 = net_clamp(a.up_ptr[b + 1], a.E);
    for (long long t0 = a.T - 1; t0 >= 0; t0 -= CH) {
      double gyv[CH], gdv[CH], I[CH], yo[CH];
#pragma unroll
      for (int u = 0; u < CH; u++) gyv[u] = a.gy[net_row<-1>(t0, u, a.T) * a.B + b];
#pragma unroll
      for (int u = 0; u < CH; u++) gdv[u] = has ? gd[net_row<-1>(t0, u, a.T) * a.B] : 0.0;
      if (GC) {
#pragma unroll
        for (int u = 0; u < CH; u++) yo[u] = a.y[net_row<-1>(t0, u, a.T) * a.B + b];
        net_inflow<CH, -1>(a.x, a.y, a.up_idx, a.T, a.B, b, e0, e1, t0, I);
      }
#pragma unroll
      for (int u = 0; u < CH; u++)
        if (t0 - u >= 0) {
          const long long t = t0 - u;
          const double av = has ? gyv[u] + gdv[u] : gyv[u];
          const double lam = av + c2 * lam_next;
          a.gx[t * a.B + b] = c0 * lam + c1 * lam_next;
          if (GC) {
            g0 = g0 + lam * I[u];
            if (t < a.T - 1) {
              g1 = g1 + lam_next * I[u];
              g2 = g2 + lam_next * yo[u];
            }
          }
          lam_next = lam;
        }
    }
    if (GC) {
      g1 = g1 + lam_next * (a.state_in ? a.state_in[b] : 0.0);
      g2 = g2 + lam_next * (a.state_in ? a.state_in[a.B + b] : 0.0);
    }
  }
  if (GC) {
    a.gc[b] = g0;
    a.gc[a.B + b] = g1;
    a.gc[2 * a.B + b] = g2;
  }
}

// ---- what the entry points refuse (host code: level_ptr is HOST memory, the one array the library reads on the host) ----------
// level_ptr[n_levels + 1] must start at 0, end at B and never decrease.
inline bool net_levels_ok(const int32_t *level_ptr, int32_t n_levels, int32_t B) {
  if (!level_ptr || level_ptr[0] != 0 || level_ptr[n_levels] != B) return false;
  for (int32_t l = 0; l < n_levels; l++)
    if (level_ptr[l + 1] < level_ptr[l]) return false;
  return true;
}

// 0: launch; 1: nothing to do; LGAR_E_ARG
inline int net_route_check(const double *x, int32_t T, int32_t B, const double *coef, const int32_t *up_ptr, const int32_t *up_idx,
                           int32_t E, const int32_t *order, const int32_t *level_ptr, int32_t n_levels, double *state_out,
                           double *y) {
  if (T < 0 || B < 0 || E < 0 || n_levels < 0) return LGAR_E_ARG;
  if (B == 0) return 1;
  if (!net_levels_ok(level_ptr, n_levels, B)) return LGAR_E_ARG;
  if (T == 0 && !state_out) return 1;
  if (!order) return LGAR_E_ARG;
  if (T > 0 && (!x || !y || !coef || !up_ptr || (E > 0 && !up_idx))) return LGAR_E_ARG;
  return 0;
}

inline int net_grad_check(const double *gy, int32_t T, int32_t B, const double *coef, const int32_t *down, const int32_t *order,
                          const int32_t *level_ptr, int32_t n_levels, double *gx, const double *x, const double *y,
                          const int32_t *up_ptr, const int32_t *up_idx, int32_t E, double *gc) {
  if (T < 0 || B < 0 || E < 0 || n_levels < 0) return LGAR_E_ARG;
  if (B == 0) return 1;
  if (!net_levels_ok(level_ptr, n_levels, B)) return LGAR_E_ARG;
  if (T == 0 && !gc) return 1;
  if (!order) return LGAR_E_ARG;
  if (T > 0 && (!gy || !gx || !coef || !down)) return LGAR_E_ARG;
  if (T > 0 && gc && (!x || !y || !up_ptr || (E > 0 && !up_idx))) return LGAR_E_ARG;
  return 0;
}

#ifdef LGAR_DEVSIM
// the kernels' work, one lane at a time, one level after the other
inline void net_route_all(const NetArgs &a, const int32_t *level_ptr, int32_t n_levels) {
  for (int32_t l = 0; l < n_levels; l++)
    for (long long p = level_ptr[l]; p < level_ptr[l + 1]; p++) net_walk(a, net_reach(a.order, p, a.B));
}

inline void net_grad_all(const NetGradArgs &a, const int32_t *level_ptr, int32_t n_levels) {
  for (int32_t l = n_levels - 1; l >= 0; l--)
    for (long long p = level_ptr[l]; p < level_ptr[l + 1]; p++) {
      if (a.gc) net_walk_back<true>(a, net_reach(a.order, p, a.B));
      else net_walk_back<false>(a, net_reach(a.order, p, a.B));
    }
}
#endif

}  // namespace lgar
