// lgar_network_mc.hpp -- catchment network: Muskingum-Cunge reaches whose storage constant is a power law of the reach's own
// previous discharge, their adjoint and the gradients with respect to the three reach parameters and the initial state
// (lgar_network_route_mc / lgar_network_route_mc_grad, include/lgar.h has the full statement).
//
// Everything is fp64, catchment fastest.  The topology, `order`, the host level_ptr, state_in / state_out [2][B] = Iprev, Oprev
// and the inflow fold are lgar_network.hpp's (net_inflow, net_reach, net_clamp, net_row: included, not restated).
// par[4][B] = kref, beta, X, qref; half = 0.5 * dt_h, formed once.  One reach b, for t = 0 .. T - 1 (mc_row):
//
//     I   = x[t][b] (+ y[t][up_idx[e]], ascending e)
//     rho = Oprev / qref
//     rc  = rho < rmin ? rmin : (rho > rmax ? rmax : rho)
//     L   = mc_ln(rc);   tau = beta * L                                  K = kref rc^(-beta)
//     ta  = tau < 0 ? -tau : tau;   tc = ta > LGAR_GW_ZMAX ? LGAR_GW_ZMAX : ta
//     e   = gw_exp(tc)                                                    (lgar_baseflow.hpp's, as it is)
//     K   = tau > 0 ? kref / e : kref * e
//     KX  = K * X;   u = K - KX;   D = u + half
//     c0  = (half - KX) / D;   c1 = (half + KX) / D;   c2 = (u - half) / D
//     O   = (c0 * I + c1 * Iprev) + c2 * Oprev;   y[t][b] = O;   Iprev = I;   Oprev = O
//
// Every decision is a select: a NaN takes the last alternative, and the wave stays converged.  mc_ln, like gw_exp, is built from
// operations numpy restates one for one -- no libm, no fma (-ffp-contract=off), no hardware reciprocal.
//
// A reach is one lane's work (mc_walk), the rows in chunks of LGAR_NET_CHUNK whose loads are issued before the first row's
// arithmetic, as net_walk.  The adjoint (mc_walk_back) walks the rows downward; a chunk loads one row more of the inflow (I[t - 1]
// of its last row) and the rows t - 1 of the stored y, and takes K, the coefficients and the regime of row t from mc_row with
// Oprev = y[t - 1][b] (row 0: state_in): the forward's own function, the same bits.  It carries pI = c1 lam and
// pO = c2 lam + GK dKdq of the row above, so one pass is enough.
//
// Like lgar_network.hpp this header also compiles for the host with -DLGAR_DEVSIM: tests/network_mc_host runs the same text
// against the numpy statement of the definition.
#pragma once
#include "lgar_baseflow.hpp"
#include "lgar_network.hpp"

namespace lgar {

// One forward call.  par: [4][B] = kref, beta, X, qref.  state_in / state_out: [2][B] = Iprev, Oprev (NULL: zeros / not wanted).
struct McArgs {
  const double *x, *par, *state_in;
  double *y, *state_out;
  const int32_t *order, *up_ptr, *up_idx;
  double dt_h, rmin, rmax;
  long long T, B, E;
};

// One adjoint call.  gpar ([3][B] = gkref, gbeta, gX) / gstate ([2][B]) == NULL: not wanted.
struct McGradArgs {
  const double *gy, *x, *y, *par, *state_in;
  double *gx, *gpar, *gstate;
  const int32_t *order, *down, *up_ptr, *up_idx;
  double dt_h, rmin, rmax;
  long long T, B, E;
};

// ln(x) for a positive normal double x:
//     (m, k) = frexp(x)                         by integer operations on the bits: m in [0.5, 1), x = m 2^k
//     m < fl(sqrt 1/2) ?  m = 2 m, k = k - 1    (exact)  now m in [sqrt 1/2, sqrt 2)
//     s = (m - 1) / (m + 1);   z = s * s        ln m = 2 atanh s = 2 s sum_j z^j / (2 j + 1)
//     p = sum_{j <= 10} z^j / (2 j + 1)         Horner: p = p * z + c_j, one rounded multiply and one rounded add per step
//     L = k * LN2_HI + ((2 * s) * p + k * LN2_LO)
// LN2_HI / LN2_LO are gw_exp's: LN2_HI has 32 trailing zero bits, so k LN2_HI is exact for |k| <= 61.  The coefficients are the
// correctly rounded 1 / (2 j + 1).
// The error, to first order in u = 2^-53.  m - 1 is exact (Sterbenz: m is within a factor 2 of 1); m + 1 and the quotient round
// once each: s carries 2 u, z = s * s 5 u.  |s| <= (sqrt 2 - 1) / (sqrt 2 + 1) = 0.1716, z <= 0.02944.  Term j of the computed p
// carries the rounding of c_j, two roundings per Horner step below it and j factors z: at most 7 j + 2 factors (1 + d), so
// |p - sum| <= u sum_j (7 j + 2) z^j / (2 j + 1) < 2.1 u, counted as 3.  t = (2 s) p: 2 + 3 + 1 = 6 u relative to ln m; the series
// cut after j = 10 misses ln m by at most 2 |s| z^11 / (23 (1 - z)) <= 6.5e-19 |ln m|.  k LN2_LO rounds once and LN2_HI + LN2_LO
// misses ln 2 by 1.2e-26; the inner sum t + k LN2_LO and the outer sum round once each.  With k = 0 (every x in [sqrt 1/2,
// sqrt 2): the whole neighbourhood of 1) both sums are exact and L = t.  With k != 0, |t| <= ln sqrt 2 <= |L|, so the error
// relative to L is at most (6 + 1 + 1 + 1) u: in all gamma_9 + 7e-19 = 1.0e-15.  Measured against mpmath.log at 40 digits:
// profiles/r14/error_bound.txt.
// A NaN, an infinity, zero, a negative or a subnormal argument gives what the bit operations give (no meaning): rc never is one.
LGAR_GW_FN double mc_ln(double x) {
  const double LN2_HI = 0x1.62e42fee00000p-1, LN2_LO = 0x1.a39ef35793c76p-33, SQRT_HALF = 0x1.6a09e667f3bcdp-1;
  uint64_t bits;
  memcpy(&bits, &x, sizeof bits);
  const int32_t k0 = (int32_t)((bits >> 52) & 0x7ff) - 1022;
  const uint64_t mbits = (bits & 0x000fffffffffffffULL) | (1022ULL << 52);
  double m0;
  memcpy(&m0, &mbits, sizeof m0);
  const bool low = m0 < SQRT_HALF;
  const double m = low ? m0 + m0 : m0;
  const double k = (double)(low ? k0 - 1 : k0);
  const double s = (m - 1.0) / (m + 1.0);
  const double z = s * s;
  double p = 0x1.8618618618618p-5;     // 1 / 21
  p = p * z + 0x1.af286bca1af28p-5;    // 1 / 19
  p = p * z + 0x1.e1e1e1e1e1e1ep-5;    // 1 / 17
  p = p * z + 0x1.1111111111111p-4;    // 1 / 15
  p = p * z + 0x1.3b13b13b13b14p-4;    // 1 / 13
  p = p * z + 0x1.745d1745d1746p-4;    // 1 / 11
  p = p * z + 0x1.c71c71c71c71cp-4;    // 1 / 9
  p = p * z + 0x1.2492492492492p-3;    // 1 / 7
  p = p * z + 0x1.999999999999ap-3;    // 1 / 5
  p = p * z + 0x1.5555555555555p-2;    // 1 / 3
  p = p * z + 1.0;
  return k * LN2_HI + ((2.0 * s) * p + k * LN2_LO);
}

// What one row takes from Oprev and the reach's constants: the regime and the coefficients.
struct McRow {
  double L, K, D, c0, c1, c2;
  bool inside, big;  // inside: neither select of rc fired and ta <= ZMAX (K follows Oprev);  big: ta > ZMAX (K does not follow beta)
};

LGAR_GW_FN McRow mc_row(double Oprev, double kref, double beta, double X, double qref, double half, double rmin, double rmax) {
  McRow o;
  const double rho = Oprev / qref;
  const bool lo = rho < rmin, hi = !lo && rho > rmax;
  const double rc = lo ? rmin : (hi ? rmax : rho);
  o.L = mc_ln(rc);
  const double tau = beta * o.L;
  const double ta = tau < 0.0 ? -tau : tau;
  o.big = ta > LGAR_GW_ZMAX;
  const double tc = o.big ? LGAR_GW_ZMAX : ta;
  const double e = gw_exp(tc);
  o.K = tau > 0.0 ? kref / e : kref * e;
  const double KX = o.K * X;
  const double u = o.K - KX;
  o.D = u + half;
  o.c0 = (half - KX) / o.D;
  o.c1 = (half + KX) / o.D;
  o.c2 = (u - half) / o.D;
  o.inside = !lo && !hi && !o.big;
  return o;
}

// The forward walk of reach b over all rows.
LGAR_NET_FN void mc_walk(const McArgs &a, long long b) {
  constexpr int CH = LGAR_NET_CHUNK;
  double Iprev = a.state_in ? a.state_in[b] : 0.0, Oprev = a.state_in ? a.state_in[a.B + b] : 0.0;
  if (a.T > 0) {
    const double kref = a.par[b], beta = a.par[a.B + b], X = a.par[2 * a.B + b], qref = a.par[3 * a.B + b];
    const double half = 0.5 * a.dt_h;
    const long long e0 = net_clamp(a.up_ptr[b], a.E), e1 = net_clamp(a.up_ptr[b + 1], a.E);
    for (long long t0 = 0; t0 < a.T; t0 += CH) {
      double I[CH];
      net_inflow<CH, 1>(a.x, a.y, a.up_idx, a.T, a.B, b, e0, e1, t0, I);
#pragma unroll
      for (int u = 0; u < CH; u++)
        if (t0 + u < a.T) {
          const McRow r = mc_row(Oprev, kref, beta, X, qref, half, a.rmin, a.rmax);
          const double O = (r.c0 * I[u] + r.c1 * Iprev) + r.c2 * Oprev;
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

// The adjoint walk of reach b, rows T - 1 down to 0, with pI = pO = +0.0 and three accumulators from +0.0.  Row t, with
// Ip = I[t - 1], Op = y[t - 1][b] (row 0: state_in, or zeros), r = mc_row(Op, ..) and omx = 1.0 - X (once per reach):
//     av    = gy[t][b] (+ gx[t][down[b]]);   lam = av + pO;   gx[t][b] = r.c0 * lam + pI
//     dK    = ((I * (-(X + c0 * omx)) + Ip * (X - c1 * omx)) + Op * (omx * (1.0 - c2))) / D;          GK = lam * dK
//     dX    = ((I * (-(1.0 - c0)) + Ip * (1.0 + c1)) + Op * (-(1.0 - c2))) * (K / D);                 GX = lam * dX
//     gkref = gkref + GK * (K / kref);   gbeta = big ? gbeta : gbeta + GK * (-(K * L));   gX = gX + GX
//     pI    = c1 * lam;   pO = inside ? c2 * lam + GK * ((-(beta * K)) / Op) : c2 * lam
// and gstate = pI, pO after row 0.  The regimes are selects on the forward's own values; an accumulator that receives no term in
// a row is left as it is (a select of the accumulator, not an added zero).  GP: the parameter gradient is wanted.
template <bool GP> LGAR_NET_FN void mc_walk_back(const McGradArgs &a, long long b) {
  constexpr int CH = LGAR_NET_CHUNK;
  double pI = 0.0, pO = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
  if (a.T > 0) {
    const double kref = a.par[b], beta = a.par[a.B + b], X = a.par[2 * a.B + b], qref = a.par[3 * a.B + b];
    const double half = 0.5 * a.dt_h, omx = 1.0 - X;
    const double I0 = a.state_in ? a.state_in[b] : 0.0, O0 = a.state_in ? a.state_in[a.B + b] : 0.0;
    const long long d_raw = a.down[b];
    const bool has = d_raw >= 0;
    const double *gd = a.gx + net_clamp(d_raw, a.B - 1);
    const long long e0 = net_clamp(a.up_ptr[b], a.E), e1 = net_clamp(a.up_ptr[b + 1], a.E);
    for (long long t0 = a.T - 1; t0 >= 0; t0 -= CH) {
      double gyv[CH], gdv[CH], yo[CH], I[CH + 1];
#pragma unroll
      for (int u = 0; u < CH; u++) gyv[u] = a.gy[net_row<-1>(t0, u, a.T) * a.B + b];
#pragma unroll
      for (int u = 0; u < CH; u++) gdv[u] = has ? gd[net_row<-1>(t0, u, a.T) * a.B] : 0.0;
#pragma unroll
      for (int u = 0; u < CH; u++) yo[u] = a.y[net_row<-1>(t0 - 1, u, a.T) * a.B + b];  // y[t - 1]; row 0 takes O0 below
      net_inflow<CH + 1, -1>(a.x, a.y, a.up_idx, a.T, a.B, b, e0, e1, t0, I);          // I[t] and I[t - 1]; row 0 takes I0
#pragma unroll
      for (int u = 0; u < CH; u++)
        if (t0 - u >= 0) {
          const long long t = t0 - u;
          const double Ip = t > 0 ? I[u + 1] : I0, Op = t > 0 ? yo[u] : O0;
          const McRow r = mc_row(Op, kref, beta, X, qref, half, a.rmin, a.rmax);
          const double av = has ? gyv[u] + gdv[u] : gyv[u];
          const double lam = av + pO;
          a.gx[t * a.B + b] = r.c0 * lam + pI;
          const double dK = ((I[u] * (-(X + r.c0 * omx)) + Ip * (X - r.c1 * omx)) + Op * (omx * (1.0 - r.c2))) / r.D;
          const double GK = lam * dK;
          if (GP) {
            const double dX = ((I[u] * (-(1.0 - r.c0)) + Ip * (1.0 + r.c1)) + Op * (-(1.0 - r.c2))) * (r.K / r.D);
            g0 = g0 + GK * (r.K / kref);
            g1 = r.big ? g1 : g1 + GK * (-(r.K * r.L));
            g2 = g2 + lam * dX;
          }
          const double c2l = r.c2 * lam;
          pI = r.c1 * lam;
          pO = r.inside ? c2l + GK * ((-(beta * r.K)) / Op) : c2l;
        }
    }
  }
  if (GP) {
    a.gpar[b] = g0;
    a.gpar[a.B + b] = g1;
    a.gpar[2 * a.B + b] = g2;
  }
  if (a.gstate) {
    a.gstate[b] = pI;
    a.gstate[a.B + b] = pO;
  }
}

// ---- what the entry points refuse (host code) -------------------------------------------------------------------------------
// dt_h finite and > 0 (gw_dt_ok); rmin, rmax finite with 2^-60 <= rmin <= rmax <= 2^60 (a NaN fails every comparison): rc is a
// positive normal double whatever Oprev is, and k LN2_HI of mc_ln is exact.
inline bool mc_scalars_ok(double dt_h, double rmin, double rmax) {
  return gw_dt_ok(dt_h) && rmin >= 0x1p-60 && rmax <= 0x1p60 && rmin <= rmax;
}

// 0: launch; 1: nothing to do; LGAR_E_ARG.  The sizes, level_ptr and the pointers are lgar_network_route's (par in coef's place);
// a null par is refused whenever there is a reach (B > 0), also where T = 0 would not read it.
inline int mc_route_check(const double *x, int32_t T, int32_t B, const double *par, double dt_h, double rmin, double rmax,
                          const int32_t *up_ptr, const int32_t *up_idx, int32_t E, const int32_t *order, const int32_t *level_ptr,
                          int32_t n_levels, double *state_out, double *y) {
  if (!mc_scalars_ok(dt_h, rmin, rmax)) return LGAR_E_ARG;
  const int rc = net_route_check(x, T, B, par, up_ptr, up_idx, E, order, level_ptr, n_levels, state_out, y);
  if (rc < 0 || B == 0) return rc;
  return par ? rc : LGAR_E_ARG;
}

inline int mc_grad_check(const double *gy, int32_t T, int32_t B, const double *par, double dt_h, double rmin, double rmax,
                         const int32_t *down, const int32_t *order, const int32_t *level_ptr, int32_t n_levels, double *gx,
                         const double *x, const double *y, const int32_t *up_ptr, const int32_t *up_idx, int32_t E, double *gpar,
                         double *gstate) {
  if (T < 0 || B < 0 || E < 0 || n_levels < 0 || !mc_scalars_ok(dt_h, rmin, rmax)) return LGAR_E_ARG;
  if (B == 0) return 1;
  if (!net_levels_ok(level_ptr, n_levels, B) || !par) return LGAR_E_ARG;
  if (T == 0 && !gpar && !gstate) return 1;
  if (!order) return LGAR_E_ARG;
  if (T > 0 && (!gy || !gx || !down || !x || !y || !up_ptr || (E > 0 && !up_idx))) return LGAR_E_ARG;
  return 0;
}

#ifdef LGAR_DEVSIM
// the kernels' work, one lane at a time, one level after the other
inline void mc_route_all(const McArgs &a, const int32_t *level_ptr, int32_t n_levels) {
  for (int32_t l = 0; l < n_levels; l++)
    for (long long p = level_ptr[l]; p < level_ptr[l + 1]; p++) mc_walk(a, net_reach(a.order, p, a.B));
}

inline void mc_grad_all(const McGradArgs &a, const int32_t *level_ptr, int32_t n_levels) {
  for (int32_t l = n_levels - 1; l >= 0; l--)
    for (long long p = level_ptr[l]; p < level_ptr[l + 1]; p++) {
      if (a.gpar) mc_walk_back<true>(a, net_reach(a.order, p, a.B));
      else mc_walk_back<false>(a, net_reach(a.order, p, a.B));
    }
}
#endif

}  // namespace lgar
