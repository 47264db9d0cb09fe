// lgar_network_pool.hpp -- catchment network with two node kinds: Muskingum-Cunge reaches (lgar_network_mc.hpp's mc_row, as it is)
// and level-pool reservoirs, their adjoint and the gradients with respect to the reach parameters, four pool parameters and the
// initial state (lgar_network_route_pool / lgar_network_route_pool_grad, include/lgar.h has the full statement; DESIGN.md
// section 18).
//
// Everything is fp64, catchment fastest.  The topology, the inflow fold, par_mc[4][B], state_in / state_out [2][B] and the reach
// walks are lgar_network.hpp's and lgar_network_mc.hpp's (included, not restated).  The KIND of a node is never a lane's branch:
// inside every level of `order` the reaches come first and the pools after them, and the host array pool_ptr[n_levels] gives the
// split (level_ptr[l] <= pool_ptr[l] <= level_ptr[l + 1]); a level gets a reach launch and a pool launch.  The pool data are
// compact over the P pools: pool_slot[B] (device; the pool's index, -1 at a reach; clamped into 0 .. P - 1 when read),
// par_pool[5][P] = cq, m, s0, sref, smax, storage[T][P].  The state of a pool is (Iprev, S).  One pool b of slot s, with
// half = 0.5 * dt_h and cap = smax - s0 formed once, for t = 0 .. T - 1 (pool_row):
//
//     I    = x[t][b] (+ y[t][up_idx[e]], ascending e)
//     vin  = half * (I + Iprev)                                  the volume that arrives in the step (trapezoid)
//     a    = S - s0;   rho = a / sref
//     lo   = rho < prmin;  hi = !lo && rho > prmax;  rc = lo ? prmin : (hi ? prmax : rho)
//     L    = mc_ln(rc);   tau = m * L
//     ta   = tau < 0 ? -tau : tau;   big = ta > LGAR_GW_ZMAX;   tc = big ? LGAR_GW_ZMAX : ta
//     e    = gw_exp(tc)
//     Ql   = tau > 0 ? cq * e : cq / e                           the release law cq rc^m
//     av   = a + vin;   qa = av / dt_h                           what could leave if the pool drained to s0
//     free = Ql < qa;   Q = free ? Ql : qa                       (a NaN qa stays)
//     empty = Q < 0;    Q = empty ? 0.0 : Q                      (a NaN Q stays)
//     r    = av - dt_h * Q                                       arithmetic, not a select: a NaN reaches the storage
//     ex   = r - cap;   spill = ex > 0
//     O    = spill ? Q + ex / dt_h : Q
//     S    = (spill ? cap : r) + s0
//     y[t][b] = O;   storage[t][s] = S;   Iprev = I
//
// Every decision is a select; no libm, no fma (-ffp-contract=off), no hardware reciprocal.  In real arithmetic
// S_t - S_{t-1} = vin_t - dt_h O_t in every regime: the stage conserves volume.
//
// The release law's error.  rc is a positive normal double in 2^-60 .. 2^60, so L = ln rc (1 + dL), |dL| <= 1.0e-15 (mc_ln's
// bound, lgar_network_mc.hpp); tau = m L rounds once: |tau - m ln rc| <= |tau| (1.0e-15 + u) to first order.  e = gw_exp(|tau|)
// turns that absolute error into a relative one and adds its own 4.56e-15 (gw_exp's bound, tests/test_baseflow_host.py and
// profiles/r11/error_bound.txt); cq * e or cq / e rounds once more.  For |tau| <= LGAR_GW_ZMAX:
//     |Ql - cq rc^m| / (cq rc^m) <= |tau| (1.0e-15 + u) + 4.56e-15 + u  (first order; the second-order terms are below 1e-27)
// that is 4.9e-14 at |tau| = 40 and 4.7e-15 at tau = 0.  Measured against mpmath.power at 40 digits: profiles/r15/error_bound.txt.
//
// A pool is one lane's work (pool_walk), the rows in chunks of LGAR_NET_CHUNK whose loads are issued before the first row's
// arithmetic, as mc_walk.  The adjoint (pool_walk_back) walks the rows downward; a chunk loads one row more of the inflow and the
// rows t - 1 of the stored storage, and takes the regime, L, Ql and a of row t from pool_row with S = storage[t - 1][s] (row 0:
// state_in): the forward's own function, the same bits.  It carries pI and pS of the row above, so one pass is enough.
//
// Like its siblings this header also compiles for the host with -DLGAR_DEVSIM: tests/network_pool_host runs the same text against
// the numpy statement of the definition.
#pragma once
#include "lgar_baseflow.hpp"
#include "lgar_network.hpp"
#include "lgar_network_mc.hpp"

namespace lgar {

// One forward call: the reach walk's block (mc.par = par_mc, mc.state_* with S in Oprev's place at a pool) and the pool data.
struct PoolArgs {
  McArgs mc;
  const double *par_pool;  // [5][P] = cq, m, s0, sref, smax
  const int32_t *pool_slot;
  double *storage;  // [T][P], NULL: not wanted
  double prmin, prmax;
  long long P;
};

// One adjoint call.  mc.gpar ([3][B]; +0.0 at a pool) / gpool ([4][P] = gcq, gm, gs0, gsmax) / mc.gstate == NULL: not wanted.
struct PoolGradArgs {
  McGradArgs mc;
  const double *par_pool, *storage;
  const int32_t *pool_slot;
  double *gpool;
  double prmin, prmax;
  long long P;
};

// What one row makes of S, the volume in and the pool's constants.
struct PoolRow {
  double a, L, e, Ql, O, S;
  bool up;  // tau > 0: Ql = cq * e (else cq / e)
  bool inside, big, free, empty, spill;  // inside: neither select of rc fired and ta <= ZMAX (Ql follows S);  big: Ql does not follow m
};

LGAR_GW_FN PoolRow pool_row(double S, double vin, double cq, double m, double s0, double sref, double cap, double dt_h, double prmin,
                            double prmax) {
  PoolRow o;
  o.a = S - s0;
  const double rho = o.a / sref;
  const bool lo = rho < prmin, hi = !lo && rho > prmax;
  const double rc = lo ? prmin : (hi ? prmax : rho);
  o.L = mc_ln(rc);
  const double tau = m * o.L;
  const double ta = tau < 0.0 ? -tau : tau;
  o.big = ta > LGAR_GW_ZMAX;
  const double tc = o.big ? LGAR_GW_ZMAX : ta;
  o.e = gw_exp(tc);
  o.up = tau > 0.0;
  o.Ql = o.up ? cq * o.e : cq / o.e;
  const double av = o.a + vin;
  const double qa = av / dt_h;
  o.free = o.Ql < qa;
  const double Q0 = o.free ? o.Ql : qa;
  o.empty = Q0 < 0.0;
  const double Q = o.empty ? 0.0 : Q0;
  const double r = av - dt_h * Q;
  const double ex = r - cap;
  o.spill = ex > 0.0;
  o.O = o.spill ? Q + ex / dt_h : Q;
  o.S = (o.spill ? cap : r) + s0;
  o.inside = !lo && !hi && !o.big;
  return o;
}

// the slot of pool b, kept inside 0 .. P - 1
LGAR_NET_FN long long pool_slot_of(const int32_t *pool_slot, long long b, long long P) { return net_clamp(pool_slot[b], P - 1); }

// The forward walk of pool b over all rows.
LGAR_NET_FN void pool_walk(const PoolArgs &p, long long b) {
  constexpr int CH = LGAR_NET_CHUNK;
  const McArgs &a = p.mc;
  double Iprev = a.state_in ? a.state_in[b] : 0.0, S = a.state_in ? a.state_in[a.B + b] : 0.0;
  if (a.T > 0) {
    const long long s = pool_slot_of(p.pool_slot, b, p.P);
    const double cq = p.par_pool[s], m = p.par_pool[p.P + s], s0 = p.par_pool[2 * p.P + s], sref = p.par_pool[3 * p.P + s];
    const double cap = p.par_pool[4 * p.P + s] - s0, half = 0.5 * a.dt_h;
    const long long e0 = net_clamp(a.up_ptr[b], a.E), e1 = net_clamp(a.up_ptr[b + 1], a.E);
    for (long long t0 = 0; t0 < a.T; t0 += CH) {
      double I[CH];
      net_inflow<CH, 1>(a.x, a.y, a.up_idx, a.T, a.B, b, e0, e1, t0, I);
#pragma unroll
      for (int u = 0; u < CH; u++)
        if (t0 + u < a.T) {
          const PoolRow r = pool_row(S, half * (I[u] + Iprev), cq, m, s0, sref, cap, a.dt_h, p.prmin, p.prmax);
          a.y[(t0 + u) * a.B + b] = r.O;
          if (p.storage) p.storage[(t0 + u) * p.P + s] = r.S;
          Iprev = I[u];
          S = r.S;
        }
    }
  }
  if (a.state_out) {
    a.state_out[b] = Iprev;
    a.state_out[a.B + b] = S;
  }
}

// The adjoint walk of pool b, rows T - 1 down to 0, with pI = pS = +0.0 and four accumulators from +0.0.  Row t, with
// Ip = I[t - 1], Sp = storage[t - 1][s] (row 0: state_in, or zeros), r = pool_row(Sp, half * (I + Ip), ..) and
// pw = r.up ? e : 1.0 / e (= dQl/dcq):
//     lamO  = gy[t][b] (+ gx[t][down[b]]);   lamS = pS;   q = lamO / dt_h
//     gr    = spill ? q : lamS;              gcap = lamS - q                              (used where spill)
//     gs0   = gs0 + (spill ? lamS - gcap : lamS);   gsmax = spill ? gsmax + gcap : gsmax
//     gQ    = empty ? 0.0 : lamO - dt_h * gr
//     gav   = free ? gr : gr + gQ / dt_h
//     gcq   = free ? gcq + gQ * pw : gcq
//     gm    = free && !big ? gm + (gQ * Ql) * L : gm
//     ga    = free && inside ? gav + ((gQ * m) * Ql) / a : gav
//     hg    = half * gav;   gx[t][b] = hg + pI;   pI = hg;   pS = ga;   gs0 = gs0 - ga
// and gstate = pI, pS after row 0.  The regimes are selects on the forward's own values; an accumulator that receives no term in
// a row is left as it is; `inside` is a select, not a multiply by zero (a may be 0 outside).  GP: gpool is wanted.  The three
// reach gradients of a pool are written +0.0.
template <bool GP> LGAR_NET_FN void pool_walk_back(const PoolGradArgs &p, long long b) {
  constexpr int CH = LGAR_NET_CHUNK;
  const McGradArgs &a = p.mc;
  double pI = 0.0, pS = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0, g3 = 0.0;
  const long long s = pool_slot_of(p.pool_slot, b, p.P);
  if (a.T > 0) {
    const double cq = p.par_pool[s], m = p.par_pool[p.P + s], s0 = p.par_pool[2 * p.P + s], sref = p.par_pool[3 * p.P + s];
    const double cap = p.par_pool[4 * p.P + s] - s0, half = 0.5 * a.dt_h;
    const double I0 = a.state_in ? a.state_in[b] : 0.0, S0 = a.state_in ? a.state_in[a.B + b] : 0.0;
    const long long d_raw = a.down[b];
    const bool has = d_raw >= 0;
    const double *gd = a.gx + net_clamp(d_raw, a.B - 1);
    const long long e0 = net_clamp(a.up_ptr[b], a.E), e1 = net_clamp(a.up_ptr[b + 1], a.E);
    for (long long t0 = a.T - 1; t0 >= 0; t0 -= CH) {
      double gyv[CH], gdv[CH], so[CH], I[CH + 1];
#pragma unroll
      for (int u = 0; u < CH; u++) gyv[u] = a.gy[net_row<-1>(t0, u, a.T) * a.B + b];
#pragma unroll
      for (int u = 0; u < CH; u++) gdv[u] = has ? gd[net_row<-1>(t0, u, a.T) * a.B] : 0.0;
#pragma unroll
      for (int u = 0; u < CH; u++) so[u] = p.storage[net_row<-1>(t0 - 1, u, a.T) * p.P + s];  // S of row t - 1; row 0 takes S0 below
      net_inflow<CH + 1, -1>(a.x, a.y, a.up_idx, a.T, a.B, b, e0, e1, t0, I);                // I[t] and I[t - 1]; row 0 takes I0
#pragma unroll
      for (int u = 0; u < CH; u++)
        if (t0 - u >= 0) {
          const long long t = t0 - u;
          const double Ip = t > 0 ? I[u + 1] : I0, Sp = t > 0 ? so[u] : S0;
          const PoolRow r = pool_row(Sp, half * (I[u] + Ip), cq, m, s0, sref, cap, a.dt_h, p.prmin, p.prmax);
          const double lamO = has ? gyv[u] + gdv[u] : gyv[u];
          const double lamS = pS;
          const double q = lamO / a.dt_h;
          const double gr = r.spill ? q : lamS;
          const double gcap = lamS - q;
          const double gQ = r.empty ? 0.0 : lamO - a.dt_h * gr;
          const double gav = r.free ? gr : gr + gQ / a.dt_h;
          const double ga = r.free && r.inside ? gav + ((gQ * m) * r.Ql) / r.a : gav;
          if (GP) {
            const double pw = r.up ? r.e : 1.0 / r.e;
            g0 = r.free ? g0 + gQ * pw : g0;
            g1 = r.free && !r.big ? g1 + (gQ * r.Ql) * r.L : g1;
            g2 = (g2 + (r.spill ? lamS - gcap : lamS)) - ga;
            g3 = r.spill ? g3 + gcap : g3;
          }
          const double hg = half * gav;
          a.gx[t * a.B + b] = hg + pI;
          pI = hg;
          pS = ga;
        }
    }
  }
  if (GP) {
    p.gpool[s] = g0;
    p.gpool[p.P + s] = g1;
    p.gpool[2 * p.P + s] = g2;
    p.gpool[3 * p.P + s] = g3;
  }
  if (a.gpar) {
    a.gpar[b] = 0.0;
    a.gpar[a.B + b] = 0.0;
    a.gpar[2 * a.B + b] = 0.0;
  }
  if (a.gstate) {
    a.gstate[b] = pI;
    a.gstate[a.B + b] = pS;
  }
}

// ---- what the entry points refuse (host code) -------------------------------------------------------------------------------
// prmin, prmax: mc's admissible range (rc is a positive normal double whatever S is, and k LN2_HI of mc_ln is exact)
inline bool pool_scalars_ok(double dt_h, double rmin, double rmax, double prmin, double prmax) {
  return mc_scalars_ok(dt_h, rmin, rmax) && prmin >= 0x1p-60 && prmax <= 0x1p60 && prmin <= prmax;
}

// pool_ptr[n_levels] (HOST memory, like level_ptr, which must have passed net_levels_ok): every split inside its level; with no
// pool data (P = 0) no level may have a pool segment.
inline bool pool_levels_ok(const int32_t *pool_ptr, const int32_t *level_ptr, int32_t n_levels, int32_t P) {
  if (n_levels > 0 && !pool_ptr) return false;
  for (int32_t l = 0; l < n_levels; l++) {
    if (pool_ptr[l] < level_ptr[l] || pool_ptr[l] > level_ptr[l + 1]) return false;
    if (P == 0 && pool_ptr[l] != level_ptr[l + 1]) return false;
  }
  return true;
}

// 0: launch; 1: nothing to do; LGAR_E_ARG.  The scalars first, then everything lgar_network_route_mc refuses (its own function),
// then the pool arguments.
inline int pool_route_check(const double *x, int32_t T, int32_t B, const double *par_mc, const double *par_pool, int32_t P, double dt_h,
                            double rmin, double rmax, double prmin, double prmax, const int32_t *up_ptr, const int32_t *up_idx, int32_t E,
                            const int32_t *order, const int32_t *level_ptr, const int32_t *pool_ptr, int32_t n_levels,
                            const int32_t *pool_slot, double *state_out, double *y) {
  if (!pool_scalars_ok(dt_h, rmin, rmax, prmin, prmax) || P < 0) return LGAR_E_ARG;
  const int rc = mc_route_check(x, T, B, par_mc, dt_h, rmin, rmax, up_ptr, up_idx, E, order, level_ptr, n_levels, state_out, y);
  if (rc < 0 || B == 0) return rc;
  if (!pool_levels_ok(pool_ptr, level_ptr, n_levels, P) || (P > 0 && (!par_pool || !pool_slot))) return LGAR_E_ARG;
  return rc;
}

// (mc_grad_check only asks whether ANY parameter or state gradient is wanted when T = 0: gpool counts as one)
inline int pool_grad_check(const double *gy, int32_t T, int32_t B, const double *par_mc, const double *par_pool, int32_t P, double dt_h,
                           double rmin, double rmax, double prmin, double prmax, const int32_t *down, const int32_t *order,
                           const int32_t *level_ptr, const int32_t *pool_ptr, int32_t n_levels, const int32_t *pool_slot, double *gx,
                           const double *x, const double *y, const double *storage, const int32_t *up_ptr, const int32_t *up_idx,
                           int32_t E, double *gpar_mc, double *gpool, double *gstate) {
  if (!pool_scalars_ok(dt_h, rmin, rmax, prmin, prmax) || P < 0) return LGAR_E_ARG;
  const int rc = mc_grad_check(gy, T, B, par_mc, dt_h, rmin, rmax, down, order, level_ptr, n_levels, gx, x, y, up_ptr, up_idx, E,
                               gpar_mc ? gpar_mc : gpool, gstate);
  if (rc < 0 || B == 0) return rc;
  if (!pool_levels_ok(pool_ptr, level_ptr, n_levels, P) || (P > 0 && (!par_pool || !pool_slot))) return LGAR_E_ARG;
  if (T > 0 && P > 0 && !storage) return LGAR_E_ARG;
  return rc;
}

#ifdef LGAR_DEVSIM
// the kernels' work, one lane at a time, one level after the other, a level's reaches before its pools
inline void pool_route_all(const PoolArgs &p, const int32_t *level_ptr, const int32_t *pool_ptr, int32_t n_levels) {
  for (int32_t l = 0; l < n_levels; l++) {
    for (long long q = level_ptr[l]; q < pool_ptr[l]; q++) mc_walk(p.mc, net_reach(p.mc.order, q, p.mc.B));
    for (long long q = pool_ptr[l]; q < level_ptr[l + 1]; q++) pool_walk(p, net_reach(p.mc.order, q, p.mc.B));
  }
}

inline void pool_grad_all(const PoolGradArgs &p, const int32_t *level_ptr, const int32_t *pool_ptr, int32_t n_levels) {
  for (int32_t l = n_levels - 1; l >= 0; l--) {
    for (long long q = level_ptr[l]; q < pool_ptr[l]; q++) {
      if (p.mc.gpar) mc_walk_back<true>(p.mc, net_reach(p.mc.order, q, p.mc.B));
      else mc_walk_back<false>(p.mc, net_reach(p.mc.order, q, p.mc.B));
    }
    for (long long q = pool_ptr[l]; q < level_ptr[l + 1]; q++) {
      if (p.gpool) pool_walk_back<true>(p, net_reach(p.mc.order, q, p.mc.B));
      else pool_walk_back<false>(p, net_reach(p.mc.order, q, p.mc.B));
    }
  }
}
#endif

}  // namespace lgar
