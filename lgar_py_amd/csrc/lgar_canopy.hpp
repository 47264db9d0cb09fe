// lgar_canopy.hpp -- catchment canopy: the interception store ahead of the snowpack and the columns (a depth of water held on
// the leaves per forcing cell), its adjoint and its forward-mode tangent (lgar_catchment_canopy / lgar_catchment_canopy_grad /
// lgar_catchment_canopy_tangent, include/lgar.h has the full statement).
//
// All arrays are fp64, cell fastest: the precipitation rate p[T][B], the PET rate e[T][B], the relative leaf area lai[T][B] (NULL:
// 1, and then cap = cmax with no multiplication), the throughfall rate w[T][B], the PET left to the columns pet_out[T][B], the
// store store[T][B] and the wet-canopy evaporation rate evap[T][B], par[3][B] = cmax, fe, cover, the state [1][B] = s.  One cell b,
// with fc = fe * cover (once) and s = state_in (NULL: +0.0), for t = 0 .. T - 1 (cn_step):
//
//     pd   = p[t][b] * dt_h;      ed = e[t][b] * dt_h
//     hit  = cover * pd;          direct = pd - hit
//     cap  = cmax * lai[t][b]
//     s1   = s + hit;             full = s1 > cap
//     drip = full ? s1 - cap : 0.0
//     s2   = full ? cap : s1
//     dem  = fc * ed;             lim = dem > s2
//     ei   = lim ? s2 : dem
//     s    = s2 - ei
//     neg  = ei > ed
//     r    = neg ? 0.0 : ed - ei
//     w[t][b] = (direct + drip) / dt_h;   pet_out[t][b] = r / dt_h;   store[t][b] = s;   evap[t][b] = ei / dt_h
//
// Every decision is a select: the wave stays converged, and a NaN fails every comparison and so takes the last alternative.  What
// that means per input, for its cell alone:
//   a NaN in p[t][b]:   hit, direct and s1 are NaN, full is false (drip = 0.0, s2 = s1), lim is false (ei = dem): w of row t is NaN,
//                       evap and pet_out of row t are clean, store is NaN from row t on.  In the rows after it s1 is NaN, so drip =
//                       0.0 and ei = dem: w = direct / dt_h, evap = dem / dt_h and pet_out are clean -- the store carries the NaN.
//   a NaN in e[t][b]:   dem is NaN, lim is false (ei = dem = NaN), neg is false (r = ed - ei = NaN): evap and pet_out of row t are
//                       NaN, w of row t is clean, store is NaN from row t on (and the later rows are as above).
//   a NaN in lai[t][b]: cap is NaN, full is false: drip = 0.0 and s2 = s1 -- the row holds all that hit it and the NaN is gone.
//   a NaN in state_in:  as the rows after a NaN in p.
// No libm, no fma (-ffp-contract=off), IEEE divisions.
//
// A cell is one lane's work: it walks all rows (cn_walk), in chunks of LGAR_CN_CHUNK rows whose loads are all issued before the
// first of them is used (a chunk that reaches past the rows re-reads its last row: every load stays inside the arrays).  The
// recurrence is serial, so the bits are the definition's whatever the chunk is.  The adjoint (cn_walk_back) walks the rows downward;
// it re-forms row t from store[t - 1][b] (row 0: state_in) through cn_step, the forward's own function: every flag has the
// forward's bits.  Offsets are 64-bit.
//
// Like lgar_snow.hpp this header also compiles for the host with -DLGAR_DEVSIM: tests/canopy_host runs the same text against the
// numpy statement of the definition.
#pragma once
#ifndef LGAR_DEVSIM
#include <hip/hip_runtime.h>
#define LGAR_CN_FN __device__ __forceinline__
#else
#define LGAR_CN_FN inline
#endif
#include <stddef.h>
#include <stdint.h>

#include "../../include/lgar.h"

namespace lgar {

#define LGAR_CN_CHUNK 8  // rows of a cell whose loads are in flight together (as LGAR_SN_CHUNK)
#define LGAR_CN_NPAR 3   // cmax, fe, cover

// One forward call.  lai: [T][B] or NULL (= 1).  par: [3][B].  state_in / state_out: [1][B] (NULL: zeros / not wanted).  store,
// evap: both or neither.
struct CnArgs {
  const double *p, *e, *lai, *par, *state_in;
  double *w, *pet, *store, *evap, *state_out;
  double dt_h;
  long long T, B;
};

// One adjoint call.  gstore, gevap == NULL: zeros (each on its own).  glai ([T][B]) / gpar ([3][B]) / gstate ([1][B]) == NULL: not
// wanted.  store: the forward's.
struct CnGradArgs {
  const double *gw, *gpet, *gstore, *gevap, *p, *e, *lai, *store, *par, *state_in;
  double *gp, *ge, *glai, *gpar, *gstate;
  double dt_h;
  long long T, B;
};

// The parameters of one cell as the rows use them: fc = fe * cover (one rounding, once).
struct CnPar {
  double cmax, fe, cover, fc;
};

LGAR_CN_FN CnPar cn_par(const double *par, long long B, long long b) {
  CnPar c;
  c.cmax = par[b], c.fe = par[B + b], c.cover = par[2 * B + b];
  c.fc = c.fe * c.cover;
  return c;
}

// One row of the recurrence from the store before it (s), pd = p[t][b] * dt_h, ed = e[t][b] * dt_h and cap (cmax * lai[t][b], or
// cmax itself without leaf area).
struct CnRow {
  double tf, ei, r, s;  // direct + drip, the evaporation, the PET left (all depths), the store behind the row
  bool full, lim, neg;
};

LGAR_CN_FN CnRow cn_step(double s, double pd, double ed, double cap, const CnPar &c) {
  CnRow o;
  const double hit = c.cover * pd;
  const double direct = pd - hit;
  const double s1 = s + hit;
  o.full = s1 > cap;
  const double drip = o.full ? s1 - cap : 0.0;
  const double s2 = o.full ? cap : s1;
  const double dem = c.fc * ed;
  o.lim = dem > s2;
  o.ei = o.lim ? s2 : dem;
  o.s = s2 - o.ei;
  o.neg = o.ei > ed;
  o.r = o.neg ? 0.0 : ed - o.ei;
  o.tf = direct + drip;
  return o;
}

// row u of a chunk that starts at t0 and runs upward (DIR = +1) or downward (DIR = -1), kept inside 0 .. T - 1
template <int DIR> LGAR_CN_FN long long cn_row(long long t0, int u, long long T) {
  return DIR > 0 ? (t0 + u < T ? t0 + u : T - 1) : (t0 - u > 0 ? t0 - u : 0);
}

// The forward walk of cell b over all rows.
LGAR_CN_FN void cn_walk(const CnArgs &a, long long b) {
  constexpr int CH = LGAR_CN_CHUNK;
  double s = a.state_in ? a.state_in[b] : 0.0;
  if (a.T > 0) {
    const CnPar c = cn_par(a.par, a.B, b);
    for (long long t0 = 0; t0 < a.T; t0 += CH) {
      double pv[CH], ev[CH], lv[CH];
#pragma unroll
      for (int u = 0; u < CH; u++) pv[u] = a.p[cn_row<1>(t0, u, a.T) * a.B + b];
#pragma unroll
      for (int u = 0; u < CH; u++) ev[u] = a.e[cn_row<1>(t0, u, a.T) * a.B + b];
      if (a.lai) {
#pragma unroll
        for (int u = 0; u < CH; u++) lv[u] = a.lai[cn_row<1>(t0, u, a.T) * a.B + b];
      }
#pragma unroll
      for (int u = 0; u < CH; u++)
        if (t0 + u < a.T) {
          const double cap = a.lai ? c.cmax * lv[u] : c.cmax;
          const CnRow o = cn_step(s, pv[u] * a.dt_h, ev[u] * a.dt_h, cap, c);
          a.w[(t0 + u) * a.B + b] = o.tf / a.dt_h;
          a.pet[(t0 + u) * a.B + b] = o.r / a.dt_h;
          if (a.store) {
            a.store[(t0 + u) * a.B + b] = o.s;
            a.evap[(t0 + u) * a.B + b] = o.ei / a.dt_h;
          }
          s = o.s;
        }
    }
  }
  if (a.state_out) a.state_out[b] = s;
}

// The adjoint walk of cell b, rows T - 1 down to 0, with ls = +0.0 (the adjoint of s behind the row) and the accumulators gcmax,
// gfc, gcover from +0.0; full, lim, neg = cn_step of the row (the forward's bits), lai = lai[t][b] (NULL: 1.0):
//     ls   = ls + gstore[t][b];  gtf = gw[t][b] / dt_h;  gr = gpet[t][b] / dt_h;  gei = gevap[t][b] / dt_h
//     dr   = neg ? 0.0 : gr;          dei  = (gei - dr) - ls
//     ds2  = lim ? ls + dei : ls;     ddem = lim ? 0.0 : dei
//     gfc  = lim ? gfc : gfc + ddem * ed;          ged = dr + ddem * fc
//     ds1  = full ? gtf : ds2;        dcap = full ? ds2 - gtf : 0.0
//     gcmax = full ? gcmax + dcap * lai : gcmax;   glai[t][b] = dcap * cmax
//     dhit = ds1 - gtf;               gcover = gcover + dhit * pd
//     gp[t][b] = (gtf + dhit * cover) * dt_h;      ge[t][b] = ged * dt_h;      ls = ds1
// and after row 0: gfe = gfc * cover, gcover = gcover + gfc * fe, gstate = ls.  The regimes are selects on the forward's own flags,
// so a tie belongs to the branch the forward's select sends it to.  An accumulator that receives no term in a row is left as it
// is (a select of the accumulator, not an added zero).  GP: the parameter gradient is wanted.
template <bool GP> LGAR_CN_FN void cn_walk_back(const CnGradArgs &a, long long b) {
  constexpr int CH = LGAR_CN_CHUNK;
  double ls = 0.0, gcmax = 0.0, gfc = 0.0, gcover = 0.0, gfe = 0.0;
  if (a.T > 0) {
    const CnPar c = cn_par(a.par, a.B, b);
    const double s0 = a.state_in ? a.state_in[b] : 0.0;
    for (long long t0 = a.T - 1; t0 >= 0; t0 -= CH) {
      double gwv[CH], gpv[CH], gsv[CH], gev[CH], pv[CH], ev[CH], lv[CH], sv[CH];
#pragma unroll
      for (int u = 0; u < CH; u++) gwv[u] = a.gw[cn_row<-1>(t0, u, a.T) * a.B + b];
#pragma unroll
      for (int u = 0; u < CH; u++) gpv[u] = a.gpet[cn_row<-1>(t0, u, a.T) * a.B + b];
#pragma unroll
      for (int u = 0; u < CH; u++) gsv[u] = a.gstore ? a.gstore[cn_row<-1>(t0, u, a.T) * a.B + b] : 0.0;
#pragma unroll
      for (int u = 0; u < CH; u++) gev[u] = a.gevap ? a.gevap[cn_row<-1>(t0, u, a.T) * a.B + b] : 0.0;
#pragma unroll
      for (int u = 0; u < CH; u++) pv[u] = a.p[cn_row<-1>(t0, u, a.T) * a.B + b];
#pragma unroll
      for (int u = 0; u < CH; u++) ev[u] = a.e[cn_row<-1>(t0, u, a.T) * a.B + b];
#pragma unroll
      for (int u = 0; u < CH; u++) lv[u] = a.lai ? a.lai[cn_row<-1>(t0, u, a.T) * a.B + b] : 1.0;
#pragma unroll
      for (int u = 0; u < CH; u++) sv[u] = a.store[cn_row<-1>(t0 - 1, u, a.T) * a.B + b];  // store[t - 1]; row 0 takes s0 below
#pragma unroll
      for (int u = 0; u < CH; u++)
        if (t0 - u >= 0) {
          const long long t = t0 - u;
          const double pd = pv[u] * a.dt_h, ed = ev[u] * a.dt_h;
          const double cap = a.lai ? c.cmax * lv[u] : c.cmax;
          const CnRow o = cn_step(t > 0 ? sv[u] : s0, pd, ed, cap, c);
          ls = ls + gsv[u];
          const double gtf = gwv[u] / a.dt_h, gr = gpv[u] / a.dt_h, gei = gev[u] / a.dt_h;
          const double dr = o.neg ? 0.0 : gr;
          const double dei = (gei - dr) - ls;
          const double ds2 = o.lim ? ls + dei : ls;
          const double ddem = o.lim ? 0.0 : dei;
          const double ged = dr + ddem * c.fc;
          const double ds1 = o.full ? gtf : ds2;
          const double dcap = o.full ? ds2 - gtf : 0.0;
          const double dhit = ds1 - gtf;
          if (GP) {
            gfc = o.lim ? gfc : gfc + ddem * ed;
            gcmax = o.full ? gcmax + dcap * lv[u] : gcmax;
            gcover = gcover + dhit * pd;
          }
          if (a.glai) a.glai[t * a.B + b] = dcap * c.cmax;
          a.gp[t * a.B + b] = (gtf + dhit * c.cover) * a.dt_h;
          a.ge[t * a.B + b] = ged * a.dt_h;
          ls = ds1;
        }
    }
    if (GP) {
      gfe = gfc * c.cover;
      gcover = gcover + gfc * c.fe;
    }
  }
  if (GP) {
    a.gpar[b] = gcmax;
    a.gpar[a.B + b] = gfe;
    a.gpar[2 * a.B + b] = gcover;
  }
  if (a.gstate) a.gstate[b] = ls;
}

// ---- the forward-mode tangent (lgar_catchment_canopy_tangent) ------------------------------------------------------------------
// One lane per (cell b, direction k), k < D: lane i = k * B + b, cell fastest, so the loads of dp / de / dlai [D][T][B] and of the
// values are coalesced.  The VALUE recurrence of the lane is cn_step itself from state_in (every flag has the forward's bits);
// beside it runs s' from dstate_in (NULL: +0.0).  Once per lane, with cmax', fe', cover' = dpar[k][0..2][b] (NULL: 0):
//     fc' = fe' * cover + fe * cover'
// and per row, selects on the forward's flags, with lai = lai[t][b] (NULL: 1.0) and lai' = dlai[k][t][b] (NULL: 0.0):
//     pd'   = dp * dt_h;                    ed' = de * dt_h
//     hit'  = cover' * pd + cover * pd';    direct' = pd' - hit'
//     cap'  = cmax' * lai + cmax * lai'
//     s1'   = s' + hit';   drip' = full ? s1' - cap' : 0.0;   s2' = full ? cap' : s1'
//     dem'  = fc' * ed + fc * ed';          ei' = lim ? s2' : dem'
//     s'    = s2' - ei';   r' = neg ? 0.0 : ed' - ei'
//     dw[(t * B + b) * ld + k0 + k] = (direct' + drip') / dt_h;   dpet[(t * B + b) * ld + k0 + k] = r' / dt_h
//     dstore[k][t][b] = s';   devap[k][t][b] = ei' / dt_h
// ld >= k0 + D: the lane writes straight into the two [T][B][G] blocks of forcing tangents lgar_forward_tangent_forced reads.
// dpet == NULL: not wanted.  T = 0 copies dstate.  Rows in chunks of LGAR_CN_CHUNK as the forward walk; no fma, IEEE divisions.
struct CnTanArgs {
  const double *p, *e, *lai, *par, *state_in;          // the forward's inputs
  const double *dp, *de, *dlai, *dpar, *dstate_in;     // [D][T][B] x 3, [D][3][B], [D][B]; NULL: zeros
  double *dw, *dpet, *dstore, *devap, *dstate_out;     // dw, dpet [T][B][ld] at k0 + k; dstore, devap [D][T][B] (both or neither)
  double dt_h;
  long long T, B, D, ld, k0;
};

LGAR_CN_FN void cn_walk_tangent(const CnTanArgs &a, long long b, long long k) {
  constexpr int CH = LGAR_CN_CHUNK;
  const long long TB = a.T * a.B;
  double s = a.state_in ? a.state_in[b] : 0.0;
  double ds = a.dstate_in ? a.dstate_in[k * a.B + b] : 0.0;
  if (a.T > 0) {
    const CnPar c = cn_par(a.par, a.B, b);
    const double *dq = a.dpar ? a.dpar + k * LGAR_CN_NPAR * a.B + b : nullptr;
    const double dcmax = dq ? dq[0] : 0.0, dfe = dq ? dq[a.B] : 0.0, dcover = dq ? dq[2 * a.B] : 0.0;
    const double dfc = dfe * c.cover + c.fe * dcover;
    for (long long t0 = 0; t0 < a.T; t0 += CH) {
      double pv[CH], ev[CH], lv[CH], dpv[CH], dev[CH], dlv[CH];
#pragma unroll
      for (int u = 0; u < CH; u++) pv[u] = a.p[cn_row<1>(t0, u, a.T) * a.B + b];
#pragma unroll
      for (int u = 0; u < CH; u++) ev[u] = a.e[cn_row<1>(t0, u, a.T) * a.B + b];
#pragma unroll
      for (int u = 0; u < CH; u++) lv[u] = a.lai ? a.lai[cn_row<1>(t0, u, a.T) * a.B + b] : 1.0;
#pragma unroll
      for (int u = 0; u < CH; u++) dpv[u] = a.dp ? a.dp[k * TB + cn_row<1>(t0, u, a.T) * a.B + b] : 0.0;
#pragma unroll
      for (int u = 0; u < CH; u++) dev[u] = a.de ? a.de[k * TB + cn_row<1>(t0, u, a.T) * a.B + b] : 0.0;
#pragma unroll
      for (int u = 0; u < CH; u++) dlv[u] = a.dlai ? a.dlai[k * TB + cn_row<1>(t0, u, a.T) * a.B + b] : 0.0;
#pragma unroll
      for (int u = 0; u < CH; u++)
        if (t0 + u < a.T) {
          const long long t = t0 + u;
          const double pd = pv[u] * a.dt_h, ed = ev[u] * a.dt_h;
          const double cap = a.lai ? c.cmax * lv[u] : c.cmax;
          const CnRow o = cn_step(s, pd, ed, cap, c);
          const double dpd = dpv[u] * a.dt_h, ded = dev[u] * a.dt_h;
          const double dhit = dcover * pd + c.cover * dpd;
          const double ddirect = dpd - dhit;
          const double dcap = dcmax * lv[u] + c.cmax * dlv[u];
          const double ds1 = ds + dhit;
          const double ddrip = o.full ? ds1 - dcap : 0.0;
          const double ds2 = o.full ? dcap : ds1;
          const double ddem = dfc * ed + c.fc * ded;
          const double dei = o.lim ? ds2 : ddem;
          ds = ds2 - dei;
          const double dr = o.neg ? 0.0 : ded - dei;
          s = o.s;
          const long long at = (t * a.B + b) * a.ld + a.k0 + k;
          a.dw[at] = (ddirect + ddrip) / a.dt_h;
          if (a.dpet) a.dpet[at] = dr / a.dt_h;
          if (a.dstore) {
            a.dstore[k * TB + t * a.B + b] = ds;
            a.devap[k * TB + t * a.B + b] = dei / a.dt_h;
          }
        }
    }
  }
  if (a.dstate_out) a.dstate_out[k * a.B + b] = ds;
}

// ---- what the entry points refuse (host code) -------------------------------------------------------------------------------
inline bool cn_dt_ok(double dt_h) { return dt_h > 0.0 && dt_h <= 1.7976931348623157e308; }  // finite and > 0 (a NaN fails both)

// 0: launch; 1: nothing to do; LGAR_E_ARG
inline int cn_check(const double *p, const double *e, int32_t T, int32_t B, const double *par, double dt_h, const double *state_out,
                    const double *w, const double *pet, const double *store, const double *evap) {
  if (T < 0 || B < 0 || !cn_dt_ok(dt_h)) return LGAR_E_ARG;
  if ((store == nullptr) != (evap == nullptr)) return LGAR_E_ARG;
  if (B == 0) return 1;
  if (T == 0) return state_out ? 0 : 1;
  if (!p || !e || !par || !w || !pet) return LGAR_E_ARG;
  return 0;
}

inline int cn_grad_check(const double *gw, const double *gpet, const double *p, const double *e, const double *store, int32_t T,
                         int32_t B, const double *par, double dt_h, const double *gp, const double *ge, const double *gpar,
                         const double *gstate) {
  if (T < 0 || B < 0 || !cn_dt_ok(dt_h)) return LGAR_E_ARG;
  if (B == 0) return 1;
  if (T == 0) return gpar || gstate ? 0 : 1;
  if (!gw || !gpet || !p || !e || !store || !par || !gp || !ge) return LGAR_E_ARG;
  return 0;
}

inline int cn_tangent_check(const double *p, const double *e, int32_t T, int32_t B, const double *par, double dt_h, int32_t D,
                            const double *dw, int32_t ld, int32_t k0, const double *dstore, const double *devap,
                            const double *dstate_out) {
  if (T < 0 || B < 0 || D < 0 || k0 < 0 || !cn_dt_ok(dt_h)) return LGAR_E_ARG;
  if ((dstore == nullptr) != (devap == nullptr)) return LGAR_E_ARG;
  if ((long long)ld < (long long)k0 + (long long)D) return LGAR_E_ARG;
  if (B == 0 || D == 0) return 1;
  if (T == 0) return dstate_out ? 0 : 1;
  if (!p || !e || !par || !dw) return LGAR_E_ARG;
  return 0;
}

#ifdef LGAR_DEVSIM
// the kernels' work, one lane at a time
inline void cn_all(const CnArgs &a) {
  for (long long b = 0; b < a.B; b++) cn_walk(a, b);
}

inline void cn_grad_all(const CnGradArgs &a) {
  for (long long b = 0; b < a.B; b++) {
    if (a.gpar) cn_walk_back<true>(a, b);
    else cn_walk_back<false>(a, b);
  }
}

inline void cn_tangent_all(const CnTanArgs &a) {
  for (long long k = 0; k < a.D; k++)
    for (long long b = 0; b < a.B; b++) cn_walk_tangent(a, b, k);
}
#endif

}  // namespace lgar
