// lgar_snow.hpp -- catchment snowpack: the temperature-index store ahead of the columns (ice and held liquid water per forcing
// cell), its adjoint and the gradients with respect to its seven parameters, its forcing and its initial state
// (lgar_catchment_snow / lgar_catchment_snow_grad, include/lgar.h has the full statement).
//
// All arrays are fp64, cell fastest: the precipitation rate p[T][B], the air temperature ta[T][B], the water input rate w[T][B],
// the pack ice[T][B] and liq[T][B], par[7][B] = tlo, thi, tm, sfcf, cfmax, cfr, cwh, the state [2][B] = ice, liq.  One cell b, with
// cd = cfmax * dt_h and cr = cfr * cd (once), span = thi - tlo (once) and (ice, liq) = state_in (NULL: +0.0), for t = 0 .. T - 1
// (sn_step):
//
//     Ta   = ta[t][b];   pd = p[t][b] * dt_h
//     lo   = Ta <= tlo;  hi = !lo && Ta >= thi
//     fr   = lo ? 0.0 : (hi ? 1.0 : (Ta - tlo) / span)
//     rain = pd * fr;    dry = pd - rain;   snow = sfcf * dry
//     d    = Ta - tm;    warm = d > 0
//     ice1 = ice + snow
//     pm   = cd * d;     ml = pm > ice1
//     melt = warm ? (ml ? ice1 : pm) : 0.0
//     pr   = cr * (-d);  rl = pr > liq
//     refr = warm ? 0.0 : (rl ? liq : pr)
//     ice2 = (ice1 - melt) + refr
//     liq1 = ((liq + rain) + melt) - refr
//     cap  = cwh * ice2; over = liq1 > cap
//     out  = over ? liq1 - cap : 0.0
//     liq  = over ? cap : liq1;   ice = ice2
//     w[t][b] = out / dt_h;   ice[t][b] = ice;   liq[t][b] = liq
//
// Every decision is a select: the wave stays converged, and a NaN fails every comparison and so takes the last alternative.  A NaN
// in p or ta therefore stays in ice and liq of its cell from its row on (out's last alternative is the constant 0.0: w of such a
// row is +0.0, the pack carries the NaN).  No libm, no fma (-ffp-contract=off), IEEE divisions.
//
// A cell is one lane's work: it walks all rows (sn_walk), in chunks of LGAR_SN_CHUNK rows whose loads are all issued before the
// first of them is used (a chunk that reaches past the rows re-reads its last row: every load stays inside the arrays).  The
// recurrence is serial, so the bits are the definition's whatever the chunk is.  The adjoint (sn_walk_back) walks the rows downward;
// it re-forms row t from ice[t - 1][b], liq[t - 1][b] (row 0: state_in) through sn_step, the forward's own function: every flag and
// value has the forward's bits.  Offsets are 64-bit.
//
// Like lgar_baseflow.hpp this header also compiles for the host with -DLGAR_DEVSIM: tests/snow_host runs the same text against
// the numpy statement of the definition.
#pragma once
#ifndef LGAR_DEVSIM
#include <hip/hip_runtime.h>
#define LGAR_SN_FN __device__ __forceinline__
#else
#define LGAR_SN_FN inline
#endif
#include <stddef.h>
#include <stdint.h>

#include "../../include/lgar.h"

namespace lgar {

#define LGAR_SN_CHUNK 8  // rows of a cell whose loads are in flight together (as LGAR_GW_CHUNK)
#define LGAR_SN_NPAR 7   // tlo, thi, tm, sfcf, cfmax, cfr, cwh

// One forward call.  par: [7][B].  state_in / state_out: [2][B] (NULL: zeros / not wanted).  ice, liq: both or neither.
struct SnArgs {
  const double *p, *ta, *par, *state_in;
  double *w, *ice, *liq, *state_out;
  double dt_h;
  long long T, B;
};

// One adjoint call.  gice, gliq == NULL: zeros.  gta ([T][B]) / gpar ([7][B]) / gstate ([2][B]) == NULL: not wanted.
struct SnGradArgs {
  const double *gw, *gice, *gliq, *p, *ta, *ice, *liq, *par, *state_in;
  double *gp, *gta, *gpar, *gstate;
  double dt_h;
  long long T, B;
};

// The parameters of one cell as the rows use them: cd = cfmax * dt_h, cr = cfr * cd, span = thi - tlo (one rounding each, once).
struct SnPar {
  double tlo, thi, tm, sfcf, cfr, cwh, cd, cr, span;
};

LGAR_SN_FN SnPar sn_par(const double *par, long long B, long long b, double dt_h) {
  SnPar c;
  c.tlo = par[b], c.thi = par[B + b], c.tm = par[2 * B + b], c.sfcf = par[3 * B + b];
  c.cfr = par[5 * B + b], c.cwh = par[6 * B + b];
  c.cd = par[4 * B + b] * dt_h;
  c.cr = c.cfr * c.cd;
  c.span = c.thi - c.tlo;
  return c;
}

// One row of the recurrence from the pack before it (ice, liq), pd = p[t][b] * dt_h and Ta.
struct SnRow {
  double fr, dry, d, ice2, out, ice, liq;
  bool lo, hi, warm, ml, rl, over;
};

LGAR_SN_FN SnRow sn_step(double ice, double liq, double pd, double Ta, const SnPar &c) {
  SnRow o;
  o.lo = Ta <= c.tlo;
  o.hi = !o.lo && Ta >= c.thi;
  const double ramp = (Ta - c.tlo) / c.span;  // formed for every lane (a ?: around the division would be a branch), then selected
  o.fr = o.lo ? 0.0 : (o.hi ? 1.0 : ramp);
  const double rain = pd * o.fr;
  o.dry = pd - rain;
  const double snow = c.sfcf * o.dry;
  o.d = Ta - c.tm;
  o.warm = o.d > 0.0;
  const double ice1 = ice + snow;
  const double pm = c.cd * o.d;
  o.ml = pm > ice1;
  const double melt = o.warm ? (o.ml ? ice1 : pm) : 0.0;
  const double pr = c.cr * (-o.d);
  o.rl = pr > liq;
  const double refr = o.warm ? 0.0 : (o.rl ? liq : pr);
  o.ice2 = (ice1 - melt) + refr;
  const double liq1 = ((liq + rain) + melt) - refr;
  const double cap = c.cwh * o.ice2;
  o.over = liq1 > cap;
  o.out = o.over ? liq1 - cap : 0.0;
  o.liq = o.over ? cap : liq1;
  o.ice = o.ice2;
  return o;
}

// row u of a chunk that starts at t0 and runs upward (DIR = +1) or downward (DIR = -1), kept inside 0 .. T - 1
template <int DIR> LGAR_SN_FN long long sn_row(long long t0, int u, long long T) {
  return DIR > 0 ? (t0 + u < T ? t0 + u : T - 1) : (t0 - u > 0 ? t0 - u : 0);
}

// The forward walk of cell b over all rows.
LGAR_SN_FN void sn_walk(const SnArgs &a, long long b) {
  constexpr int CH = LGAR_SN_CHUNK;
  double ice = a.state_in ? a.state_in[b] : 0.0, liq = a.state_in ? a.state_in[a.B + b] : 0.0;
  if (a.T > 0) {
    const SnPar c = sn_par(a.par, a.B, b, a.dt_h);
    for (long long t0 = 0; t0 < a.T; t0 += CH) {
      double pv[CH], tv[CH];
#pragma unroll
      for (int u = 0; u < CH; u++) pv[u] = a.p[sn_row<1>(t0, u, a.T) * a.B + b];
#pragma unroll
      for (int u = 0; u < CH; u++) tv[u] = a.ta[sn_row<1>(t0, u, a.T) * a.B + b];
#pragma unroll
      for (int u = 0; u < CH; u++)
        if (t0 + u < a.T) {
          const SnRow o = sn_step(ice, liq, pv[u] * a.dt_h, tv[u], c);
          a.w[(t0 + u) * a.B + b] = o.out / a.dt_h;
          if (a.ice) {
            a.ice[(t0 + u) * a.B + b] = o.ice;
            a.liq[(t0 + u) * a.B + b] = o.liq;
          }
          ice = o.ice, liq = o.liq;
        }
    }
  }
  if (a.state_out) {
    a.state_out[b] = ice;
    a.state_out[a.B + b] = liq;
  }
}

// The adjoint walk of cell b, rows T - 1 down to 0, with li = ll = +0.0 (the adjoints of ice and liq behind the row) and the
// accumulators gtlo, gthi, gtm, gsfcf, gcd, gcr, gcwh from +0.0; o = sn_step of the row (the forward's bits), mid = !lo && !hi:
//     li   = li + gice[t][b];   ll = ll + gliq[t][b];   go = gw[t][b] / dt_h
//     dl1  = over ? go : ll;    dcap = over ? ll - go : 0.0
//     di2  = li + cwh * dcap;   gcwh = over ? gcwh + dcap * ice2 : gcwh
//     dmelt = dl1 - di2;        drefr = di2 - dl1
//     wm = warm && ml;  wf = warm && !ml;  cl = !warm && rl;  cf = !warm && !rl
//     di1  = wm ? di2 + dmelt : di2;      dliq = cl ? dl1 + drefr : dl1
//     gcd  = wf ? gcd + dmelt * d : gcd;  gcr  = cf ? gcr + drefr * (-d) : gcr
//     gd   = wf ? dmelt * cd : (cf ? -(drefr * cr) : 0.0)
//     gtm  = wf || cf ? gtm - gd : gtm
//     gsfcf = gsfcf + di1 * dry
//     sd   = sfcf * di1;   drain = dl1 - sd;   dpd = sd + drain * fr;   dfr = drain * pd
//     gTa  = mid ? gd + dfr / span : gd
//     gtlo = mid ? gtlo + (dfr * (Ta - thi)) / (span * span) : gtlo
//     gthi = mid ? gthi - (dfr * (Ta - tlo)) / (span * span) : gthi
//     gp[t][b] = dpd * dt_h;   gta[t][b] = gTa;   li = di1;   ll = dliq
// and after row 0: gcfmax = dt_h * (gcd + cfr * gcr), gcfr = cd * gcr, gstate = (li, ll).  The regimes are selects on the forward's
// own values, so a tie belongs to the branch the forward's selects send it to.  An accumulator that receives no term in a row is
// left as it is (a select of the accumulator, not an added zero); a quotient by span is formed only inside a select that discards
// it outside mid.  GP: the parameter gradient is wanted.
template <bool GP> LGAR_SN_FN void sn_walk_back(const SnGradArgs &a, long long b) {
  constexpr int CH = LGAR_SN_CHUNK;
  double li = 0.0, ll = 0.0;
  double gtlo = 0.0, gthi = 0.0, gtm = 0.0, gsfcf = 0.0, gcd = 0.0, gcr = 0.0, gcwh = 0.0, gcfmax = 0.0, gcfr = 0.0;
  if (a.T > 0) {
    const SnPar c = sn_par(a.par, a.B, b, a.dt_h);
    const double ice0 = a.state_in ? a.state_in[b] : 0.0, liq0 = a.state_in ? a.state_in[a.B + b] : 0.0;
    const double span2 = c.span * c.span;
    for (long long t0 = a.T - 1; t0 >= 0; t0 -= CH) {
      double gwv[CH], giv[CH], glv[CH], pv[CH], tv[CH], iv[CH], lv[CH];
#pragma unroll
      for (int u = 0; u < CH; u++) gwv[u] = a.gw[sn_row<-1>(t0, u, a.T) * a.B + b];
#pragma unroll
      for (int u = 0; u < CH; u++) giv[u] = a.gice ? a.gice[sn_row<-1>(t0, u, a.T) * a.B + b] : 0.0;
#pragma unroll
      for (int u = 0; u < CH; u++) glv[u] = a.gliq ? a.gliq[sn_row<-1>(t0, u, a.T) * a.B + b] : 0.0;
#pragma unroll
      for (int u = 0; u < CH; u++) pv[u] = a.p[sn_row<-1>(t0, u, a.T) * a.B + b];
#pragma unroll
      for (int u = 0; u < CH; u++) tv[u] = a.ta[sn_row<-1>(t0, u, a.T) * a.B + b];
#pragma unroll
      for (int u = 0; u < CH; u++) iv[u] = a.ice[sn_row<-1>(t0 - 1, u, a.T) * a.B + b];  // ice[t - 1]; row 0 takes ice0 below
#pragma unroll
      for (int u = 0; u < CH; u++) lv[u] = a.liq[sn_row<-1>(t0 - 1, u, a.T) * a.B + b];
#pragma unroll
      for (int u = 0; u < CH; u++)
        if (t0 - u >= 0) {
          const long long t = t0 - u;
          const double Ta = tv[u], pd = pv[u] * a.dt_h;
          const SnRow o = sn_step(t > 0 ? iv[u] : ice0, t > 0 ? lv[u] : liq0, pd, Ta, c);
          const bool mid = !o.lo && !o.hi;
          const bool wm = o.warm && o.ml, wf = o.warm && !o.ml, cl = !o.warm && o.rl, cf = !o.warm && !o.rl;
          li = li + giv[u];
          ll = ll + glv[u];
          const double go = gwv[u] / a.dt_h;
          const double dl1 = o.over ? go : ll;
          const double dcap = o.over ? ll - go : 0.0;
          const double di2 = li + c.cwh * dcap;
          const double dmelt = dl1 - di2, drefr = di2 - dl1;
          const double di1 = wm ? di2 + dmelt : di2;
          const double dliq = cl ? dl1 + drefr : dl1;
          const double gd = wf ? dmelt * c.cd : (cf ? -(drefr * c.cr) : 0.0);
          const double sd = c.sfcf * di1;
          const double drain = dl1 - sd;
          const double dpd = sd + drain * o.fr;
          const double dfr = drain * pd;
          // the quotients by span are formed for every lane and discarded by the selects outside mid (a ?: around a division would
          // be a branch: the lanes of a wave stay together)
          const double qta = dfr / c.span;
          if (GP) {
            const double qlo = (dfr * (Ta - c.thi)) / span2, qhi = (dfr * (Ta - c.tlo)) / span2;
            gcwh = o.over ? gcwh + dcap * o.ice2 : gcwh;
            gcd = wf ? gcd + dmelt * o.d : gcd;
            gcr = cf ? gcr + drefr * (-o.d) : gcr;
            gtm = (wf || cf) ? gtm - gd : gtm;
            gsfcf = gsfcf + di1 * o.dry;
            gtlo = mid ? gtlo + qlo : gtlo;
            gthi = mid ? gthi - qhi : gthi;
          }
          a.gp[t * a.B + b] = dpd * a.dt_h;
          if (a.gta) a.gta[t * a.B + b] = mid ? gd + qta : gd;
          li = di1, ll = dliq;
        }
    }
    if (GP) {
      gcfmax = a.dt_h * (gcd + c.cfr * gcr);
      gcfr = c.cd * gcr;
    }
  }
  if (GP) {
    a.gpar[b] = gtlo;
    a.gpar[a.B + b] = gthi;
    a.gpar[2 * a.B + b] = gtm;
    a.gpar[3 * a.B + b] = gsfcf;
    a.gpar[4 * a.B + b] = gcfmax;
    a.gpar[5 * a.B + b] = gcfr;
    a.gpar[6 * a.B + b] = gcwh;
  }
  if (a.gstate) {
    a.gstate[b] = li;
    a.gstate[a.B + b] = ll;
  }
}

// ---- the forward-mode tangent (lgar_catchment_snow_tangent) ----------------------------------------------
// One lane per (cell b, direction k), k < D: lane i = k * B + b, cell fastest, so the loads of dp / dta [D][T][B] and of the values
// are coalesced.  The VALUE recurrence of the lane is sn_step itself from state_in (every flag has the forward's bits); beside it
// run ice', liq' from dstate_in (NULL: +0.0).  Once per lane, with tlo' .. cwh' = dpar[k][0..6][b] (NULL: 0):
//     cd' = cfmax' * dt_h;   cr' = cfr' * cd + cfr * cd';   span' = thi' - tlo'
// and per row, selects on the forward's flags with the adjoint's tie conventions (mid = !lo && !hi):
//     pd'   = dp * dt_h
//     fr'   = mid ? ((Ta' - tlo') - fr * span') / span : 0.0        (the quotient formed for every lane, then selected)
//     rain' = pd' * fr + pd * fr';   dry' = pd' - rain';   snow' = sfcf' * dry + sfcf * dry'
//     d'    = Ta' - tm';             ice1' = ice' + snow'
//     pm'   = cd' * d + cd * d';     melt' = warm ? (ml ? ice1' : pm') : 0.0
//     pr'   = cr' * (-d) - cr * d';  refr' = warm ? 0.0 : (rl ? liq' : pr')
//     ice2' = (ice1' - melt') + refr';   liq1' = ((liq' + rain') + melt') - refr'
//     cap'  = cwh' * ice2 + cwh * ice2'; out' = over ? liq1' - cap' : 0.0
//     liq'  = over ? cap' : liq1';       ice' = ice2'
//     dw[(t * B + b) * ld + k0 + k] = out' / dt_h;   dice[k][t][b] = ice';   dliq[k][t][b] = liq'
// ld >= k0 + D: the lane writes straight into the [T][B][G] block of forcing tangents lgar_forward_tangent_forced reads.  T = 0
// copies dstate.  Rows in chunks of LGAR_SN_CHUNK as the forward walk; no fma, IEEE divisions.
struct SnTanArgs {
  const double *p, *ta, *par, *state_in;      // the forward's inputs
  const double *dp, *dta, *dpar, *dstate_in;  // [D][T][B], [D][T][B], [D][7][B], [D][2][B]; NULL: zeros
  double *dw, *dice, *dliq, *dstate_out;      // dw [T][B][ld] at k0 + k; dice, dliq [D][T][B] (both or neither); dstate_out [D][2][B]
  double dt_h;
  long long T, B, D, ld, k0;
};

LGAR_SN_FN void sn_walk_tangent(const SnTanArgs &a, long long b, long long k) {
  constexpr int CH = LGAR_SN_CHUNK;
  const long long TB = a.T * a.B;
  double ice = a.state_in ? a.state_in[b] : 0.0, liq = a.state_in ? a.state_in[a.B + b] : 0.0;
  double dice = a.dstate_in ? a.dstate_in[(k * 2 + 0) * a.B + b] : 0.0, dliq = a.dstate_in ? a.dstate_in[(k * 2 + 1) * a.B + b] : 0.0;
  if (a.T > 0) {
    const SnPar c = sn_par(a.par, a.B, b, a.dt_h);
    const double *dq = a.dpar ? a.dpar + k * LGAR_SN_NPAR * a.B + b : nullptr;
    const double dtlo = dq ? dq[0] : 0.0, dthi = dq ? dq[a.B] : 0.0, dtm = dq ? dq[2 * a.B] : 0.0, dsfcf = dq ? dq[3 * a.B] : 0.0;
    const double dcfmax = dq ? dq[4 * a.B] : 0.0, dcfr = dq ? dq[5 * a.B] : 0.0, dcwh = dq ? dq[6 * a.B] : 0.0;
    const double dcd = dcfmax * a.dt_h;
    const double dcr = dcfr * c.cd + c.cfr * dcd;
    const double dspan = dthi - dtlo;
    for (long long t0 = 0; t0 < a.T; t0 += CH) {
      double pv[CH], tv[CH], dpv[CH], dtv[CH];
#pragma unroll
      for (int u = 0; u < CH; u++) pv[u] = a.p[sn_row<1>(t0, u, a.T) * a.B + b];
#pragma unroll
      for (int u = 0; u < CH; u++) tv[u] = a.ta[sn_row<1>(t0, u, a.T) * a.B + b];
#pragma unroll
      for (int u = 0; u < CH; u++) dpv[u] = a.dp ? a.dp[k * TB + sn_row<1>(t0, u, a.T) * a.B + b] : 0.0;
#pragma unroll
      for (int u = 0; u < CH; u++) dtv[u] = a.dta ? a.dta[k * TB + sn_row<1>(t0, u, a.T) * a.B + b] : 0.0;
#pragma unroll
      for (int u = 0; u < CH; u++)
        if (t0 + u < a.T) {
          const long long t = t0 + u;
          const double pd = pv[u] * a.dt_h;
          const SnRow o = sn_step(ice, liq, pd, tv[u], c);
          const bool mid = !o.lo && !o.hi;
          const double dpd = dpv[u] * a.dt_h;
          const double q = ((dtv[u] - dtlo) - o.fr * dspan) / c.span;  // formed for every lane, then selected
          const double dfr = mid ? q : 0.0;
          const double drain = dpd * o.fr + pd * dfr;
          const double ddry = dpd - drain;
          const double dsnow = dsfcf * o.dry + c.sfcf * ddry;
          const double dd = dtv[u] - dtm;
          const double dice1 = dice + dsnow;
          const double dpm = dcd * o.d + c.cd * dd;
          const double dmelt = o.warm ? (o.ml ? dice1 : dpm) : 0.0;
          const double dpr = dcr * (-o.d) - c.cr * dd;
          const double drefr = o.warm ? 0.0 : (o.rl ? dliq : dpr);
          const double dice2 = (dice1 - dmelt) + drefr;
          const double dliq1 = ((dliq + drain) + dmelt) - drefr;
          const double dcap = dcwh * o.ice2 + c.cwh * dice2;
          const double dout = o.over ? dliq1 - dcap : 0.0;
          dliq = o.over ? dcap : dliq1;
          dice = dice2;
          ice = o.ice, liq = o.liq;
          a.dw[(t * a.B + b) * a.ld + a.k0 + k] = dout / a.dt_h;
          if (a.dice) {
            a.dice[k * TB + t * a.B + b] = dice;
            a.dliq[k * TB + t * a.B + b] = dliq;
          }
        }
    }
  }
  if (a.dstate_out) {
    a.dstate_out[(k * 2 + 0) * a.B + b] = dice;
    a.dstate_out[(k * 2 + 1) * a.B + b] = dliq;
  }
}

// 0: launch; 1: nothing to do; LGAR_E_ARG
inline int sn_tangent_check(const double *p, const double *ta, int32_t T, int32_t B, const double *par, double dt_h, int32_t D,
                            const double *dw, int32_t ld, int32_t k0, const double *dice, const double *dliq, const double *dstate_out) {
  if (T < 0 || B < 0 || D < 0 || k0 < 0 || !(dt_h > 0.0 && dt_h <= 1.7976931348623157e308)) return LGAR_E_ARG;
  if ((dice == nullptr) != (dliq == nullptr)) return LGAR_E_ARG;
  if ((long long)ld < (long long)k0 + (long long)D) return LGAR_E_ARG;
  if (B == 0 || D == 0) return 1;
  if (T == 0) return dstate_out ? 0 : 1;
  if (!p || !ta || !par || !dw) return LGAR_E_ARG;
  return 0;
}

#ifdef LGAR_DEVSIM
inline void sn_tangent_all(const SnTanArgs &a) {
  for (long long k = 0; k < a.D; k++)
    for (long long b = 0; b < a.B; b++) sn_walk_tangent(a, b, k);
}
#endif

// ---- what the entry points refuse (host code) -------------------------------------------------------------------------------
inline bool sn_dt_ok(double dt_h) { return dt_h > 0.0 && dt_h <= 1.7976931348623157e308; }  // finite and > 0 (a NaN fails both)

// 0: launch; 1: nothing to do; LGAR_E_ARG
inline int sn_check(const double *p, const double *ta, int32_t T, int32_t B, const double *par, double dt_h, double *state_out,
                    double *w, double *ice, double *liq) {
  if (T < 0 || B < 0 || !sn_dt_ok(dt_h)) return LGAR_E_ARG;
  if ((ice == nullptr) != (liq == nullptr)) return LGAR_E_ARG;
  if (B == 0) return 1;
  if (T == 0) return state_out ? 0 : 1;
  if (!p || !ta || !par || !w) return LGAR_E_ARG;
  return 0;
}

inline int sn_grad_check(const double *gw, const double *p, const double *ta, const double *ice, const double *liq, int32_t T,
                         int32_t B, const double *par, double dt_h, double *gp, double *gpar, double *gstate) {
  if (T < 0 || B < 0 || !sn_dt_ok(dt_h)) return LGAR_E_ARG;
  if ((ice == nullptr) != (liq == nullptr)) return LGAR_E_ARG;
  if (B == 0) return 1;
  if (T == 0) return gpar || gstate ? 0 : 1;
  if (!ice || !gw || !p || !ta || !par || !gp) return LGAR_E_ARG;
  return 0;
}

#ifdef LGAR_DEVSIM
// the kernels' work, one lane at a time
inline void sn_all(const SnArgs &a) {
  for (long long b = 0; b < a.B; b++) sn_walk(a, b);
}

inline void sn_grad_all(const SnGradArgs &a) {
  for (long long b = 0; b < a.B; b++) {
    if (a.gpar) sn_walk_back<true>(a, b);
    else sn_walk_back<false>(a, b);
  }
}
#endif

}  // namespace lgar
