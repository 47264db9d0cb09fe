// lgar_baseflow.hpp -- catchment baseflow: the exponential storage-discharge groundwater store fed by percolation, its adjoint
// and the gradients with respect to its three parameters and its initial storage (lgar_catchment_baseflow /
// lgar_catchment_baseflow_grad, include/lgar.h has the full statement).
//
// All arrays are fp64, catchment fastest: the recharge r[T][B], the baseflow q[T][B], the storage s[T][B], par[3][B] = cgw, expon,
// smax.  One catchment b, with S = state_in[b] (NULL: +0.0), for t = 0 .. T - 1 (gw_step):
//
//     A  = S + r[t][b]
//     z  = expon * (A / smax)
//     zc = z < 0 ? 0 : (z > LGAR_GW_ZMAX ? LGAR_GW_ZMAX : z)
//     e  = gw_exp(zc)
//     f  = (cgw * dt_h) * (e - 1.0)
//     qq = f > A ? A : f;   qq = qq < 0 ? 0 : qq
//     S  = A - qq;   q[t][b] = qq;   s[t][b] = S
//
// Every decision is a select: a NaN takes the last alternative and stays a NaN, and the wave stays converged.  gw_exp is built
// from operations numpy restates one for one -- no libm, no fma (-ffp-contract=off), no hardware reciprocal.
//
// A catchment is one lane's work: it walks all rows (gw_walk), in chunks of LGAR_GW_CHUNK rows whose loads are all issued before
// the first of them is used (a chunk that reaches past the rows re-reads its last row: every load stays inside the arrays).  The
// recurrence is serial, so the bits are the definition's whatever the chunk is.  The adjoint (gw_walk_back) walks the rows
// downward; it re-forms A of row t as s[t - 1][b] + r[t][b] (row 0: state_in) and takes zc, e, f and the regime of the row from
// gw_step, the forward's own function: the same bits.  Offsets are 64-bit.
//
// Like lgar_network.hpp this header also compiles for the host with -DLGAR_DEVSIM: tests/baseflow_host runs the same text
// against the numpy statement of the definition.
#pragma once
#ifndef LGAR_DEVSIM
#include <hip/hip_runtime.h>
#define LGAR_GW_FN __device__ __forceinline__
#else
#define LGAR_GW_FN inline
#endif
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/lgar.h"

namespace lgar {

#define LGAR_GW_CHUNK 8  // rows of a catchment whose loads are in flight together (as LGAR_NET_CHUNK)

// One forward call.  par: [3][B] = cgw, expon, smax.  state_in / state_out: [B] (NULL: zeros / not wanted).  s: NULL = not wanted.
struct GwArgs {
  const double *r, *par, *state_in;
  double *q, *s, *state_out;
  double dt_h;
  long long T, B;
};

// One adjoint call.  gs == NULL: zeros.  gpar ([3][B]) / gstate ([B]) == NULL: not wanted.
struct GwGradArgs {
  const double *gq, *gs, *r, *s, *par, *state_in;
  double *gr, *gpar, *gstate;
  double dt_h;
  long long T, B;
};

// exp(zc) for 0 <= zc <= LGAR_GW_ZMAX:
//     k = rint(zc LOG2E)                        as (zc LOG2E + 1.5 2^52) - 1.5 2^52: two rounded adds, ties to even
//     r = (zc - k LN2_HI) - k LN2_LO            LN2_HI has 32 trailing zero bits: k LN2_HI is exact for k <= 58
//     p = sum_{j <= 13} r^j / j!                Horner: p = p * r + c_j, one rounded multiply and one rounded add per step
//     e = p 2^k                                 exact: 2^k is put together from its exponent bits
// The coefficients are the correctly rounded 1 / j!.  A NaN gives a NaN (k counts as 0 for the scaling).
LGAR_GW_FN double gw_exp(double zc) {
  const double LOG2E = 0x1.71547652b82fep+0, LN2_HI = 0x1.62e42fee00000p-1, LN2_LO = 0x1.a39ef35793c76p-33;
  const double MAGIC = 6755399441055744.0;  // 1.5 2^52
  const double k = (zc * LOG2E + MAGIC) - MAGIC;
  const double r = (zc - k * LN2_HI) - k * LN2_LO;
  double p = 0x1.6124613a86d09p-33;  // 1 / 13!
  p = p * r + 0x1.1eed8eff8d898p-29;  // 1 / 12!
  p = p * r + 0x1.ae64567f544e4p-26;  // 1 / 11!
  p = p * r + 0x1.27e4fb7789f5cp-22;  // 1 / 10!
  p = p * r + 0x1.71de3a556c734p-19;  // 1 / 9!
  p = p * r + 0x1.a01a01a01a01ap-16;  // 1 / 8!
  p = p * r + 0x1.a01a01a01a01ap-13;  // 1 / 7!
  p = p * r + 0x1.6c16c16c16c17p-10;  // 1 / 6!
  p = p * r + 0x1.1111111111111p-7;   // 1 / 5!
  p = p * r + 0x1.5555555555555p-5;   // 1 / 4!
  p = p * r + 0x1.5555555555555p-3;   // 1 / 3!
  p = p * r + 0.5;
  p = p * r + 1.0;
  p = p * r + 1.0;
  const int32_t ki = (k >= 0.0 && k <= 58.0) ? (int32_t)k : 0;  // (a NaN, or an argument outside the domain: no scaling)
  const uint64_t bits = (uint64_t)(uint32_t)(1023 + ki) << 52;
  double scale;
  memcpy(&scale, &bits, sizeof scale);
  return p * scale;
}

// One row of the recurrence from A = S + r[t][b]; cd = cgw * dt_h (one rounded multiply, once per catchment).
struct GwRow {
  double z, zc, e, f, qq, S;
};

LGAR_GW_FN GwRow gw_step(double A, double cd, double expon, double smax) {
  GwRow o;
  o.z = expon * (A / smax);
  o.zc = o.z < 0.0 ? 0.0 : (o.z > LGAR_GW_ZMAX ? LGAR_GW_ZMAX : o.z);
  o.e = gw_exp(o.zc);
  o.f = cd * (o.e - 1.0);
  const double pre = o.f > A ? A : o.f;
  o.qq = pre < 0.0 ? 0.0 : pre;
  o.S = A - o.qq;
  return o;
}

// row u of a chunk that starts at t0 and runs upward (DIR = +1) or downward (DIR = -1), kept inside 0 .. T - 1
template <int DIR> LGAR_GW_FN long long gw_row(long long t0, int u, long long T) {
  return DIR > 0 ? (t0 + u < T ? t0 + u : T - 1) : (t0 - u > 0 ? t0 - u : 0);
}

// The forward walk of catchment b over all rows.
LGAR_GW_FN void gw_walk(const GwArgs &a, long long b) {
  constexpr int CH = LGAR_GW_CHUNK;
  double S = a.state_in ? a.state_in[b] : 0.0;
  if (a.T > 0) {
    const double cd = a.par[b] * a.dt_h, expon = a.par[a.B + b], smax = a.par[2 * a.B + b];
    for (long long t0 = 0; t0 < a.T; t0 += CH) {
      double rv[CH];
#pragma unroll
      for (int u = 0; u < CH; u++) rv[u] = a.r[gw_row<1>(t0, u, a.T) * a.B + b];
#pragma unroll
      for (int u = 0; u < CH; u++)
        if (t0 + u < a.T) {
          const GwRow o = gw_step(S + rv[u], cd, expon, smax);
          a.q[(t0 + u) * a.B + b] = o.qq;
          if (a.s) a.s[(t0 + u) * a.B + b] = o.S;
          S = o.S;
        }
    }
  }
  if (a.state_out) a.state_out[b] = S;
}

// The adjoint walk of catchment b, rows T - 1 down to 0, lam = +0.0:
//     lam = lam + gs[t][b];   w = gq[t][b] - lam;   ce = (cgw dt_h) e
//     zero    (the forward clamped qq to 0):   dA = 0
//     emptied (f > A, qq = A >= 0):            dA = 1
//     flux, z clamped:                         dA = 0;                   gcgw += w (dt_h (e - 1))
//     flux, 0 <= z <= ZMAX:                    dA = ce (expon / smax);   gcgw += w (dt_h (e - 1));
//                                              gexpon += w (ce (A / smax));   gsmax += w (-(ce zc) / smax)
//     gr[t][b] = lam + w dA;   lam = gr[t][b]
// and gstate[b] = lam after row 0.  The regimes are selects on the forward's own values, so a tie (f == A, z == 0, z == ZMAX)
// belongs to the branch the forward's selects send it to.  An accumulator that receives no term in a row is left as it is
// (a select of the accumulator, not an added zero).  GP: the parameter gradient is wanted.
template <bool GP> LGAR_GW_FN void gw_walk_back(const GwGradArgs &a, long long b) {
  constexpr int CH = LGAR_GW_CHUNK;
  double lam = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
  if (a.T > 0) {
    const double cd = a.par[b] * a.dt_h, expon = a.par[a.B + b], smax = a.par[2 * a.B + b];
    const double S0 = a.state_in ? a.state_in[b] : 0.0;
    const double slope = expon / smax;
    for (long long t0 = a.T - 1; t0 >= 0; t0 -= CH) {
      double gqv[CH], gsv[CH], rv[CH], sv[CH];
#pragma unroll
      for (int u = 0; u < CH; u++) gqv[u] = a.gq[gw_row<-1>(t0, u, a.T) * a.B + b];
#pragma unroll
      for (int u = 0; u < CH; u++) gsv[u] = a.gs ? a.gs[gw_row<-1>(t0, u, a.T) * a.B + b] : 0.0;
#pragma unroll
      for (int u = 0; u < CH; u++) rv[u] = a.r[gw_row<-1>(t0, u, a.T) * a.B + b];
#pragma unroll
      for (int u = 0; u < CH; u++) sv[u] = a.s[gw_row<-1>(t0 - 1, u, a.T) * a.B + b];  // s[t - 1]; row 0 takes S0 below
#pragma unroll
      for (int u = 0; u < CH; u++)
        if (t0 - u >= 0) {
          const long long t = t0 - u;
          const double A = (t > 0 ? sv[u] : S0) + rv[u];
          const GwRow o = gw_step(A, cd, expon, smax);
          const bool zero = (o.f > A ? A : o.f) < 0.0;
          const bool emptied = !zero && o.f > A;
          const bool flux = !zero && !(o.f > A);
          const bool inside = flux && !(o.z < 0.0) && !(o.z > LGAR_GW_ZMAX);
          lam = lam + gsv[u];
          const double w = gqv[u] - lam;
          const double ce = cd * o.e;
          const double dA = zero ? 0.0 : (emptied ? 1.0 : (inside ? ce * slope : 0.0));
          if (GP) {
            g0 = flux ? g0 + w * (a.dt_h * (o.e - 1.0)) : g0;
            g1 = inside ? g1 + w * (ce * (A / smax)) : g1;
            g2 = inside ? g2 + w * (-(ce * o.zc) / smax) : g2;
          }
          lam = lam + w * dA;
          a.gr[t * a.B + b] = lam;
        }
    }
  }
  if (GP) {
    a.gpar[b] = g0;
    a.gpar[a.B + b] = g1;
    a.gpar[2 * a.B + b] = g2;
  }
  if (a.gstate) a.gstate[b] = lam;
}

// ---- what the entry points refuse (host code) -------------------------------------------------------------------------------
inline bool gw_dt_ok(double dt_h) { return dt_h > 0.0 && dt_h <= 1.7976931348623157e308; }  // finite and > 0 (a NaN fails both)

// 0: launch; 1: nothing to do; LGAR_E_ARG
inline int gw_check(const double *r, int32_t T, int32_t B, const double *par, double dt_h, double *state_out, double *q) {
  if (T < 0 || B < 0 || !gw_dt_ok(dt_h)) return LGAR_E_ARG;
  if (B == 0) return 1;
  if (T == 0) return state_out ? 0 : 1;
  if (!r || !par || !q) return LGAR_E_ARG;
  return 0;
}

inline int gw_grad_check(const double *gq, const double *r, const double *s, int32_t T, int32_t B, const double *par, double dt_h,
                         double *gr, double *gpar, double *gstate) {
  if (T < 0 || B < 0 || !gw_dt_ok(dt_h)) return LGAR_E_ARG;
  if (B == 0) return 1;
  if (T == 0) return gpar || gstate ? 0 : 1;
  if ((gpar || gstate) && !s) return LGAR_E_ARG;
  if (!gq || !r || !s || !par || !gr) return LGAR_E_ARG;
  return 0;
}

#ifdef LGAR_DEVSIM
// the kernels' work, one lane at a time
inline void gw_all(const GwArgs &a) {
  for (long long b = 0; b < a.B; b++) gw_walk(a, b);
}

inline void gw_grad_all(const GwGradArgs &a) {
  for (long long b = 0; b < a.B; b++) {
    if (a.gpar) gw_walk_back<true>(a, b);
    else gw_walk_back<false>(a, b);
  }
}
#endif

}  // namespace lgar
