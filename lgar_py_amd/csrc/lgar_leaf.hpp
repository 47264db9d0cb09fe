// lgar_leaf.hpp -- the element-wise leaf dispatcher of the known-answer tests (lgar_leaf_batch, include/lgar.h): one function
// of an item's soil parameters and operands per op number.  The leaf kernel (lgar_kernels.hip) and the tests' host build of
// the device code (tests/leaf_host, -DLGAR_DEVSIM) both call leaf_eval, so what a test pins on the host is what the kernel runs.
#pragma once
#include "lgar_geff.hpp"

namespace lgar {

template <typename R> struct LeafArgs {
  int op, n, nint;
  const R *x, *y, *alpha, *nn, *ksat, *te, *tr;
  R z, wp_psi;
  R *out;
};

constexpr int LEAF_OP_LAST = 23;      // ops 0 .. 23
constexpr int LEAF_OP_F32_FIRST = 15;  // ops from here on exist for float only (the fp32 fast mode's arithmetic, POL_RCP32)

// item i of a leaf batch.  The layer's derived parameters (m, 1/m, 1/n) are formed here in R, as the engine's set-up forms them.
template <typename R> __device__ __forceinline__ R leaf_eval(const LeafArgs<R> &a, int i) {
  LayerK<R> l;
  l.alpha = a.alpha[i];
  l.n = a.nn[i];
  l.m = R(1.0) - (R(1.0) / l.n);
  l.inv_m = R(1.0) / l.m;
  l.inv_n = R(1.0) / l.n;
  l.ksat = a.ksat[i];
  l.te = a.te[i];
  l.tr = a.tr[i];
  const R x = a.x[i];
  const R y = a.y ? a.y[i] : R(0);
  R r = R(0);
  switch (a.op) {
    case 0: r = theta_from_h(l, x); break;
    case 1: r = se_from_h(l, x); break;
    case 2: r = k_from_se(l, x); break;
    case 3: r = h_from_se(l, x); break;
    case 4: r = geff(l, x, y, a.nint); break;
    case 5: r = aet_fn(l, y, a.z, x, a.wp_psi); break;
    case 6: r = geff_literal<R, ScalarKind<R>::f64 ? POL_LIBRARY : POL_LEAN>(l, x, y, a.nint); break;
    case 7: r = lg2p(x); break;
    case 8: r = ex2p(x); break;
    case 9: r = pw(x, y); break;
    case 10:
      if constexpr (ScalarKind<R>::f64) r = geff_mixed(l.alpha, l.n, l.m, l.inv_m, l.inv_n, l.ksat, l.te, l.tr, x, y, a.nint);
      else r = geff(l, x, y, a.nint);
      break;
    case 11: r = dv<POL_LEAN>(x, y); break;   // the fast modes' quotient (double precision: lean_div)
    case 12: r = pwp<POL_MIXED>(x, y); break;  // the mixed-precision kernels' pow (pairwise-combined polynomials)
    case 13:
      if constexpr (ScalarKind<R>::f64) r = lg2e(x);
      else r = lg2p(x);
      break;
    case 14:
      if constexpr (ScalarKind<R>::f64) r = ex2e(x);
      else r = ex2p(x);
      break;
    default:
      // the fp32 fast mode's own arithmetic (POL_RCP32: a * v_rcp_f32(b), v_log_f32 / v_exp_f32 pow, v_sqrt_f32) and the
      // leaves no other op reaches: the trapezoid from two heads (calc_dzdt's site) and the closed-form Geff
      if constexpr (ScalarKind<R>::plain_f32) {
        switch (a.op) {
          case 15: r = dv<POL_RCP32>(x, y); break;
          case 16: r = sq(x); break;
          case 17: r = theta_from_h<float, POL_RCP32>(l, x); break;
          case 18: r = se_from_h<float, POL_RCP32>(l, x); break;
          case 19: r = k_from_se<float, POL_RCP32>(l, x); break;
          case 20: r = h_from_se<float, POL_RCP32>(l, x); break;
          case 21: r = aet_fn<float, POL_RCP32>(l, y, a.z, x, a.wp_psi); break;
          case 22: r = geff_f32_from_heads(l, x, y, a.nint); break;
          case 23: r = geff_closed<float, POL_RCP32>(l, x, y); break;
        }
      }
      break;
  }
  return r;
}

}  // namespace lgar
