// lgar_leaf.hpp -- the element-wise leaf dispatcher of the known-answer tests (lgar_leaf_batch, include/lgar.h): one function
// of an item's soil parameters and operands per op number.  The leaf kernel (lgar_kernels.hip) and the tests' host build of
// the device code (tests/leaf_host, -DLGAR_DEVSIM) both call leaf_eval, so what a test pins on the host is what the kernel runs.
// leaf_tangent_eval is the same for the dual numbers of the tangent kernels (lgar_leaf_tangent_batch): value and one tangent.
#pragma once
#include "lgar_dual.hpp"

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
  derive_layer(l.n, l.m, l.inv_m, l.inv_n);
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

// ---------------------------------------------------------------------------------------------
// the tangent leaves (lgar_leaf_tangent_batch, include/lgar.h): the same functions of dual numbers
// ---------------------------------------------------------------------------------------------
constexpr int LEAF_NSEED = 7;  // d_alpha, d_n, d_ksat, d_theta_e, d_theta_r, d_x, d_y
template <typename R> struct LeafTangentArgs {
  int op, pol, share, n, nint;  // share: 0, or the W lanes of a group that carry one item along W directions
  const R *x, *y, *alpha, *nn, *ksat, *te, *tr;
  const R *seed[LEAF_NSEED];  // [n] each ([n][share] with share): a null pointer is a seed of 0
  R z, wp_psi;
  R *value, *tangent;  // [n] ([n][share])
};
constexpr int LEAF_TOP_LAST = 32;
// ops that take the arithmetic policy (POL_LEAN / POL_LIBRARY), ops that read y, the fused trapezoid
__host__ __device__ inline bool leaf_tangent_op_exists(int op) {
  return (op >= 0 && op <= 9) || op == 11 || op == 16 || (op >= 23 && op <= LEAF_TOP_LAST);
}
__host__ __device__ inline bool leaf_tangent_op_needs_y(int op) {
  return op == 4 || op == 5 || op == 6 || op == 9 || op == 11 || op == 23 || (op >= 25 && op <= 28) || op == 31;
}
constexpr int LEAF_TOP_GEFF = 4;

template <typename R, int POL>
__device__ __forceinline__ Dual<R> leaf_tangent_policy_op(const LeafTangentArgs<R> &a, const LayerK<Dual<R>> &l, const Dual<R> &x,
                                                          const Dual<R> &y) {
  using S = Dual<R>;
  switch (a.op) {
    case 0: return theta_from_h<S, POL>(l, x);
    case 1: return se_from_h<S, POL>(l, x);
    case 2: return k_from_se<S, POL>(l, x);
    case 3: return h_from_se<S, POL>(l, x);
    case 5: return aet_fn<S, POL>(l, y, a.z, x, a.wp_psi);
    case 23: return geff_closed<S, POL>(l, x, y);
    default: return se_from_theta(l, x);  // 24
  }
}

// direction `k` (an index into the seed arrays: the item, or item * share + lane of the group) of item i.  xchg, W: the wave's
// exchange buffer and the group width of the shared trapezoid (op 4 in double precision only), as Column::capillary_drive passes them.
template <typename R>
__device__ __forceinline__ Dual<R> leaf_tangent_eval(const LeafTangentArgs<R> &a, int i, int k, R *xchg = nullptr, int W = 0) {
  using S = Dual<R>;
  auto seed = [&](int j) { return a.seed[j] ? a.seed[j][k] : R(0); };
  LayerK<S> l;
  l.alpha = S(a.alpha[i], seed(0));
  l.n = S(a.nn[i], seed(1));
  derive_layer(l.n, l.m, l.inv_m, l.inv_n);
  l.ksat = S(a.ksat[i], seed(2));
  l.te = S(a.te[i], seed(3));
  l.tr = S(a.tr[i], seed(4));
  const S x(a.x[i], seed(5));
  const S y(a.y ? a.y[i] : R(0), seed(6));
  (void)xchg; (void)W;
  switch (a.op) {
    case 4:
      if constexpr (ScalarKind<R>::f64) {
        if (W >= 2) return geff_fused<S>(l, x, y, a.nint, xchg, W);
      }
      return geff(l, x, y, a.nint);
    case 6: return geff_literal<S, POL_LIBRARY>(l, x, y, a.nint);
    case 7: return lg2p(x);
    case 8: return ex2p(x);
    case 9: return pw(x, y);
    case 11: return dv<POL_LEAN>(x, y);
    case 16: return sq(x);
    case 25: return pwx<true>(x, y);
    case 26: return dv<POL_LEAN>(x, y.v);
    case 27: return dv<POL_LEAN>(x.v, y);
    case 28: return x / y;
    case 29: return lg2(x);
    case 30: return ex2(x);
    case 31: return mn(x, y);
    case 32: return ab(x);
    default:
      return a.pol == POL_LIBRARY ? leaf_tangent_policy_op<R, POL_LIBRARY>(a, l, x, y) : leaf_tangent_policy_op<R, POL_LEAN>(a, l, x, y);
  }
}
// the argument checks of lgar_leaf_tangent_batch, shared by the library and the tests' host build (which has no shared trapezoid)
template <bool HOST = false>
inline int leaf_tangent_check(int op, int policy, int share, int n_items, const void *x, const void *y, const void *alpha, const void *n,
                              const void *ksat, const void *theta_e, const void *theta_r, const void *out_value, const void *out_tangent,
                              int dtype) {
  if (!leaf_tangent_op_exists(op) || n_items <= 0 || !x || !alpha || !n || !ksat || !theta_e || !theta_r || !out_value || !out_tangent)
    return LGAR_E_ARG;
  if (dtype != LGAR_F32 && dtype != LGAR_F64) return LGAR_E_ARG;
  if (policy != POL_LEAN && policy != POL_LIBRARY) return LGAR_E_ARG;
  if (leaf_tangent_op_needs_y(op) && !y) return LGAR_E_ARG;
  if (share != 0 && (HOST || share < 2 || share > 32 || dtype != LGAR_F64 || op != LEAF_TOP_GEFF)) return LGAR_E_ARG;
  return 0;
}

}  // namespace lgar
