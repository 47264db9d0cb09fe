// lgar_vg.hpp -- van Genuchten leaf functions, the reference's trapezoid (geff_literal), the generic Geff and its fused node,
// the closed-form Geff and the AET closures: functions of one layer's parameters, templated on the scalar type.
#pragma once
#include "lgar_scalar.hpp"

namespace lgar {

// ---------------------------------------------------------------------------------------------
// van Genuchten leaf functions (models/physics/utils.py)
// ---------------------------------------------------------------------------------------------
// calc_theta_from_h, utils.py:35-51
template <typename S, int POL = POL_LEAN> __device__ __forceinline__ S theta_from_h(const LayerK<S> &l, S h) {
  using R = real_t<S>;
  S ap = pwq<S, POL>(l.alpha * h, l.n);
  S op = pwq<S, POL>(R(1.0) + ap, l.m);
  return (dv<POL>(S(R(1.0)), op) * (l.te - l.tr)) + l.tr;
}
// ... also handing out (alpha h)^n, the quantity that says how close to saturation the head is
template <typename S, int POL = POL_LEAN> __device__ __forceinline__ S theta_from_h_ap(const LayerK<S> &l, S h, S &ap) {
  using R = real_t<S>;
  ap = pwq<S, POL>(l.alpha * h, l.n);
  S op = pwq<S, POL>(R(1.0) + ap, l.m);
  return (dv<POL>(S(R(1.0)), op) * (l.te - l.tr)) + l.tr;
}
// calc_se_from_theta, utils.py:102-112
template <typename S> __device__ __forceinline__ S se_from_theta(const LayerK<S> &l, S theta) {
  return (theta - l.tr) / (l.te - l.tr);
}

// calc_se_from_h, utils.py:115-131 (exactly 1 for |h| < 0.1)
template <typename S, int POL = POL_LEAN> __device__ __forceinline__ S se_from_h(const LayerK<S> &l, S h) {
  using R = real_t<S>;
  if (ab(val(h)) < R(1.0e-01)) return S(R(1.0));
  S is = pwq<S, POL>(l.alpha * h, l.n);
  return dv<POL>(S(R(1.0)), pwq<S, POL>(R(1.0) + is, l.m));
}
// calc_k_from_se, utils.py:134-156; torch.isclose(base, 0, rtol=1e-12) => |base| <= 1e-8 (default atol)
template <typename S, int POL = POL_LEAN> __device__ __forceinline__ S k_from_se(const LayerK<S> &l, S se) {
  using R = real_t<S>;
  S sp = pwq<S, POL>(se, l.inv_m);
  S base = R(1.0) - sp;
  if (ab(val(base)) <= R(1e-8)) base = base + R(1e-12);
  S op = pwq<S, POL>(base, l.m);
  S t = R(1.0) - op;
  return l.ksat * sq(se) * (t * t);
}
// ... at Se == 1 (the trapezoid's K under the |h| < 0.1 rule): Se^(1/m) is exactly 1, the base exactly 0 and nudged to 1e-12 --
// calc_k_from_se's value and tangent, bit for bit, without the first pow
template <typename S, int POL = POL_LEAN> __device__ __forceinline__ S k_from_se_one(const LayerK<S> &l) {
  using R = real_t<S>;
  S op = pwq<S, POL>(S(R(1e-12)), l.m);
  S t = R(1.0) - op;
  return l.ksat * sq(S(R(1.0))) * (t * t);
}
// calc_h_from_se, utils.py:159-174
template <typename S, int POL = POL_LEAN> __device__ __forceinline__ S h_from_se(const LayerK<S> &l, S se) {
  using R = real_t<S>;
  S sp = pwq<S, POL>(se, -l.inv_m);
  S base = sp - R(1.0);
  if (ab(val(base)) <= R(1e-8)) base = base + R(1e-12);
  S op = pwq<S, POL>(base, l.inv_n);
  return dv<POL>(S(R(1.0)), l.alpha) * op;
}
// calc_geff, models/physics/lgar/green_ampt.py:45-84: nint-interval trapezoid of K(h) dh / Ksat.
// The discretisation error is part of the answer: same nodes (h accumulated by repeated += dh).
template <typename S, int POL = POL_LEAN> __device__ __forceinline__ S geff_literal(const LayerK<S> &l, S theta1, S theta2, int nint) {
  using R = real_t<S>;
  S se_i = se_from_theta(l, theta1);
  S se_f = se_from_theta(l, theta2);
  S h_i = h_from_se<S, POL>(l, se_i);
  S h_f = h_from_se<S, POL>(l, se_f);
  S dh = (h_f - h_i) / R(nint);
  S g = S(R(0.0));
  S k1 = k_from_se<S, POL>(l, se_i);
  S h2 = h_i + dh;
  S hdh = dh / R(2.0);
  for (int i = 0; i < nint; i++) {
    // rounding in the repeated h2 += dh can carry the last nodes past 0 (by ~1e-10 in fp64): a negative head is
    // saturation (Se = 1, the |h| < 0.1 rule), never pow of a negative base
    S se2 = (val(h2) < R(0.0)) ? S(R(1.0)) : se_from_h<S, POL>(l, h2);
    S k2 = k_from_se<S, POL>(l, se2);
    g = g + ((k1 + k2) * hdh);
    k1 = k2;
    h2 = h2 + dh;
  }
  return ab(g / l.ksat);
}
// the trapezoid the kernels use by default: specialised below for float / double (and the dual numbers, lgar_dual.hpp)
template <typename S> __device__ __forceinline__ S geff(const LayerK<S> &l, S theta1, S theta2, int nint) {
  return geff_literal<S, POL_LEAN>(l, theta1, theta2, nint);
}

// Fused Geff (fp64, and the dual numbers of the differentiable path): the same 121 nodes with Se(h) -> K(Se) fused per
// node.  With x = alpha h, a = x^n and n m = n - 1:
//   P = x^(n-1) = a^m,  a = x P,  sqrt(Se) = (1+a)^(-m/2),  (a/(1+a))^m = P Se
// so K = Ksat sqrt(Se) (1 - P Se)^2 needs 2 log2 + 2 exp2 and no division, instead of the reference's 4 pow + sqrt +
// divide.  (The 1e-12 nudge of calc_k_from_se applies only for a <= 1e-8, i.e. |h| far below the 0.1 cm cut where Se is 1
// anyway.)  fp64 keeps the reference's running sum h2 += dh; a float instantiation would place the nodes directly
// (h_i + (i+1) dh, last node = h_f): its running sum drifts by ~nint ulps of h_i, cm-scale for very dry soil, and the last
// trapezoid dominates the integral.  The plain-float kernels use the packed loop further down instead.
// K(h) of one trapezoid node, fused (see above); nm1 = n - 1, half_m = -m/2.  lgar_dual.hpp overloads it for dual numbers
// (same value operations, hand-derived tangent).
template <typename S> __device__ __forceinline__ S geff_node(const LayerK<S> &l, const S &nm1, const S &half_m, const S &h) {
  using R = real_t<S>;
  const S x = l.alpha * h;
  const S P = ex2p(nm1 * lg2p(x));
  const S l1 = lg2p(R(1.0) + x * P);
  const S sqrt_se = ex2p(half_m * l1);
  const S t = R(1.0) - P * (sqrt_se * sqrt_se);
  return l.ksat * sqrt_se * (t * t);
}
// `nb` blocks of W consecutive safe nodes of the trapezoid (h2, g, k1 advanced as W nb passes of the plain loop would).
// lgar_dual.hpp overloads it for dual numbers whose W neighbouring lanes carry the SAME column with different parameter
// directions: each lane evaluates one node of a block and the W exchange the values.
template <typename S>
__device__ __forceinline__ void geff_shared_blocks(const LayerK<S> &l, const S &nm1, const S &half_m, S &h2, const S &dh, const S &hdh, S &g,
                                                   S &k1, int nb, int W, real_t<S> *xchg, int rem) {
  (void)xchg;
  for (int j = 0; j < W * nb + rem; j++) {
    const S k2 = geff_node(l, nm1, half_m, h2);
    g = g + ((k1 + k2) * hdh);
    k1 = k2;
    h2 = h2 + dh;
  }
}
// calc_geff with use_closed_form_G (lgar/green_ampt.py:85-98): Brooks-Corey estimate from the van Genuchten parameters
// (calc_bc_lambda / calc_bc_psib, physics/utils.py:54-64, 84-99).  Operator precedence as written in the reference:
// geff = h_c * Se_i^e - Se_f^e / (1 - Se_f^e), with Se_f from theta_1 and Se_i from theta_2; inf/nan -> h_c.
template <typename S, int POL = POL_LEAN> __device__ __forceinline__ S geff_closed(const LayerK<S> &l, S theta1, S theta2) {
  using R = real_t<S>;
  const S p = R(1.0) + (R(2.0) / l.m);
  const S lambda = R(2.0) / (p - R(3.0));
  const S psib = (p + R(3.0)) * (R(147.8) + R(8.1) * p + R(0.092) * p * p) /
                 (R(2.0) * l.alpha * p * (p - R(1.0)) * (R(55.6) + R(7.4) * p + p * p));
  const S se_f = se_from_theta(l, theta1);
  const S se_i = se_from_theta(l, theta2);
  const S h_c = psib * (R(2.0) + R(3.0) * lambda) / (R(1.0) + R(3.0) * lambda);
  const S e = R(3.0) + R(1.0) / lambda;
  const S pf = pwq<S, POL>(se_f, e);
  S g = h_c * pwq<S, POL>(se_i, e) - pf / (R(1.0) - pf);
  const R gv = val(g);
  if (gv != gv || gv - gv != R(0.0)) g = h_c;  // torch.isinf / torch.isnan
  return g;
}

// calc_aet, models/physics/lgar/aet.py:17-51 (0.75: GlobalParams.py:75; clamp upper bound = PET rate).  The head at which
// uptake halves (aet.py:31-40) depends on the top layer's parameters only: aet_psi_wp computes it, the column keeps it.
template <typename S, int POL = POL_LEAN> __device__ __forceinline__ S aet_psi_wp(const LayerK<S> &l, real_t<S> wp_psi) {
  using R = real_t<S>;
  S theta_fc = (l.te - l.tr) * R(0.75) + l.tr;
  S wp_head_theta = theta_from_h<S, POL>(l, S(wp_psi));
  S theta_wp = (theta_fc - wp_head_theta) * R(0.5) + wp_head_theta;
  S se = se_from_theta(l, theta_wp);
  return h_from_se<S, POL>(l, se);
}
template <typename S, int POL = POL_LEAN> __device__ __forceinline__ S aet_from_psi_wp(S pet, real_t<S> dt_h, S psi, S psi_wp) {
  using R = real_t<S>;
  S r = psi / psi_wp;
  S h_ratio = R(1.0) + r * r * r;
  S a = pet * (R(1.0) / h_ratio) * dt_h;
  if (val(a) < R(0.0)) a = S(R(0.0));
  if (val(a) > val(pet)) a = pet;
  return a;
}
template <typename S, int POL = POL_LEAN> __device__ __forceinline__ S aet_fn(const LayerK<S> &l, S pet, real_t<S> dt_h, S psi, real_t<S> wp_psi) {
  using R = real_t<S>;
  S psi_wp = aet_psi_wp<S, POL>(l, wp_psi);
  S r = psi / psi_wp;
  S h_ratio = R(1.0) + r * r * r;
  S a = pet * (R(1.0) / h_ratio) * dt_h;
  if (val(a) < R(0.0)) a = S(R(0.0));
  if (val(a) > val(pet)) a = pet;
  return a;
}

}  // namespace lgar
