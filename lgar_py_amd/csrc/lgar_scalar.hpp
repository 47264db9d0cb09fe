// lgar_scalar.hpp -- scalar-type plumbing of the device code: the wavefront width, the real type of a scalar (float, double,
// or a dual number of lgar_dual.hpp), wave-level lane primitives, pow and division by arithmetic policy, the measurement-point
// hook, tolerances and the per-layer van Genuchten parameters of a column.
#pragma once
#ifndef LGAR_DEVSIM
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#include "../../include/lgar.h"
#include "lgar_math.hpp"

// Kernel arguments are read where they are used, as scalar loads from the kernarg segment (constant address space),
// instead of being held in SGPRs for the whole kernel: the argument block (35 pointers + the run-time constants) is
// larger than the SGPR file, and everything the register allocator cannot keep becomes v_writelane / v_readlane traffic
// on the vector ALU -- the unit this kernel is bound by.
#ifndef LGAR_DEVSIM
#define LGAR_KARG __attribute__((address_space(4)))
#else
#define LGAR_KARG
#endif

namespace lgar {

constexpr int WAVE = 64;

// ---------------------------------------------------------------------------------------------
// scalar-type plumbing
// ---------------------------------------------------------------------------------------------
template <typename S> struct Real { using type = S; };
template <typename S> using real_t = typename Real<S>::type;
// What a scalar type is: its arithmetic (the real type R = real_t<S>: fp32 or fp64) and whether it is a plain number or a dual
// number (value + tangent, lgar_dual.hpp).  sizeof(S) == 8 alone holds for double and Dual<float> alike: ask these instead.
template <typename S> struct ScalarKind {
  using R = real_t<S>;
  static constexpr bool f64 = sizeof(R) == 8;         // double, Dual<double>
  static constexpr bool f32 = !f64;                    // float, Dual<float>
  static constexpr bool dual = sizeof(S) != sizeof(R);  // Dual<R>: two reals
  static constexpr bool plain_f64 = f64 && !dual;      // double
  static constexpr bool plain_f32 = f32 && !dual;      // float
};

// Arithmetic policy of the leaf functions and the column physics (template parameter POL; ModeTraits::pol picks a kernel's):
//   POL_LEAN     lean pow (lgar_math.hpp), IEEE division                    -- fp64 fast mode, dual numbers
//   POL_LIBRARY  library pow, IEEE division                                 -- verification mode in double precision
//   POL_RCP32    v_log/v_exp pow, division as a * v_rcp_f32(b) (<= 2 ulp: 1.83 measured on an MI355X, v_rcp_f32 itself being good
//                to 1 ulp; tests/test_gpu_leaf_f32.py) -- fp32 fast mode: the correctly rounded fp32
//                divide is ~10 instructions, the path takes ~20 of them per column-step.
//   POL_MIXED    POL_LEAN with the lean pow's pairwise-combined polynomials (lgar_math.hpp, ESTRIN) -- the mixed-precision kernels
// Se = (theta - theta_r)/(theta_e - theta_r) keeps the IEEE divide in every policy: Se must be exactly 1 at saturation
// (x/x == 1), or the pow bases go negative.
constexpr int POL_LEAN = 0, POL_LIBRARY = 1, POL_RCP32 = 2, POL_MIXED = 3;

__device__ __forceinline__ double val(double x) { return x; }
__device__ __forceinline__ float val(float x) { return x; }
__device__ __forceinline__ double pw(double x, double y) { return fast_pow<false>(x, y); }  // lgar_math.hpp, ~1e-14 relative
// fp32: v_log_f32 / v_exp_f32 (quarter-rate transcendentals), each within 1 ulp (measured: 1.00 and 0.77; the logarithm keeps its
// relative accuracy next to 1).  The pow made of them is NOT a few ulp: the logarithm's ulp is multiplied by y, so the error grows
// like 2.08 |y log2 x| + 1.5 ulp at worst -- 1.4 ulp for |y log2 x| <= 1, 157 ulp at |y log2 x| = 100 (tests/test_gpu_leaf_f32.py)
// log2 / exp2 (fused Geff node, dual-number pow)
#ifndef LGAR_DEVSIM
__device__ __forceinline__ float lg2(float x) { return __builtin_amdgcn_logf(x); }
__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float sq(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float clamp01(float x) { return __builtin_amdgcn_fmed3f(x, 0.0f, 1.0f); }  // v_med3_f32
__device__ __forceinline__ unsigned long long any_lane(bool p) { return __ballot(p); }
__device__ __forceinline__ bool first_active_lane() {
  const unsigned long long m = __ballot(1);
  return (int)(threadIdx.x & 63u) == __ffsll((long long)m) - 1;
}
// between the stores and the loads of an exchange through the wave's LDS (cooperating lanes): one wave = one workgroup and a
// wave's LDS operations complete in order, so this only pins the compiler
__device__ __forceinline__ void lds_exchange_point() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}
// a value loaded from memory a step ahead is taken into its register HERE (the wait for the load is placed at this point):
// loads and stores share one counter, and a wait placed after later stores would wait for those as well
template <typename T> __device__ __forceinline__ void settle_load(T &x) { asm volatile("" : "+v"(x)); }
#else  // tests/devsim: the same device code compiled for the host, one lane at a time (test infrastructure only)
__device__ __forceinline__ float lg2(float x) { return log2f(x); }
__device__ __forceinline__ float ex2(float x) { return exp2f(x); }
__device__ __forceinline__ float sq(float x) { return sqrtf(x); }
__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
__device__ __forceinline__ unsigned long long any_lane(bool p) { return p ? 1ull : 0ull; }
__device__ __forceinline__ bool first_active_lane() { return true; }
__device__ __forceinline__ void lds_exchange_point() {}
template <typename T> __device__ __forceinline__ void settle_load(T &) {}
#endif
__device__ __forceinline__ float pw(float x, float y) { return ex2(y * lg2(x)); }
// EX = true (verification mode, double precision only): the correctly rounded library pow, as the reference's torch.pow;
// otherwise the lean pow above
template <bool EX> __device__ __forceinline__ double pwx(double x, double y) {
  if constexpr (EX) return pow(x, y);
  return pw(x, y);
}
template <bool EX> __device__ __forceinline__ float pwx(float x, float y) { return pw(x, y); }
// pow by arithmetic policy POL (see POL_LEAN)
template <int POL> __device__ __forceinline__ double pwp(double x, double y) {
  if constexpr (POL == POL_LIBRARY) return pow(x, y);
  if constexpr (POL == POL_MIXED) return fast_pow<true>(x, y);
  return fast_pow<false>(x, y);
}
template <int POL> __device__ __forceinline__ float pwp(float x, float y) { return pw(x, y); }
// ... for any scalar type of the column physics: plain reals by pwp, dual numbers by their own pwx (lgar_dual.hpp)
template <typename S, int POL> __device__ __forceinline__ S pwq(const S &x, const S &y) {
  if constexpr (!ScalarKind<S>::dual) return pwp<POL>(x, y);
  else return pwx<POL == POL_LIBRARY>(x, y);
}

// division by arithmetic policy POL
#ifndef LGAR_DEVSIM
__device__ __forceinline__ float rcp32(float b) { return __builtin_amdgcn_rcpf(b); }
#else
__device__ __forceinline__ float rcp32(float b) { return 1.0f / b; }
#endif
template <int POL> __device__ __forceinline__ float dv(float a, float b) {
  if constexpr (POL == POL_RCP32) return a * rcp32(b);
  return a / b;
}
// POL_LEAN / POL_MIXED in double precision (fast modes): a / b as a * (1 / b) from v_rcp_f64, one Newton step on the reciprocal and one
// correction of the quotient -- six instructions, within an ulp of the IEEE quotient, against the ~14 of the correctly rounded
// divide (v_div_scale / v_div_fmas / v_div_fixup); a column step takes ~25 of them, each on its wave's critical path.  The
// divisors of the column physics are as a rule finite and non-zero (depths, theta differences that were tested > 0,
// 1 + (alpha psi)^n); where one is not -- b = 0, inf or denormal, a = inf: the Newton steps meet inf * 0 and come out NaN
// where the quotient is inf, 0 or finite (an overflowed (alpha h)^n in theta_from_h must give theta_r, not NaN) -- the NaN
// result sends the lanes concerned through the IEEE divide (a compare and a branch that is practically never taken).
// Se = (theta - theta_r) / (theta_e - theta_r) keeps the IEEE divide (se_from_theta: x / x must be exactly 1).
#ifndef LGAR_DEVSIM
__device__ __forceinline__ double lean_div(double a, double b) {
  double r = __builtin_amdgcn_rcp(b);
  r = __builtin_fma(__builtin_fma(-b, r, 1.0), r, r);
  const double q = a * r;
  double res = __builtin_fma(__builtin_fma(-b, q, a), r, q);
  if (__builtin_expect(res != res, 0)) res = a / b;
  return res;
}
#else
__device__ __forceinline__ double lean_div(double a, double b) { return a / b; }
#endif
template <int POL> __device__ __forceinline__ double dv(double a, double b) {
  if constexpr (POL == POL_LEAN || POL == POL_MIXED) return lean_div(a, b);
  return a / b;
}
__device__ __forceinline__ double lg2(double x) { return fast_log2<false>(x); }
__device__ __forceinline__ double ex2(double x) { return fast_exp2<false>(x); }
// (the mixed-precision trapezoid's own double-precision logarithms and exponentials: see fast_pow on ESTRIN)
__device__ __forceinline__ double lg2e(double x) { return fast_log2<true>(x); }
__device__ __forceinline__ double ex2e(double x) { return fast_exp2<true>(x); }
// log2 / exp2 of arguments known to be positive / not NaN (the interior of the Geff trapezoid): no special-case selects
__device__ __forceinline__ float lg2p(float x) { return lg2(x); }
__device__ __forceinline__ float ex2p(float x) { return ex2(x); }
__device__ __forceinline__ double lg2p(double x) { return fast_log2_core<false>(x); }
__device__ __forceinline__ double ex2p(double x) { return fast_exp2_core<false, false>(x); }
__device__ __forceinline__ double sq(double x) { return sqrt(x); }
__device__ __forceinline__ double ab(double x) { return fabs(x); }
__device__ __forceinline__ float ab(float x) { return fabsf(x); }
__device__ __forceinline__ double mn(double a, double b) { return fmin(a, b); }
__device__ __forceinline__ float mn(float a, float b) { return fminf(a, b); }
__device__ __forceinline__ bool is_nan(double x) { return x != x; }
__device__ __forceinline__ bool is_nan(float x) { return x != x; }
__device__ __forceinline__ bool same_bits(double a, double b) { return a == b; }  // (NaN never matches: recomputed)
__device__ __forceinline__ bool same_bits(float a, float b) { return a == b; }

// Measurement points (cost attribution, tools/ablate.py): LGAR_MEASURE_POINT(NAME, args) marks a place where a measurement
// build can run a routine twice or count something, LGAR_ABLATABLE(NAME, statement) a statement such a build can leave out.
// In the product both are transparent: the point is empty, the statement is just the statement.  Only
// lgar_py_amd.build.build_variant passes -DLGAR_MEASURE, which takes the definitions from lgar_measure.hpp instead.
#ifdef LGAR_MEASURE
#include "lgar_measure.hpp"
#else
#define LGAR_MEASURE_POINT(NAME, ...)
#define LGAR_ABLATABLE(NAME, ...) __VA_ARGS__
// one lane per wave-level Geff evaluation adds 1 above the fault bits of its status word (no register, no LDS word; summed
// over the wave at the end of the block): bits 8..31 are otherwise unused while a column is integrated
#ifndef LGAR_COUNT_TOP_LAYER_STEP
#define LGAR_COUNT_GEFF_CALL(site) \
  if (count_geff && first_active_lane()) status += (1 << LGAR_ST_STEP_SHIFT);
#else
#define LGAR_COUNT_GEFF_CALL(site)
#endif
#endif
// -DLGAR_COUNT_TOP_LAYER_STEP=1 / =0 (tests only; the simulator's build can pass it too): the counter above counts the wave-level
// sub-steps whose sweep took the top-layer step (1) or the generic one (0) INSTEAD of the Geff evaluations
#ifdef LGAR_COUNT_TOP_LAYER_STEP
#define LGAR_COUNT_TOP_STEP(fast) \
  if (count_geff && first_active_lane() && (fast) == (LGAR_COUNT_TOP_LAYER_STEP != 0)) status += (1 << LGAR_ST_STEP_SHIFT);
#else
#define LGAR_COUNT_TOP_STEP(fast)
#endif

// tolerances: the reference's absolute 1e-12 (layers/Layer.py:60) is unreachable in fp32
template <typename R> struct Tol;
template <> struct Tol<double> {
  static constexpr double mass = 1e-12;      // Layer.tolerance
  static constexpr double nochange = 1e-15;  // Layer.py:307,309
  static constexpr double tiny = 1e-50;      // Layer.py:315
};
template <> struct Tol<float> {
  static constexpr float mass = 2e-5f;
  static constexpr float nochange = 1e-9f;
  static constexpr float tiny = 1e-30f;
};

template <typename S> struct LayerK {
  S alpha, n, m, inv_m, inv_n, ksat, te, tr;
};

// the derived parameters of a layer, m = 1 - 1/n, 1/m and 1/n, in the scalar type S (for dual numbers: with their tangents along
// dn).  The tangent kernels (tangent_lane) and the leaf dispatchers (lgar_leaf.hpp) both form them here: what a leaf test pins is
// what the kernels run.
template <typename S> __device__ __forceinline__ void derive_layer(const S &n, S &m, S &inv_m, S &inv_n) {
  using R = real_t<S>;
  m = R(1.0) - (R(1.0) / n);
  inv_m = R(1.0) / m;
  inv_n = R(1.0) / n;
}

template <typename S, int NL> struct ColParams {
  S alpha[NL], n[NL], m[NL], inv_m[NL], inv_n[NL], ksat[NL], te[NL], tr[NL], thick[NL], cum[NL];
};

// c ? a : b on VALUES (a dual number selects component by component: a ternary on two structs can become a select of
// addresses + a load, which sends the operands through scratch memory)
__device__ __forceinline__ float choose(bool c, float a, float b) { return c ? a : b; }
__device__ __forceinline__ double choose(bool c, double a, double b) { return c ? a : b; }

template <typename S, int NL> __device__ __forceinline__ S sel(const S (&a)[NL], int k) {
  // load every element unconditionally, then select on VALUES: a lazily evaluated a[j] becomes a
  // select of addresses + one load, which pins the whole parameter block in scratch memory
  S v[NL];
#pragma unroll
  for (int j = 0; j < NL; j++) v[j] = a[j];
  S r = v[0];
#pragma unroll
  for (int j = 1; j < NL; j++) r = choose(k == j, v[j], r);
  return r;
}

template <typename S, int NL> __device__ __forceinline__ LayerK<S> pick(const ColParams<S, NL> &P, int k) {
  LayerK<S> l;
  l.alpha = sel<S, NL>(P.alpha, k);
  l.n = sel<S, NL>(P.n, k);
  l.m = sel<S, NL>(P.m, k);
  l.ksat = sel<S, NL>(P.ksat, k);
  l.inv_m = sel<S, NL>(P.inv_m, k);
  l.inv_n = sel<S, NL>(P.inv_n, k);
  l.te = sel<S, NL>(P.te, k);
  l.tr = sel<S, NL>(P.tr, k);
  return l;
}
template <typename S, int NL> __device__ __forceinline__ LayerK<S> pick_static(const ColParams<S, NL> &P, int j) {
  LayerK<S> l;
  l.alpha = P.alpha[j]; l.n = P.n[j]; l.m = P.m[j]; l.inv_m = P.inv_m[j];
  l.inv_n = P.inv_n[j]; l.ksat = P.ksat[j]; l.te = P.te[j]; l.tr = P.tr[j];
  return l;
}

}  // namespace lgar
