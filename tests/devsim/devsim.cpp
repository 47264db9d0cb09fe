// devsim.cpp -- TEST INFRASTRUCTURE ONLY: the device code of lgar_py_amd/csrc compiled for the host.
//
// The column physics (lgar_column.hpp), the per-lane kernel bodies (lgar_forward_body.hpp, lgar_tangent_body.hpp) and the
// front-capacity chain are plain C++ templates; with -DLGAR_DEVSIM the few GPU intrinsics they use map to libm and
// wave-level operations degenerate to a single lane.  This lets the CPU test suite (-m "not gpu") run the SAME source the
// GPU executes against the reference's golden vectors, so logic errors surface without a GPU.  It is not a fallback: the
// product package (lgar_py_amd) never builds, loads or references this file, and nothing here is shipped or timed.
#define LGAR_DEVSIM 1
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#define __device__
#define __host__
#define __global__
#define __forceinline__ inline __attribute__((always_inline))

#include "../../lgar_py_amd/csrc/lgar_plan.hpp"
#include "../../lgar_py_amd/csrc/lgar_tangent_body.hpp"

using namespace lgar;

namespace {

template <typename R, int NL, int CAP, int MODE> void run_forward(const KArgs<R> &a) {
  std::vector<WaveLDS<R, CAP>> lds(1);
  for (int c = 0; c < a.N; c++) forward_lane<R, NL, CAP, MODE>(&a, (size_t)c, true, 0, lds[0]);
}

// The library's own argument blocks and plans (lgar_plan.hpp) with the job's real block count.  The simulator runs one lane,
// so the cooperating lanes a plan gives a small fp64 job are ignored: they are bit-identical to one lane per column by design.
constexpr unsigned SIMDS = 1024;  // (an MI355X: 256 CUs x 4)

template <typename R, int NL, int MODE> void run_forward_cap(const KArgs<R> &a, int cap) {
  if (cap == LGAR_CAP_SMALL) run_forward<R, NL, LGAR_CAP_SMALL, MODE>(a);
  else if (cap == LGAR_CAP_MID) run_forward<R, NL, LGAR_CAP_MID, MODE>(a);
  else run_forward<R, NL, LGAR_FMAX, MODE>(a);
}

template <typename R, int NL>
int forward_typed(const LgarDims *d, const LgarParams *p, LgarState *s, const LgarForcing *f, const LgarStepOut *o, int32_t *status) {
  KArgs<R> a = make_args<R>(d, p, s, f, o, status);
  const ForwardPlan plan = forward_plan<R>(d, NL, SIMDS);
  for (int i = 0; i < plan.n; i++) {
    chain_step(a, i, plan.n, nullptr);
    if constexpr (ScalarKind<R>::f64) {
      if (plan.mixed) { run_forward_cap<R, NL, MODE_MIXED>(a, plan.caps[i]); continue; }
    }
    if (plan.literal) run_forward<R, NL, LGAR_FMAX, MODE_LITERAL>(a);
    else run_forward_cap<R, NL, MODE_FAST>(a, plan.caps[i]);
  }
  return 0;
}

template <typename R, int NL> int init_typed(const LgarDims *d, const LgarParams *p, LgarState *s, int32_t *status) {
  KArgs<R> a = make_args<R>(d, p, s, nullptr, nullptr, status);
  std::vector<WaveLDS<R, LGAR_CAP_SMALL>> lds(1);
  for (int c = 0; c < a.N; c++) init_lane<R, NL, LGAR_CAP_SMALL>(&a, (size_t)c, 0, lds[0]);
  return 0;
}

// (the plan's walk is the library's own: tangent_chain, lgar_tangent_body.hpp)
template <typename R, int NL>
int tangent_typed(const LgarDims *d, const LgarParams *p, const LgarParams *dir, const LgarForcing *f, const void *wr, const void *wp,
                  void *grad, void *tser, int32_t *status) {
  TArgs<R> a = make_targs<R>(d, p, dir, f, wr, wp, grad, tser, status);
  return tangent_chain(a, tangent_plan(d, NL), nullptr, [&](auto cap, auto mode, unsigned *) {
    std::vector<WaveLDS<Dual<R>, decltype(cap)::value, 1>> lds(1);
    for (int c = 0; c < a.N; c++) tangent_lane<R, NL, decltype(cap)::value, decltype(mode)::value>(&a, (size_t)c, 0, lds[0]);
    return 0;
  });
}

}  // namespace

extern "C" {

// element-wise access to the lean fp64 math (lgar_math.hpp): op 0 exp2, 1 log2, 2 pow(x, y), 3 exp2_core, 4 log2_core;
// 10..14: the same with the polynomials' high-order terms combined pairwise (ESTRIN: the mixed-precision kernels)
void devsim_math(int op, int n, const double *x, const double *y, double *out) {
  for (int i = 0; i < n; i++) {
    switch (op) {
      case 0: out[i] = fast_exp2(x[i]); break;
      case 1: out[i] = fast_log2(x[i]); break;
      case 2: out[i] = fast_pow(x[i], y[i]); break;
      case 3: out[i] = fast_exp2_core<false>(x[i]); break;
      case 4: out[i] = fast_log2_core(x[i]); break;
      case 10: out[i] = fast_exp2<true>(x[i]); break;
      case 11: out[i] = fast_log2<true>(x[i]); break;
      case 12: out[i] = fast_pow<true>(x[i], y[i]); break;
      case 13: out[i] = fast_exp2_core<false, true>(x[i]); break;
      case 14: out[i] = fast_log2_core<true>(x[i]); break;
    }
  }
}

// element-wise Geff variants on host doubles: 0 fused fp64 (fast modes), 1 mixed precision (geff_mode 1), 2 the reference's
// literal trapezoid with the library pow, 3 the packed fp32 loop (inputs rounded to float)
void devsim_geff(int variant, int n, const double *theta1, const double *theta2, const double *alpha, const double *nn,
                 const double *ksat, const double *te, const double *tr, int nint, double *out) {
  for (int i = 0; i < n; i++) {
    LayerK<double> l;
    l.alpha = alpha[i]; l.n = nn[i]; l.m = 1.0 - 1.0 / l.n; l.inv_m = 1.0 / l.m; l.inv_n = 1.0 / l.n;
    l.ksat = ksat[i]; l.te = te[i]; l.tr = tr[i];
    if (variant == 0) out[i] = geff_fused<double>(l, theta1[i], theta2[i], nint);
    else if (variant == 1) out[i] = geff_mixed(l.alpha, l.n, l.m, l.inv_m, l.inv_n, l.ksat, l.te, l.tr, theta1[i], theta2[i], nint);
    else if (variant == 2) out[i] = geff_literal<double, POL_LIBRARY>(l, theta1[i], theta2[i], nint);
    else {
      LayerK<float> f;
      f.alpha = (float)l.alpha; f.n = (float)l.n; f.m = 1.0f - 1.0f / f.n; f.inv_m = 1.0f / f.m; f.inv_n = 1.0f / f.n;
      f.ksat = (float)l.ksat; f.te = (float)l.te; f.tr = (float)l.tr;
      out[i] = (double)geff<float>(f, (float)theta1[i], (float)theta2[i], nint);
    }
  }
}

int devsim_state_init(const LgarDims *d, const LgarParams *p, LgarState *s, int32_t *status, int dtype) {
#define X(n) if (d->n_layers == n) return dtype == LGAR_F64 ? init_typed<double, n>(d, p, s, status) : init_typed<float, n>(d, p, s, status);
  LGAR_LAYERS(X)
#undef X
  return LGAR_E_ARG;
}

int devsim_forward(const LgarDims *d, const LgarParams *p, LgarState *s, const LgarForcing *f, const LgarStepOut *o, int32_t *status, int dtype) {
#define X(n) if (d->n_layers == n) return dtype == LGAR_F64 ? forward_typed<double, n>(d, p, s, f, o, status) : forward_typed<float, n>(d, p, s, f, o, status);
  LGAR_LAYERS(X)
#undef X
  return LGAR_E_ARG;
}

int devsim_tangent(const LgarDims *d, const LgarParams *p, const LgarParams *dir, const LgarForcing *f, const void *wr, const void *wp,
                   void *grad, void *tser, int32_t *status, int dtype) {
#define X(n) if (d->n_layers == n) return dtype == LGAR_F64 ? tangent_typed<double, n>(d, p, dir, f, wr, wp, grad, tser, status) \
                                                             : tangent_typed<float, n>(d, p, dir, f, wr, wp, grad, tser, status);
  LGAR_LAYERS(X)
#undef X
  return LGAR_E_ARG;
}

}  // extern "C"
