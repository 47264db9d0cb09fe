// forced_host.cpp -- TEST INFRASTRUCTURE ONLY: the tangent with a forcing direction (lgar_forward_tangent_forced) compiled for
// the host.
//
// The same headers the lgar_tangent_forced_kernel family of lgar_py_amd/csrc/lgar_tangent_forced_nl.hip is made of --
// tangent_lane<..., WINDOW = true, FORCED = true>, make_tfargs, tangent_plan, tangent_chain, the argument checks -- under
// -DLGAR_DEVSIM, one lane at a time, as tests/window_host does for the window family.  The product package never builds, loads
// or references this file.
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

template <typename R, int NL>
int forced_typed(const LgarDims *d, const LgarParams *p, const LgarParams *dir, const LgarForcing *f, const LgarForcing *df,
                 const void *wr, const void *wp, const LgarTangentWindow *win, void *grad, void *tser, int32_t *status) {
  TFArgs<R> a = make_tfargs<R>(d, p, dir, f, df, wr, wp, win, grad, tser, status);
  return tangent_chain(a, tangent_plan(d, NL), nullptr, [&](auto cap, auto mode, unsigned *) {
    std::vector<WaveLDS<Dual<R>, decltype(cap)::value, 1>> lds(1);
    for (int c = 0; c < a.a.N; c++)
      tangent_lane<R, NL, decltype(cap)::value, decltype(mode)::value, true, true>(&a.a, (size_t)c, 0, lds[0], nullptr, &a.w, &a.f);
    return 0;
  });
}

}  // namespace

// lgar_forward_tangent_forced without the stream and the work counters
extern "C" int forcedhost_forward_tangent_forced(const LgarDims *d, const LgarParams *p, const LgarParams *dir, const LgarForcing *f,
                                                 const LgarForcing *df, const void *wr, const void *wp, const LgarTangentWindow *win,
                                                 void *grad, void *tser, int32_t *status, int dtype) {
  int rc = check_tangent_call(d, p, dir, f, grad, status);
  if (rc) return rc;
  rc = check_window(win);
  if (rc) return rc;
  rc = check_forcing_direction(df);
  if (rc) return rc;
  if (dtype != LGAR_F64 && dtype != LGAR_F32) return LGAR_E_ARG;
#define X(n) if (d->n_layers == n) return dtype == LGAR_F64 ? forced_typed<double, n>(d, p, dir, f, df, wr, wp, win, grad, tser, status) \
                                                             : forced_typed<float, n>(d, p, dir, f, df, wr, wp, win, grad, tser, status);
  LGAR_LAYERS(X)
#undef X
  return LGAR_E_ARG;
}
