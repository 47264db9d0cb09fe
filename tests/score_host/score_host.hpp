// TEST INFRASTRUCTURE ONLY -- the catchment-score entry points of include/lgar.h with the host in the GPU's place.
//
// The per-lane functions the kernels run (lgar_py_amd/csrc/lgar_score.hpp) are plain C++; with -DLGAR_DEVSIM they compile for
// the host, one lane after the other.  This header holds what lgar_score.hip puts around them -- the argument refusals of the
// C-ABI wrappers and the launchers' early-outs -- once: one function per entry point, with the argument list of include/lgar.h
// minus the stream.  Compiled on its own it is libscorehost.so, which SimCatchmentScore (tests/score_host) puts behind the
// product's calling surface; score_host.cpp is the stand-alone program around it, which also runs under AddressSanitizer +
// UBSan.  Never built or used by the product.
#ifndef LGAR_TESTS_SCORE_HOST_HPP
#define LGAR_TESTS_SCORE_HOST_HPP
#define LGAR_DEVSIM 1
#include <stddef.h>
#include <stdint.h>

#include "../../lgar_py_amd/csrc/lgar_score.hpp"

namespace score_host {

inline lgar::ScoreArgs args(const double *sim, const double *obs, int32_t To, int32_t B, int32_t window) {
  lgar::ScoreArgs a;
  a.sim = sim, a.obs = obs, a.To = To, a.B = B, a.r = window;
  return a;
}

}  // namespace score_host

extern "C" {

int64_t scorehost_catchment_moments_workspace(int32_t n_obs_rows, int32_t n_catchments) {
  if (n_obs_rows < 0 || n_catchments < 0) return LGAR_E_ARG;
  return (int64_t)lgar::score_workspace_bytes(n_obs_rows, n_catchments);
}

int32_t scorehost_catchment_moments(const double *sim, const double *obs, int32_t n_obs_rows, int32_t n_catchments, int32_t window,
                                    double *moments, void *workspace) {
  // what the C-ABI wrappers themselves refuse (lgar_score.hip)
  if (n_obs_rows < 0 || n_catchments < 0 || window < 1 || (int64_t)n_obs_rows * window > INT32_MAX) return LGAR_E_ARG;
  if (n_catchments > 0 && (!moments || (n_obs_rows > 0 && (!sim || !obs || !workspace)))) return LGAR_E_ARG;
  if (n_catchments == 0) return 0;
  lgar::score_moments_all(score_host::args(sim, obs, n_obs_rows, n_catchments, window), moments, (double *)workspace);
  return 0;
}

int32_t scorehost_catchment_moments_grad(const double *sim, const double *obs, int32_t n_obs_rows, int32_t n_catchments, int32_t window,
                                         const double *moments, const double *coef, double *grad_sim) {
  if (n_obs_rows < 0 || n_catchments < 0 || window < 1 || (int64_t)n_obs_rows * window > INT32_MAX) return LGAR_E_ARG;
  if (n_catchments > 0 && n_obs_rows > 0 && (!sim || !obs || !moments || !coef || !grad_sim)) return LGAR_E_ARG;
  if (n_catchments == 0 || n_obs_rows == 0) return 0;
  lgar::score_grad_all(score_host::args(sim, obs, n_obs_rows, n_catchments, window), moments, coef, grad_sim);
  return 0;
}

}  // extern "C"
#endif
