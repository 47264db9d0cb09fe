// lgar_score.hip -- the catchment-score kernels and their C-ABI entry points (lgar_catchment_moments_workspace /
// lgar_catchment_moments / lgar_catchment_moments_grad, include/lgar.h; lgar_score.hpp holds the aggregated simulation, the
// block partials, the fold of the partials and the gradient element).
//
// Lanes run along the catchments -- 64 lanes are one 512-byte row segment of sim, obs and every moment row -- so a fold needs no
// cross-lane step and no atomics.  The parallelism along the rows is the block structure of the definition: a wave owns (block
// k of 64 observation rows, 64 catchments), walks its at most 64 x window simulation rows and writes its partials to the
// workspace.  The four waves of a workgroup take four consecutive blocks of the same 64 catchments and the workgroups are
// numbered segment-fastest; the grid is capped and the workgroups stride over the (four blocks, segment) pairs, so any
// To x B launches.  A second small kernel, one lane per catchment, folds the block partials in increasing k and forms the
// means; the centred pass is the same pair again with the four centred terms.  Four launches, all on the caller's stream.
// Gradient: one lane per (observation row, catchment) writes the `window` simulation rows under it; workgroups of (four rows,
// 64 catchments), segment-fastest, the same cap and stride.
#include <hip/hip_runtime.h>

#include "lgar_host.hpp"
#include "lgar_score.hpp"

namespace lgar {

#define LGAR_SCORE_GRID_CAP 4096  // workgroups of four waves: twice the chip's 8192 wave slots at 8 waves per SIMD

// PASS 1: (n, sum o, sum s); PASS 2: the four centred sums, about the means the first pass left in moments
template <int PASS> __global__ __launch_bounds__(256) void lgar_score_partial_kernel(ScoreArgs a, const double *moments, double *ws) {
  const long long lane = (long long)(threadIdx.x & 63u), wave = (long long)(threadIdx.x >> 6);
  const long long segs = (a.B + LGAR_SCORE_LANES - 1) / LGAR_SCORE_LANES;
  const long long n_blocks = score_blocks(a.To);
  const long long total = ((n_blocks + 3) / 4) * segs;
  for (long long w = blockIdx.x; w < total; w += gridDim.x) {
    const long long kg = w / segs, seg = w - kg * segs;
    const long long k = kg * 4 + wave, b = seg * LGAR_SCORE_LANES + lane;
    if (k >= n_blocks || b >= a.B) continue;
    if (PASS == 1) {
      double part[3];
      score_block_first(a, k, b, part);
      score_store<3>(ws, k, a.B, b, part);
    } else {
      double part[4];
      score_block_centred(a, k, b, moments[a.B + b], moments[2 * a.B + b], part);
      score_store<4>(ws, k, a.B, b, part);
    }
  }
}

template <int PASS> __global__ __launch_bounds__(256) void lgar_score_fold_kernel(const double *ws, long long n_blocks, long long B, double *moments) {
  for (long long b = (long long)blockIdx.x * 256 + threadIdx.x; b < B; b += (long long)gridDim.x * 256) {
    if (PASS == 1) score_means(ws, n_blocks, B, b, moments);
    else score_centred(ws, n_blocks, B, b, moments);
  }
}

__global__ __launch_bounds__(256) void lgar_score_grad_kernel(ScoreArgs a, const double *moments, const double *coef, double *grad_sim) {
  const long long lane = (long long)(threadIdx.x & 63u), wave = (long long)(threadIdx.x >> 6);
  const long long segs = (a.B + LGAR_SCORE_LANES - 1) / LGAR_SCORE_LANES;
  const long long total = ((a.To + 3) / 4) * segs;
  for (long long w = blockIdx.x; w < total; w += gridDim.x) {
    const long long rg = w / segs, seg = w - rg * segs;
    const long long j = rg * 4 + wave, b = seg * LGAR_SCORE_LANES + lane;
    if (j < a.To && b < a.B) score_grad_store(a, j, b, score_grad_element(a, moments, coef, j, b), grad_sim);
  }
}

static dim3 capped(long long blocks) { return dim3((unsigned)(blocks < LGAR_SCORE_GRID_CAP ? blocks : LGAR_SCORE_GRID_CAP)); }

int launch_catchment_moments(const double *sim, const double *obs, int n_obs_rows, int n_catchments, int window, double *moments,
                             double *workspace, hipStream_t stream) {
  if (n_catchments == 0) return 0;
  ScoreArgs a;
  a.sim = sim, a.obs = obs, a.To = n_obs_rows, a.B = n_catchments, a.r = window;
  const long long segs = (a.B + LGAR_SCORE_LANES - 1) / LGAR_SCORE_LANES;
  const long long n_blocks = score_blocks(a.To);
  const dim3 part_grid = capped(((n_blocks + 3) / 4) * segs), fold_grid = capped((a.B + 255) / 256);
  // (no observation rows: no partials, the folds start and end at +0.0 -- n = 0, NaN means, zero sums)
  if (n_blocks > 0) hipLaunchKernelGGL(lgar_score_partial_kernel<1>, part_grid, dim3(256), 0, stream, a, (const double *)moments, workspace);
  hipLaunchKernelGGL(lgar_score_fold_kernel<1>, fold_grid, dim3(256), 0, stream, (const double *)workspace, n_blocks, a.B, moments);
  if (n_blocks > 0) hipLaunchKernelGGL(lgar_score_partial_kernel<2>, part_grid, dim3(256), 0, stream, a, (const double *)moments, workspace);
  hipLaunchKernelGGL(lgar_score_fold_kernel<2>, fold_grid, dim3(256), 0, stream, (const double *)workspace, n_blocks, a.B, moments);
  return launch_status();
}

int launch_catchment_moments_grad(const double *sim, const double *obs, int n_obs_rows, int n_catchments, int window,
                                  const double *moments, const double *coef, double *grad_sim, hipStream_t stream) {
  if (n_catchments == 0 || n_obs_rows == 0) return 0;
  ScoreArgs a;
  a.sim = sim, a.obs = obs, a.To = n_obs_rows, a.B = n_catchments, a.r = window;
  const long long segs = (a.B + LGAR_SCORE_LANES - 1) / LGAR_SCORE_LANES;
  hipLaunchKernelGGL(lgar_score_grad_kernel, capped(((a.To + 3) / 4) * segs), dim3(256), 0, stream, a, moments, coef, grad_sim);
  return launch_status();
}

}  // namespace lgar

// The C-ABI entry points live here, not with the other wrappers in lgar_kernels.hip: the forward translation units stay
// byte-identical.
extern "C" {

int64_t lgar_catchment_moments_workspace(int32_t n_obs_rows, int32_t n_catchments) {
  if (n_obs_rows < 0 || n_catchments < 0) return LGAR_E_ARG;
  return (int64_t)lgar::score_workspace_bytes(n_obs_rows, n_catchments);
}

int32_t lgar_catchment_moments(const double *sim, const double *obs, int32_t n_obs_rows, int32_t n_catchments, int32_t window,
                               double *moments, void *workspace, void *stream) {
  if (n_obs_rows < 0 || n_catchments < 0 || window < 1 || (int64_t)n_obs_rows * window > INT32_MAX) return LGAR_E_ARG;
  if (n_catchments > 0 && (!moments || (n_obs_rows > 0 && (!sim || !obs || !workspace)))) return LGAR_E_ARG;
  return lgar::launch_catchment_moments(sim, obs, n_obs_rows, n_catchments, window, moments, (double *)workspace, (hipStream_t)stream);
}

int32_t lgar_catchment_moments_grad(const double *sim, const double *obs, int32_t n_obs_rows, int32_t n_catchments, int32_t window,
                                    const double *moments, const double *coef, double *grad_sim, void *stream) {
  if (n_obs_rows < 0 || n_catchments < 0 || window < 1 || (int64_t)n_obs_rows * window > INT32_MAX) return LGAR_E_ARG;
  if (n_catchments > 0 && n_obs_rows > 0 && (!sim || !obs || !moments || !coef || !grad_sim)) return LGAR_E_ARG;
  return lgar::launch_catchment_moments_grad(sim, obs, n_obs_rows, n_catchments, window, moments, coef, grad_sim, (hipStream_t)stream);
}

}  // extern "C"
