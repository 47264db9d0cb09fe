// lgar_leaf_tangent.hip -- the element-wise tangent leaf kernels of the known-answer tests (lgar_leaf_tangent_batch,
// include/lgar.h): one dual number per item through leaf_tangent_eval (lgar_leaf.hpp), and the shared trapezoid launched as the
// tangent kernels launch it (lgar_tangent_nl.hip): one-wave workgroups, floor(64 / W) groups of W adjacent lanes, one item per
// group, lane r of a group along direction r, the wave's exchange buffer in LDS.
#include <hip/hip_runtime.h>

#include "lgar_host.hpp"
#include "lgar_leaf.hpp"

namespace lgar {

template <typename R> __global__ void lgar_leaf_tangent_kernel(LeafTangentArgs<R> a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const Dual<R> r = leaf_tangent_eval(a, i, i);
  a.value[i] = r.v;
  a.tangent[i] = r.d;
}

// (double precision only: what geff_fused shares)
__global__ __launch_bounds__(WAVE) void lgar_leaf_tangent_shared_kernel(LeafTangentArgs<double> a) {
  __shared__ double xchg[LGAR_XCHG_WORDS];
  const int lane = threadIdx.x;
  const int W = a.share;
  const int groups = WAVE / W;
  // lanes beyond the last full group are idle, as are the groups past the last item
  const int g = lane / W;
  const long long item = (long long)blockIdx.x * groups + g;
  if (g >= groups || item >= a.n) return;
  const int i = (int)item;
  const int k = i * W + (lane - g * W);
  const Dual<double> r = leaf_tangent_eval(a, i, k, &xchg[0], W);
  a.value[k] = r.v;
  a.tangent[k] = r.d;
}

template <typename R>
static LeafTangentArgs<R> make_leaf_tangent_args(int op, int policy, int share, int n_items, const void *x, const void *y, double z,
                                                 const void *alpha, const void *n, const void *ksat, const void *theta_e,
                                                 const void *theta_r, const void *const *seeds, int nint, double wp, void *out_value,
                                                 void *out_tangent) {
  LeafTangentArgs<R> a;
  a.op = op; a.pol = policy; a.share = share; a.n = n_items; a.nint = nint;
  a.x = (const R *)x; a.y = (const R *)y; a.alpha = (const R *)alpha; a.nn = (const R *)n; a.ksat = (const R *)ksat;
  a.te = (const R *)theta_e; a.tr = (const R *)theta_r;
  for (int j = 0; j < LEAF_NSEED; j++) a.seed[j] = (const R *)seeds[j];
  a.z = (R)z; a.wp_psi = (R)wp;
  a.value = (R *)out_value; a.tangent = (R *)out_tangent;
  return a;
}

}  // namespace lgar

using namespace lgar;

extern "C" int32_t lgar_leaf_tangent_batch(int32_t op, int32_t policy, int32_t share, int32_t n_items, const void *x, const void *y,
                                           double z, const void *alpha, const void *n, const void *ksat, const void *theta_e,
                                           const void *theta_r, const void *d_alpha, const void *d_n, const void *d_ksat,
                                           const void *d_theta_e, const void *d_theta_r, const void *d_x, const void *d_y, int32_t nint,
                                           double wilting_point_psi, void *out_value, void *out_tangent, int32_t dtype, void *stream) {
  const int rc = leaf_tangent_check(op, policy, share, n_items, x, y, alpha, n, ksat, theta_e, theta_r, out_value, out_tangent, dtype);
  if (rc) return rc;
  if (share != 0 && (long long)n_items * share > 0x7fffffffLL) return LGAR_E_ARG;  // (the outputs' index is an int)
  const void *seeds[LEAF_NSEED] = {d_alpha, d_n, d_ksat, d_theta_e, d_theta_r, d_x, d_y};
  hipStream_t st = (hipStream_t)stream;
  if (share != 0) {
    const unsigned groups = (unsigned)(WAVE / share);
    const unsigned grid = ((unsigned)n_items + groups - 1) / groups;
    hipLaunchKernelGGL(lgar_leaf_tangent_shared_kernel, dim3(grid), dim3(WAVE), 0, st,
                       make_leaf_tangent_args<double>(op, policy, share, n_items, x, y, z, alpha, n, ksat, theta_e, theta_r, seeds, nint,
                                                      wilting_point_psi, out_value, out_tangent));
  } else {
    const unsigned grid = (unsigned)((n_items + 255) / 256);
    if (dtype == LGAR_F64)
      hipLaunchKernelGGL(lgar_leaf_tangent_kernel<double>, dim3(grid), dim3(256), 0, st,
                         make_leaf_tangent_args<double>(op, policy, share, n_items, x, y, z, alpha, n, ksat, theta_e, theta_r, seeds,
                                                        nint, wilting_point_psi, out_value, out_tangent));
    else
      hipLaunchKernelGGL(lgar_leaf_tangent_kernel<float>, dim3(grid), dim3(256), 0, st,
                         make_leaf_tangent_args<float>(op, policy, share, n_items, x, y, z, alpha, n, ksat, theta_e, theta_r, seeds,
                                                       nint, wilting_point_psi, out_value, out_tangent));
  }
  return launch_status();
}
