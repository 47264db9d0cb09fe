// leaf_host.cpp -- TEST INFRASTRUCTURE ONLY: the leaf dispatcher of the device code (lgar_py_amd/csrc/lgar_leaf.hpp) compiled
// for the host with -DLGAR_DEVSIM (v_log_f32 / v_exp_f32 / v_sqrt_f32 / v_rcp_f32 become log2f / exp2f / sqrtf / 1.0f / b, a
// wavefront is one lane) as a shared library: leafhost_batch is lgar_leaf_batch (include/lgar.h) without the stream, a plain
// loop over leaf_eval.  Never built, loaded or referenced by the product package.
#include <cmath>
#include <cstdint>

#define __device__
#define __host__
#define __global__
#define __forceinline__ inline __attribute__((always_inline))

#include "../../lgar_py_amd/csrc/lgar_leaf.hpp"

using namespace lgar;

template <typename R>
static void run(int op, int n, const void *x, const void *y, double z, const void *alpha, const void *nn, const void *ksat, const void *te,
                const void *tr, int nint, double wp, void *out) {
  LeafArgs<R> a{op, n, nint, (const R *)x, (const R *)y, (const R *)alpha, (const R *)nn, (const R *)ksat, (const R *)te, (const R *)tr,
                (R)z, (R)wp, (R *)out};
  for (int i = 0; i < n; i++) a.out[i] = leaf_eval<R>(a, i);
}

extern "C" int32_t leafhost_batch(int32_t op, int32_t n_items, const void *x, const void *y, double z, const void *alpha, const void *n,
                                  const void *ksat, const void *theta_e, const void *theta_r, int32_t nint, double wilting_point_psi,
                                  void *out, int32_t dtype) {
  if (op < 0 || op > LEAF_OP_LAST || n_items <= 0 || !x || !alpha || !n || !ksat || !theta_e || !theta_r || !out) return LGAR_E_ARG;
  if (op >= LEAF_OP_F32_FIRST && dtype != LGAR_F32) return LGAR_E_ARG;
  if (dtype == LGAR_F64) run<double>(op, n_items, x, y, z, alpha, n, ksat, theta_e, theta_r, nint, wilting_point_psi, out);
  else if (dtype == LGAR_F32) run<float>(op, n_items, x, y, z, alpha, n, ksat, theta_e, theta_r, nint, wilting_point_psi, out);
  else return LGAR_E_ARG;
  return 0;
}

// lgar_leaf_tangent_batch without the stream and without the shared trapezoid (share != 0 is refused: the exchange through LDS
// has no host counterpart): a plain loop over leaf_tangent_eval.
template <typename R>
static void run_tangent(int op, int policy, int n, const void *x, const void *y, double z, const void *alpha, const void *nn,
                        const void *ksat, const void *te, const void *tr, const void *const *seeds, int nint, double wp, void *value,
                        void *tangent) {
  LeafTangentArgs<R> a;
  a.op = op; a.pol = policy; a.share = 0; a.n = n; a.nint = nint;
  a.x = (const R *)x; a.y = (const R *)y; a.alpha = (const R *)alpha; a.nn = (const R *)nn; a.ksat = (const R *)ksat;
  a.te = (const R *)te; a.tr = (const R *)tr;
  for (int j = 0; j < LEAF_NSEED; j++) a.seed[j] = (const R *)seeds[j];
  a.z = (R)z; a.wp_psi = (R)wp;
  a.value = (R *)value; a.tangent = (R *)tangent;
  for (int i = 0; i < n; i++) {
    const Dual<R> r = leaf_tangent_eval<R>(a, i, i);
    a.value[i] = r.v;
    a.tangent[i] = r.d;
  }
}

extern "C" int32_t leafhost_tangent_batch(int32_t op, int32_t policy, int32_t share, int32_t n_items, const void *x, const void *y,
                                          double z, const void *alpha, const void *n, const void *ksat, const void *theta_e,
                                          const void *theta_r, const void *d_alpha, const void *d_n, const void *d_ksat,
                                          const void *d_theta_e, const void *d_theta_r, const void *d_x, const void *d_y, int32_t nint,
                                          double wilting_point_psi, void *out_value, void *out_tangent, int32_t dtype) {
  const int rc = leaf_tangent_check<true>(op, policy, share, n_items, x, y, alpha, n, ksat, theta_e, theta_r, out_value, out_tangent, dtype);
  if (rc) return rc;
  const void *seeds[LEAF_NSEED] = {d_alpha, d_n, d_ksat, d_theta_e, d_theta_r, d_x, d_y};
  if (dtype == LGAR_F64)
    run_tangent<double>(op, policy, n_items, x, y, z, alpha, n, ksat, theta_e, theta_r, seeds, nint, wilting_point_psi, out_value, out_tangent);
  else
    run_tangent<float>(op, policy, n_items, x, y, z, alpha, n, ksat, theta_e, theta_r, seeds, nint, wilting_point_psi, out_value, out_tangent);
  return 0;
}
