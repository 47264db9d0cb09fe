// lgar_kernels.hip -- the C-ABI (include/lgar.h) of the many-column LGAR engine: argument checks and dispatch on the
// soil-layer count to the per-layer-count translation units (lgar_launch.hpp), plus the element-wise leaf kernel used by
// the known-answer tests.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "lgar_catchment.hpp"
#include "lgar_geff.hpp"
#include "lgar_host.hpp"
#include "lgar_launch.hpp"
#include "lgar_leaf.hpp"
#include "lgar_moisture.hpp"

namespace lgar {

template <typename R> __global__ void lgar_leaf_kernel(LeafArgs<R> a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  a.out[i] = leaf_eval(a, i);
}

static int check_state(const LgarParams *p, const LgarState *s, const int32_t *status) {
  if (!p || !s || !status) return LGAR_E_ARG;
  if (!p->alpha || !p->n || !p->ksat || !p->theta_e || !p->theta_r || !p->thickness) return LGAR_E_ARG;
  if (!s->depth || !s->theta || !s->psi || !s->k || !s->dzdt || !s->flags || !s->n_fronts || !s->scalars || !s->totals)
    return LGAR_E_ARG;
  return 0;
}

}  // namespace lgar

using namespace lgar;

// dispatch on the soil-layer count: f(std::integral_constant<int, n>).  A count that is not in LGAR_LAYERS (lgar_plan.hpp;
// measurement variants link fewer, build.py build_variant) has no translation unit in the library and is a bad argument.
template <typename F> static int by_layers(int n_layers, F &&f) {
  switch (n_layers) {
#define LGAR_X(n) case n: return f(std::integral_constant<int, n>());
    LGAR_LAYERS(LGAR_X)
#undef LGAR_X
    default: return LGAR_E_ARG;
  }
}

// Basin aggregation of a STORED series (LgarStepOut.basin with series[j] present): basin[t] += sum_c weight[c] series[t][c]
// (physics/MassBalance.py:77-108 over many columns).  One workgroup per step; every thread sums a fixed strided subset of the
// columns in independent chains, then wave, then workgroup, each in a fixed order: the same inputs give the same bits on
// every run.  The forward kernels' own path (one fp64 atomic per wave and step, for callers that keep no series) costs 11 % of
// the fp32 launch on 1M columns -- 2.4M atomics on T addresses -- against 1 % for this pass over data the launch wrote anyway.
template <typename R> struct Vec16;  // 16-byte packets of the series
template <> struct Vec16<float> { typedef float4 type; static constexpr int n = 4; };
template <> struct Vec16<double> { typedef double2 type; static constexpr int n = 2; };
__device__ __forceinline__ void basin_add(double (&s)[4], const float4 &v) {
  s[0] += (double)v.x; s[1] += (double)v.y; s[2] += (double)v.z; s[3] += (double)v.w;
}
__device__ __forceinline__ void basin_add(double (&s)[4], const double2 &v) { s[0] += v.x; s[1] += v.y; }
__device__ __forceinline__ void basin_add(double (&s)[4], const float4 &v, const float4 &w) {
  s[0] += (double)w.x * (double)v.x; s[1] += (double)w.y * (double)v.y; s[2] += (double)w.z * (double)v.z; s[3] += (double)w.w * (double)v.w;
}
__device__ __forceinline__ void basin_add(double (&s)[4], const double2 &v, const double2 &w) { s[0] += w.x * v.x; s[1] += w.y * v.y; }

// VEC: rows are 16-byte aligned (N a multiple of the packet, base pointers aligned): every thread keeps four 16-byte loads in
// flight (a workgroup streams its 4 MB row at the rate of a CU's memory pipeline instead of one 4-byte load at a time)
template <typename R, bool VEC>
__global__ __launch_bounds__(1024) void lgar_basin_reduce_kernel(const R *series, const R *weights, double *basin, long long N) {
  __shared__ double part[16];
  const int t = blockIdx.x;
  const R *row = series + (size_t)t * (size_t)N;
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  if constexpr (VEC) {
    typedef typename Vec16<R>::type V;
    const long long NV = N / Vec16<R>::n;
    const V *rv = (const V *)row;
    const V *wv = (const V *)weights;
    long long c = threadIdx.x;
    for (; c + 3072 < NV; c += 4096) {
      const V a0 = rv[c], a1 = rv[c + 1024], a2 = rv[c + 2048], a3 = rv[c + 3072];
      if (wv == nullptr) {
        basin_add(s, a0); basin_add(s, a1); basin_add(s, a2); basin_add(s, a3);
      } else {
        const V w0 = wv[c], w1 = wv[c + 1024], w2 = wv[c + 2048], w3 = wv[c + 3072];
        basin_add(s, a0, w0); basin_add(s, a1, w1); basin_add(s, a2, w2); basin_add(s, a3, w3);
      }
    }
    for (; c < NV; c += 1024) {
      if (wv == nullptr) basin_add(s, rv[c]);
      else basin_add(s, rv[c], wv[c]);
    }
  } else {
    for (long long c = threadIdx.x; c < N; c += 1024) s[0] += (weights ? (double)weights[c] : 1.0) * (double)row[c];
  }
  double v = (s[0] + s[1]) + (s[2] + s[3]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tot = 0.0;
    for (int i = 0; i < 16; i++) tot += part[i];
    basin[t] += tot;
  }
}

template <typename R>
static void launch_basin_reduce(const void *series, const void *weights, double *row, long long N, int T, hipStream_t st) {
  const bool vec = (N % Vec16<R>::n == 0) && ((uintptr_t)series % 16 == 0) && ((uintptr_t)weights % 16 == 0);
  if (vec)
    hipLaunchKernelGGL((lgar_basin_reduce_kernel<R, true>), dim3((unsigned)T), dim3(1024), 0, st, (const R *)series,
                       (const R *)weights, row, N);
  else
    hipLaunchKernelGGL((lgar_basin_reduce_kernel<R, false>), dim3((unsigned)T), dim3(1024), 0, st, (const R *)series,
                       (const R *)weights, row, N);
}

static int forward_by_layers(const LgarDims *dims, const LgarParams *params, LgarState *state, const LgarForcing *forcing,
                             const LgarStepOut *out, int32_t *status, int32_t dtype, hipStream_t stream) {
  return by_layers(dims->n_layers, [&](auto nl) {
    return launch_forward_nl<decltype(nl)::value>(dims, params, state, forcing, out, status, dtype, stream);
  });
}

extern "C" {

const char *lgar_version(void) { return "lgar-hip 0.4 (gfx950)"; }
int32_t lgar_abi_version(void) { return LGAR_ABI_VERSION; }
int32_t lgar_sizeof_dims(void) { return (int32_t)sizeof(LgarDims); }
int32_t lgar_fmax(void) { return LGAR_FMAX; }
int32_t lgar_lmax(void) { return LGAR_LMAX; }
int32_t lgar_cooperating_lanes(const LgarDims *dims, int32_t dtype) {
  if (check_dims(dims) != 0 || (dtype != LGAR_F32 && dtype != LGAR_F64)) return LGAR_E_ARG;
  // (the function forward_plan itself calls, lgar_plan.hpp)
  return dtype == LGAR_F64 ? cooperating_lanes<double>(dims, wave_slots(1)) : cooperating_lanes<float>(dims, wave_slots(1));
}

int32_t lgar_state_init(const LgarDims *dims, const LgarParams *params, LgarState *state, int32_t *status, int32_t dtype,
                        void *stream) {
  int rc = check_dims(dims);
  if (rc) return rc;
  rc = check_state(params, state, status);
  if (rc) return rc;
  return by_layers(dims->n_layers, [&](auto nl) {
    return launch_init_nl<decltype(nl)::value>(dims, params, state, status, dtype, (hipStream_t)stream);
  });
}

int32_t lgar_forward(const LgarDims *dims, const LgarParams *params, LgarState *state, const LgarForcing *forcing,
                     const LgarStepOut *out, int32_t *status, int32_t dtype, void *stream) {
  int rc = check_dims(dims);
  if (rc) return rc;
  rc = check_state(params, state, status);
  if (rc) return rc;
  rc = check_forcing_layout(dims, forcing);
  if (rc) return rc;
  if (dims->n_steps == 0) return 0;  // empty run: nothing to read
  if (!forcing || !forcing->precip || !forcing->pet) return LGAR_E_ARG;
  // basin sums of accumulators whose series this call stores anyway are taken from the stored series afterwards (one pass,
  // fixed summation order); the forward kernels aggregate only what has no series
  LgarStepOut kernel_out;
  uint32_t from_series = 0;
  if (out && out->basin && out->basin_mask) {
    for (int j = 0; j < LGAR_NACC; j++)
      if (((out->basin_mask >> j) & 1u) && out->series[j]) from_series |= 1u << j;
    if (from_series) {
      kernel_out = *out;
      kernel_out.basin_mask &= ~from_series;
      out = &kernel_out;
    }
  }
  rc = forward_by_layers(dims, params, state, forcing, out, status, dtype, (hipStream_t)stream);
  if (rc || !from_series) return rc;
  const long long N = dims->n_columns;
  const int T = dims->n_steps;
  for (int j = 0; j < LGAR_NACC; j++) {
    if (!((from_series >> j) & 1u)) continue;
    double *row = out->basin + (size_t)j * (size_t)T;
    if (dtype == LGAR_F64) launch_basin_reduce<double>(out->series[j], out->weights, row, N, T, (hipStream_t)stream);
    else launch_basin_reduce<float>(out->series[j], out->weights, row, N, T, (hipStream_t)stream);
  }
  return launch_status();
}

#ifndef LGAR_NO_TANGENT
int32_t lgar_forward_tangent(const LgarDims *dims, const LgarParams *params, const LgarParams *direction,
                             const LgarForcing *forcing, const void *w_runoff, const void *w_perc, void *grad_out,
                             void *tangent_runoff, int32_t *status, int32_t dtype, void *stream, uint32_t *tickets) {
  const int rc = check_tangent_call(dims, params, direction, forcing, grad_out, status);
  if (rc) return rc;
  return by_layers(dims->n_layers, [&](auto nl) {
    return launch_tangent_nl<decltype(nl)::value>(dims, params, direction, forcing, w_runoff, w_perc, grad_out, tangent_runoff,
                                                  status, dtype, (hipStream_t)stream, tickets);
  });
}

int32_t lgar_forward_tangent_window(const LgarDims *dims, const LgarParams *params, const LgarParams *direction,
                                    const LgarForcing *forcing, const void *w_runoff, const void *w_perc,
                                    const LgarTangentWindow *window, void *grad_out, void *tangent_runoff, int32_t *status,
                                    int32_t dtype, void *stream, uint32_t *tickets) {
  int rc = check_tangent_call(dims, params, direction, forcing, grad_out, status);
  if (rc) return rc;
  rc = check_window(window);
  if (rc) return rc;
  return by_layers(dims->n_layers, [&](auto nl) {
    return launch_tangent_window_nl<decltype(nl)::value>(dims, params, direction, forcing, w_runoff, w_perc, window, grad_out,
                                                         tangent_runoff, status, dtype, (hipStream_t)stream, tickets);
  });
}

int32_t lgar_forward_tangent_forced(const LgarDims *dims, const LgarParams *params, const LgarParams *direction,
                                    const LgarForcing *forcing, const LgarForcing *dforcing, const void *w_runoff,
                                    const void *w_perc, const LgarTangentWindow *window, void *grad_out, void *tangent_runoff,
                                    int32_t *status, int32_t dtype, void *stream, uint32_t *tickets) {
  int rc = check_tangent_call(dims, params, direction, forcing, grad_out, status);
  if (rc) return rc;
  rc = check_window(window);
  if (rc) return rc;
  rc = check_forcing_direction(dforcing);
  if (rc) return rc;
  return by_layers(dims->n_layers, [&](auto nl) {
    return launch_tangent_forced_nl<decltype(nl)::value>(dims, params, direction, forcing, dforcing, w_runoff, w_perc, window,
                                                         grad_out, tangent_runoff, status, dtype, (hipStream_t)stream, tickets);
  });
}
#endif

int32_t lgar_soil_moisture(const LgarDims *dims, const LgarParams *params, const LgarState *state, const double *edges,
                           int32_t n_bins, int32_t what, void *out, const void *weights, double *basin, int32_t dtype,
                           void *stream) {
  int rc = check_dims(dims);
  if (rc) return rc;
  if (!params || !params->thickness || !state || !state->depth || !state->theta || !state->flags || !state->n_fronts || !out)
    return LGAR_E_ARG;
  if (dtype != LGAR_F32 && dtype != LGAR_F64) return LGAR_E_ARG;
  if (what != 0 && what != 1) return LGAR_E_ARG;
  if (n_bins < 1 || n_bins > LGAR_MOIST_BINS || (!edges && n_bins != dims->n_layers)) return LGAR_E_ARG;
  rc = launch_soil_moisture(dims, params, state, edges, n_bins, what, out, dtype, (hipStream_t)stream);
  if (rc || !basin) return rc;
  // [n_bins][n_columns] has the layout of a [T][n_columns] series: the stored-series pass, with its fixed summation order
  if (dtype == LGAR_F64) launch_basin_reduce<double>(out, weights, basin, dims->n_columns, n_bins, (hipStream_t)stream);
  else launch_basin_reduce<float>(out, weights, basin, dims->n_columns, n_bins, (hipStream_t)stream);
  return launch_status();
}

int32_t lgar_totals_replay(const LgarDims *dims, const LgarStepOut *stored, int32_t n_rows, void *running, int32_t dtype,
                           void *stream) {
  int rc = check_dims(dims);
  if (rc) return rc;
  if (!stored || !running || n_rows < 0 || (dtype != LGAR_F32 && dtype != LGAR_F64)) return LGAR_E_ARG;
  if (n_rows == 0) return 0;
  return launch_totals_replay(dims, stored, n_rows, running, dtype, (hipStream_t)stream);
}

int32_t lgar_catchment_sums(const void *series, int32_t n_rows, int32_t n_columns, const int32_t *offsets, int32_t n_catchments,
                            const int32_t *order, int32_t n_order, const void *weights, const int32_t *status, double *out,
                            double *weight_sums, int32_t dtype, void *stream) {
  if (n_rows < 0 || n_columns < 0 || n_catchments < 0 || !offsets || (order && n_order < 0)) return LGAR_E_ARG;
  // (a job without columns has nothing to read: every sum is +0.0, and an empty series may come as a null pointer)
  if (n_rows > 0 && n_catchments > 0 && (!out || (!series && n_columns > 0))) return LGAR_E_ARG;
  return launch_catchment_sums(series, n_rows, n_columns, offsets, n_catchments, order, n_order, weights, status, out, weight_sums,
                               dtype, (hipStream_t)stream);
}

int32_t lgar_catchment_spread(const double *grad, int32_t n_rows, int32_t n_catchments, const int32_t *catchment_of,
                              int32_t n_columns, const void *weights, const int32_t *status, void *out, int32_t dtype,
                              void *stream) {
  if (n_rows < 0 || n_columns < 0 || n_catchments < 0) return LGAR_E_ARG;
  if (n_rows > 0 && n_columns > 0 && (!catchment_of || !out || (n_catchments > 0 && !grad))) return LGAR_E_ARG;
  return launch_catchment_spread(grad, n_rows, n_catchments, catchment_of, n_columns, weights, status, out, dtype,
                                 (hipStream_t)stream);
}

int32_t lgar_leaf_batch(int32_t op, int32_t n_items, const void *x, const void *y, double z, const void *alpha,
                        const void *n, const void *ksat, const void *theta_e, const void *theta_r, int32_t nint,
                        double wilting_point_psi, void *out, int32_t dtype, void *stream) {
  if (op < 0 || op > LEAF_OP_LAST || n_items <= 0 || !x || !alpha || !n || !ksat || !theta_e || !theta_r || !out) return LGAR_E_ARG;
  if (op >= LEAF_OP_F32_FIRST && dtype != LGAR_F32) return LGAR_E_ARG;  // the fp32 fast mode's arithmetic: float only
  if ((op == 4 || op == 5 || op == 6 || op == 10 || op == 15 || op == 21 || op == 22 || op == 23) && !y) return LGAR_E_ARG;
  const unsigned grid = (unsigned)((n_items + 255) / 256);
  hipStream_t st = (hipStream_t)stream;
  if (dtype == LGAR_F64) {
    LeafArgs<double> a{op, n_items, nint, (const double *)x, (const double *)y, (const double *)alpha, (const double *)n,
                       (const double *)ksat, (const double *)theta_e, (const double *)theta_r, z, wilting_point_psi,
                       (double *)out};
    hipLaunchKernelGGL(lgar_leaf_kernel<double>, dim3(grid), dim3(256), 0, st, a);
  } else if (dtype == LGAR_F32) {
    LeafArgs<float> a{op, n_items, nint, (const float *)x, (const float *)y, (const float *)alpha, (const float *)n,
                      (const float *)ksat, (const float *)theta_e, (const float *)theta_r, (float)z,
                      (float)wilting_point_psi, (float *)out};
    hipLaunchKernelGGL(lgar_leaf_kernel<float>, dim3(grid), dim3(256), 0, st, a);
  } else {
    return LGAR_E_ARG;
  }
  return launch_status();
}

}  // extern "C"
