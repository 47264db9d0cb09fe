// lgar_tangent_window_nl.hip -- the resumable tangent kernels (lgar_forward_tangent_window) for ONE soil-layer count (compiled
// with -DLGAR_NL=<n>): tangent_lane<..., WINDOW = true> of lgar_tangent_body.hpp, which starts from a carried state and stores
// the end state.  A translation unit of its own: the kernels of lgar_tangent_nl.hip are compiled from what they were compiled
// from before the window existed.  Same plan (tangent_plan), same launch shape, same persistent-wave loop, same occupancy rule.
#include <hip/hip_runtime.h>

#include "lgar_host.hpp"
#include "lgar_launch.hpp"
#include "lgar_tangent_body.hpp"

#ifndef LGAR_NL
#error "compile with -DLGAR_NL=<number of soil layers>"
#endif

namespace lgar {

// (lgar_tangent_nl.hip TangentOccupancy: the 8-front fp32 kernel is held to two waves per SIMD, the others run one)
#ifndef LGAR_TAN_F32_WAVES
#define LGAR_TAN_F32_WAVES 2
#endif
template <typename R, int CAP> struct WindowOccupancy {
  static constexpr int waves = (ScalarKind<R>::f32 && CAP == LGAR_CAP_SMALL) ? LGAR_TAN_F32_WAVES : 1;
};
template <typename R, int NL, int CAP, int MODE>
__global__ __launch_bounds__(WAVE, (WindowOccupancy<R, CAP>::waves)) void lgar_tangent_window_kernel(TWArgs<R> a) {
  __shared__ WaveLDS<Dual<R>, CAP, 1> lds;
  __shared__ R xchg[LGAR_XCHG_WORDS];
  const int lane = threadIdx.x;
  // the argument block is read in place (kernarg segment), see LGAR_KARG in lgar_scalar.hpp
  const LGAR_KARG TWArgs<R> *wa = (const LGAR_KARG TWArgs<R> *)__builtin_amdgcn_kernarg_segment_ptr();
  const LGAR_KARG TArgs<R> *ap = &wa->a;
  if (ap->pending_in != nullptr && *ap->pending_in == 0u) return;  // no column was handed over to this kernel
  const size_t N = (size_t)ap->N;
  unsigned *ticket = ap->ticket;
  const unsigned cpb = columns_per_block(ap->share);
  const unsigned nblocks = (unsigned)((N + cpb - 1) / cpb);
  for (bool first = true;; first = false) {
    unsigned blk = blockIdx.x;
    if (ticket != nullptr) {
      if (lane == 0) blk = atomicAdd(ticket, 1u);
      blk = __builtin_amdgcn_readfirstlane(blk);
      if (blk >= nblocks) break;
    } else if (!first) {
      break;
    }
    const size_t c = (size_t)blk * cpb + lane;
    // (c < N bounds every access of the lane: the state arrays are [rows][N] with rows <= front_slots, read and written at
    // [i * N + c], i < min(n_fronts, front_slots))
    if ((unsigned)lane < cpb && c < N) tangent_lane<R, NL, CAP, MODE, true>(ap, c, lane, lds, &xchg[0], &wa->w);
  }
}

template <typename R, int NL, int CAP, int MODE>
static void launch_one(TWArgs<R> &a, unsigned nblocks, unsigned *ticket, hipStream_t st) {
  a.a.ticket = ticket;
  unsigned grid = nblocks;
  if (ticket != nullptr) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      cus = 256;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, lgar_tangent_window_kernel<R, NL, CAP, MODE>, WAVE, 0) != hipSuccess || per_cu <= 0)
      per_cu = 4;
    const unsigned slots = (unsigned)cus * (unsigned)per_cu;
    grid = nblocks < slots ? nblocks : slots;
  }
  hipLaunchKernelGGL((lgar_tangent_window_kernel<R, NL, CAP, MODE>), dim3(grid), dim3(WAVE), 0, st, a);
}

template <typename R, int NL>
static int window_typed(const LgarDims *dims, const LgarParams *params, const LgarParams *direction, const LgarForcing *forcing,
                        const void *w_runoff, const void *w_perc, const LgarTangentWindow *window, void *grad_out,
                        void *tangent_runoff, int32_t *status, hipStream_t st, unsigned *tickets) {
  if (tickets != nullptr && hipMemsetAsync(tickets, 0, LGAR_NTICKETS * sizeof(unsigned), st) != hipSuccess) return LGAR_E_LAUNCH;
  TWArgs<R> a = make_twargs<R>(dims, params, direction, forcing, w_runoff, w_perc, window, grad_out, tangent_runoff, status);
  const TangentPlan plan = tangent_plan(dims, NL);
  for (int i = 0; i < plan.n; i++) {
    unsigned *tk = chain_step(a.a, i, plan.n, tickets);
    if (plan.literal) launch_one<R, NL, LGAR_FMAX, MODE_LITERAL>(a, plan.blocks, tk, st);
    else if (plan.caps[i] == LGAR_CAP_SMALL) launch_one<R, NL, LGAR_CAP_SMALL, MODE_FAST>(a, plan.blocks, tk, st);
    else launch_one<R, NL, LGAR_FMAX, MODE_FAST>(a, plan.blocks, tk, st);
    const int rc = launch_status();
    if (rc) return rc;
  }
  return 0;
}

template <int NL>
int launch_tangent_window_nl(const LgarDims *dims, const LgarParams *params, const LgarParams *direction, const LgarForcing *forcing,
                             const void *w_runoff, const void *w_perc, const LgarTangentWindow *window, void *grad_out,
                             void *tangent_runoff, int32_t *status, int dtype, hipStream_t st, unsigned *tickets) {
  if (dtype == LGAR_F64)
    return window_typed<double, NL>(dims, params, direction, forcing, w_runoff, w_perc, window, grad_out, tangent_runoff, status, st, tickets);
  if (dtype == LGAR_F32)
    return window_typed<float, NL>(dims, params, direction, forcing, w_runoff, w_perc, window, grad_out, tangent_runoff, status, st, tickets);
  return LGAR_E_ARG;
}

template int launch_tangent_window_nl<LGAR_NL>(const LgarDims *, const LgarParams *, const LgarParams *, const LgarForcing *,
                                               const void *, const void *, const LgarTangentWindow *, void *, void *, int32_t *,
                                               int, hipStream_t, unsigned *);

}  // namespace lgar
