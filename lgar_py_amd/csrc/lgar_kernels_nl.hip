// lgar_kernels_nl.hip -- gfx950 forward / init kernels for ONE soil-layer count (compiled with -DLGAR_NL=<n>).
//
// Launch geometry: one 64-thread workgroup == one wavefront == 64 soil columns; a grid of ceil(N/64) workgroups
// (>> 256 CUs for the 1M-column configs).  One-wave workgroups keep the LDS allocation per wave, so the number of
// resident waves per CU is set by LDS (front tables) and VGPRs alone, and no barrier is ever needed: lanes never share
// data.  Occupancy by front capacity (fp32): 8 slots = 8.7 KB LDS/wave and <= 128 VGPRs -> 4 waves/SIMD, which also
// makes the 1M-column grid (16 384 waves) exactly 4 rounds of the chip's 4 096 wave slots; 16 / 32 slots serve the
// (rare) columns handed over by the capacity chain (lgar_forward_body.hpp).
//
// HBM traffic per launch (all coalesced, column-fastest): parameters 6*L*N, front state 2*(5*n_fronts+1)*N,
// scalars/totals, and per forcing step 2 loads + (number of requested series) stores per column.
#include <hip/hip_runtime.h>

#include "lgar_forward_body.hpp"
#include "lgar_host.hpp"
#include "lgar_launch.hpp"

#ifndef LGAR_NL
#error "compile with -DLGAR_NL=<number of soil layers>"
#endif

namespace lgar {

// waves per SIMD the register allocator has to make room for
#ifndef LGAR_OCC_F32_SMALL
#define LGAR_OCC_F32_SMALL 4
#endif
#ifndef LGAR_OCC_F64_SMALL
#define LGAR_OCC_F64_SMALL 2
#endif
template <typename R, int CAP> struct Occupancy {
  static constexpr int waves = ScalarKind<R>::f32 ? ((CAP <= LGAR_CAP_SMALL) ? LGAR_OCC_F32_SMALL : ((CAP <= LGAR_CAP_MID) ? 2 : 1))
                                                : ((CAP <= LGAR_CAP_SMALL) ? LGAR_OCC_F64_SMALL : 1);
};

template <typename R, int NL, int CAP>
__global__ __launch_bounds__(WAVE) void lgar_init_kernel(KArgs<R> a) {
  __shared__ WaveLDS<R, CAP> lds;
  const int lane = threadIdx.x;
  const size_t c = (size_t)blockIdx.x * WAVE + lane;
  if (c >= (size_t)a.N) return;
  init_lane<R, NL, CAP>((const LGAR_KARG KArgs<R> *)__builtin_amdgcn_kernarg_segment_ptr(), c, lane, lds);
}

// LDS tables through which cooperating lanes exchange trapezoid heads and nodes (lgar_geff.hpp geff_nodes_cooperative,
// geff_mixed_core<true>), sweep thetas and mass evaluations: one per group of lanes, in the cooperating-lanes kernels only
// (MODE_COOP: native double-precision trapezoid, MODE_MIXED_COOP: mixed-precision trapezoid).  With the front table kept once per group as
// well, a 32-front wave of such a kernel takes 34 KB of LDS (front table 17 KB, these tables 16.6 KB, the groups' sums): four
// waves per CU, one per SIMD -- all a cooperating job may have.
template <typename R, int MODE> struct CoopLDS {
  static constexpr bool on = ModeTraits<R, MODE>::coop_f64;
  R tab[on ? LGAR_COOP_GROUPS : 1][on ? LGAR_COOP_TAB_ROW : 1];
};

// Every forward kernel exists twice: as it always was, and reading its forcing through LgarForcing.column_map.  The index is
// one load per column before the time loop, but one kernel with both paths ran 1 % slower WITHOUT a map (measured: fp32
// 11.88 -> 12.00 ms, mixed precision 28.51 -> 28.73 ms, through register allocation alone), so the map is a compile-time
// matter and the two kernels share their text (lgar_forward_wave.hpp).
template <typename R, int NL, int CAP, int MODE>
__global__ __launch_bounds__(WAVE, (Occupancy<R, CAP>::waves)) void lgar_forward_kernel(KArgs<R> a) {
  __shared__ ForwardLDS<R, CAP, MODE> lds;
  __shared__ CoopLDS<R, MODE> coop_lds;
#define LGAR_FORWARD_MAPPED 0
#include "lgar_forward_wave.hpp"
#undef LGAR_FORWARD_MAPPED
}
template <typename R, int NL, int CAP, int MODE>
__global__ __launch_bounds__(WAVE, (Occupancy<R, CAP>::waves)) void lgar_forward_mapped_kernel(KArgs<R> a) {
  __shared__ ForwardLDS<R, CAP, MODE> lds;
  __shared__ CoopLDS<R, MODE> coop_lds;
#define LGAR_FORWARD_MAPPED 1
#include "lgar_forward_wave.hpp"
#undef LGAR_FORWARD_MAPPED
}

template <typename R, int NL>
static int init_typed(const LgarDims *dims, const LgarParams *params, LgarState *state, int32_t *status, hipStream_t st) {
  const unsigned grid = (unsigned)((dims->n_columns + WAVE - 1) / WAVE);
  KArgs<R> a = make_args<R>(dims, params, state, nullptr, nullptr, status);
  hipLaunchKernelGGL((lgar_init_kernel<R, NL, LGAR_CAP_SMALL>), dim3(grid), dim3(WAVE), 0, st, a);
  return launch_status();
}

template <typename R, int NL, int CAP, int MODE>
static void launch_forward_kernel(KArgs<R> &a, unsigned nblocks, unsigned *ticket, hipStream_t st) {
  a.ticket = ticket;
  if (!CoopLDS<R, MODE>::on) a.coop = 1;
  const unsigned cpb = (unsigned)(WAVE / a.coop);  // columns per wavefront
  nblocks = (unsigned)(((size_t)a.N + cpb - 1) / cpb);
  unsigned grid = nblocks;
  if (ticket != nullptr) {
    const unsigned slots = wave_slots(Occupancy<R, CAP>::waves);
    grid = nblocks < slots ? nblocks : slots;
  }
  if (a.fmap != nullptr) hipLaunchKernelGGL((lgar_forward_mapped_kernel<R, NL, CAP, MODE>), dim3(grid), dim3(WAVE), 0, st, a);
  else hipLaunchKernelGGL((lgar_forward_kernel<R, NL, CAP, MODE>), dim3(grid), dim3(WAVE), 0, st, a);
}

// fast-mode kernel of capacity CAP: MODE_FAST, or -- double precision with LgarDims.geff_mode = 1 -- MODE_MIXED (mixed-precision
// trapezoid, lgar_geff.hpp geff_mixed)
template <typename R, int NL, int CAP>
static void launch_fast_kernel(KArgs<R> &a, unsigned nblocks, unsigned *ticket, hipStream_t st, bool mixed) {
  if constexpr (ScalarKind<R>::f64) {
    if (mixed) {
      if (a.coop > 1) {  // cooperating lanes with the mixed-precision trapezoid: the 32-front kernel only, as MODE_COOP
        if constexpr (CAP == LGAR_FMAX) launch_forward_kernel<R, NL, CAP, MODE_MIXED_COOP>(a, nblocks, ticket, st);
        return;
      }
      launch_forward_kernel<R, NL, CAP, MODE_MIXED>(a, nblocks, ticket, st);
      return;
    }
  }
#if defined(LGAR_MEASURE) && defined(LGAR_ONLY_MIXED)  // measurement builds that compile the mixed-precision kernels only
  (void)nblocks; (void)ticket; (void)st;
#else
  if constexpr (ScalarKind<R>::f64) {
    if (a.coop > 1) {  // cooperating lanes: the 32-front kernel, whose LDS is per group of lanes (forward_typed)
      if constexpr (CAP == LGAR_FMAX) launch_forward_kernel<R, NL, CAP, MODE_COOP>(a, nblocks, ticket, st);
      return;
    }
  }
  (void)mixed;
  launch_forward_kernel<R, NL, CAP, MODE_FAST>(a, nblocks, ticket, st);
#endif
}

// One lgar_forward call: the argument block, the plan (lgar_plan.hpp: the front-capacity chain), one launch per kernel of it.
template <typename R, int NL>
static int forward_typed(const LgarDims *dims, const LgarParams *params, LgarState *state, const LgarForcing *forcing,
                         const LgarStepOut *out, int32_t *status, hipStream_t st) {
  const unsigned grid = (unsigned)((dims->n_columns + WAVE - 1) / WAVE);
  KArgs<R> a = make_args<R>(dims, params, state, forcing, out, status);
  unsigned *tickets = state->tickets;
  if (tickets != nullptr && hipMemsetAsync(tickets, 0, LGAR_NTICKETS * sizeof(unsigned), st) != hipSuccess) return LGAR_E_LAUNCH;
  const ForwardPlan plan = forward_plan<R>(dims, NL, wave_slots(1));
  a.coop = plan.coop;
  for (int i = 0; i < plan.n; i++) {
    unsigned *tk = chain_step(a, i, plan.n, tickets);
#if !(defined(LGAR_MEASURE) && (defined(LGAR_ONLY_MIXED) || defined(LGAR_ONLY_F32)))
    if (plan.literal) {
      launch_forward_kernel<R, NL, LGAR_FMAX, MODE_LITERAL>(a, grid, tk, st);
      return launch_status();
    }
#endif
    switch (plan.caps[i]) {
      case LGAR_CAP_SMALL: launch_fast_kernel<R, NL, LGAR_CAP_SMALL>(a, grid, tk, st, plan.mixed); break;
      case LGAR_CAP_MID: launch_fast_kernel<R, NL, LGAR_CAP_MID>(a, grid, tk, st, plan.mixed); break;
      default: launch_fast_kernel<R, NL, LGAR_FMAX>(a, grid, tk, st, plan.mixed); break;
    }
    const int rc = launch_status();
    if (rc) return rc;
  }
  return 0;
}

template <int NL>
int launch_init_nl(const LgarDims *dims, const LgarParams *params, LgarState *state, int32_t *status, int dtype, hipStream_t st) {
  if (dtype == LGAR_F64) return init_typed<double, NL>(dims, params, state, status, st);
  if (dtype == LGAR_F32) return init_typed<float, NL>(dims, params, state, status, st);
  return LGAR_E_ARG;
}
template <int NL>
int launch_forward_nl(const LgarDims *dims, const LgarParams *params, LgarState *state, const LgarForcing *forcing,
                      const LgarStepOut *out, int32_t *status, int dtype, hipStream_t st) {
#if !(defined(LGAR_MEASURE) && defined(LGAR_ONLY_F32))  // (measurement builds of the fp32 kernels alone)
  if (dtype == LGAR_F64) return forward_typed<double, NL>(dims, params, state, forcing, out, status, st);
#endif
  if (dtype == LGAR_F32) return forward_typed<float, NL>(dims, params, state, forcing, out, status, st);
  return LGAR_E_ARG;
}

#if defined(LGAR_MEASURE) && defined(LGAR_COUNT_GEFFM_REGIONS)
// measurement builds that count: read (and zero) the debug counters of this translation unit (lgar_measure.hpp).  Like the
// clocks below it exists once per layer count's unit, so only in the one-layer-count builds that use it (build.py build_variant)
extern "C" int lgar_debug_counters(unsigned long long *out, int reset) {
  unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(lgar_dbg_counters), sizeof(z)) != hipSuccess) return -1;
  if (reset && hipMemcpyToSymbol(HIP_SYMBOL(lgar_dbg_counters), z, sizeof(z)) != hipSuccess) return -1;
  return 0;
}
#endif

#if defined(LGAR_MEASURE) && defined(LGAR_CLOCKS)
extern "C" int lgar_debug_clocks(unsigned long long *out, int reset) {
  unsigned long long z[64] = {0};
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(lgar_dbg_clk), sizeof(z)) != hipSuccess) return -1;
  if (reset && hipMemcpyToSymbol(HIP_SYMBOL(lgar_dbg_clk), z, sizeof(z)) != hipSuccess) return -1;
  return 0;
}
#endif

template int launch_init_nl<LGAR_NL>(const LgarDims *, const LgarParams *, LgarState *, int32_t *, int, hipStream_t);
template int launch_forward_nl<LGAR_NL>(const LgarDims *, const LgarParams *, LgarState *, const LgarForcing *,
                                        const LgarStepOut *, int32_t *, int, hipStream_t);

}  // namespace lgar
