// lgar_route.hip -- the catchment-routing kernels and their C-ABI entry points (lgar_catchment_route /
// lgar_catchment_route_grad, include/lgar.h; lgar_route.hpp holds the fold, the hand-over and the gradient accumulation).
//
// Route (forward and reverse): lanes run along the catchments -- 64 lanes are one 512-byte row segment of x, y and g[k][.] --
// and one lane owns one output: it folds its K terms oldest first and writes y[r][b] (or, for the K virtual rows behind the
// last one, queue_out[r - T][b]): no atomics, nothing to zero.  The four waves of a workgroup take four consecutive rows of the
// same 64 catchments and the workgroups are numbered segment-fastest, so the K rows of x an output reads are the rows its
// neighbours in flight read too: each is fetched from memory once and re-read from the caches.  The grid is capped and the
// workgroups stride over the (four rows, segment) pairs, so any T x B launches.
// -DLGAR_ROUTE_TILED (a measurement variant, build.build_variant): the tiled shape instead -- a wave owns 64 catchments and a
// tile of rows, walks the rows upward and keeps the last K rows of x in an LDS ring [K rounded up to a power of two][64], so x
// comes from memory once plus a K - 1 row halo per tile.  The same fold, the same bits; DESIGN.md section 12 has both shapes'
// numbers and why the plain one stays.
// Ordinate gradient: one lane per (LGAR_ROUTE_KG ordinates, catchment) walks all rows; workgroups are numbered segment-fastest.
#include <hip/hip_runtime.h>

#include "lgar_host.hpp"
#include "lgar_route.hpp"

namespace lgar {

#define LGAR_ROUTE_GRID_CAP 4096  // workgroups of four waves: twice the chip's 8192 wave slots at 8 waves per SIMD

#ifndef LGAR_ROUTE_TILED
__global__ __launch_bounds__(256) void lgar_catchment_route_kernel(RouteArgs a) {
  const long long lane = (long long)(threadIdx.x & 63u), wave = (long long)(threadIdx.x >> 6);
  const long long rows = route_rows(a);
  const long long segs = (a.B + LGAR_ROUTE_LANES - 1) / LGAR_ROUTE_LANES;
  const long long total = ((rows + 3) / 4) * segs;
  for (long long w = blockIdx.x; w < total; w += gridDim.x) {
    const long long rg = w / segs, seg = w - rg * segs;
    const long long r = rg * 4 + wave, b = seg * LGAR_ROUTE_LANES + lane;
    if (r < rows && b < a.B) route_store(a, r, b, route_fold(a, r, b));
  }
}
#else
// tile_rows: rows of a tile; ring_mask: slots of the ring - 1 (a power of two >= K slots of 64 doubles per wave)
__global__ __launch_bounds__(256) void lgar_catchment_route_kernel(RouteArgs a, long long tile_rows, int ring_mask) {
  extern __shared__ __attribute__((aligned(16))) double route_ring[];
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  double *ring = route_ring + (size_t)wave * (size_t)(ring_mask + 1) * LGAR_ROUTE_LANES + lane;  // this lane's column of it
  const long long rows = route_rows(a);
  const long long segs = (a.B + LGAR_ROUTE_LANES - 1) / LGAR_ROUTE_LANES;
  const long long total = ((rows + tile_rows - 1) / tile_rows) * segs;
  for (long long w = (long long)blockIdx.x * 4 + wave; w < total; w += (long long)gridDim.x * 4) {
    const long long tile = w / segs, seg = w - tile * segs;
    const long long b = seg * LGAR_ROUTE_LANES + lane;
    if (b >= a.B) continue;  // (a lane reads and writes only its own column of the ring: the wave needs no barrier)
    const long long r0 = tile * tile_rows, r1 = r0 + tile_rows < rows ? r0 + tile_rows : rows;
    const double *x = a.x + b;
    for (long long j = r0 - (a.K - 1) < 0 ? 0 : r0 - (a.K - 1); j < r0 && j < a.T; j++)  // the halo
      ring[(size_t)(j & ring_mask) * LGAR_ROUTE_LANES] = x[j * a.x_stride];
    for (long long r = r0; r < r1; r++) {
      if (r < a.T) ring[(size_t)(r & ring_mask) * LGAR_ROUTE_LANES] = x[r * a.x_stride];
      route_store(a, r, b, route_fold(a, r, b, [ring, ring_mask](long long j) { return ring[(size_t)(j & ring_mask) * LGAR_ROUTE_LANES]; }));
    }
  }
}
#endif

struct RouteGradArgs {
  const double *x, *gy;
  double *g_out;
  long long T, B;
  int K;
};

__global__ __launch_bounds__(256) void lgar_catchment_route_grad_kernel(RouteGradArgs a) {
  const long long lane = (long long)(threadIdx.x & 63u), wave = (long long)(threadIdx.x >> 6);
  const long long segs = (a.B + LGAR_ROUTE_LANES - 1) / LGAR_ROUTE_LANES;
  const long long groups = (a.K + LGAR_ROUTE_KG - 1) / LGAR_ROUTE_KG;
  const long long total = ((groups + 3) / 4) * segs;
  for (long long w = blockIdx.x; w < total; w += gridDim.x) {
    const long long gq = w / segs, seg = w - gq * segs;
    const long long k0 = (gq * 4 + wave) * LGAR_ROUTE_KG, b = seg * LGAR_ROUTE_LANES + lane;
    if (k0 >= a.K || b >= a.B) continue;
    double acc[LGAR_ROUTE_KG];
    route_grad_lane<LGAR_ROUTE_KG>(a.x, a.gy, a.T, a.B, b, k0, acc);
#pragma unroll
    for (int j = 0; j < LGAR_ROUTE_KG; j++)
      if (k0 + j < a.K) a.g_out[(size_t)(k0 + j) * (size_t)a.B + (size_t)b] = acc[j];
  }
}

int launch_catchment_route(const double *x, int n_rows, int n_catchments, const double *ordinates, int n_ordinates,
                           int per_catchment, const double *queue_in, double *queue_out, double *y, int reverse,
                           hipStream_t stream) {
  if (n_catchments == 0) return 0;
  const RouteArgs a = route_args(x, n_rows, n_catchments, ordinates, n_ordinates, per_catchment != 0, queue_in, queue_out, y, reverse != 0);
  const long long rows = route_rows(a);
  if (rows == 0) return 0;
  const long long segs = ((long long)n_catchments + LGAR_ROUTE_LANES - 1) / LGAR_ROUTE_LANES;
#ifndef LGAR_ROUTE_TILED
  const long long blocks = ((rows + 3) / 4) * segs;
  const dim3 grid((unsigned)(blocks < LGAR_ROUTE_GRID_CAP ? blocks : LGAR_ROUTE_GRID_CAP));
  hipLaunchKernelGGL(lgar_catchment_route_kernel, grid, dim3(256), 0, stream, a);
#else
  // tiles as long as still leave the chip about 4096 waves, and no shorter than 8 rows (a tile re-reads K - 1 rows of halo)
  int slots = 1;
  while (slots < n_ordinates) slots *= 2;
  const long long tiles_wanted = (4096 + segs - 1) / segs;
  long long tile_rows = (rows + tiles_wanted - 1) / tiles_wanted;
  if (tile_rows < 8) tile_rows = 8;
  const long long blocks = (((rows + tile_rows - 1) / tile_rows) * segs + 3) / 4;
  const dim3 grid((unsigned)(blocks < LGAR_ROUTE_GRID_CAP ? blocks : LGAR_ROUTE_GRID_CAP));
  const size_t lds = (size_t)4 * slots * LGAR_ROUTE_LANES * sizeof(double);  // 128 KB at K = 64: beyond the 64 KB default
  if (hipFuncSetAttribute((const void *)lgar_catchment_route_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return LGAR_E_LAUNCH;
  hipLaunchKernelGGL(lgar_catchment_route_kernel, grid, dim3(256), lds, stream, a, tile_rows, slots - 1);
#endif
  return launch_status();
}

int launch_catchment_route_grad(const double *x, const double *gy, int n_rows, int n_catchments, int n_ordinates, double *g_out,
                                hipStream_t stream) {
  if (n_catchments == 0) return 0;
  RouteGradArgs a;
  a.x = x;
  a.gy = gy;
  a.g_out = g_out;
  a.T = n_rows;
  a.B = n_catchments;
  a.K = n_ordinates;
  const long long segs = ((long long)n_catchments + LGAR_ROUTE_LANES - 1) / LGAR_ROUTE_LANES;
  const long long groups = (n_ordinates + LGAR_ROUTE_KG - 1) / LGAR_ROUTE_KG;
  const long long blocks = ((groups + 3) / 4) * segs;
  const dim3 grid((unsigned)(blocks < LGAR_ROUTE_GRID_CAP ? blocks : LGAR_ROUTE_GRID_CAP));
  hipLaunchKernelGGL(lgar_catchment_route_grad_kernel, grid, dim3(256), 0, stream, a);
  return launch_status();
}

}  // namespace lgar

// The C-ABI entry points live here, not with the other wrappers in lgar_kernels.hip: the forward translation units stay
// byte-identical.
extern "C" {

int32_t lgar_catchment_route(const double *x, int32_t n_rows, int32_t n_catchments, const double *ordinates,
                             int32_t n_ordinates, int32_t per_catchment, const double *queue_in, double *queue_out, double *y,
                             int32_t reverse, void *stream) {
  if (n_rows < 0 || n_catchments < 0 || n_ordinates < 1 || n_ordinates > LGAR_ROUTE_KMAX || !ordinates) return LGAR_E_ARG;
  if (n_rows > 0 && n_catchments > 0 && (!x || !y)) return LGAR_E_ARG;
  if (reverse && (queue_in || queue_out)) return LGAR_E_ARG;
  return lgar::launch_catchment_route(x, n_rows, n_catchments, ordinates, n_ordinates, per_catchment, queue_in, queue_out, y, reverse,
                                      (hipStream_t)stream);
}

int32_t lgar_catchment_route_grad(const double *x, const double *gy, int32_t n_rows, int32_t n_catchments, int32_t n_ordinates,
                                  double *g_out, void *stream) {
  if (n_rows < 0 || n_catchments < 0 || n_ordinates < 1 || n_ordinates > LGAR_ROUTE_KMAX) return LGAR_E_ARG;
  if (n_catchments > 0 && (!g_out || (n_rows > 0 && (!x || !gy)))) return LGAR_E_ARG;
  return lgar::launch_catchment_route_grad(x, gy, n_rows, n_catchments, n_ordinates, g_out, (hipStream_t)stream);
}

}  // extern "C"
