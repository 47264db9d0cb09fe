// lgar_network.hip -- the catchment-network kernels and their C-ABI entry points (lgar_network_route / lgar_network_route_grad,
// include/lgar.h; lgar_network.hpp holds the per-reach walk, the inflow fold, the adjoint step, the clamps and the refusals).
//
// One launch per level of the network, on the caller's stream: a reach reads the discharge of reaches of lower levels only (the
// adjoint: the gradient of its downstream reach, of a higher level), so the order of the launches on the stream is the only
// dependence between levels.  No flags, no waiting between workgroups, no cooperative launch.  Within a level lane p owns reach
// order[p] and walks all rows: 64 lanes are 64 reaches of the level, and with catchments numbered in level order their loads
// and stores are 512-byte row segments.  Workgroups of 256 lanes; the grid is capped and the lanes stride over the level, so a
// level of any width launches.  An empty level launches nothing.  level_ptr is read HERE, on the host, to size the launches.
// The weak spot: near the outlets a level is narrower than a wave, down to one lane walking T rows.
#include <hip/hip_runtime.h>

#include "lgar_host.hpp"
#include "lgar_network.hpp"

namespace lgar {

#define LGAR_NET_GRID_CAP 4096  // workgroups of four waves, as LGAR_ROUTE_GRID_CAP

__global__ __launch_bounds__(256) void lgar_network_route_kernel(NetArgs a, long long p0, long long p1) {
  for (long long p = p0 + (long long)blockIdx.x * 256 + threadIdx.x; p < p1; p += (long long)gridDim.x * 256)
    net_walk(a, net_reach(a.order, p, a.B));
}

template <bool GC> __global__ __launch_bounds__(256) void lgar_network_grad_kernel(NetGradArgs a, long long p0, long long p1) {
  for (long long p = p0 + (long long)blockIdx.x * 256 + threadIdx.x; p < p1; p += (long long)gridDim.x * 256)
    net_walk_back<GC>(a, net_reach(a.order, p, a.B));
}

static dim3 level_grid(long long width) {
  const long long blocks = (width + 255) / 256;
  return dim3((unsigned)(blocks < LGAR_NET_GRID_CAP ? blocks : LGAR_NET_GRID_CAP));
}

int launch_network_route(const NetArgs &a, const int32_t *level_ptr, int n_levels, hipStream_t stream) {
  for (int l = 0; l < n_levels; l++) {
    const long long p0 = level_ptr[l], p1 = level_ptr[l + 1];
    if (p1 > p0) hipLaunchKernelGGL(lgar_network_route_kernel, level_grid(p1 - p0), dim3(256), 0, stream, a, p0, p1);
  }
  return launch_status();
}

int launch_network_grad(const NetGradArgs &a, const int32_t *level_ptr, int n_levels, hipStream_t stream) {
  for (int l = n_levels - 1; l >= 0; l--) {
    const long long p0 = level_ptr[l], p1 = level_ptr[l + 1];
    if (p1 <= p0) continue;
    if (a.gc) hipLaunchKernelGGL(lgar_network_grad_kernel<true>, level_grid(p1 - p0), dim3(256), 0, stream, a, p0, p1);
    else hipLaunchKernelGGL(lgar_network_grad_kernel<false>, level_grid(p1 - p0), dim3(256), 0, stream, a, p0, p1);
  }
  return launch_status();
}

}  // namespace lgar

// The C-ABI entry points live here, not with the other wrappers in lgar_kernels.hip: the forward translation units stay
// byte-identical.
extern "C" {

int32_t lgar_network_route(const double *x, int32_t n_rows, int32_t n_catchments, const double *coef, const int32_t *up_ptr,
                           const int32_t *up_idx, int32_t n_edges, const int32_t *order, const int32_t *level_ptr, int32_t n_levels,
                           const double *state_in, double *state_out, double *y, void *stream) {
  const int rc = lgar::net_route_check(x, n_rows, n_catchments, coef, up_ptr, up_idx, n_edges, order, level_ptr, n_levels, state_out, y);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::NetArgs a;
  a.x = x, a.coef = coef, a.state_in = state_in, a.y = y, a.state_out = state_out;
  a.order = order, a.up_ptr = up_ptr, a.up_idx = up_idx;
  a.T = n_rows, a.B = n_catchments, a.E = n_edges;
  return lgar::launch_network_route(a, level_ptr, n_levels, (hipStream_t)stream);
}

int32_t lgar_network_route_grad(const double *gy, int32_t n_rows, int32_t n_catchments, const double *coef, const int32_t *down,
                                const int32_t *order, const int32_t *level_ptr, int32_t n_levels, double *gx, const double *x,
                                const double *y, const int32_t *up_ptr, const int32_t *up_idx, int32_t n_edges,
                                const double *state_in, double *gc, void *stream) {
  const int rc = lgar::net_grad_check(gy, n_rows, n_catchments, coef, down, order, level_ptr, n_levels, gx, x, y, up_ptr, up_idx, n_edges, gc);
  if (rc != 0) return rc < 0 ? rc : 0;
  lgar::NetGradArgs a;
  a.gy = gy, a.coef = coef, a.x = x, a.y = y, a.state_in = state_in, a.gx = gx, a.gc = gc;
  a.order = order, a.down = down, a.up_ptr = up_ptr, a.up_idx = up_idx;
  a.T = n_rows, a.B = n_catchments, a.E = n_edges;
  return lgar::launch_network_grad(a, level_ptr, n_levels, (hipStream_t)stream);
}

}  // extern "C"
