// lgar_moisture.hpp -- soil-moisture output: the water a column's front table holds in depth bins.
//
// The theta profile implied by a front table is piecewise constant.  Fronts are stored top -> bottom; front j has depth d_j,
// water content theta_j and layer tag k_j, and reaches up to t_j = d_{j-1} when front j-1 carries the same layer tag, else to
// the top of layer k_j (0 for layer 0, else the sum of the thicknesses above it).  For a depth bin [a, b]
//
//     S(a, b) = sum_{j = 0 .. nf-1}  theta_j * ( clip(d_j, a, b) - clip(t_j, a, b) ),      clip(x, a, b) = min(max(x, a), b)
//
// summed in that order with plain multiplies and adds (the library is built with -ffp-contract=off).  Widths are SIGNED: the
// reference leaves a column's depths transiently non-monotone in a few steps (a front has overtaken the one below it and the
// merge happens in the next step), and signed widths are what its Layer.mass_balance (layers/Layer.py:795-824) implies -- the
// bins that cover a column then still sum to ending_volume.  With Z the column's total thickness a bin's in-column width is
// w = clip(Z, a, b) - a; the mean volumetric water content is S / w, NaN when w <= 0 (the bin lies wholly below the column;
// S is 0 there).
//
// All arithmetic is fp64 whatever the engine's dtype (fp32 inputs convert exactly); layer tops are the sequential fp64 sum of the
// thicknesses; the result is rounded once to the output dtype.  It is therefore a pure function of the stored state.
//
// Like the other device headers this one also compiles for the host with -DLGAR_DEVSIM (one lane at a time, "any lane of
// the wave" = this lane): tests/moisture_host runs it over the reference's own front tables.
#pragma once
#ifndef LGAR_DEVSIM
#include <hip/hip_runtime.h>
#define LGAR_MOIST_FN __device__ __forceinline__
#else
#define LGAR_MOIST_FN inline
#endif
#include <stddef.h>
#include <stdint.h>

#include "../../include/lgar.h"

namespace lgar {

#define LGAR_MOIST_THETA 0    /* `what`: mean volumetric water content of the bin */
#define LGAR_MOIST_STORAGE 1  /* `what`: water stored in the bin, cm */

#ifndef LGAR_DEVSIM
LGAR_MOIST_FN bool moist_any_lane(bool p) { return __ballot(p) != 0ull; }
#else
LGAR_MOIST_FN bool moist_any_lane(bool p) { return p; }
#endif

LGAR_MOIST_FN double moist_clip(double x, double a, double b) {
  x = x < a ? a : x;
  return x > b ? b : x;
}

// The bins' water of ONE column.  R: element type of the state and parameter arrays (column-fastest: element [row][c] of an
// array with N columns is p[row * N + c]).  NB: compiled bin capacity, n_bins <= NB of it in use (n_bins is the same for every
// lane, so the guards below are scalar branches and S stays in registers: every index into it is a compile-time constant).
// LAYER_BINS: the bins are the column's own soil layers (n_bins == n_layers), else edges[0 .. n_bins] (the same for all columns).
// Each front row (depth, theta, flags) is read once, while any lane of the wave still has a front in it: the loads of a row are
// lane-contiguous.  Memory safety before meaning: n_fronts is clamped to [0, front_slots] and layer tags to [0, n_layers - 1],
// so whatever a faulted column left behind cannot index out of bounds.
template <typename R, int NB, bool LAYER_BINS>
LGAR_MOIST_FN void moist_column(const R *depth, const R *theta, const uint8_t *flags, const int32_t *n_fronts, const R *thickness,
                                const double *edges, size_t N, size_t c, int n_layers, int front_slots, int n_bins, int what,
                                R *out) {
  static_assert(!LAYER_BINS || NB >= LGAR_LMAX, "layer bins need a bin per layer");
  // layer tops: top[l] = thickness[0] + ... + thickness[l-1], top[n_layers] = Z (entries beyond it repeat Z)
  double top[LGAR_LMAX + 1];
  top[0] = 0.0;
#pragma unroll
  for (int l = 0; l < LGAR_LMAX; l++) top[l + 1] = l < n_layers ? top[l] + (double)thickness[(size_t)l * N + c] : top[l];
  const double Z = top[LGAR_LMAX];
  double e[NB + 1];
#pragma unroll
  for (int i = 0; i <= NB; i++) {
    if constexpr (LAYER_BINS) e[i] = top[i < LGAR_LMAX ? i : LGAR_LMAX];
    else e[i] = i <= n_bins ? edges[i] : 0.0;
  }
  double S[NB];
#pragma unroll
  for (int i = 0; i < NB; i++) S[i] = 0.0;

  int nf = n_fronts[c];
  nf = nf < 0 ? 0 : (nf > front_slots ? front_slots : nf);
  double prev_d = 0.0;
  int prev_k = -1;
  for (int j = 0; moist_any_lane(j < nf); j++) {
    if (j < nf) {
      const size_t at = (size_t)j * N + c;
      const double d = (double)depth[at];
      const double th = (double)theta[at];
      int k = (int)(flags[at] & 0x7Fu);
      k = k > n_layers - 1 ? n_layers - 1 : k;
      double t = 0.0;  // top of layer k
#pragma unroll
      for (int l = 1; l < LGAR_LMAX; l++) t = k >= l ? top[l] : t;
      t = k == prev_k ? prev_d : t;
#pragma unroll
      for (int i = 0; i < NB; i++)
        if (i < n_bins) S[i] = S[i] + th * (moist_clip(d, e[i], e[i + 1]) - moist_clip(t, e[i], e[i + 1]));
      prev_d = d;
      prev_k = k;
    }
  }
#pragma unroll
  for (int i = 0; i < NB; i++) {
    if (i < n_bins) {
      double r = S[i];
      if (what == LGAR_MOIST_THETA) {
        const double w = moist_clip(Z, e[i], e[i + 1]) - e[i];
        r = w > 0.0 ? S[i] / w : __builtin_nan("");
      }
      out[(size_t)i * N + c] = (R)r;
    }
  }
}

#ifndef LGAR_DEVSIM
// host-side launch (lgar_moisture.hip); arguments already checked by lgar_soil_moisture (lgar_kernels.hip).  Returns 0 / LGAR_E_*.
int launch_soil_moisture(const LgarDims *dims, const LgarParams *params, const LgarState *state, const double *edges,
                         int n_bins, int what, void *out, int dtype, hipStream_t stream);
// lgar_totals_replay (include/lgar.h): the one-call summation order of the run totals over series stored chunk by chunk
int launch_totals_replay(const LgarDims *dims, const LgarStepOut *stored, int n_rows, void *running, int dtype, hipStream_t stream);
#endif

}  // namespace lgar
