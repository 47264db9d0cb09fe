// lgar_moisture_tangent.hpp -- the tangent of the soil-moisture output (lgar_soil_moisture_tangent, include/lgar.h): the derivative
// of the depth bins of lgar_moisture.hpp along the direction a tangent state was integrated for.
//
// With lgar_moisture.hpp's notation (front j: depth d_j, content theta_j, layer tag k_j, top t_j = d_{j-1} when front j-1 has the
// same tag, else the top of layer k_j) and the tangents d'_j, theta'_j, t'_j = d'_{j-1} or +0.0 (thickness is not differentiated),
// bin i = [a, b] has
//
//     in(x) = x >= a && x < b
//     S'_i  = sum_j  theta'_j * (clip(d_j, a, b) - clip(t_j, a, b))  +  (in(d_j) ? theta_j * d'_j : 0.0)  -  (in(t_j) ? theta_j * t'_j : 0.0)
//
// in front order, per front acc = ((acc + first) + second) - third, plain fp64 multiplies and adds (-ffp-contract=off); every
// decision is a select, so a product under a false `in` is discarded whatever it is.
//
// The tie rule.  clip(x, a, b) has two one-sided derivatives at x = a and at x = b.  The half-open `in` takes the right-hand one
// at both: a depth exactly on the edge between two adjacent bins moves the water of the LOWER bin (x >= a there) and not of the
// upper one (x < b fails).  Every depth therefore lies in exactly one of two adjacent bins, and the bins that cover a column sum
// to sum_j theta'_j (d_j - t_j) + theta_j (d'_j - t'_j), the tangent of the stored volume, also when a front sits on an edge.  Any
// other choice (both sides, or neither) counts such a front twice or not at all and breaks that closure.  (A depth on the LAST
// edge of a covering set is in no bin; the fronts that sit on a layer's bottom carry d' = 0, the thickness being a constant.)
//
// what = LGAR_MOIST_STORAGE gives m'_i = S'_i; LGAR_MOIST_THETA gives m'_i = w_i > 0 ? S'_i / w_i : +0.0 with lgar_moisture.hpp's
// in-column width w_i (a constant): below the column the value is NaN, its tangent is zero.
//
// Two outputs, either or both.  out[i][c] = m'_i rounded once to R.  The contraction with a cotangent cot [n_bins][N / group]
// (fp64; lane c reads column c / group, the forcing_group convention of the tangent launches):
//     acc = +0.0;  for i ascending: acc = acc + (live_i ? cot_i * m'_i : 0.0);      live_i = w_i > 0 (theta) or true (storage)
//     grad[c] = (R)((double)grad[c] + acc)
// with the unrounded fp64 m'_i; a NaN cotangent under a dead bin is discarded by the select.
//
// Like lgar_moisture.hpp this compiles for the host with -DLGAR_DEVSIM (tests/moisture_tangent_host).
#pragma once
#include "lgar_moisture.hpp"

namespace lgar {

// The bins' tangents of ONE lane-column.  Template parameters, layouts, the clamps of n_fronts and of the layer tags and the
// wave-level row loop are moist_column's; ddepth / dtheta are the tangent state's rows [front_slots][N].  The accumulators are
// indexed by compile-time constants only (n_bins is wave-uniform: the guards are scalar branches).  out, or cot and grad, may be
// null; n_cot = N / group.
template <typename R, int NB, bool LAYER_BINS>
LGAR_MOIST_FN void moist_tangent_column(const R *depth, const R *theta, const uint8_t *flags, const int32_t *n_fronts,
                                        const R *ddepth, const R *dtheta, const R *thickness, const double *edges, size_t N, size_t c,
                                        int n_layers, int front_slots, int n_bins, int what, R *out, const double *cot, size_t group,
                                        R *grad) {
  static_assert(!LAYER_BINS || NB >= LGAR_LMAX, "layer bins need a bin per layer");
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
  double prev_d = 0.0, prev_dd = 0.0;
  int prev_k = -1;
  for (int j = 0; moist_any_lane(j < nf); j++) {
    if (j < nf) {
      const size_t at = (size_t)j * N + c;
      const double d = (double)depth[at];
      const double th = (double)theta[at];
      const double dd = (double)ddepth[at];
      const double dth = (double)dtheta[at];
      int k = (int)(flags[at] & 0x7Fu);
      k = k > n_layers - 1 ? n_layers - 1 : k;
      double t = 0.0;  // top of layer k
#pragma unroll
      for (int l = 1; l < LGAR_LMAX; l++) t = k >= l ? top[l] : t;
      const bool same = k == prev_k;
      t = same ? prev_d : t;
      const double dt = same ? prev_dd : 0.0;
      const double at_d = th * dd, at_t = th * dt;
#pragma unroll
      for (int i = 0; i < NB; i++)
        if (i < n_bins) {
          const double a = e[i], b = e[i + 1];
          const double first = dth * (moist_clip(d, a, b) - moist_clip(t, a, b));
          const double second = (d >= a && d < b) ? at_d : 0.0;
          const double third = (t >= a && t < b) ? at_t : 0.0;
          S[i] = ((S[i] + first) + second) - third;
        }
      prev_d = d;
      prev_dd = dd;
      prev_k = k;
    }
  }
  const size_t n_cot = N / group, cc = c / group;
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < NB; i++) {
    if (i < n_bins) {
      double m = S[i];
      bool live = true;
      if (what == LGAR_MOIST_THETA) {
        const double w = moist_clip(Z, e[i], e[i + 1]) - e[i];
        live = w > 0.0;
        m = live ? S[i] / w : 0.0;
      }
      if (out != nullptr) out[(size_t)i * N + c] = (R)m;
      if (cot != nullptr) {
        const double term = cot[(size_t)i * n_cot + cc] * m;
        acc = acc + (live ? term : 0.0);
      }
    }
  }
  if (cot != nullptr) grad[c] = (R)((double)grad[c] + acc);
}

// What lgar_soil_moisture_tangent refuses (include/lgar.h), for the library and the host build alike: 0, or LGAR_E_ARG.  The
// dims' fields the kernel uses are checked as lgar_soil_moisture's wrapper checks them, but for n_columns = 0, which is a job
// of no lanes (the caller returns 0 without a launch).
inline int moist_tangent_check(const LgarDims *d, const LgarParams *p, const LgarState *s, const LgarState *ds, const double *edges,
                               int n_bins, int what, const void *out, const double *cot, int group, const void *grad, int dtype) {
  if (!d || d->n_columns < 0 || d->n_layers < LGAR_LMIN || d->n_layers > LGAR_LMAX) return LGAR_E_ARG;
  if (d->front_slots < 0 || d->front_slots > LGAR_FMAX || (d->front_slots > 0 && d->front_slots < d->n_layers + 1)) return LGAR_E_ARG;
  if (!p || !p->thickness || !s || !s->depth || !s->theta || !s->flags || !s->n_fronts) return LGAR_E_ARG;
  if (!ds || !ds->depth || !ds->theta) return LGAR_E_ARG;
  if (dtype != LGAR_F32 && dtype != LGAR_F64) return LGAR_E_ARG;
  if (what != LGAR_MOIST_THETA && what != LGAR_MOIST_STORAGE) return LGAR_E_ARG;
  if (n_bins < 1 || n_bins > LGAR_MOIST_BINS || (!edges && n_bins != d->n_layers)) return LGAR_E_ARG;
  if ((cot != nullptr) != (grad != nullptr)) return LGAR_E_ARG;
  if (!out && !cot) return LGAR_E_ARG;
  if (group < 1 || d->n_columns % group != 0) return LGAR_E_ARG;
  return 0;
}

#ifndef LGAR_DEVSIM
// host-side launch (lgar_moisture_tangent.hip); arguments already checked.  Returns 0 / LGAR_E_*.
int launch_soil_moisture_tangent(const LgarDims *dims, const LgarParams *params, const LgarState *state, const LgarState *dstate,
                                 const double *edges, int n_bins, int what, void *out, const double *cot, int group, void *grad,
                                 int dtype, hipStream_t stream);
#endif

}  // namespace lgar
