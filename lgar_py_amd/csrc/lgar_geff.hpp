// lgar_geff.hpp -- the Geff trapezoid kernels: node exchange of cooperating lanes, the packed fp32 loop and the fused loop
// (geff_fused), and the mixed-precision trapezoid (geff_mixed*).
#pragma once
#include "lgar_vg.hpp"

namespace lgar {

// (sizes of the cooperating lanes' exchange table: plain constants, the simulator's build sees them too)
#define LGAR_COOP_TAB 128      /* most trapezoid intervals a cooperating job may have (LgarDims.nint; 120 in every bundled config) */
#define LGAR_COOP_TAB_ROW 130  /* doubles per group's table in LDS: padded so that the groups' tables start on different banks */
#define LGAR_COOP_PAIR_LANES 12 /* groups of at least this many lanes take two moving fronts at a time (Column::calc_dzdt_pairs) */
#ifndef LGAR_DEVSIM
// The trapezoid's interior for COOPERATING lanes (forward kernels on jobs too small to fill the chip, LgarDims.forward_lanes):
// the `lanes` lanes of an aligned group all carry the SAME column -- same values, same branches.  `tab` is the group's table
// of LGAR_COOP_TAB doubles in LDS.
//   1. the group's first lane runs the plain loop's running sum h2 += dh and leaves head j in tab[j];
//   2. lane r evaluates nodes r, r + lanes, r + 2 lanes, ... -- two or four at a time -- and puts K(head) where the head was
//      (no other lane reads that head);
//   3. lane r turns its nodes into the trapezoid's terms (K_{j-1} + K_j) dh/2, in place;
//   4. every lane adds the 120 terms up in order.
// Heads, node values, terms and the sum are those of the plain loop bit for bit: each goes through the same operations on the
// same operands, only once per group instead of once per lane.
// (r: my place in the group.  The last group of a wavefront also takes the lanes left over when `lanes` does not divide 64:
// their r >= lanes; they evaluate no node -- a node's table slot must be read as a head and rewritten by ONE lane -- and take
// part in everything else.)
// W nodes per lane and round (independent chains of ~100 dependent double-precision operations each: one wave alone on its SIMD
// issues a dependent operation every ~10 cycles, so the chains of a round overlap)
template <int W>
__device__ __forceinline__ void geff_coop_node_rounds(const LayerK<double> &l, double nm1, double half_m, double k_sat1, double k_first,
                                                      double hdh, int nint, int lanes, double *tab, int r) {
  const int stride = W * lanes;
  for (int first = 0; first < nint; first += stride) {
    double h[W], k[W];
    bool ok[W];
#pragma unroll
    for (int u = 0; u < W; u++) {
      const int j = first + r + u * lanes;
      ok[u] = (r < lanes) && (j < nint);
      h[u] = tab[ok[u] ? j : 0];
    }
#pragma unroll
    for (int u = 0; u < W; u++) k[u] = geff_node(l, nm1, half_m, h[u]);
#pragma unroll
    for (int u = 0; u < W; u++) {
      k[u] = (fabs(h[u]) < 0.1 || h[u] < 0.0) ? k_sat1 : k[u];  // utils.py:124-128 (never true on the nodes the plain loop leaves unchecked)
      if (ok[u]) tab[first + r + u * lanes] = k[u];
    }
  }
  lds_exchange_point();
  LGAR_MEASURE_POINT(CLK, 14)
  // the trapezoid's terms (K_{j-1} + K_j) dh/2, in place: the rounds run from the LAST to the first, so that a round only
  // overwrites nodes no later round reads (its own, whose predecessors belong to it or to a round still to come)
  for (int first = ((nint - 1) / stride) * stride; first >= 0; first -= stride) {
    double p[W], k[W];
    bool ok[W];
#pragma unroll
    for (int u = 0; u < W; u++) {
      const int j = first + r + u * lanes;
      ok[u] = (r < lanes) && (j < nint);
      p[u] = tab[(ok[u] && j > 0) ? j - 1 : 0];
      k[u] = tab[ok[u] ? j : 0];
    }
    lds_exchange_point();  // every lane has its operands before any term replaces a node
#pragma unroll
    for (int u = 0; u < W; u++) {
      const int j = first + r + u * lanes;
      if (ok[u]) tab[j] = (((j > 0) ? p[u] : k_first) + k[u]) * hdh;
    }
  }
}
__device__ __forceinline__ void geff_nodes_cooperative(const LayerK<double> &l, double nm1, double half_m, double k_sat1, double &h2,
                                                       double dh, double hdh, double &g, double &k1, int nint, int lanes, double *tab, int r) {
  // one wave = one workgroup: LDS operations of a wave complete in order, the fences only pin the compiler
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");  // (earlier loads of the table stay in front of these stores)
  // 1. the heads: a chain of nint dependent additions; ONE lane of the group runs it (64 lanes storing to one address are
  //    64 conflicting writes: 24 cycles per head, measured)
  if (r == 0) {
    double h = h2;
    int j = 0;
    for (; j + 16 <= nint; j += 16) {
      // (sixteen heads in registers of their own, then their stores: an addition that overwrites a register a store still
      // reads waits for that store)
      double hh[16];
#pragma unroll
      for (int u = 0; u < 16; u++) {
        hh[u] = h;
        h = h + dh;
      }
#pragma unroll
      for (int u = 0; u < 16; u++) tab[j + u] = hh[u];
    }
    for (; j < nint; j++) {
      tab[j] = h;
      h = h + dh;
    }
  }
  lds_exchange_point();
  LGAR_MEASURE_POINT(CLK, 13)
  // 2. nodes, 3. terms: two per lane and round, four when two would take more than one round
  if (nint > 2 * lanes) geff_coop_node_rounds<4>(l, nm1, half_m, k_sat1, k1, hdh, nint, lanes, tab, r);
  else geff_coop_node_rounds<2>(l, nm1, half_m, k_sat1, k1, hdh, nint, lanes, tab, r);
  lds_exchange_point();
  LGAR_MEASURE_POINT(CLK, 15)
  // 4. every lane adds the terms up in order (the same address in every lane of the group: a broadcast).  The additions are
  //    one dependent chain; the reads of the next sixteen terms are in flight while the chain works through the present ones.
  {
    const int nb = nint >> 4;  // batches of sixteen terms, alternately in two sets of registers
    const double *tail = tab + (nb << 4);
    double ta[16], tb[16], tc[8];
    if (nb > 0) {
#pragma unroll
      for (int j = 0; j < 16; j++) ta[j] = tab[j];
    }
    if (nint & 8) {
#pragma unroll
      for (int j = 0; j < 8; j++) tc[j] = tail[j];
    }
#pragma unroll
    for (int i = 0; i < LGAR_COOP_TAB / 16; i++) {
      if (i < nb) {
        const double *next = tab + 16 * (i + 1);
        // (the next batch is read whether it exists or not -- unconditional loads keep the waits exact; the table has
        // LGAR_COOP_TAB_ROW >= 16 (i + 2) entries for every i that gets here with another batch to come)
        if (i & 1) {
          if (i + 1 < LGAR_COOP_TAB / 16) {
#pragma unroll
            for (int j = 0; j < 16; j++) ta[j] = next[j];
          }
#pragma unroll
          for (int j = 0; j < 16; j++) g = g + tb[j];
        } else {
          if (i + 1 < LGAR_COOP_TAB / 16) {
#pragma unroll
            for (int j = 0; j < 16; j++) tb[j] = next[j];
          }
#pragma unroll
          for (int j = 0; j < 16; j++) g = g + ta[j];
        }
      }
    }
    int q0 = nb << 4;
    if (nint & 8) {
#pragma unroll
      for (int j = 0; j < 8; j++) g = g + tc[j];
      q0 += 8;
    }
    for (; q0 < nint; q0++) g = g + tab[q0];
  }
  lds_exchange_point();  // the next call's stores stay behind these loads
  LGAR_MEASURE_POINT(CLK, 16)
}
#endif
// (cooperating lanes, calc_dzdt: conductivities that ride along with the evaluations that open a trapezoid -- see
// geff_ends_cooperative)
struct CoopRiders {
  int n = 0;           // riders of this call (the group needs 4 + n lanes)
  LayerK<double> l;    // MY rider's layer and Se (lanes 4 .. 4 + n - 1; anything elsewhere)
  double se = 1.0;
  double k[LGAR_LMAX]; // out: K of rider e
};
#ifndef LGAR_DEVSIM
// The four two-pow evaluations that open a trapezoid -- h(Se_i), h(Se_f) (calc_h_from_se), K(Se_i), K(1) (calc_k_from_se) -- for
// COOPERATING lanes: lane r of a group evaluates number r mod 4 and the group exchanges the results.  Both functions are
// "pow, offset from 1, nudge, pow, finish": the lanes run ONE instruction stream with their own exponents and pick their own
// finish, every value going through exactly the operations h_from_se / k_from_se apply to it (bit-identical results; the
// serial chain of eight pows becomes one of two).
// Riders (calc_dzdt): up to LGAR_LMAX more conductivities K(Se) of OTHER evaluations -- the moving front's own K(theta) and the
// K of every layer above at the front's psi (calc_bottom_sum, Layer.py:1557-1582) -- are the same "pow, offset, nudge, pow,
// finish": lane 4 + e of the group takes rider e, with that rider's layer (xl) and Se (xse) as ITS operands, and every lane
// reads the n_riders results back into xk before the table is reused for the trapezoid's heads.
__device__ __forceinline__ void geff_ends_cooperative(const LayerK<double> &l, double se_i, double se_f, double &h_i, double &h_f,
                                                      double &k_i, double &k_sat1, double *xchg, int r, CoopRiders *rd = nullptr) {
  const bool rider = (rd != nullptr) && (r >= 4) && (r - 4 < rd->n);
  const int which = rider ? 2 : (r & 3);  // 0: h(Se_i), 1: h(Se_f), 2: K(Se_i), 3: K(1)
  const bool is_h = which < 2;
  double se = (which == 1) ? se_f : ((which == 3) ? 1.0 : se_i);
  double inv_m = l.inv_m, m = l.m, ksat = l.ksat;
  if (rd != nullptr) {
    se = rider ? rd->se : se;
    inv_m = rider ? rd->l.inv_m : inv_m; m = rider ? rd->l.m : m; ksat = rider ? rd->l.ksat : ksat;
  }
  const double sp = pw(se, is_h ? -inv_m : inv_m);
  double base = is_h ? sp - 1.0 : 1.0 - sp;
  if (fabs(base) <= 1e-8) base = base + 1e-12;
  const double op = pw(base, is_h ? l.inv_n : m);
  const double t = 1.0 - op;
  const double mine = is_h ? (1.0 / l.alpha) * op : ksat * sqrt(se) * (t * t);
  double *grp = xchg;  // the group's table
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  if (r < 4) grp[which] = mine;  // lanes 0..3 of the group (a group has at least 4)
  if (rider) grp[r] = mine;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
  h_i = grp[0]; h_f = grp[1]; k_i = grp[2]; k_sat1 = grp[3];
  if (rd != nullptr) {
#pragma unroll
    for (int e = 0; e < LGAR_LMAX; e++) rd->k[e] = grp[4 + e];  // (slots past the last rider: stale values nobody uses)
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}
#endif
template <typename S>
__device__ __forceinline__ S geff_fused(const LayerK<S> &l, S theta1, S theta2, int nint, real_t<S> *xchg = nullptr, int coop = 0,
                                        int rank = 0, CoopRiders *riders = nullptr) {
  using R = real_t<S>;
  using K = ScalarKind<S>;
  const S se_i = se_from_theta(l, theta1);
  const S se_f = se_from_theta(l, theta2);
  S h_i, h_f, k_sat1, k1;  // h(Se) of both ends; K at Se == 1 (|h| < 0.1); K(Se_i)
  bool ends_done = false;
#ifndef LGAR_DEVSIM
  if constexpr (K::plain_f64) {
    if (coop >= 4 && xchg != nullptr) {
      LGAR_MEASURE_POINT(CLK, 11)
      geff_ends_cooperative(l, se_i, se_f, h_i, h_f, k1, k_sat1, xchg, rank, riders);
      LGAR_MEASURE_POINT(CLK, 12)
      ends_done = true;
    }
  }
#endif
  if (!ends_done) {
    LGAR_MEASURE_POINT(CLK, 25)
    h_i = h_from_se(l, se_i);
    h_f = h_from_se(l, se_f);
    k_sat1 = k_from_se_one(l);
    k1 = k_from_se(l, se_i);
    LGAR_MEASURE_POINT(CLK, 26)
  }
  // lg2p / ex2p take finite positive arguments (the exponent of 2^x goes through a float -> int conversion, undefined for
  // NaN): an end point outside the domain (Se > 1 -> negative pow base -> NaN head; the reference raises ValueError there,
  // physics/utils.py:25-27) is replaced by a harmless one for the nodes and put back into the result below
  const S h_i_own = h_i, h_f_own = h_f;
  const bool outside = is_nan(val(h_i)) || is_nan(val(h_f));
  if (outside) { h_i = S(R(1.0)); h_f = S(R(1.0)); }
  const S dh = (h_f - h_i) / R(nint);
  const S hdh = dh / R(2.0);
  const S half_m = R(-0.5) * l.m;
  const S nm1 = l.n - R(1.0);  // n m = n - 1: a^m = (alpha h)^(n-1)
  S g = S(R(0.0));
  S h2 = h_i + dh;
  // four transcendentals per node: P = a^m = x^(n-1), a = x P, sqrt(Se) = (1+a)^(-m/2), (a/(1+a))^m = P Se
  auto node = [&](const S &h) { return geff_node(l, nm1, half_m, h); };
  int i = 0;
#ifndef LGAR_DEVSIM
  bool nodes_done = false;
  if constexpr (K::plain_f64) {
    if (coop > 1 && xchg != nullptr) {  // cooperating lanes: every node is checked against the |h| < 0.1 rule by its evaluator
      geff_nodes_cooperative(l, nm1, half_m, k_sat1, h2, dh, hdh, g, k1, nint, coop, xchg, rank);
      nodes_done = true;
    }
  }
  if (nodes_done) i = nint;
#endif
  // The |h| < 0.1 -> Se = 1 rule (utils.py:124-128) can only bind on a SUFFIX of the nodes (h falls monotonically from
  // h_i to h_f): a wave-uniform count of leading nodes that no lane needs to test runs select-free.
  int n_safe = nint;
  if (i < nint) {
    // (node j sits at h_i + j dh: nodes up to floor((h_i - 0.1) / -dh) - 1 lie a whole interval above the cut, far more than the
    // running sum's rounding can move them)
    const R jf = (val(h_i) - R(0.1)) / -val(dh) - R(1.0);
    const int safe = (jf > R(0.0)) ? ((jf < R(nint)) ? int(jf) : nint) : 0;  // NaN (dh == 0) -> 0
    if (any_lane(safe < nint) != 0ull) {
      n_safe = 0;
      for (int bit = 128; bit; bit >>= 1) {
        const int cand = n_safe + bit;
        if (cand <= nint && any_lane(safe < cand) == 0ull) n_safe = cand;
      }
    }
  }
  if constexpr (K::dual && K::f64) {
    if (xchg != nullptr && coop >= 2 && n_safe >= coop) {  // coop: the W lanes that share this column (LgarDims.tangent_share)
      LGAR_MEASURE_POINT(CLK, 27)
      geff_shared_blocks(l, nm1, half_m, h2, dh, hdh, g, k1, n_safe / coop, coop, xchg, n_safe % coop);
      i = n_safe;  // (the safe nodes left over after the full blocks are one more, partial block)
      LGAR_MEASURE_POINT(CLK, 28)
    }
  }

  // fp64 and its dual numbers: two nodes per iteration give the scheduler two independent chains (same sums in the same
  // order; measured: backward -1.5 %, fp64 forward -1 %, a job of 157 waves -3 %)
  if constexpr (K::f64) {
    for (; i + 1 < n_safe; i += 2) {
      const S hb = h2 + dh;
      const S ka = node(h2);
      const S kb = node(hb);
      g = g + ((k1 + ka) * hdh);
      g = g + ((ka + kb) * hdh);
      k1 = kb;
      h2 = hb + dh;
    }
  }
  for (; i < n_safe; i++) {
    if (K::f32) h2 = (i + 1 >= nint) ? h_f : h_i + R(i + 1) * dh;
    const S k2 = node(h2);
    g = g + ((k1 + k2) * hdh);
    k1 = k2;
    if (K::f64) h2 = h2 + dh;
  }
  for (; i < nint; i++) {
    if (K::f32) h2 = (i + 1 >= nint) ? h_f : h_i + R(i + 1) * dh;
    S k2 = node(h2);
    k2 = choose(ab(val(h2)) < R(0.1) || val(h2) < R(0.0), k_sat1, k2);
    g = g + ((k1 + k2) * hdh);
    k1 = k2;
    if (K::f64) h2 = h2 + dh;
  }
  // (an end point outside the domain must still surface as NaN for the status word)
  const S res = ab(g / l.ksat);
  LGAR_MEASURE_POINT(CLK, 29)
  return outside ? res + (h_i_own + h_f_own) : res;
}
// fp32 Geff, lean form (what bench.py measures).  Per node, with x = alpha h and K_r = K / Ksat (Ksat cancels in
// G = |integral of K dh| / Ksat):
//     lg = log2 x;  P = 2^((n-1) lg) = x^(n-1) = a^m   [a = x^n, n m = n - 1];   a = x P;
//     l1 = log2(1 + a);  s = 2^(-m/2 l1) = sqrt(Se);  K_r = s (1 - P s^2)^2        [(a/(1+a))^m = a^m Se]
// i.e. FOUR transcendentals per node (v_log, v_exp, v_log, v_exp) instead of five, and no division.  The vector ALU
// issues a transcendental in 8 cycles, a packed op in 4 and a v_cndmask_b32 in 16 (measured, tools/valu_probe.py), so
// the loop is laid out to be select-free: the |h| < 0.1 -> Se = 1 rule (utils.py:124-128) can only bind on a SUFFIX of
// the nodes (h falls monotonically from h_i to h_f), so a wave-uniform count of leading node pairs that no lane needs
// to test runs in a select-free loop, the rest in a checked loop.  The trapezoid is summed as
// dh/2 (K_0 + K_n + 2 sum of interior nodes): one packed add per node pair.  Interior nodes sit at h_i + j dh (no running
// sum: it drifts by cm for very dry soil); the last node is h_f itself, which dominates the integral for dry soil.
typedef float f32x2 __attribute__((ext_vector_type(2)));
// (the trapezoid given its two heads; kn_out, when asked for: K_r of the wet end node)
__device__ __forceinline__ float geff_f32_from_heads(const LayerK<float> &l, float h_i, float h_f, int nint, float *kn_out = nullptr) {
  const float dh = (h_f - h_i) * (1.0f / float(nint));
  const float nm1 = l.n - 1.0f;
  const float hm = -0.5f * l.m;
  const float x0 = l.alpha * h_i, dx = l.alpha * dh, xcut = 0.1f * l.alpha;
  // K_r at Se == 1 (calc_k_from_se's 1e-12 nudge, utils.py:147-150): (1 - (1e-12)^m)^2
  const float tsat = 1.0f - ex2(l.m * -39.863137f);
  const float ksat1 = tsat * tsat;
  auto node = [&](float x) {
    const float lg = lg2(x);
    const float P = ex2(nm1 * lg);
    const float l1 = lg2(__builtin_fmaf(x, P, 1.0f));
    const float sr = ex2(hm * l1);
    const float t = __builtin_fmaf(-P, sr * sr, 1.0f);
    const float k = sr * (t * t);
    return (x < xcut) ? ksat1 : k;
  };
  const int M = nint - 1;       // interior nodes j = 1 .. nint-1
  const int pairs = M >> 1;
  // leading interior nodes with h >= 0.1 for certain: j < (x0 - xcut) / -dx (one node of margin for rounding)
#ifndef LGAR_DEVSIM
  const float jf = (x0 - xcut) * __builtin_amdgcn_rcpf(-dx) - 1.5f;
#else
  const float jf = (x0 - xcut) / -dx - 1.5f;
#endif
  int safe = (jf > 0.0f) ? ((jf < float(M)) ? int(jf) : M) : 0;  // NaN (dx == 0) -> 0
  safe >>= 1;
  // wave-uniform minimum: usually every lane is safe for the whole interior (only the end point h_f is near zero)
  int safe_pairs = pairs;
  if (any_lane(safe < pairs) != 0ull) {
    safe_pairs = 0;  // bisection on ballots (plain compares + scalar ops)
    for (int bit = 64; bit; bit >>= 1) {
      const int cand = safe_pairs + bit;
      if (cand <= pairs && any_lane(safe < cand) == 0ull) safe_pairs = cand;
    }
  }
  const f32x2 dx2 = {dx, dx}, x02 = {x0, x0}, nm12 = {nm1, nm1}, hm2 = {hm, hm};
  const f32x2 one2 = {1.0f, 1.0f}, two2 = {2.0f, 2.0f}, four2 = {4.0f, 4.0f};
  // A column's result must not depend on which columns share its wavefront (safe_pairs is a property of the wave): node
  // pair p always sits at x0 + (2p+1, 2p+2) dx (one fma, never a running sum), always goes through the same operations,
  // and always lands in accumulator p & 1 -- whichever of the three loops below handles it.
  f32x2 ja = {1.0f, 2.0f};
  f32x2 acc = {0.0f, 0.0f}, accb = {0.0f, 0.0f};
  // one node pair: 4 transcendentals + 4 packed ops per node-pair -> sqrt(Se) and (1 - P Se)^2 of two nodes
#define LGAR_GEFF_PAIR(X, SR, TT)                                              \
  {                                                                            \
    f32x2 lg, P, l1;                                                           \
    lg.x = lg2((X).x); lg.y = lg2((X).y);                                      \
    const f32x2 e0 = nm12 * lg;                                                \
    P.x = ex2(e0.x); P.y = ex2(e0.y);                                          \
    const f32x2 opa = __builtin_elementwise_fma((X), P, one2);                 \
    l1.x = lg2(opa.x); l1.y = lg2(opa.y);                                      \
    const f32x2 e1 = hm2 * l1;                                                 \
    (SR).x = ex2(e1.x); (SR).y = ex2(e1.y);                                    \
    const f32x2 t = __builtin_elementwise_fma(-P, (SR) * (SR), one2);          \
    (TT) = t * t;                                                              \
  }
  int it = 0;
  // four nodes per iteration: two independent chains
  for (; it + 1 < safe_pairs; it += 2) {
    const f32x2 xa = __builtin_elementwise_fma(ja, dx2, x02);
    const f32x2 xb = __builtin_elementwise_fma(ja + two2, dx2, x02);
    ja = ja + four2;
    f32x2 sa, ta, sb, tb;
    LGAR_GEFF_PAIR(xa, sa, ta)
    acc = __builtin_elementwise_fma(sa, ta, acc);
    LGAR_GEFF_PAIR(xb, sb, tb)
    accb = __builtin_elementwise_fma(sb, tb, accb);
  }
  if (it < safe_pairs) {  // `it` is even here
    const f32x2 x = __builtin_elementwise_fma(ja, dx2, x02);
    f32x2 sr, tt;
    LGAR_GEFF_PAIR(x, sr, tt)
    acc = __builtin_elementwise_fma(sr, tt, acc);
    it++;
  }
  for (; it < pairs; it++) {  // nodes that may fall under the |h| < 0.1 cut: K_r = ksat1 there
    const float j0 = float(2 * it + 1);
    const f32x2 j2 = {j0, j0 + 1.0f};
    const f32x2 x = __builtin_elementwise_fma(j2, dx2, x02);
    f32x2 sr, tt;
    LGAR_GEFF_PAIR(x, sr, tt)
    sr.x = (x.x < xcut) ? ksat1 : sr.x;
    tt.x = (x.x < xcut) ? 1.0f : tt.x;
    sr.y = (x.y < xcut) ? ksat1 : sr.y;
    tt.y = (x.y < xcut) ? 1.0f : tt.y;
    if (it & 1) accb = __builtin_elementwise_fma(sr, tt, accb);
    else acc = __builtin_elementwise_fma(sr, tt, acc);
  }
  acc = acc + accb;
  float sum = acc.x + acc.y;
  if (M & 1) sum += node(__builtin_fmaf(float(M), dx, x0));
#ifndef LGAR_NO_GEFF_ENDS
  // the two END nodes as one more pair, checked as the loop above checks its pairs (K_r = ksat1 * 1 under the cut): every value
  // goes through node()'s operations, the eight transcendentals as four packed steps instead of two dependent chains
  float k0, kn;
  {
    const f32x2 xe = {x0, l.alpha * h_f};
    f32x2 sr, tt;
    LGAR_GEFF_PAIR(xe, sr, tt)
    sr.x = (xe.x < xcut) ? ksat1 : sr.x;
    tt.x = (xe.x < xcut) ? 1.0f : tt.x;
    sr.y = (xe.y < xcut) ? ksat1 : sr.y;
    tt.y = (xe.y < xcut) ? 1.0f : tt.y;
    const f32x2 ke = sr * tt;
    k0 = ke.x; kn = ke.y;
  }
#else
  const float k0 = node(x0), kn = node(l.alpha * h_f);
#endif
#undef LGAR_GEFF_PAIR
  if (kn_out != nullptr) *kn_out = kn;
  return fabsf((0.5f * dh) * ((k0 + kn) + 2.0f * sum));
}
template <> __device__ __forceinline__ float geff<float>(const LayerK<float> &l, float theta1, float theta2, int nint) {
  const float se_i = se_from_theta(l, theta1);
  const float se_f = se_from_theta(l, theta2);
  // h(Se) of both end points (calc_h_from_se, utils.py:159-174) with one reciprocal of alpha
  const float inv_alpha = 1.0f / l.alpha;
#ifndef LGAR_NO_GEFF_ENDS
  // both heads statement by statement (each is a chain of two logarithms and two exponentials in which every operation waits
  // for the one before it: see mixed_k_pair); the operations of head() below on the same operands
  const float ni = -l.inv_m;
  const float la = lg2(se_i), lb = lg2(se_f);
  const float pa = ex2(ni * la), pb = ex2(ni * lb);
  float ba = pa - 1.0f, bb = pb - 1.0f;
  if (fabsf(ba) <= 1e-8f) ba = ba + 1e-12f;
  if (fabsf(bb) <= 1e-8f) bb = bb + 1e-12f;
  const float ua = lg2(ba), ub = lg2(bb);
  const float oa = ex2(l.inv_n * ua), ob = ex2(l.inv_n * ub);
  return geff_f32_from_heads(l, inv_alpha * oa, inv_alpha * ob, nint);
#else
  auto head = [&](float se) {
    float base = pw(se, -l.inv_m) - 1.0f;
    if (fabsf(base) <= 1e-8f) base = base + 1e-12f;
    return inv_alpha * pw(base, l.inv_n);
  };
  return geff_f32_from_heads(l, head(se_i), head(se_f), nint);
#endif
}
// geff<float>, NOT inlined: for the call sites of the plain fp32 kernels that run rarely (insert_water on a memo miss, the
// dry-depth evaluation -- see geff_mixed, which does the same for the mixed-precision kernels, on why and on the scalar
// arguments).  calc_dzdt, the hot site, keeps its inlined copy.  The same function on the same operands: the same values bit for
// bit.  (Ksat cancels in G and is no argument.)
__device__ __attribute__((noinline)) float geff_f32_rare(float alpha, float n, float m, float inv_m, float inv_n, float te, float tr,
                                                         float theta1, float theta2, int nint) {
  const LayerK<float> l{alpha, n, m, inv_m, inv_n, 1.0f, te, tr};
  return geff<float>(l, theta1, theta2, nint);
}
template <> __device__ __forceinline__ double geff<double>(const LayerK<double> &l, double t1, double t2, int nint) {
  return geff_fused<double>(l, t1, t2, nint);
}

// Mixed-precision Geff (LgarDims.geff_mode = 1, fp64 runs): the column state, every branch and the mass bookkeeping stay
// in double precision; of the trapezoid, only the 119 INTERIOR nodes are evaluated with the fp32 hardware transcendentals.
//   * both heads h(Se) (calc_h_from_se, utils.py:159-174), dh, and the two END nodes K(Se_i), K(Se_f)
//     (calc_k_from_se, utils.py:134-156) are double precision.  K falls steeply with h (like h^-3.7 for the bundled soils),
//     so over a wide range the wet end node carries most of the sum: it must not carry fp32 rounding;
//   * interior node j sits at x_j = alpha h_i + j alpha dh, formed from fp32 hi + lo pairs of both terms (within 1 ulp of
//     the double-precision value); the exponents
//     n - 1 and -m/2 enter as fp32 pairs hi + lo (their rounding would otherwise be a SYSTEMATIC relative error of
//     ~1e-7 |log2 x| in every node; what remains -- the 1-ulp errors of v_log_f32 / v_exp_f32 and of x -- is random from
//     node to node and averages over the sum);
//   * the nodes' K_r are added up in double (per group of four nodes: two fp32 adds, one convert, one fp64 add).
// Per interior node: five hardware transcendentals + ~12 packed fp32 operations (the node is written without the cancelling
// difference 1 - (a/(1+a))^m of the fp32 loop: see LGAR_GEFFM_PAIR), against the ~93 fp64 instructions of the fused fp64 node.
// The |h| < 0.1 -> Se = 1 rule and the wave-uniform select-free prefix are those of the fp32 loop above; as there, a group of
// nodes always goes through the same operations in the same order, so a column's result does not depend on its wavefront.
// One end of the trapezoid in double precision: h(Se) (calc_h_from_se, utils.py:159-174) and K(Se) / Ksat (calc_k_from_se,
// utils.py:134-156) from SHARED logarithms.  With q = log2 Se^(1/m), C = 2^q and u = log2(1 - C):
//     K_r = sqrt(Se) (1 - 2^(m u))^2,     h = (1/alpha) 2^((u - q)/n)      [Se^(-1/m) - 1 = (1 - C)/C]
// i.e. two logarithms and three exponentials where the two functions on their own take four pows.  The reference's nudges
// (|base| <= 1e-8 -> base + 1e-12, both functions) are reproduced: at Se == 1 both bases are exactly 0 and share the
// logarithm of 1e-12; a base in (0, 1e-8] (Se within 1e-8 of 1 but not 1) takes its own logarithm on a wave-uniform branch.
#define LGAR_LOG2_1EM12 -39.863137138648355  // log2(1e-12): the nudged base at Se == 1
__device__ __forceinline__ void mixed_end(const LayerK<double> &l, double se, double &h, double &kr) {
  const double q = lg2e(se) * l.inv_m;
  const double C = ex2e(q);  // Se^(1/m)
  const double omc = 1.0 - C;
  const bool k_nudged = fabs(omc) <= 1e-8;
  const double bk = k_nudged ? omc + 1e-12 : omc;
  const double u = (omc == 0.0) ? LGAR_LOG2_1EM12 : lg2e(bk);  // (the constant: the saturated end below takes the same value)
  const double t = 1.0 - ex2e(l.m * u);
  kr = sqrt(se) * (t * t);
  const double bh = omc / C;  // Se^(-1/m) - 1
  const bool h_nudged = fabs(bh) <= 1e-8;
  double lbh = (omc == 0.0) ? u : u - q;  // log2 of the (nudged) base of h
  if (any_lane((k_nudged || h_nudged) && omc != 0.0) != 0ull) {
    const double own = lg2e(h_nudged ? bh + 1e-12 : bh);
    lbh = ((k_nudged || h_nudged) && omc != 0.0) ? own : lbh;
  }
  h = (1.0 / l.alpha) * ex2e(lbh * l.inv_n);
}
// The interior of the mixed-precision trapezoid and its closing formula, given both heads, K_r of both end nodes and K_r at
// Se == 1 (see geff_mixed / geff_mixed_heads for where they come from).
// COOPERATE (cooperating lanes, MODE_MIXED_COOP): the lanes of a group carry the same column; lane r of `lanes` evaluates the
// four-node groups r, r + lanes, ... in the general, checked form -- the value every form gives a group, bit for bit -- and
// leaves each group's sum in the group's LDS table `tab`; every lane then adds the groups up in order, as the loops below do.
template <bool COOPERATE = false>
__device__ __forceinline__ double geff_mixed_core(const LayerK<double> &l, double h_i, double h_f, double k0, double kn_own, double ksat1,
                                                  int nint, double *tab = nullptr, int lanes = 0, int r = 0) {
  (void)tab; (void)lanes; (void)r;
  const float ksat1f = (float)ksat1;
  const double dh = (h_f - h_i) / double(nint);
  const double x0 = l.alpha * h_i, dx = l.alpha * dh, xcut = 0.1 * l.alpha;
  // exponents as fp32 pairs
  const double hmd = -0.5 * l.m;
  const float hm = (float)hmd, hm_lo = (float)(hmd - (double)hm);
  const int M = nint - 1;  // interior nodes j = 1 .. nint-1
  const int pairs = M >> 1;
  // (node counts from abscissae: one reciprocal of -dx serves the three of them; each count keeps a node or more of margin, and
  // which loop evaluates a node never changes its value)
  const double inv_ndx = 1.0 / -dx;
  const double jf = (x0 - xcut) * inv_ndx - 1.5;
  int safe = (jf > 0.0) ? ((jf < double(M)) ? int(jf) : M) : 0;  // NaN (dx == 0, or a head outside the domain) -> 0
  safe >>= 1;
  int safe_pairs = pairs;
  if (!COOPERATE && any_lane(safe < pairs) != 0ull) {
    safe_pairs = 0;
    for (int bit = 64; bit; bit >>= 1) {
      const int cand = safe_pairs + bit;
      if (cand <= pairs && any_lane(safe < cand) == 0ull) safe_pairs = cand;
    }
  }
  const float xcutf = (float)xcut;
  const float nf = (float)l.n, nf_lo = (float)(l.n - (double)nf), mmf = (float)(-l.m), mmf_lo = (float)(-l.m - (double)mmf);
  const f32x2 n2 = {nf, nf}, nl2 = {nf_lo, nf_lo}, hm2 = {hm, hm}, hml2 = {hm_lo, hm_lo}, one2 = {1.0f, 1.0f};
  // expm1(E ln 2) / E = ln 2 + E (ln^2 2 / 2 + E (ln^3 2 / 6 + E (ln^4 2 / 24 + E ln^5 2 / 120)))
  const f32x2 ln2_2 = {0.693147181f, 0.693147181f}, c2_2 = {0.240226507f, 0.240226507f}, c3_2 = {0.0555041087f, 0.0555041087f};
  const f32x2 c4_2 = {0.00961812911f, 0.00961812911f}, c5_2 = {0.00133335581f, 0.00133335581f};
  const f32x2 mm2 = {mmf, mmf}, mml2 = {mmf_lo, mmf_lo}, ilog2 = {1.44269504f, 1.44269504f}, two_ilog2 = {2.88539008f, 2.88539008f};
  const f32x2 half2 = {0.5f, 0.5f};
  // one node pair: sqrt(Se) and (1 - P Se)^2 of the nodes at X.x, X.y.
  // KIND says what is KNOWN about the pair (a compile-time literal; it never changes a result, only which of two values that
  // the general form computes and then discards is not computed at all):
  //   0  nothing: t = 1 - 2^E and its series are both formed and chosen between by 2^E > 7/8 (the general form);
  //   1  2^E > 7/8 for certain (dry nodes): the series only -- no 2^E, no select, and 1 + r < 2 needs no clamp;
  //   2  2^E <= 7/8 for certain (wet nodes): the difference only -- no series, no select.
#define LGAR_GEFFM_PAIR(X, SR, TT, KIND)                                                    \
  {                                                                                         \
    /* log2 a = n log2 x;  r = 1/a;  L = log2(1 + r) from c = fl(1 + r), compensated for the rounding of the sum  */ \
    f32x2 lg, r, Lc;                                                                        \
    lg.x = lg2((X).x); lg.y = lg2((X).y);                                                   \
    const f32x2 la = __builtin_elementwise_fma(n2, lg, nl2 * lg);                           \
    r.x = ex2(-la.x); r.y = ex2(-la.y);                                                     \
    const f32x2 c = one2 + r;                                                               \
    const f32x2 rho = r - (c - one2);                                                       \
    Lc.x = lg2(c.x); Lc.y = lg2(c.y);                                                       \
    /* (2 - c) / ln 2 ~ 1 / (c ln 2) where the correction matters (c near 1); nothing for c >= 2 */ \
    f32x2 ic = __builtin_elementwise_fma(-ilog2, c, two_ilog2);                             \
    if ((KIND) != 1) { ic.x = fmaxf(ic.x, 0.0f); ic.y = fmaxf(ic.y, 0.0f); }                \
    const f32x2 L = __builtin_elementwise_fma(rho, ic, Lc);                                 \
    /* E = -m L = log2 (a/(1+a))^m;  sqrt(Se) = (1 + a)^(-m/2) = 2^(-m/2 (log2 a + L)) = 2^(-m/2 log2 a + E/2) */ \
    const f32x2 E = __builtin_elementwise_fma(mm2, L, mml2 * L);                            \
    const f32x2 e1 = __builtin_elementwise_fma(hm2, la, __builtin_elementwise_fma(hml2, la, half2 * E)); \
    (SR).x = ex2(e1.x); (SR).y = ex2(e1.y);                                                 \
    /* t = 1 - 2^E.  Dry nodes have 2^E -> 1: there t = -expm1(E ln 2) by its series in E (5 terms for 2^E > 7/8), not by \
       the cancelling difference */                                                         \
    f32x2 t;                                                                                \
    if ((KIND) == 1) {                                                                      \
      f32x2 p = __builtin_elementwise_fma(c5_2, E, c4_2);                                   \
      p = __builtin_elementwise_fma(p, E, c3_2);                                            \
      p = __builtin_elementwise_fma(p, E, c2_2);                                            \
      p = __builtin_elementwise_fma(p, E, ln2_2);                                           \
      t = -E * p;                                                                           \
    } else if ((KIND) == 2) {                                                               \
      f32x2 w;                                                                              \
      w.x = ex2(E.x); w.y = ex2(E.y);                                                       \
      t = one2 - w;                                                                         \
    } else {                                                                                \
      f32x2 w;                                                                              \
      w.x = ex2(E.x); w.y = ex2(E.y);                                                       \
      f32x2 p = __builtin_elementwise_fma(c5_2, E, c4_2);                                   \
      p = __builtin_elementwise_fma(p, E, c3_2);                                            \
      p = __builtin_elementwise_fma(p, E, c2_2);                                            \
      p = __builtin_elementwise_fma(p, E, ln2_2);                                           \
      const f32x2 ts = -E * p;                                                              \
      t = one2 - w;                                                                         \
      t.x = (w.x > 0.875f) ? ts.x : t.x;                                                    \
      t.y = (w.y > 0.875f) ? ts.y : t.y;                                                    \
    }                                                                                       \
    (TT) = t * t;                                                                           \
  }
  // node abscissae x_j = x0 + j dx in fp32 from hi + lo pairs of x0 and dx: t = fma(j, dx_hi, x0_hi) is rounded once (and is
  // exact where x0 and j dx cancel), the lo parts restore what the hi parts dropped; x_j is within 1 ulp of the double-precision
  // value rounded to fp32 (the node's own v_log_f32 error is ten times that)
  const float x0h = (float)x0, dxh = (float)dx;
  const float x0l = (fabsf(x0h) < __builtin_inff()) ? (float)(x0 - (double)x0h) : 0.0f;
  const float dxl = (fabsf(dxh) < __builtin_inff()) ? (float)(dx - (double)dxh) : 0.0f;
  const f32x2 x0h2 = {x0h, x0h}, x0l2 = {x0l, x0l}, dxh2 = {dxh, dxh}, dxl2 = {dxl, dxl};
  const f32x2 four2 = {4.0f, 4.0f};
  double sum = 0.0;
  int it = 0;
  f32x2 ja = {1.0f, 2.0f}, jb = {3.0f, 4.0f};  // node indices of the current pairs: small integers, exact in fp32
  // four nodes per iteration, two independent chains; their K_r are added in fp32 ({K_j + K_j+2, K_j+1 + K_j+3}, then the two
  // halves) and the group's sum goes into the double-precision accumulator.  Groups whose nodes may fall under the
  // |h| < 0.1 cut (wave-uniform test) take K_r = ksat1 there: the same operations otherwise, so a column's result does not
  // depend on its wavefront
  // The two pairs of a group go through the node formula in LOCKSTEP, statement by statement: every packed operation of a
  // node depends on the one before it, and a dependent operation cannot issue in the slot after its producer (the compiler
  // fills those slots with s_nop when it has nothing else) -- a wave that walks one chain after the other spends half its issue
  // slots waiting.  Same operations on the same operands as LGAR_GEFFM_PAIR, pair by pair: the same values bit for bit.
#define LGAR_GEFFM_GROUP(CUT, KIND, SINK)                                                   \
  {                                                                                         \
    const f32x2 xha = __builtin_elementwise_fma(ja, dxh2, x0h2), xhb = __builtin_elementwise_fma(jb, dxh2, x0h2); \
    const f32x2 xla = __builtin_elementwise_fma(ja, dxl2, x0l2), xlb = __builtin_elementwise_fma(jb, dxl2, x0l2); \
    const f32x2 xa = xha + xla, xb = xhb + xlb;                                             \
    f32x2 lga, lgb, ra, rb, Lca, Lcb, sa, sb, ta, tb;                                       \
    lga.x = lg2(xa.x); lgb.x = lg2(xb.x); lga.y = lg2(xa.y); lgb.y = lg2(xb.y);             \
    const f32x2 ua = nl2 * lga, ub = nl2 * lgb;                                             \
    const f32x2 laa = __builtin_elementwise_fma(n2, lga, ua), lab = __builtin_elementwise_fma(n2, lgb, ub); \
    ra.x = ex2(-laa.x); rb.x = ex2(-lab.x); ra.y = ex2(-laa.y); rb.y = ex2(-lab.y);         \
    const f32x2 ca = one2 + ra, cb = one2 + rb;                                             \
    Lca.x = lg2(ca.x); Lcb.x = lg2(cb.x); Lca.y = lg2(ca.y); Lcb.y = lg2(cb.y);             \
    const f32x2 da = ca - one2, db = cb - one2;                                             \
    f32x2 ica = __builtin_elementwise_fma(-ilog2, ca, two_ilog2), icb = __builtin_elementwise_fma(-ilog2, cb, two_ilog2); \
    const f32x2 rhoa = ra - da, rhob = rb - db;                                             \
    if ((KIND) != 1) {                                                                      \
      ica.x = fmaxf(ica.x, 0.0f); icb.x = fmaxf(icb.x, 0.0f); ica.y = fmaxf(ica.y, 0.0f); icb.y = fmaxf(icb.y, 0.0f); \
    }                                                                                       \
    const f32x2 La = __builtin_elementwise_fma(rhoa, ica, Lca), Lb = __builtin_elementwise_fma(rhob, icb, Lcb); \
    const f32x2 va = mml2 * La, vb = mml2 * Lb;                                             \
    const f32x2 Ea = __builtin_elementwise_fma(mm2, La, va), Eb = __builtin_elementwise_fma(mm2, Lb, vb); \
    const f32x2 ha = half2 * Ea, hb = half2 * Eb;                                           \
    const f32x2 ga = __builtin_elementwise_fma(hml2, laa, ha), gb = __builtin_elementwise_fma(hml2, lab, hb); \
    const f32x2 e1a = __builtin_elementwise_fma(hm2, laa, ga), e1b = __builtin_elementwise_fma(hm2, lab, gb); \
    sa.x = ex2(e1a.x); sb.x = ex2(e1b.x); sa.y = ex2(e1a.y); sb.y = ex2(e1b.y);             \
    f32x2 wa, wb, pa, pb, t1a, t1b;                                                         \
    if ((KIND) != 1) {                                                                      \
      wa.x = ex2(Ea.x); wb.x = ex2(Eb.x); wa.y = ex2(Ea.y); wb.y = ex2(Eb.y);               \
      t1a = one2 - wa; t1b = one2 - wb;                                                     \
    }                                                                                       \
    if ((KIND) != 2) {                                                                      \
      pa = __builtin_elementwise_fma(c5_2, Ea, c4_2); pb = __builtin_elementwise_fma(c5_2, Eb, c4_2); \
      pa = __builtin_elementwise_fma(pa, Ea, c3_2); pb = __builtin_elementwise_fma(pb, Eb, c3_2); \
      pa = __builtin_elementwise_fma(pa, Ea, c2_2); pb = __builtin_elementwise_fma(pb, Eb, c2_2); \
      pa = __builtin_elementwise_fma(pa, Ea, ln2_2); pb = __builtin_elementwise_fma(pb, Eb, ln2_2); \
      pa = -Ea * pa; pb = -Eb * pb;                                                         \
    }                                                                                       \
    if ((KIND) == 1) { t1a = pa; t1b = pb; }                                                \
    if ((KIND) == 0) {                                                                      \
      t1a.x = (wa.x > 0.875f) ? pa.x : t1a.x; t1b.x = (wb.x > 0.875f) ? pb.x : t1b.x;       \
      t1a.y = (wa.y > 0.875f) ? pa.y : t1a.y; t1b.y = (wb.y > 0.875f) ? pb.y : t1b.y;       \
    }                                                                                       \
    ta = t1a * t1a; tb = t1b * t1b;                                                         \
    if (CUT) {                                                                              \
      sa.x = (xa.x < xcutf) ? ksat1f : sa.x; sb.x = (xb.x < xcutf) ? ksat1f : sb.x;         \
      ta.x = (xa.x < xcutf) ? 1.0f : ta.x; tb.x = (xb.x < xcutf) ? 1.0f : tb.x;             \
      sa.y = (xa.y < xcutf) ? ksat1f : sa.y; sb.y = (xb.y < xcutf) ? ksat1f : sb.y;         \
      ta.y = (xa.y < xcutf) ? 1.0f : ta.y; tb.y = (xb.y < xcutf) ? 1.0f : tb.y;             \
    }                                                                                       \
    const f32x2 ka = sa * ta;                                                               \
    const f32x2 kb = __builtin_elementwise_fma(sb, tb, ka);                                 \
    SINK((double)(kb.x + kb.y))                                                             \
  }
#define LGAR_GEFFM_TO_SUM(v) sum = sum + (v);
  // Which of the two forms of t a node takes depends on 2^E > 7/8, and E rises monotonically with x = alpha h: the series
  // region is a PREFIX of the nodes (x > x_thr, the dry end), the difference region a suffix.  x_thr -- (1 + x^-n)^-m = 7/8 --
  // is a function of the layer's n alone; a node further than 1e-4 (relative) from it is decided whatever the rounding of
  // its E (1e-4 in x moves E by >= 1e-5, the computed E and 2^E are good to ~3e-7).  Each lane counts the leading nodes that
  // are series for certain and the first node from which all are differences for certain; the wavefront runs the series-only
  // form up to the smallest of the former, the difference-only form from the largest of the latter, the general form in
  // between -- every node gets exactly the value the general form alone would give it (bit for bit: tests/devsim).
  int ser_pairs = 0, dir_pair = pairs + 1;  // (a reversed or empty range, or NaN: the general form throughout)
  if constexpr (COOPERATE) {
    const int ngroups = pairs >> 1;  // the full groups of four interior nodes
    lds_exchange_point();            // (earlier loads of the table stay in front of these stores)
    for (int q = (r < lanes) ? r : ngroups; q < ngroups; q += lanes) {
      const float j0 = (float)(4 * q);
      ja = f32x2{j0 + 1.0f, j0 + 2.0f};
      jb = f32x2{j0 + 3.0f, j0 + 4.0f};
#define LGAR_GEFFM_TO_TAB(v) tab[q] = (v);
      LGAR_GEFFM_GROUP(true, 0, LGAR_GEFFM_TO_TAB)
#undef LGAR_GEFFM_TO_TAB
    }
    lds_exchange_point();
    {
      int q0 = 0;
      for (; q0 + 8 <= ngroups; q0 += 8) {
        double tq[8];
#pragma unroll
        for (int j = 0; j < 8; j++) tq[j] = tab[q0 + j];  // same address in every lane of the group: a broadcast
#pragma unroll
        for (int j = 0; j < 8; j++) sum = sum + tq[j];
      }
      for (; q0 < ngroups; q0++) sum = sum + tab[q0];
    }
    lds_exchange_point();
    it = 2 * ngroups;
    {
      const float j0 = (float)(4 * ngroups);
      ja = f32x2{j0 + 1.0f, j0 + 2.0f};
      jb = f32x2{j0 + 3.0f, j0 + 4.0f};
    }
  }
  if (!COOPERATE && dx < 0.0) {
    const float x_thr = pw(pw(8.0f / 7.0f, (float)l.inv_m) - 1.0f, -(float)l.inv_n);
    const double js_f = (x0 - (double)(x_thr * 1.0001f)) * inv_ndx - 1.0;  // nodes 1 .. js: x_j > x_thr (1 + 1e-4)
    const int js = (js_f > 0.0) ? ((js_f < double(M)) ? int(js_f) : M) : 0;
    ser_pairs = js >> 1;                                               // pairs 0 .. ser_pairs - 1 hold only such nodes
    const double jd_f = (x0 - (double)(x_thr * 0.9999f)) * inv_ndx + 2.0;  // nodes jd ..: x_j < x_thr (1 - 1e-4)
    const int jd = !(jd_f < double(M + 2)) ? M + 2 : ((jd_f > 0.0) ? int(jd_f) : 0);
    dir_pair = jd >> 1;                                                // pairs from dir_pair on hold only such nodes
  }
  LGAR_MEASURE_POINT(GEFFM_GENERAL_ONLY, ser_pairs, dir_pair, pairs)
  int ser_all = safe_pairs;  // the wavefront's: min of ser_pairs (at most safe_pairs), max of dir_pair
  if (!COOPERATE && any_lane(ser_pairs < ser_all) != 0ull) {
    ser_all = 0;
    for (int bit = 64; bit; bit >>= 1) {
      const int cand = ser_all + bit;
      if (cand <= safe_pairs && any_lane(ser_pairs < cand) == 0ull) ser_all = cand;
    }
  }
  int dir_all = 0;
  if constexpr (!COOPERATE) {
  for (int bit = 64; bit; bit >>= 1) {
    const int cand = dir_all + bit;
    if (any_lane(dir_pair >= cand) != 0ull) dir_all = cand;
  }
  LGAR_MEASURE_POINT(CLK, 13)
  for (; it + 1 < ser_all; it += 2, ja = ja + four2, jb = jb + four2) LGAR_GEFFM_GROUP(false, 1, LGAR_GEFFM_TO_SUM)
  const int it_a = it;
  for (; it + 1 < safe_pairs && it < dir_all; it += 2, ja = ja + four2, jb = jb + four2) LGAR_GEFFM_GROUP(false, 0, LGAR_GEFFM_TO_SUM)
  const int it_b = it;
  for (; it + 1 < safe_pairs; it += 2, ja = ja + four2, jb = jb + four2) LGAR_GEFFM_GROUP(false, 2, LGAR_GEFFM_TO_SUM)
  const int it_c = it;
  for (; it + 1 < pairs; it += 2, ja = ja + four2, jb = jb + four2) LGAR_GEFFM_GROUP(true, 0, LGAR_GEFFM_TO_SUM)
  LGAR_MEASURE_POINT(GEFFM_REGIONS, it_a >> 1, (it_b - it_a) >> 1, (it_c - it_b) >> 1, (it - it_c) >> 1)
  LGAR_MEASURE_POINT(CLK, 14)
  }
#undef LGAR_GEFFM_GROUP
#undef LGAR_GEFFM_TO_SUM
  const int rem = M - 2 * it;  // interior nodes left over by the groups of four: 0..3 (3 for the reference's 120 intervals)
  if (rem > 0) {             // ... as one more group whose surplus nodes count as zero
    const f32x2 xa = __builtin_elementwise_fma(ja, dxh2, x0h2) + __builtin_elementwise_fma(ja, dxl2, x0l2);
    const f32x2 xb = __builtin_elementwise_fma(jb, dxh2, x0h2) + __builtin_elementwise_fma(jb, dxl2, x0l2);
    f32x2 sa, ta, sb, tb;
    LGAR_GEFFM_PAIR(xa, sa, ta, 0)
    LGAR_GEFFM_PAIR(xb, sb, tb, 0)
    f32x2 ka = sa * ta, kb = sb * tb;
    ka.x = (xa.x < xcutf) ? ksat1f : ka.x;
    ka.y = (xa.y < xcutf) ? ksat1f : ka.y;
    kb.x = (xb.x < xcutf) ? ksat1f : kb.x;
    ka.y = (rem >= 2) ? ka.y : 0.0f;
    kb.x = (rem >= 3) ? kb.x : 0.0f;
    sum = sum + (double)((ka.x + kb.x) + ka.y);
  }
#undef LGAR_GEFFM_PAIR
  // end nodes in double precision, with the reference's own formulas (|h| < 0.1 -> Se = 1 applies to the LAST node only:
  // the first node's K is calc_k_from_se(Se_i) as it stands, green_ampt.py:60)
  // (the last node's Se is Se(h(Se_f)) in the reference: Se_f up to the rounding of the round trip)
  const double kn = (fabs(h_f) < 0.1 || h_f < 0.0) ? ksat1 : kn_own;
  const double res = fabs((0.5 * dh) * ((k0 + kn) + 2.0 * sum));
  const bool outside = is_nan(h_i) || is_nan(h_f);
  LGAR_MEASURE_POINT(CLK, 16)
  return outside ? res + (h_i + h_f) : res;
}
// calc_geff(theta1 -> theta2) in the mixed-precision mode: heads and end nodes from the two water contents (mixed_end).
// NOT inlined: its callers are the two call sites that run rarely (insert_water on a memo miss: 16 % of the wave-level
// evaluations; the dry-depth evaluation: 1 %) -- calc_dzdt, the hot one, has its own inlined copy (geff_mixed_heads).  Two fewer
// copies of the trapezoid in the kernel: 93 -> 52 spilled registers, and the size of the code is part of its speed (build.py).
// (Round 5, same-box A/B: inlined it is 1.7 % slower -- 30.2 against 29.7 ms, 130 spilled registers against 86 -- although the
// register saves around this call are 3.6 GB of the kernel's 13.5 GB of scratch write-back per launch.)
// (The layer's parameters travel as eight scalar arguments -- in registers.  A LayerK by reference is a struct the caller must
// first build in scratch memory: 64 bytes per lane stored at every call and loaded back by the callee, and by value the
// aggregate is past the 16 argument registers the ABI gives a struct, so it would go through scratch all the same.)
__device__ __attribute__((noinline)) double geff_mixed(double alpha, double n, double m, double inv_m, double inv_n, double ksat, double te,
                                                       double tr, double theta1, double theta2, int nint) {
  const LayerK<double> l{alpha, n, m, inv_m, inv_n, ksat, te, tr};
  const double se_i = se_from_theta(l, theta1);
  const double se_f = se_from_theta(l, theta2);
  // K_r at Se == 1 (the 1e-12 nudge of calc_k_from_se): (1 - (1e-12)^m)^2
  const double tsat = 1.0 - ex2p(l.m * LGAR_LOG2_1EM12);
  const double ksat1 = tsat * tsat;
  double h_i, h_f, k0, kn_own;
  mixed_end(l, se_i, h_i, k0);
  if (any_lane(se_f != 1.0) != 0ull) {
    mixed_end(l, se_f, h_f, kn_own);
  } else {  // every lane's wet end is saturated (theta_2 == theta_e: new fronts, infiltration): what mixed_end returns for Se == 1
    h_f = (1.0 / l.alpha) * ex2e(LGAR_LOG2_1EM12 * l.inv_n);
    kn_own = ksat1;
  }
  return geff_mixed_core(l, h_i, h_f, k0, kn_own, ksat1, nint);
}
// ... for cooperating lanes (MODE_MIXED_COOP: insert_water, the dry-depth evaluation): the same ends, the interior split over the lanes
__device__ __attribute__((noinline)) double geff_mixed_coop(double alpha, double n, double m, double inv_m, double inv_n, double ksat,
                                                            double te, double tr, double theta1, double theta2, int nint, double *tab,
                                                            int lanes, int r) {
  const LayerK<double> l{alpha, n, m, inv_m, inv_n, ksat, te, tr};
  const double se_i = se_from_theta(l, theta1);
  const double se_f = se_from_theta(l, theta2);
  const double tsat = 1.0 - ex2p(l.m * LGAR_LOG2_1EM12);
  const double ksat1 = tsat * tsat;
  double h_i, h_f, k0, kn_own;
  mixed_end(l, se_i, h_i, k0);
  mixed_end(l, se_f, h_f, kn_own);  // (geff_mixed's wave-wide shortcut for Se_f == 1 returns what mixed_end returns there)
  return geff_mixed_core<true>(l, h_i, h_f, k0, kn_own, ksat1, nint, tab, lanes, r);
}
// K(Se) / Ksat of both ends of a trapezoid (calc_k_from_se, utils.py:134-156, nudge included), the two evaluated in lockstep:
// each is a chain of two logarithms and two exponentials in which every operation waits for the one before it.
__device__ __forceinline__ void mixed_k_pair(const LayerK<double> &l, double se_a, double se_b, double &kr_a, double &kr_b) {
  const double qa = lg2e(se_a) * l.inv_m, qb = lg2e(se_b) * l.inv_m;
  const double oa = 1.0 - ex2e(qa), ob = 1.0 - ex2e(qb);  // 1 - Se^(1/m)
  const double ba = (fabs(oa) <= 1e-8) ? oa + 1e-12 : oa, bb = (fabs(ob) <= 1e-8) ? ob + 1e-12 : ob;
  const double ua = (oa == 0.0) ? LGAR_LOG2_1EM12 : lg2e(ba), ub = (ob == 0.0) ? LGAR_LOG2_1EM12 : lg2e(bb);
  const double ta = 1.0 - ex2e(l.m * ua), tb = 1.0 - ex2e(l.m * ub);
  kr_a = sqrt(se_a) * (ta * ta);
  kr_b = sqrt(se_b) * (tb * tb);
}
// calc_geff(theta1 -> theta2) for two FRONTS of the table, mixed-precision mode (calc_dzdt, calc_dry_depth): the heads are the
// fronts' own psi -- every front carries psi = h(Se(theta)) or the psi its theta was computed from (Column::move_wetting_front),
// so h(Se(theta)) need not be formed again: it would differ from psi by the rounding of the round trip, ~1e-10 relative, three
// orders below what the fp32 interior resolves -- and only K_r of the two end nodes is evaluated.  kr_f: K(theta2) / Ksat, which
// calc_dzdt needs as the front's own conductivity (Layer.py:1212-1216) and would otherwise compute a second time.
template <bool COOPERATE = false>
__device__ __forceinline__ double geff_mixed_heads(const LayerK<double> &l, double theta1, double theta2, double psi1, double psi2, int nint,
                                                   double &kr_f, double *tab = nullptr, int lanes = 0, int r = 0) {
  const double se_i = se_from_theta(l, theta1);
  const double se_f = se_from_theta(l, theta2);
  const double tsat = 1.0 - ex2p(l.m * LGAR_LOG2_1EM12);
  const double ksat1 = tsat * tsat;
  double k0, kn_own;
  LGAR_MEASURE_POINT(CLK, 11)
  mixed_k_pair(l, se_i, se_f, k0, kn_own);
  LGAR_MEASURE_POINT(CLK, 12)
  kr_f = kn_own;
  return geff_mixed_core<COOPERATE>(l, psi1, psi2, k0, kn_own, ksat1, nint, tab, lanes, r);
}

}  // namespace lgar
