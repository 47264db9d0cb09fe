// lgar_column.hpp -- device-side LGAR column physics for gfx950 (CDNA4), lane-per-column.
//
// One wavefront = 64 independent soil columns.  Per-front state of the wave lives in LDS as
// [field][front][lane] (lane-contiguous => bank-conflict-free for any per-lane front index), the
// per-layer van Genuchten parameters and the column scalars live in registers, and the time loop
// runs inside the kernel.  The scalar type S is float, double, or a forward-mode dual number
// (lgar_dual.hpp) for the differentiable path.
//
// What each routine computes follows the reference's Python (paths relative to
// /root/reference/dpLGAR/); the data layout and control structure do not: the reference keeps a
// linked list of Layer objects each owning a Python list of WettingFront objects, here a column is
// ONE flat top->bottom front array tagged with layer numbers.
#pragma once
#include "lgar_geff.hpp"

namespace lgar {

// ---------------------------------------------------------------------------------------------
// run-time constants shared by all columns (kernel argument -> SGPRs)
// ---------------------------------------------------------------------------------------------
template <typename R> struct Glob {
  R dt_h, initial_psi, pdm, wp_psi, frozen;
  R giuh[LGAR_GMAX];
  int nint, nsub, ng, bottom_mode, closed_form;
  long long iter_cap;
};

// LDS view of one lane's fronts: element i of field f sits at base[(f * FMAX + i) * WAVE] (one base address per lane; the
// field offsets are compile-time constants folded into the ds_read / ds_write offsets)
// STRIDE: table slots per front row -- 64, one per lane; the cooperating-lanes kernels (MODE_COOP) keep ONE table per group of
// lanes (LGAR_COOP_GROUPS slots: the lanes of a group hold the same column, read the same address -- an LDS broadcast -- and
// write the same value to it), which is what lets a 32-front table of such a wave fit four waves per CU.
#define LGAR_COOP_GROUPS 16
template <typename S, int FMAX, int STRIDE = WAVE> struct FrontsView {
  S *base;             // &lds.f[0][0][slot]
  unsigned char *fl;   // &lds.fl[0][slot]
  __device__ __forceinline__ S &Z(int i) const { return base[(0 * FMAX + i) * STRIDE]; }
  __device__ __forceinline__ S &TH(int i) const { return base[(1 * FMAX + i) * STRIDE]; }
  __device__ __forceinline__ S &PS(int i) const { return base[(2 * FMAX + i) * STRIDE]; }
  __device__ __forceinline__ S &DZ(int i) const { return base[(3 * FMAX + i) * STRIDE]; }
  __device__ __forceinline__ unsigned char &flag(int i) const { return fl[i * STRIDE]; }
  __device__ __forceinline__ int layer(int i) const { return fl[i * STRIDE] & 0x7f; }
  __device__ __forceinline__ bool bottom(int i) const { return (fl[i * STRIDE] & LGAR_FLAG_BOTTOM) != 0; }
  __device__ __forceinline__ void set_flag(int i, int layer, bool bottom) const {
    fl[i * STRIDE] = (unsigned char)(layer | (bottom ? LGAR_FLAG_BOTTOM : 0));
  }
  __device__ __forceinline__ void copy(int dst, int src) const {
    Z(dst) = Z(src); TH(dst) = TH(src); PS(dst) = PS(src); DZ(dst) = DZ(src);
    fl[dst * STRIDE] = fl[src * STRIDE];
  }
};

// ---------------------------------------------------------------------------------------------
// kernel modes
// ---------------------------------------------------------------------------------------------
// The values of the kernels' `int MODE` template parameter.  It stays an int: the kernels are looked up by their names
// (bench.py, the committed profiles: lgar_forward_kernel<float, 3, 8, 1>), and an enum type would name them differently.
// MODE_LITERAL: the reference's literal line searches, its update_psi pass and per-sub-step NaN scan.
// MODE_FAST (default of the engine, what bench.py measures): the same roots by bracketed Newton / closed-form jumps; the
// passes that are provably no-ops between events are skipped (see forward()).
// MODE_MIXED (double precision only, LgarDims.geff_mode = 1): MODE_FAST with the mixed-precision trapezoid (geff_mixed).
// MODE_COOP (double precision only, jobs under one wave per SIMD): MODE_FAST with cooperating lanes (geff_*_cooperative).
// MODE_MIXED_COOP: the mixed-precision trapezoid AND cooperating lanes.
constexpr int MODE_LITERAL = 0, MODE_FAST = 1, MODE_MIXED = 3, MODE_COOP = 4, MODE_MIXED_COOP = 6;

// Everything a kernel mode decides for a column of scalar type S, derived here once.  The scalar kind (f32, f64, dual, ...)
// comes from ScalarKind.
template <typename S, int MODE> struct ModeTraits : ScalarKind<S> {
  using K = ScalarKind<S>;
  static constexpr bool literal = MODE == MODE_LITERAL;                         // the reference's literal searches
  static constexpr bool mixed = MODE == MODE_MIXED || MODE == MODE_MIXED_COOP;  // the mixed-precision trapezoid
  static constexpr bool coop = MODE == MODE_COOP || MODE == MODE_MIXED_COOP;    // cooperating lanes
  // (the kernels instantiate the mixed-precision and cooperating-lanes modes with plain double only)
  static constexpr bool mixed_f64 = mixed && K::plain_f64;
  static constexpr bool coop_f64 = coop && K::plain_f64;
  // arithmetic policy (see POL_LEAN): verification mode in double precision uses the library pow (the reference's torch.pow);
  // the plain-float fast mode divides by reciprocal; the mixed-precision kernels take the lean pow with pairwise-combined
  // polynomials; everything else is lean pow + IEEE division
  static constexpr int pol = (literal && K::f64) ? POL_LIBRARY : (!literal && K::plain_f32) ? POL_RCP32 : mixed_f64 ? POL_MIXED : POL_LEAN;
  static constexpr int stride = coop ? LGAR_COOP_GROUPS : WAVE;  // front-table slots per row (see FrontsView)
  // MODE_MIXED, one lane per column: the GIUH queue is not held in registers at all.  It is touched once per sub-step and only
  // on storm steps -- which made its 16 registers the allocator's first spill victims, and a spilled read-modify-write is a
  // scratch store every time (5.5 of the kernel's 13.5 GB of write traffic, profiles/r05/ablate_giuh_queue.jsonl).  The
  // queue is updated in place in the column's own rows of the state arrays (`scalars` rows 3.., coalesced across the lanes),
  // where it is loaded from and stored to anyway; a flag remembers whether anything is queued (giuh_live, the reference's
  // `sum(queue) > 0` test evaluated when the queue was last written, lgar/giuh.py:8-20).
  static constexpr bool giuh_mem = MODE == MODE_MIXED && !K::dual;
  // MODE_MIXED: the accumulators of the forcing alone are added at the END of the sub-step, not where the reference adds them
  // (dpLGAR.py:185-190): nothing between the two places leaves the sub-step, the sums are the same, and two fewer values wait
  // through all of the column physics.  Same-box A/B, register allocation being what it is: the mixed-precision kernel 0.9 %
  // faster, the fp32 kernel 1.7 % slower -- so the former only.
  static constexpr bool late_forcing_sums = MODE == MODE_MIXED;
  // fast modes, one lane per column: the column mass as of the end of move_wetting_front (mass_and_events), still the ending
  // volume of the sub-step when no pass fired and no front was created after it.  (Cooperating lanes keep the separate walks:
  // their column mass sums a register copy of the table, and the event scan added to it costs a lone wave more in selects than
  // the scan's own walk -- configs[1] 78.4 -> 81.8 ms, one column 43.3 -> 45.9 ms, measured.)
  static constexpr bool fused_walk = !literal && !coop;
  // plain fp32 fast mode: a wave whose columns all hold a "top-layer table" (Column::top_table) takes the sweep, the walk after it
  // and calc_dzdt with the table's shape resolved at compile time (sweep_top, mass_and_events_top, calc_dzdt's `fast`): the same
  // leaf functions on the same operands in the same order, so the same bits as the generic step.  -DLGAR_NO_TOP_LAYER_STEP
  // compiles the kernels without it.
#ifndef LGAR_NO_TOP_LAYER_STEP
  static constexpr bool top_step = K::plain_f32 && !literal;
#else
  static constexpr bool top_step = false;
#endif
};

// ---------------------------------------------------------------------------------------------
// one soil column
// ---------------------------------------------------------------------------------------------
// Column::top_table (kernels with the top-layer step only: an empty base everywhere else, so that the other kernels' Column is
// the struct it was)
template <bool ON> struct TopTableFlag { bool top_table = false; };
template <> struct TopTableFlag<false> { static constexpr bool top_table = false; };

template <typename S, int NL, int FMAX, int MODE> struct Column : TopTableFlag<ModeTraits<S, MODE>::top_step> {
  using R = real_t<S>;
  using M = ModeTraits<S, MODE>;
  using TopTableFlag<M::top_step>::top_table;  // the front table is a top-layer table: see is_top_table
  static constexpr int POL = M::pol;  // (the leaf functions' policy argument, everywhere below)
  const ColParams<S, NL> &P;
  const LGAR_KARG Glob<R> *G;  // run-time constants, in the kernarg segment (re-pointed by the kernel's time loop)
  FrontsView<S, FMAX, M::stride> F;
  int nf;
  int status;
  S ponded_water, previous_precip, ending_volume;
  S giuh_q[LGAR_GMAX];
  static constexpr int DEAD = LGAR_ST_BOTTOM | LGAR_ST_OVERFLOW | LGAR_ST_STRUCT;  // forward() leaves such a column alone
  R *giuh_mem = nullptr;   // &scalars[3 * N + c]
  size_t giuh_stride = 0;  // N
  bool giuh_live = false;
  // K(theta) is not kept per front: the reference refreshes it from theta for every front but the deepest at the end
  // of each move (update_psi, Layer.py:1166-1170) and reads it only in calc_dzdt, so it is computed there, for moving
  // fronts only.  k_deepest is the one K that is never refreshed (the domain's deepest front keeps its initial K);
  // new_front_frozen marks a front created in the current sub-step, whose K carries frozen_factor (Layer.py:1410-1412).
  S k_deepest;
  bool new_front_frozen;
  // insert_water's Geff of the last call and what it was computed from (see insert_water): layer -1 = nothing remembered
  S memo_theta, memo_g;
  int memo_layer = -1;
  unsigned near_sat_fronts = 0u;  // fronts whose psi the fast modes must send through the reference's theta -> psi round trip
  S post_mass;  // (M::fused_walk: the column mass of mass_and_events)
  bool post_mass_valid = false;
  bool post_event = false;
  bool psi_rewritten = false;  // a dry-over-wet deletion below the top layer rewrote theta and psi of the fronts above (q13)
  S aet_psi_wp_memo;          // calc_aet's half-uptake head of this column (a function of the top layer's parameters only)
  bool aet_psi_wp_known = false;
  bool count_geff = false;              // measurement: count wave-level Geff evaluations in the unused upper bits of `status`
  int share_lanes = 0;                  // tangent kernels: W = 2..32 adjacent lanes carry this same column (other directions);
                                        // forward kernels: 2..64 = that many adjacent lanes carry this very column (small jobs)
  R *xchg = nullptr;                    // ... and the wave's LDS buffer they exchange trapezoid nodes through
  int coop_rank = 0;                    // forward kernels: my place in my group of cooperating lanes
  int cap = FMAX;                       // fronts this column may hold: min(kernel capacity, rows of the state arrays)
  // accumulators drained every forcing step (physics/MassBalance.py:45-53)
  S a_precip, a_pet, a_aet, a_infil, a_runoff, a_perc, a_giuh, a_disch;

  __device__ Column(const ColParams<S, NL> &p, const LGAR_KARG Glob<R> *g, const FrontsView<S, FMAX, M::stride> &f) : P(p), G(g), F(f) {}

  __device__ __forceinline__ S cum_at(int k) const { return sel<S, NL>(P.cum, k); }
  // calc_geff (lgar/green_ampt.py:19-99): trapezoid or closed form, per cfg.data.use_closed_form_G
  __device__ __forceinline__ S capillary_drive(const LayerK<S> &lk, S theta1, S theta2, int site = 0, CoopRiders *riders = nullptr) {
    (void)site; (void)riders;
    LGAR_MEASURE_POINT(NOGEFF, lk, theta1, theta2)
    LGAR_COUNT_GEFF_CALL(site)
    LGAR_MEASURE_POINT(DUP_GEFF, lk, theta1, theta2)
    if constexpr (M::literal && M::f64) {
      // verification mode: the reference's trapezoid operation by operation (4 pow + sqrt per node, running h)
      return G->closed_form ? geff_closed<S, POL>(lk, theta1, theta2) : geff_literal<S, POL>(lk, theta1, theta2, G->nint);
    }
    if constexpr (M::dual && M::f64 && !M::literal) {
      if (share_lanes >= 2 && !G->closed_form) return geff_fused<S>(lk, theta1, theta2, G->nint, xchg, share_lanes);
    }
    if constexpr (M::coop_f64 && !M::mixed) {  // plain double: cooperating lanes (small jobs)
      if (share_lanes > 1 && !G->closed_form) return geff_fused<S>(lk, theta1, theta2, G->nint, xchg, share_lanes, coop_rank, riders);
    }
    if constexpr (M::coop_f64 && M::mixed) {  // mixed-precision trapezoid, its groups of nodes split over the lanes
      if (share_lanes > 1 && !G->closed_form)
        return geff_mixed_coop(val(lk.alpha), val(lk.n), val(lk.m), val(lk.inv_m), val(lk.inv_n), val(lk.ksat), val(lk.te), val(lk.tr),
                               theta1, theta2, G->nint, xchg, share_lanes, coop_rank);
    }
    if constexpr (M::mixed_f64) {  // plain double, LgarDims.geff_mode = 1
      if (!G->closed_form)
        return geff_mixed(val(lk.alpha), val(lk.n), val(lk.m), val(lk.inv_m), val(lk.inv_n), val(lk.ksat), val(lk.te), val(lk.tr),
                          theta1, theta2, G->nint);
    }
#ifndef LGAR_NO_F32_RARE_GEFF
    if constexpr (M::plain_f32 && !M::literal) {  // plain float: the rare sites (2 dry depth, 3 insert_water) share one out-of-line body
      if (site != 1 && !G->closed_form)
        return geff_f32_rare(lk.alpha, lk.n, lk.m, lk.inv_m, lk.inv_n, lk.te, lk.tr, theta1, theta2, G->nint);
    }
#endif
    return G->closed_form ? geff_closed<S, POL>(lk, theta1, theta2) : geff(lk, theta1, theta2, G->nint);
  }
  // calc_geff between two FRONTS of the table in the mixed-precision mode (calc_dzdt): the fronts' own psi are the trapezoid's
  // heads, and K(theta2) / Ksat of its wet end node is handed back -- the front's own conductivity (geff_mixed_heads).
  __device__ __forceinline__ double capillary_drive_fronts(const LayerK<double> &lk, double theta1, double theta2, double psi1,
                                                           double psi2, double &kr_end) {
    LGAR_MEASURE_POINT(NOGEFF_FRONTS, lk, theta1, theta2, kr_end)
    LGAR_COUNT_GEFF_CALL(1)
    if constexpr (M::coop && M::mixed) {
      if (share_lanes > 1) return geff_mixed_heads<true>(lk, theta1, theta2, psi1, psi2, G->nint, kr_end, xchg, share_lanes, coop_rank);
    }
    return geff_mixed_heads(lk, theta1, theta2, psi1, psi2, G->nint, kr_end);
  }
  __device__ __forceinline__ S cum_prev(int k) const {  // cum[k-1], 0 for k == 0
    S r = S(R(0.0));
#pragma unroll
    for (int j = 0; j < NL - 1; j++) {
      const S cj = P.cum[j];
      r = choose(k == j + 1, cj, r);
    }
    return r;
  }

  // WettingFront.is_equal (by VALUE), layers/WettingFront.py:76-84
  __device__ __forceinline__ bool feq(int a, int b) const {
    return val(F.Z(a)) == val(F.Z(b)) && val(F.PS(a)) == val(F.PS(b)) && val(F.DZ(a)) == val(F.DZ(b));
  }
  __device__ __forceinline__ void fdel(int i) {
    for (int j = i; j < nf - 1; j++) F.copy(j, j + 1);
    nf--;
  }
  // first flat index of layer k and the number of fronts tagged k
  __device__ __forceinline__ void range_of(int k, int &lo, int &len) const {
    lo = -1; len = 0;
    for (int i = 0; i < nf; i++)
      if (F.layer(i) == k) { if (len == 0) lo = i; len++; }
  }

  // Top-layer table: m = nf - NL >= 1 in-layer fronts of layer 0 (flag 0: tagged 0, no boundary front), then the boundary fronts
  // of layers 0 .. NL-1 in order -- what a column holds while its wetting fronts are all still inside the top layer (three
  // quarters of the bench's wave-steps hold it in all 64 lanes, profiles/EXPERIMENTS.md round 8).  The flags and nf change only in
  // the event passes and in create_surficial_front, never in the sweep: the predicate is evaluated when the state is loaded and
  // after those two (both rare), and costs nothing in a step without them.
  __device__ __forceinline__ bool is_top_table() const {
    const int m = nf - NL;
    bool t = m >= 1;
    for (int i = 0; i < nf; i++) {
      const int f = F.flag(i);
      t = t && (f == ((i < m) ? 0 : ((i - m) | LGAR_FLAG_BOTTOM)));
    }
    return t;
  }

  // Cooperating lanes (one wave alone on its SIMD): every dependent LDS read is ~130 cycles nothing else covers, and the column
  // mass reads the front table row by row.  A table of at most SCAN fronts (the usual case) is fetched in ONE round trip
  // instead, and the sum runs on registers with the row index a compile-time constant: the same terms in the same order, so the
  // same result bit for bit.  (The event scan and the free-drainage search gained nothing from the same treatment: what they
  // save in waits they spend on selects.)
  static constexpr int SCAN = 8;
  struct Rows {
    R z[SCAN], th[SCAN];
    int fl[SCAN];
  };
  __device__ __forceinline__ void fetch_rows(Rows &r) const {
#pragma unroll
    for (int q = 0; q < SCAN; q++) {
      r.z[q] = val(F.Z(q));
      r.th[q] = val(F.TH(q));
      r.fl[q] = F.flag(q);
    }
  }

  // Layer.mass_balance, layers/Layer.py:795-824 (layer sums combined s0 + (s1 + (s2 ...)))
  __device__ __forceinline__ S mass_balance() const {
    S ls[NL];
    if constexpr (M::coop_f64) {
      if (nf <= SCAN) {  // cooperating lanes: the table's first rows in one fetch (see Rows)
        Rows r;
        fetch_rows(r);
#pragma unroll
        for (int j = 0; j < NL; j++) ls[j] = S(R(0.0));
#pragma unroll
        for (int q = 0; q < SCAN; q++) {
          const bool on = q < nf;
          const int lay = r.fl[q] & 0x7f;
          const bool next_same = (q + 1 < nf) && ((r.fl[(q + 1 < SCAN) ? q + 1 : q] & 0x7f) == lay);
          const R dth = next_same ? r.th[q] - r.th[(q + 1 < SCAN) ? q + 1 : q] : r.th[q];
          R base = R(0.0);
#pragma unroll
          for (int j = 1; j < NL; j++) base = choose(lay == j, val(P.cum[j]) - val(P.thick[j]), base);
          const R term = (r.z[q] - base) * dth;
#pragma unroll
          for (int j = 0; j < NL; j++) ls[j] = choose(on && lay == j, ls[j] + term, ls[j]);  // (a layer's fronts are adjacent:
        }                                                                                  //  each sum grows in table order)
        S tot = ls[NL - 1];
#pragma unroll
        for (int j = NL - 2; j >= 0; j--) tot = ls[j] + tot;
        return tot;
      }
    }
    int i = 0;
#pragma unroll
    for (int j = 0; j < NL; j++) {
      S base = (j == 0) ? S(R(0.0)) : P.cum[j] - P.thick[j];
      S sum = S(R(0.0));
      while (i < nf && F.layer(i) == j) {
        bool next_same = (i + 1 < nf) && (F.layer(i + 1) == j);
        S dth = next_same ? (F.TH(i) - F.TH(i + 1)) : F.TH(i);
        sum = sum + (F.Z(i) - base) * dth;
        i++;
      }
      ls[j] = sum;
    }
    S tot = ls[NL - 1];
#pragma unroll
    for (int j = NL - 2; j >= 0; j--) tot = ls[j] + tot;
    return tot;
  }

  // Layer.mass_balance AND the triggers of the post-sweep passes (front_event_pending) in ONE walk over the front table: both
  // read every front's depth, theta and tag, and between the sweep and the end of a sub-step nothing else changes them unless a
  // pass fires or a surficial front is created -- so the fast modes walk the table once per sub-step instead of three times
  // (column-mass check, event scan, ending volume).  The mass is mass_balance()'s, term by term in the same order.
  __device__ __forceinline__ S mass_and_events(bool &ev) const {
    S ls[NL];
    bool e = false;
    int i = 0;
#pragma unroll
    for (int j = 0; j < NL; j++) {
      S base = (j == 0) ? S(R(0.0)) : P.cum[j] - P.thick[j];
      S sum = S(R(0.0));
      while (i < nf && F.layer(i) == j) {
        const bool has_next = i + 1 < nf;
        const int fn = has_next ? F.flag(i + 1) : 0;
        const bool next_same = has_next && ((fn & 0x7f) == j);
        const S zi = F.Z(i), ti = F.TH(i);
        if (has_next) {
          const S zn = F.Z(i + 1), tn = F.TH(i + 1);
          e = e || (next_same && !(fn & LGAR_FLAG_BOTTOM) && val(zi) > val(zn));
          e = e || (next_same && val(ti) <= val(tn));
          e = e || (val(zi) > val(P.cum[j]));
          sum = sum + (zi - base) * (next_same ? (ti - tn) : ti);
        } else {
          sum = sum + (zi - base) * ti;
        }
        i++;
      }
      ls[j] = sum;
    }
    S tot = ls[NL - 1];
#pragma unroll
    for (int j = NL - 2; j >= 0; j--) tot = ls[j] + tot;
    ev = e;
    return tot;
  }

  // ... and the same walk over a top-layer table (is_top_table): fronts 0 .. m are layer 0's, front m its boundary front, then
  // one boundary front per layer -- no tag is read, every front is read once.  The terms, the tests and their order are
  // mass_and_events' on such a table (a boundary front is never "passed"; the domain's deepest front is tested against nothing).
  __device__ __forceinline__ S mass_and_events_top(bool &ev) const {
    const int m = nf - NL;
    S ls[NL];
    bool e = false;
    const S base0 = S(R(0.0));
    S sum = S(R(0.0));
    S zi = F.Z(0), ti = F.TH(0);
    for (int i = 0; i < m; i++) {
      const S zn = F.Z(i + 1), tn = F.TH(i + 1);
      e = e || (i + 1 < m && val(zi) > val(zn));
      e = e || (val(ti) <= val(tn));
      e = e || (val(zi) > val(P.cum[0]));
      sum = sum + (zi - base0) * (ti - tn);
      zi = zn; ti = tn;
    }
    e = e || (val(zi) > val(P.cum[0]));
    sum = sum + (zi - base0) * ti;
    ls[0] = sum;
#pragma unroll
    for (int j = 1; j < NL; j++) {
      const S base = P.cum[j] - P.thick[j];
      const S z = F.Z(m + j), t = F.TH(m + j);
      if (j < NL - 1) e = e || (val(z) > val(P.cum[j]));
      ls[j] = S(R(0.0)) + (z - base) * t;
    }
    S tot = ls[NL - 1];
#pragma unroll
    for (int j = NL - 2; j >= 0; j--) tot = ls[j] + tot;
    ev = e;
    return tot;
  }

  // calc_wetting_front_free_drainage, Layer.py:134-162: argmin psi, ties (and isclose) go deeper
  __device__ __forceinline__ int free_drainage_front() const {
    R psi = val(F.PS(0));
    int idx = 0;
    for (int i = 0; i < nf; i++) {
      R pi = val(F.PS(i));
      if (pi <= psi) { psi = pi; idx = i; }
      else if (ab(pi - psi) <= R(1e-8) + R(1e-5) * ab(psi)) { psi = pi; idx = i; }
    }
    return idx;
  }

  // theta(psi) and d theta / d psi of one layer in plain reals (no extra pow for the slope:
  // theta' = -(theta - theta_r) m n (a psi)^n / (psi (1 + (a psi)^n)))
  __device__ __forceinline__ static void theta_slope(R alpha, R n, R m, R te, R tr, R psi, R &th, R &dth) {
    R ap = pwp<POL>(alpha * psi, n);
    R one_ap = R(1.0) + ap;
    R op = pwp<POL>(one_ap, m);
    R span = dv<POL>(R(1.0), op) * (te - tr);
    th = span + tr;
    dth = (psi > R(0.0)) ? dv<POL>(-(span * m * n * ap), psi * one_ap) : R(0.0);
  }

  // ... and the second derivative (the double-precision searches fit a power law through value, slope and curvature):
  // theta'' = theta' ((n - 1) - n (a psi)^n) / (psi (1 + (a psi)^n)).  theta is theta_from_h's operation by operation.
  __device__ __forceinline__ static void theta_slope2(R alpha, R n, R m, R te, R tr, R psi, R &th, R &dth, R &d2th) {
    R ap = pwp<POL>(alpha * psi, n);
    R one_ap = R(1.0) + ap;
    R op = pwp<POL>(one_ap, m);
    R span = dv<POL>(R(1.0), op) * (te - tr);
    th = span + tr;
    const R r = (psi > R(0.0)) ? dv<POL>(R(1.0), psi * one_ap) : R(0.0);
    dth = -(span * m * n * ap) * r;
    d2th = dth * ((n - R(1.0)) - n * ap) * r;
  }

  // search_mode 1: the same root -- psi with |sum_j thick_j (theta_j(psi) - dtheta_j) - prior_mass| <= tolerance --
  // found by a bracketed iteration on the mass and its derivatives (3-5 mass evaluations) instead of the reference's
  // fixed-step decimal search (58-82 on average, Layer.py:275-317).  theta differs from the literal search by
  // <= tolerance / thickness.
  // Gradient semantics (dual numbers): psi_final = psi_init + constant, as in the reference (Layer.py:277-288).
  // Cooperating lanes (MODE_COOP: the lanes of a group carry the SAME column): a mass evaluation is K + 1 independent
  // theta(psi) -- two pows each -- so lane r of the group evaluates layer min(r, K) with that layer's parameters as its
  // operands (ONE instruction stream) and the group exchanges the results through its LDS table; the sums are formed from
  // them in the serial order.  Every value goes through exactly the operations of the serial evaluation: bit-identical.
  // FirstEval: what the sweep evaluated BEFORE a search (sweep_layer; coop_sweep_thetas for cooperating lanes): theta and its
  // two derivatives for the layers above and the front's own layer at the front's psi -- the search's first mass evaluation
  struct FirstEval {
    bool have = false;
    R M = R(0.0), dM = R(0.0), d2M = R(0.0);  // the mass sum of the search (layers above first, in order, then the own layer)
    R thk = R(0.0);                           // theta of the front's own layer at its psi
    __device__ __forceinline__ void add(R thick, R th, R below, R dth, R d2th) {
      M += thick * (th - below);
      dM += thick * dth;
      d2M += thick * d2th;
    }
  };

  // Single precision keeps the plain bracketed Newton iteration (its pow is three instructions; the kernel is not bound by
  // this search).
  template <int K>
  __device__ __forceinline__ S theta_mass_balance_newton_f32(const LayerK<S> &lk, S psi0, S new_mass, S prior_mass,
                                                             const S (&dth)[NL], const S (&dthick)[NL], S dth_k, S dthick_k) {
    const R prior = val(prior_mass);
    R psi = val(psi0);
    R f = val(new_mass) - prior;
    if (ab(f) <= Tol<R>::mass) return theta_from_h<S, POL>(lk, psi0);
    R M = R(0.0), dM = R(0.0);
    auto eval = [&](R x) {
      R thk, dthk;
      theta_slope(val(lk.alpha), val(lk.n), val(lk.m), val(lk.te), val(lk.tr), x, thk, dthk);
      M = val(dthick_k) * (thk - val(dth_k));
      dM = val(dthick_k) * dthk;
#pragma unroll
      for (int j = 0; j < K; j++) {
        R t1, d1;
        theta_slope(val(P.alpha[j]), val(P.n[j]), val(P.m[j]), val(P.te[j]), val(P.tr[j]), x, t1, d1);
        M += val(dthick[j]) * (t1 - val(dth[j]));
        dM += val(dthick[j]) * d1;
      }
    };
    R lo = R(0.0), hi = R(-1.0);  // bracket f(lo) > 0 > f(hi); hi < 0: not found yet
    bool lo_ok = false;
    eval(psi);
    f = M - prior;
    for (int it = 0; it < 64; it++) {
      if (ab(f) <= Tol<R>::mass) break;
      if (f > R(0.0)) {
        lo = psi;
        lo_ok = true;
      } else {
        hi = psi;
        if (!lo_ok) {
          // is the target reachable at all?  mass at psi = 0 (saturation) needs no pow
          R M0 = val(dthick_k) * (((val(lk.te) - val(lk.tr)) + val(lk.tr)) - val(dth_k));
#pragma unroll
          for (int j = 0; j < K; j++) M0 += val(dthick[j]) * (((val(P.te[j]) - val(P.tr[j])) + val(P.tr[j])) - val(dth[j]));
          if (M0 - prior <= Tol<R>::mass) { psi = R(0.0); break; }  // saturated: the reference walks psi -> 0 (Layer.py:287-316)
          lo_ok = true;
        }
      }
      R pn = (dM < R(0.0)) ? psi - dv<POL>(f, dM) : R(-1.0);
      const bool inside = (pn > lo) && (hi < R(0.0) || pn < hi);
      if (!inside) pn = (hi >= R(0.0)) ? R(0.5) * (lo + hi) : psi * R(2.0) + R(1.0);
      if (pn == psi) break;  // step below resolution
      psi = pn;
      eval(psi);
      f = M - prior;
      if (it == 63) status |= LGAR_ST_ITERCAP;
    }
    const S psi_final = psi0 + (psi - val(psi0));
    return theta_from_h<S, POL>(lk, psi_final);
  }

  // Double precision (plain and dual numbers): the column mass M(psi) is, layer by layer, close to a shifted power law of psi
  // -- theta - theta_e ~ -(alpha psi)^n towards saturation, theta - theta_r ~ (alpha psi)^(1-n) in dry soil -- so every step
  // fits M ~ A - C psi^p through the value, slope and curvature of the present iterate (p = 1 + psi M''/M') and solves that
  // model for the target: psi_next = psi (1 - p f / (psi M'))^(1/p).  Third order like Halley's method, exact for a power law:
  // 3 mass evaluations where Newton took 4-5 (f: 1e-2 -> 1e-6 -> 1e-16), and 4-5 where Newton, started from a front that had
  // just crossed a layer boundary all but saturated (psi ~ 1e-8, M' ~ 0), overshot by six decades and bisected its way back
  // in 12-16 -- a wavefront waits for its slowest lane, so that tail was most of the search's wave-level cost.  The step itself
  // costs no double-precision pow: a long step (|t| > 1/64, t = f / (psi M')) takes ratio^(1/p) from the hardware's single-
  // precision log2 / exp2 (an iterate need not be better than the model), a short one its series in t to third order
  // (psi_next good to ~t^4: the final steps, t ~ 1e-5, lose nothing).  The bracket (lo, hi) and the bisection fallback are
  // the Newton version's; so are the termination test -- the true mass, in double precision, within the reference's tolerance
  // of the target -- and the saturated exit.
  template <int K>
  __device__ __forceinline__ S theta_mass_balance_newton(const LayerK<S> &lk, S psi0, S new_mass, S prior_mass,
                                                         const S (&dth)[NL], const S (&dthick)[NL], S dth_k, S dthick_k,
                                                         const FirstEval &fe) {
    if constexpr (M::f32) {
      (void)fe;
      return theta_mass_balance_newton_f32<K>(lk, psi0, new_mass, prior_mass, dth, dthick, dth_k, dthick_k);
    } else {
    const R prior = val(prior_mass);
    R psi = val(psi0);
    R f = val(new_mass) - prior;
    if (ab(f) <= Tol<R>::mass) return theta_from_h<S, POL>(lk, psi0);
    R M = R(0.0), dM = R(0.0), d2M = R(0.0);
    // my share of a mass evaluation (cooperating lanes): layer c_q's parameters
    R c_al = val(lk.alpha), c_n = val(lk.n), c_m = val(lk.m), c_te = val(lk.te), c_tr = val(lk.tr);
    int c_q = K;
    bool together = false;
    R last_x = R(-1.0), last_th = R(0.0);  // the own layer's theta of the latest mass evaluation, and its psi
    if constexpr (M::coop_f64 && K > 0) {
      together = share_lanes > K;
      c_q = coop_rank < K ? coop_rank : K;
#pragma unroll
      for (int j = 0; j < K; j++) {
        const bool mine = c_q == j;
        c_al = choose(mine, val(P.alpha[j]), c_al); c_n = choose(mine, val(P.n[j]), c_n); c_m = choose(mine, val(P.m[j]), c_m);
        c_te = choose(mine, val(P.te[j]), c_te); c_tr = choose(mine, val(P.tr[j]), c_tr);
      }
    }
    auto sums = [&](R thk, R dthk, R d2thk, const R (&tj)[NL], const R (&dj)[NL], const R (&ej)[NL]) {
      M = val(dthick_k) * (thk - val(dth_k));
      dM = val(dthick_k) * dthk;
      d2M = val(dthick_k) * d2thk;
#pragma unroll
      for (int j = 0; j < K; j++) {
        M += val(dthick[j]) * (tj[j] - val(dth[j]));
        dM += val(dthick[j]) * dj[j];
        d2M += val(dthick[j]) * ej[j];
      }
    };
    auto eval = [&](R x) {
      R thk, dthk, d2thk;
      if constexpr (M::coop_f64 && K > 0) {
        if (together) {
          R th, dt, d2, tj[NL], dj[NL], ej[NL];
          theta_slope2(c_al, c_n, c_m, c_te, c_tr, x, th, dt, d2);
          xchg[3 * c_q] = th;  // (lanes with the same c_q store the same value to the same address)
          xchg[3 * c_q + 1] = dt;
          xchg[3 * c_q + 2] = d2;
          lds_exchange_point();
          thk = xchg[3 * K];
          dthk = xchg[3 * K + 1];
          d2thk = xchg[3 * K + 2];
#pragma unroll
          for (int j = 0; j < K; j++) { tj[j] = xchg[3 * j]; dj[j] = xchg[3 * j + 1]; ej[j] = xchg[3 * j + 2]; }
          lds_exchange_point();
          sums(thk, dthk, d2thk, tj, dj, ej);
          last_x = x;
          last_th = thk;
          return;
        }
      }
      theta_slope2(val(lk.alpha), val(lk.n), val(lk.m), val(lk.te), val(lk.tr), x, thk, dthk, d2thk);
      M = val(dthick_k) * (thk - val(dth_k));
      dM = val(dthick_k) * dthk;
      d2M = val(dthick_k) * d2thk;
#pragma unroll
      for (int j = 0; j < K; j++) {
        R t1, d1, e1;
        theta_slope2(val(P.alpha[j]), val(P.n[j]), val(P.m[j]), val(P.te[j]), val(P.tr[j]), x, t1, d1, e1);
        M += val(dthick[j]) * (t1 - val(dth[j]));
        dM += val(dthick[j]) * d1;
        d2M += val(dthick[j]) * e1;
      }
      last_x = x;
      last_th = thk;
    };
    R lo = R(0.0), hi = R(-1.0);  // bracket f(lo) > 0 > f(hi); hi < 0: not found yet
    bool lo_ok = false;
    if (fe.have) {  // evaluated by the sweep, with its own thetas
      M = fe.M; dM = fe.dM; d2M = fe.d2M;
      last_x = psi;
      last_th = fe.thk;
    } else {
      eval(psi);
    }
    f = M - prior;
    const R theta_sat = (val(lk.te) - val(lk.tr)) + val(lk.tr);  // theta_from_h at psi = 0, operation by operation
    for (int it = 0; it < 64; it++) {
      if (ab(f) <= Tol<R>::mass) break;
      if (f > R(0.0)) {
        lo = psi;
        lo_ok = true;
      } else {
        hi = psi;
        if (!lo_ok) {
          // is the target reachable at all?  mass at psi = 0 (saturation) needs no pow
          R M0 = val(dthick_k) * (theta_sat - val(dth_k));
#pragma unroll
          for (int j = 0; j < K; j++) M0 += val(dthick[j]) * (((val(P.te[j]) - val(P.tr[j])) + val(P.tr[j])) - val(dth[j]));
          if (M0 - prior <= Tol<R>::mass) {  // saturated: the reference walks psi -> 0 (Layer.py:287-316)
            psi = R(0.0);
            last_x = R(0.0);
            last_th = theta_sat;
            break;
          }
          lo_ok = true;
        }
      }
      R pn = R(-1.0);
      if (dM < R(0.0) && psi > R(0.0)) {
        const R ipd = dv<POL>(R(1.0), psi * dM);
        const R t = f * ipd;                                  // the Newton step, relative to psi (negated)
        const R p = R(1.0) + (psi * psi) * d2M * ipd;         // exponent of the power law through (M, M', M'')
        const R ratio = R(1.0) - p * t;
        if (ab(t) <= R(0.015625)) {
          // psi (ratio^(1/p) - 1) = psi (-t + (1 - p) t^2 / 2 - (2 p - 1)(p - 1) t^3 / 6 + O(t^4))
          const R c2 = R(0.5) * (R(1.0) - p), c3 = (R(2.0) * p - R(1.0)) * (p - R(1.0)) * R(1.0 / 6.0);
          pn = psi - (psi * t) * (R(1.0) - t * (c2 - c3 * t));
        } else if (ratio > R(0.0)) {
          const float pf = (float)p, tf = (float)t;
          const float e = (fabsf(pf) > 1e-4f) ? lg2((float)ratio) * rcp32(pf) : -1.44269504f * tf;  // p -> 0: M ~ A - C log psi
          pn = psi * (R)ex2(e);
        }
      }
      const bool inside = (pn > lo) && (hi < R(0.0) || pn < hi);
      if (!inside) pn = (hi >= R(0.0)) ? R(0.5) * (lo + hi) : psi * R(2.0) + R(1.0);
      if (pn == psi) break;  // step below resolution
      psi = pn;
      eval(psi);
      f = M - prior;
      if (it == 63) status |= LGAR_ST_ITERCAP;
    }
    if constexpr (!M::dual) {
      // plain reals: theta(psi) was part of the last mass evaluation (theta_slope2's theta is theta_from_h's)
      if (psi == last_x) return S(last_th);
      return theta_from_h<S, POL>(lk, S(psi));
    } else {
      // dual numbers: psi_final = psi_init + constant, as in the reference's autograd (Layer.py:277-288)
      const S psi_final = psi0 + (psi - val(psi0));
      return theta_from_h<S, POL>(lk, psi_final);
    }
    }
  }

  // theta_mass_balance, Layer.py:242-318 (+ recalculate_mass :211-240).  k = the front's layer;
  // dth/dthick hold the entries of the layers above (j < K), dth_k/dthick_k the front's own.
  template <int K>
  __device__ __forceinline__ S theta_mass_balance(const LayerK<S> &lk, S psi, S new_mass, S prior_mass, const S (&dth)[NL],
                                  const S (&dthick)[NL], S dth_k, S dthick_k, const FirstEval &fe = FirstEval()) {
    R delta_mass = ab(val(new_mass) - val(prior_mass));
    bool switched = false;
    R factor = R(1.0);
    S theta = S(R(0.0));
    S psi_prev = psi;  // a tensor in the reference: psi_prev * 0.1 below carries its gradient
    R delta_mass_prev = delta_mass;
    int count_no_change = 0;
    if (delta_mass <= Tol<R>::mass) {
      if constexpr (!M::dual) {
        if (fe.have) return S(fe.thk);  // theta_from_h(lk, psi), evaluated by the sweep
      }
      return theta_from_h<S, POL>(lk, psi);
    }
    LGAR_MEASURE_POINT(NOSEARCH, lk, psi, new_mass)
    if constexpr (!M::literal) return theta_mass_balance_newton<K>(lk, psi, new_mass, prior_mass, dth, dthick, dth_k, dthick_k, fe);
    long long it = 0;
    while (delta_mass > Tol<R>::mass) {
      if (++it > G->iter_cap) { status |= LGAR_ST_ITERCAP; break; }
      if (val(new_mass) > val(prior_mass)) {
        psi = psi + (R(0.1) * factor);
        switched = false;
      } else {
        if (!switched) { switched = true; factor = factor * R(0.1); }
        psi_prev = psi;
        psi = psi - (R(0.1) * factor);
        if (val(psi) < R(0.0) && val(psi_prev) != R(0.0)) psi = psi_prev * R(0.1);
      }
      theta = theta_from_h<S, POL>(lk, psi);
      S mass = S(R(0.0));
      mass = mass + (dthick_k * (theta - dth_k));
#pragma unroll
      for (int j = 0; j < K; j++) mass = mass + dthick[j] * (theta_from_h<S, POL>(pick_static(P, j), psi) - dth[j]);
      new_mass = mass;
      delta_mass = ab(val(new_mass) - val(prior_mass));
      if (ab(val(psi) - val(psi_prev)) < Tol<R>::nochange && factor < R(1e-13)) break;
      if (ab(delta_mass - delta_mass_prev) < Tol<R>::nochange) count_no_change++; else count_no_change = 0;
      if (count_no_change == 5) break;
      if (val(psi) <= R(0.0) && val(psi_prev) < Tol<R>::tiny) break;
      delta_mass_prev = delta_mass;
    }
    return theta;
  }

  // check_column_mass, Layer.py:655-701: depth line search of the (saturated) free-drainage front
  __device__ __forceinline__ void check_column_mass(int fdd, S old_mass, S percolation, S aet) {
    S theta_e_k1 = sel<S, NL>(P.te, F.layer(fdd));
    S mass_timestep = (old_mass + percolation) - (aet + R(0.0));
    if (__builtin_expect(ab(val(F.TH(fdd)) - val(theta_e_k1)) < Tol<R>::mass, 0)) {
      S current_mass = mass_balance();
      R err = ab(val(current_mass) - val(mass_timestep));
      bool switched = false;
      R factor = R(1.0);
      S depth_new = F.Z(fdd);
      // search_mode 1: the column mass is LINEAR in this one depth (slope = theta_fdd - theta_next, or theta_fdd for
      // the last front of a layer).  (i) All but the last two fixed steps of each up/down run are taken in one jump;
      // (ii) inside the loop the mass is evaluated from the linear model instead of re-summing the front table; when
      // the model says "converged" the true mass is summed once and, if the reference's termination test does not hold
      // on it, the reference's loop simply continues on true sums.
      const bool nxt_same = (fdd + 1 < nf) && (F.layer(fdd + 1) == F.layer(fdd));
      const S slope_s = nxt_same ? F.TH(fdd) - F.TH(fdd + 1) : F.TH(fdd);
      const R slope = val(slope_s);
      const bool jump = !M::literal && (slope > R(0.0));
      bool model = jump;
      const S m0 = current_mass, d0 = depth_new;
      long long it = 0;
      if constexpr (M::f64) {
        if (jump && ab(err - Tol<R>::mass) > Tol<R>::mass) {
          // the mass is linear in this depth: one step to the root (an offset that is a constant w.r.t. the parameters, like the
          // reference's fixed steps), verified on the true mass; the reference's own loop takes over if its test does not hold
          depth_new = depth_new + dv<POL>(val(mass_timestep) - val(current_mass), slope);
          F.Z(fdd) = depth_new;
          current_mass = mass_balance();
          err = ab(val(current_mass) - val(mass_timestep));
          model = false;
        }
      }
      while (true) {
        if (!(ab(err - Tol<R>::mass) > Tol<R>::mass)) {
          if (!model) break;
          F.Z(fdd) = depth_new;  // verify on the true mass; from here on the loop is the reference's own
          current_mass = mass_balance();
          err = ab(val(current_mass) - val(mass_timestep));
          model = false;
          continue;
        }
        if (++it > G->iter_cap) { status |= LGAR_ST_ITERCAP; break; }
        R before = val(depth_new);
        if (val(current_mass) < val(mass_timestep)) {
          if (jump) {
            R nsteps = (val(mass_timestep) - R(2.0) * Tol<R>::mass - val(current_mass)) / (slope * R(0.01) * factor);
            if (nsteps > R(3.0)) depth_new = depth_new + (R(floor(nsteps)) - R(2.0)) * (R(0.01) * factor);
          }
          depth_new = depth_new + R(0.01) * factor;
          switched = false;
        } else {
          if (!switched) { switched = true; factor = factor * R(0.001); }
          if (jump) {
            R nsteps = (val(current_mass) - val(mass_timestep) - R(2.0) * Tol<R>::mass) / (slope * R(0.01) * factor);
            if (nsteps > R(3.0)) depth_new = depth_new - (R(floor(nsteps)) - R(2.0)) * (R(0.01) * factor);
          }
          depth_new = depth_new - (R(0.01) * factor);
        }
        if (M::f32 && val(depth_new) == before && factor < R(1e-6)) break;  // fp32: step below resolution
        if (model) {
          current_mass = m0 + slope_s * (depth_new - d0);
        } else {
          F.Z(fdd) = depth_new;
          current_mass = mass_balance();
        }
        err = ab(val(current_mass) - val(mass_timestep));
      }
      if (model) F.Z(fdd) = depth_new;  // left the loop (cap / resolution) while still on the model
    }
  }

  // Layer.move_wetting_fronts (Layer.py:1254-1307) with its three cases: deepest_layer_front (:389-418),
  // wetting_front_in_layer (:420-547, compute_wetting_front_mass :561-644) and base_case (:320-387,
  // populate_delta_thickness :177-209).  The reference snapshots every front first (copy_states); the
  // sweep runs deepest -> shallowest and front i only needs the pre-sweep values of i and i+1, so the
  // snapshot is two register triples carried down the sweep instead of a second front table.
  // The sweep is LAYER-MAJOR with the layer index a compile-time constant: for K = NL-1 .. 0 the lane walks up its
  // fronts tagged K.  Per-layer parameters are then plain register operands (no value-selects per front), the
  // "layers above" loops have static bounds, and layer 0's cheap closed-form update carries no search code.
  struct SweepCarry {
    int i, nf0, fdd;
    unsigned near_sat;  // bit i: front i took its psi from the front below with (alpha psi)^n < 1e-6 (see psi_round_trip)
    S infiltration, aet;
    S on_z, on_th, on_ps;  // pre-sweep values of front i+1
  };

  // Cooperating lanes: the 6 K thetas an in-layer front of layer K needs before its search (theta of every layer above at
  // the front's and the next front's psi, before and after the move -- compute_wetting_front_mass, Layer.py:561-644) are three
  // distinct evaluations per layer above (the front's own psi has not changed yet: "old" and "new" are one value), and the
  // search's first mass evaluation needs K + 1 more at the front's psi.  Lane r of the group evaluates item r (items
  // 3 j + {0: psi, 1: psi of the next front before the sweep, 2: after}; item 3 K: the front's own layer at psi), in rounds of
  // `share_lanes` items; the serial chain of 2 (7 K + 1) pows becomes one of 2 per round.  theta_slope's theta is
  // theta_from_h's operation by operation.
  template <int K>
  __device__ __forceinline__ void coop_sweep_thetas(const LayerK<S> &lk, R psi, R psi_below_old, R psi_below, R (&th)[NL], R (&dt)[NL],
                                                    R (&d2)[NL], R &thk, R &dthk, R &d2thk, R (&th_below_old)[NL], R (&th_below)[NL]) {
    constexpr int CNT = 3 * K + 1;
    for (int first = 0; first < CNT; first += share_lanes) {
      const int q = first + coop_rank;
      const bool mine = (coop_rank < share_lanes) && (q < CNT);
      R al = val(lk.alpha), n = val(lk.n), m = val(lk.m), te = val(lk.te), tr = val(lk.tr), x = psi;
#pragma unroll
      for (int j = 0; j < K; j++) {
        const bool lj = (q >= 3 * j) && (q < 3 * j + 3);
        al = choose(lj, val(P.alpha[j]), al); n = choose(lj, val(P.n[j]), n); m = choose(lj, val(P.m[j]), m);
        te = choose(lj, val(P.te[j]), te); tr = choose(lj, val(P.tr[j]), tr);
        x = choose(q == 3 * j + 1, psi_below_old, x);
        x = choose(q == 3 * j + 2, psi_below, x);
      }
      R t0, t1, t2;
      theta_slope2(al, n, m, te, tr, x, t0, t1, t2);
      if (mine) { xchg[3 * q] = t0; xchg[3 * q + 1] = t1; xchg[3 * q + 2] = t2; }
    }
    lds_exchange_point();
#pragma unroll
    for (int j = 0; j < K; j++) {
      th[j] = xchg[3 * (3 * j)];
      dt[j] = xchg[3 * (3 * j) + 1];
      d2[j] = xchg[3 * (3 * j) + 2];
      th_below_old[j] = xchg[3 * (3 * j + 1)];
      th_below[j] = xchg[3 * (3 * j + 2)];
    }
    thk = xchg[3 * (3 * K)];
    dthk = xchg[3 * (3 * K) + 1];
    d2thk = xchg[3 * (3 * K) + 2];
    lds_exchange_point();
  }

  template <int K> __device__ __forceinline__ void sweep_layer(SweepCarry &c) {
    const LayerK<S> lk = pick_static(P, K);
    const int last = c.i;  // deepest front of this layer's list (if the lane has fronts tagged K)
    while (c.i >= 0 && F.layer(c.i) == K) {
      LGAR_MEASURE_POINT(CLK, 19)
      const int i = c.i;
      const S oc_z = F.Z(i), oc_th = F.TH(i), oc_ps = F.PS(i);  // pre-sweep values of front i
      bool need_psi = false;
      if (i < c.nf0 - 1) {
        if (i == last || feq(i, last)) {
          // deepest front of a layer: psi continuity with the layer below
          // (fast modes: a boundary front whose psi IS the psi below, bit for bit, took its theta from that very psi the last
          // time round -- nothing to do; decided per lane, the evaluation skipped when no column of the wavefront needs it.  The
          // boundary above an untouched layer stays like that for the whole run.)
          const bool fresh = !M::literal && same_bits(F.PS(i), F.PS(i + 1));
          if (!fresh) {
            S ap;
            F.TH(i) = theta_from_h_ap<S, POL>(lk, F.PS(i + 1), ap);
            F.PS(i) = F.PS(i + 1);
            if constexpr (!M::literal && M::f64) {
              if (__builtin_expect(val(ap) < R(1e-6), 0)) c.near_sat |= 1u << i;
            }
          }
          LGAR_MEASURE_POINT(CLK, 20)
        } else if constexpr (K == 0) {
          S prior_mass = oc_z * (oc_th - c.on_th);
          if (i == c.fdd || feq(c.fdd, i)) prior_mass = prior_mass + (c.infiltration - (R(0.0) + c.aet));
          S z = F.Z(i) + (F.DZ(i) * G->dt_h);
          z = mn(z, P.cum[NL - 1]);
          F.Z(i) = z;
          bool zero_dzdt = ab(val(F.DZ(i))) <= R(1e-8);  // torch.isclose(dzdt, 0, rtol=1e-8): atol 1e-8
          if (!(zero_dzdt && !F.bottom(i))) {            // a just-created front keeps its theta (Layer.py:458-467)
            S potential = dv<POL>(prior_mass, z) + F.TH(i + 1);
            F.TH(i) = mn(lk.te, potential);
          }
          need_psi = true;
        } else {
          S dth[NL], dthick[NL];
          const S prev_thick = P.cum[(K > 0) ? K - 1 : 0];
          S z = F.Z(i) + (F.DZ(i) * G->dt_h);
          F.Z(i) = z;
          S psi_old = oc_ps, psi_below_old = c.on_ps;
          S psi = F.PS(i), psi_below = F.PS(i + 1);
          S prior_mass = (oc_z - prev_thick) * (oc_th - c.on_th);
          S new_mass = (z - prev_thick) * (F.TH(i) - F.TH(i + 1));
          const S t_dth_k = F.TH(i + 1);
          const S t_dthick_k = z - prev_thick;
          FirstEval fe;
          if constexpr (M::coop_f64) {
            if (share_lanes >= 4) {  // cooperating lanes: the thetas below, evaluated by the group together
              R tj[NL], dj[NL], ej[NL], tk, dk, ek, tbo[NL], tb[NL];
              coop_sweep_thetas<K>(lk, psi, psi_below_old, psi_below, tj, dj, ej, tk, dk, ek, tbo, tb);
#pragma unroll
              for (int j = 0; j < K; j++) {
                S lt = P.cum[j] - R(0.0);
                prior_mass = prior_mass + (lt * (tj[j] - tbo[j]));  // (psi_old is psi: the front's own psi has not moved yet)
                new_mass = new_mass + (lt * (tj[j] - tb[j]));
                dth[j] = tb[j];
                dthick[j] = lt;
                fe.add(val(lt), tj[j], tb[j], dj[j], ej[j]);
              }
              fe.add(val(t_dthick_k), tk, val(t_dth_k), dk, ek);
              fe.thk = tk;
              fe.have = true;
            }
          }
          if constexpr (M::f64) {
            if (!fe.have) {
              // The front's own psi has not moved yet (psi_old IS psi: theta of the layers above "before" and "after" are one
              // evaluation), and the psi of the front below is the same before and after the sweep unless that front moved --
              // for the active front of a storm it is the layer's untouched boundary front -- so theta_below is evaluated a
              // second time only when some column of the wavefront needs it.  Plain reals take theta at psi together with its
              // two derivatives: the search's first mass evaluation (FirstEval).
              const bool below_moved = any_lane(!same_bits(psi_below_old, psi_below)) != 0ull;
#pragma unroll
              for (int j = 0; j < K; j++) {
                const LayerK<S> lj = pick_static(P, j);
                const S theta_below_old = theta_from_h<S, POL>(lj, psi_below_old);
                const S theta_below = below_moved ? theta_from_h<S, POL>(lj, psi_below) : theta_below_old;
                S lt = P.cum[j] - R(0.0);  // quirk: cumulative thickness (Layer.py:603-604)
                S theta;
                if constexpr (!M::dual) {
                  R th, dt, d2;
                  theta_slope2(val(lj.alpha), val(lj.n), val(lj.m), val(lj.te), val(lj.tr), val(psi), th, dt, d2);
                  fe.add(val(lt), th, val(theta_below), dt, d2);
                  theta = S(th);
                } else {
                  theta = theta_from_h<S, POL>(lj, psi);
                }
                prior_mass = prior_mass + (lt * (theta - theta_below_old));
                new_mass = new_mass + (lt * (theta - theta_below));
                dth[j] = theta_below;
                dthick[j] = lt;
              }
              if constexpr (!M::dual) {
                R tk, dk, ek;
                theta_slope2(val(lk.alpha), val(lk.n), val(lk.m), val(lk.te), val(lk.tr), val(psi), tk, dk, ek);
                fe.add(val(t_dthick_k), tk, val(t_dth_k), dk, ek);
                fe.thk = tk;
                fe.have = true;
              }
            }
          } else {
#pragma unroll
            for (int j = 0; j < K; j++) {
              const LayerK<S> lj = pick_static(P, j);
              S theta_old = theta_from_h<S, POL>(lj, psi_old);
              S theta_below_old = theta_from_h<S, POL>(lj, psi_below_old);
              S lt = P.cum[j] - R(0.0);  // quirk: cumulative thickness (Layer.py:603-604)
              prior_mass = prior_mass + (lt * (theta_old - theta_below_old));
              S theta = theta_from_h<S, POL>(lj, psi);
              S theta_below = theta_from_h<S, POL>(lj, psi_below);
              new_mass = new_mass + (lt * (theta - theta_below));
              dth[j] = theta_below;
              dthick[j] = lt;
            }
          }
          if (i == c.fdd || feq(c.fdd, i)) prior_mass = prior_mass + c.infiltration - (R(0.0) + c.aet);
          LGAR_MEASURE_POINT(CLK, 22)
          LGAR_MEASURE_POINT(DUP_SEARCH, K, lk, psi, new_mass, prior_mass, dth, dthick, t_dth_k, t_dthick_k)
          S theta_new = theta_mass_balance<K>(lk, psi, new_mass, prior_mass, dth, dthick, t_dth_k, t_dthick_k, fe);
          F.TH(i) = mn(theta_new, lk.te);
          need_psi = true;
          LGAR_MEASURE_POINT(CLK, 23)
        }
      } else if constexpr (K == NL - 1) {
        if (c.nf0 == NL) {
          // base_case: one front per layer, uniform psi
          S dth[NL], dthick[NL];
#pragma unroll
          for (int j = 0; j < NL; j++) { dth[j] = S(R(0.0)); dthick[j] = S(R(0.0)); }
          S z = F.Z(i) + F.DZ(i) * G->dt_h;
          F.Z(i) = z;
          S psi_old = oc_ps;
          S psi = F.PS(i);
          S base = P.cum[NL - 2];
          S prior_mass = (oc_z - base) * (oc_th - R(0.0));
          S new_mass = (z - base) * (F.TH(i) - R(0.0));
          FirstEval fe;
#pragma unroll
          for (int j = 0; j < NL - 1; j++) {
            const LayerK<S> lj = pick_static(P, j);
            if constexpr (M::f64) {
              // (psi_old IS psi -- the front's psi has not moved yet: one evaluation; plain reals take the derivatives along,
              // the search's first mass evaluation)
              S theta;
              if constexpr (!M::dual) {
                R th, dt, d2;
                theta_slope2(val(lj.alpha), val(lj.n), val(lj.m), val(lj.te), val(lj.tr), val(psi), th, dt, d2);
                fe.add(val(P.thick[j]), th, R(0.0), dt, d2);
                theta = S(th);
              } else {
                theta = theta_from_h<S, POL>(lj, psi);
              }
              prior_mass = prior_mass + P.thick[j] * (theta - R(0.0));
              new_mass = new_mass + P.thick[j] * (theta - R(0.0));
            } else {
              S theta_old = theta_from_h<S, POL>(lj, psi_old);
              prior_mass = prior_mass + P.thick[j] * (theta_old - R(0.0));
              S theta = theta_from_h<S, POL>(lj, psi);
              new_mass = new_mass + P.thick[j] * (theta - R(0.0));
            }
            dthick[j] = P.thick[j];
          }
          if constexpr (M::plain_f64) {
            R tk, dk, ek;
            theta_slope2(val(lk.alpha), val(lk.n), val(lk.m), val(lk.te), val(lk.tr), val(psi), tk, dk, ek);
            fe.add(val(z) - val(base), tk, R(0.0), dk, ek);
            fe.thk = tk;
            fe.have = true;
          }
          if (F.layer(c.fdd) == NL - 1) prior_mass = prior_mass + c.infiltration - (R(0.0) + c.aet);
          S theta_new = theta_mass_balance<NL - 1>(lk, psi, new_mass, prior_mass, dth, dthick, S(R(0.0)), z - base, fe);
          F.TH(i) = mn(theta_new, lk.te);
          need_psi = true;
        }
      }
      if (need_psi) F.PS(i) = h_from_se<S, POL>(lk, se_from_theta(lk, F.TH(i)));
      LGAR_MEASURE_POINT(CLK, 24)
      c.on_z = oc_z; c.on_th = oc_th; c.on_ps = oc_ps;
      c.i = i - 1;
    }
  }
  template <int K> __device__ __forceinline__ void sweep_from(SweepCarry &c) {
    sweep_layer<K>(c);
    if constexpr (K > 0) sweep_from<K - 1>(c);
  }

  // The sweep over a top-layer table (is_top_table; every column of the wave holds one): what sweep_from does on such a table,
  // front by front in the same order, with the table's shape known.  The deepest front of the domain does nothing (the table has
  // more than NL fronts: no base case); the boundary fronts of layers NL-2 .. 0, each the one front of its layer or the last of
  // layer 0, take the continuity branch; the m fronts above run through layer 0's closed form, of whose carried pre-sweep triple
  // only theta is read.  No layer tag is read, no loop runs over layers, no search is compiled in.
  template <int K> __device__ __forceinline__ void sweep_top_boundary(int i) {
    const LayerK<S> lk = pick_static(P, K);
    const bool fresh = same_bits(F.PS(i), F.PS(i + 1));
    if (!fresh) {
      S ap;
      F.TH(i) = theta_from_h_ap<S, POL>(lk, F.PS(i + 1), ap);
      F.PS(i) = F.PS(i + 1);
    }
    if constexpr (K > 0) sweep_top_boundary<K - 1>(i - 1);
  }
  __device__ __forceinline__ void sweep_top(const SweepCarry &c) {
    const LayerK<S> lk = pick_static(P, 0);
    const int m = c.nf0 - NL;
    S on_th = F.TH(m);  // pre-sweep theta of front i + 1
    sweep_top_boundary<NL - 2>(m + NL - 2);
    for (int i = m - 1; i >= 0; i--) {
      const S oc_z = F.Z(i), oc_th = F.TH(i);
      if (feq(i, m)) {  // (value-equal to the layer's last front: the reference sends it down the continuity branch)
        const bool fresh = same_bits(F.PS(i), F.PS(i + 1));
        if (!fresh) {
          S ap;
          F.TH(i) = theta_from_h_ap<S, POL>(lk, F.PS(i + 1), ap);
          F.PS(i) = F.PS(i + 1);
        }
      } else {
        S prior_mass = oc_z * (oc_th - on_th);
        if (i == c.fdd || feq(c.fdd, i)) prior_mass = prior_mass + (c.infiltration - (R(0.0) + c.aet));
        S z = F.Z(i) + (F.DZ(i) * G->dt_h);
        z = mn(z, P.cum[NL - 1]);
        F.Z(i) = z;
        const bool zero_dzdt = ab(val(F.DZ(i))) <= R(1e-8);
        if (!zero_dzdt) {  // (flag 0: not a just-created boundary front)
          S potential = dv<POL>(prior_mass, z) + F.TH(i + 1);
          F.TH(i) = mn(lk.te, potential);
        }
        F.PS(i) = h_from_se<S, POL>(lk, se_from_theta(lk, F.TH(i)));
      }
      on_th = oc_th;
    }
  }

  __device__ __forceinline__ void move_sweep(S infiltration, S aet, S old_mass, int fdd) {
    SweepCarry c;
    c.i = nf - 1; c.nf0 = nf; c.fdd = fdd;
    c.infiltration = infiltration; c.aet = aet;
    c.on_z = c.on_th = c.on_ps = S(R(0.0));
    c.near_sat = 0u;
    if constexpr (M::top_step) {
      const bool fast = any_lane(!top_table) == 0ull;  // wave-uniform: every active column holds a top-layer table
      LGAR_COUNT_TOP_STEP(fast)
      if (fast) sweep_top(c);
      else sweep_from<NL - 1>(c);
    } else {
      sweep_from<NL - 1>(c);
    }
    near_sat_fronts = c.near_sat;
    if constexpr (!M::fused_walk) {
      check_column_mass(fdd, old_mass, infiltration, aet);  // after front 0 (Layer.py:1296-1305)
    } else {
      // check_column_mass (Layer.py:655-701) in two halves around ONE walk over the front table.  The column mass is LINEAR in
      // the depth of the (saturated) free-drainage front -- slope = theta_fdd - theta_next, or theta_fdd for the last front of
      // a layer -- so the reference's fixed-step line search has a closed-form root: one step (an offset that is a constant
      // w.r.t. the parameters, like the reference's steps), then the walk that every column takes anyway (mass_and_events)
      // verifies it on the true mass against the reference's own termination test; where that fails -- and for a slope that
      // is not positive -- the reference's loop runs from where the step landed.
      const S theta_e_k1 = sel<S, NL>(P.te, F.layer(fdd));
      const S mass_timestep = (old_mass + infiltration) - (aet + R(0.0));
      bool stepped = false, literal = false;
      if (__builtin_expect(ab(val(F.TH(fdd)) - val(theta_e_k1)) < Tol<R>::mass, 0)) {
        const S current_mass = mass_balance();
        const R err = ab(val(current_mass) - val(mass_timestep));
        if (ab(err - Tol<R>::mass) > Tol<R>::mass) {
          const bool nxt_same = (fdd + 1 < nf) && (F.layer(fdd + 1) == F.layer(fdd));
          const R slope = nxt_same ? val(F.TH(fdd)) - val(F.TH(fdd + 1)) : val(F.TH(fdd));
          if (slope > R(0.0)) {
            F.Z(fdd) = F.Z(fdd) + dv<POL>(val(mass_timestep) - val(current_mass), slope);
            stepped = true;
          } else {
            literal = true;
          }
        }
      }
      if (__builtin_expect(literal, 0)) check_column_mass(fdd, old_mass, infiltration, aet);
      if constexpr (M::top_step) {  // (the sweep changes no flag: the same lanes, the same tables, the same answer)
        if (any_lane(!top_table) == 0ull) post_mass = mass_and_events_top(post_event);
        else post_mass = mass_and_events(post_event);
      } else {
        post_mass = mass_and_events(post_event);
      }
      if (stepped) {
        const R err = ab(val(post_mass) - val(mass_timestep));
        if (__builtin_expect(ab(err - Tol<R>::mass) > Tol<R>::mass, 0)) {
          check_column_mass(fdd, old_mass, infiltration, aet);
          post_mass = mass_and_events(post_event);
        }
      }
      post_mass_valid = true;
    }
  }

  // merge_wetting_fronts / is_passing / pass_front / delete_front, Layer.py:826-892: per layer, the first
  // front that has passed its (same-layer, non-boundary) successor absorbs it; <= 1 merge per layer per call.
  __device__ __forceinline__ void merge_fronts() {
    int i = 0, lo = 0;
    while (i < nf - 1) {
      const int k = F.layer(i);
      if (i > 0 && F.layer(i - 1) != k) lo = i;
      const int nx = i + 1;
      const bool passing = (val(F.Z(i)) > val(F.Z(nx))) && (F.layer(nx) == k) && !F.bottom(nx);
      if (!passing) { i++; continue; }
      const int nn = i + 2;
      if (nn >= nf) { status |= LGAR_ST_STRUCT; return; }
      const LayerK<S> lk = pick(P, k);
      S mass = F.Z(i) * (F.TH(i) - F.TH(nx)) + F.Z(nx) * (F.TH(nx) - F.TH(nn));
      F.Z(i) = mass / (F.TH(i) - F.TH(nn));
      S se = se_from_theta(lk, F.TH(i));
      F.PS(i) = h_from_se<S, POL>(lk, se);
      // delete_front: the first front of THIS layer's list that is value-equal to `next`
      int j = lo;
      while (j < nf && F.layer(j) == k && !feq(j, nx)) j++;
      if (j < nf && F.layer(j) == k) fdel(j);
      // this layer is done: continue with the first front of the next layer
      i = lo;
      while (i < nf && F.layer(i) == k) i++;
      lo = i;
    }
  }

  // wetting_fronts_cross_layer_boundary / recalibrate, Layer.py:894-1008: a front that has advanced past its
  // layer's lower boundary swaps roles with the boundary front.  On the flat array the re-bucketing
  // (update_wetting_fronts :939-963) is just the tag change; the moved front is not revisited in this call.
  __device__ __forceinline__ void cross_layer_boundary() {
    int i = 0;
    while (i < nf - 1) {
      const int k = F.layer(i);
      const int nx = i + 1, nn = i + 2;
      const S cumk = cum_at(k);
      if (!(val(F.Z(i)) > val(cumk) && val(F.Z(nx)) == val(cumk))) { i++; continue; }
      if (k == NL - 1) {
        if (G->bottom_mode == 0) { status |= LGAR_ST_BOTTOM; return; }  // reference: AttributeError at Layer.py:980
        i++;  // LGAR-C intent: the bottom layer has no layer below; the domain-boundary step handles this front
        continue;
      }
      if (nn >= nf) { status |= LGAR_ST_STRUCT; return; }
      const LayerK<S> lk = pick(P, k);
      const LayerK<S> ln = pick(P, k + 1);
      S overshot = F.Z(i) - F.Z(nx);
      S se = se_from_theta(lk, F.TH(i));
      F.PS(i) = h_from_se<S, POL>(lk, se);
      S theta_new = theta_from_h<S, POL>(ln, F.PS(i));
      S mbal = overshot * (F.TH(i) - F.TH(nx));
      S zc = mbal / (theta_new - F.TH(nn));
      S depth_new = cumk + zc;
      F.Z(i) = cumk;
      F.TH(nx) = theta_new;
      F.PS(nx) = F.PS(i);
      // (fast modes: the reference's update_psi re-derives the new front's psi from its theta at the end of the move -- nothing
      // reads it before -- and right after a crossing that round trip is not a no-op: the front is all but saturated)
      if constexpr (!M::literal) F.PS(nx) = h_from_se<S, POL>(ln, se_from_theta(ln, theta_new));
      F.Z(nx) = depth_new;
      F.DZ(nx) = F.DZ(i);
      F.DZ(i) = S(R(0.0));
      F.set_flag(i, k, true);
      F.set_flag(nx, k + 1, false);
      i += 2;
    }
  }

  // wetting_front_cross_domain_boundary, Layer.py:1010-1053 (bottom_mode 1 only; the reference cannot reach it without
  // crashing): the second-to-last front of the domain has passed the column bottom -> its overshoot leaves as
  // percolation, the bottom front takes its theta, and it is deleted.
  __device__ __forceinline__ S cross_domain_boundary() {
    S flux = S(R(0.0));
    if (nf < 2) return flux;
    const int i = nf - 2, nx = nf - 1;
    const int k = F.layer(i);
    if (val(F.Z(i)) > val(cum_at(k))) {
      const LayerK<S> lk = pick(P, k);
      flux = (F.TH(i) - F.TH(nx)) * (F.Z(i) - F.Z(nx));
      F.TH(nx) = F.TH(i);
      S se = se_from_theta(lk, F.TH(i));
      F.PS(nx) = h_from_se<S, POL>(lk, se);
      k_deepest = k_from_se<S, POL>(lk, se);
      fdel(i);
    }
    return flux;
  }

  // fix_dry_over_wet_fronts / cleanup_wetting_fronts / update_layer_fronts, Layer.py:1055-1143: per layer,
  // the first front that is not wetter than its same-layer successor is deleted (<= 1 per layer per call).
  __device__ __forceinline__ S fix_dry_over_wet() {
    S ls[NL];
#pragma unroll
    for (int j = 0; j < NL; j++) ls[j] = S(R(0.0));
    int i = 0;
    while (i < nf - 1) {
      const int k = F.layer(i);
      const int nx = i + 1;
      if (!(val(F.TH(i)) <= val(F.TH(nx)) && F.layer(nx) == k)) { i++; continue; }
      S before = mass_balance();
      fdel(i);  // the next front now sits at index i
      if (k > 0) {
        psi_rewritten = true;
        int found = 0;
        while (found < nf && !feq(found, i)) found++;
        if (found >= nf) status |= LGAR_ST_STRUCT;
        else {
          const int lj = F.layer(found);
          const LayerK<S> lf = pick(P, lj);
          F.PS(found) = h_from_se<S, POL>(lf, se_from_theta(lf, F.TH(found)));
          const S dry_th = F.TH(found), dry_ps = F.PS(found);
          for (int q = 0; q < nf; q++) {
            const int lq = F.layer(q);
            if (lq < lj) {  // quirk: EVERY front of all shallower layers is overwritten (Layer.py:1117-1143)
              const LayerK<S> lql = pick(P, lq);
              F.PS(q) = h_from_se<S, POL>(lql, se_from_theta(lql, dry_th));
              // another layer's theta can exceed this layer's theta_e: Se > 1, a negative pow base, and the reference
              // raises (utils.py:25-27) -- but the NaN psi is overwritten by update_psi before anything reads it, so it
              // must be caught here
              if (is_nan(val(F.PS(q)))) status |= LGAR_ST_NEGBASE;
              F.TH(q) = theta_from_h<S, POL>(lql, dry_ps);
            }
          }
        }
      }
      S after = mass_balance();
      S mc = ab(after - before);
#pragma unroll
      for (int j = 0; j < NL; j++) ls[j] = choose(k == j, ls[j] + mc, ls[j]);
      // this layer is done: continue with the first front of the next layer
      while (i < nf && F.layer(i) == k) i++;
    }
    S tot = ls[NL - 1];
#pragma unroll
    for (int j = NL - 2; j >= 0; j--) tot = ls[j] + tot;
    return tot;
  }

  // update_psi, Layer.py:1157-1174: psi from theta for every front but the deepest of the domain (K: see front_k)
  __device__ __forceinline__ void update_psi() {
    for (int i = 0; i < nf - 1; i++) {
      const LayerK<S> lk = pick(P, F.layer(i));
      F.PS(i) = h_from_se<S, POL>(lk, se_from_theta(lk, F.TH(i)));
    }
  }

  // K of front i as calc_dzdt / the state dump see it
  __device__ __forceinline__ S front_k(int i, const LayerK<S> &lk) const {
    S k = k_from_se<S, POL>(lk, se_from_theta(lk, F.TH(i)));
    if (i == 0 && new_front_frozen) k = k * G->frozen;
    return k;
  }

  // Does any of the post-sweep passes have work to do?  merge (Layer.py:826-892), layer-boundary crossing (:894-1008),
  // domain-boundary crossing (:1010-1053) and dry-over-wet (:1055-1143) each act only when their trigger holds for some
  // adjacent pair, and a pass that finds no trigger changes nothing; so a column without a trigger skips the four passes
  // as a block (one cheap scan instead of five; the wave skips the code when none of its columns has one).
  __device__ __forceinline__ bool front_event_pending() const {
    bool ev = false;
    S z1 = F.Z(0), t1 = F.TH(0);
    int f1 = F.flag(0);
    for (int i = 0; i + 1 < nf; i++) {
      const S z2 = F.Z(i + 1), t2 = F.TH(i + 1);
      const int f2 = F.flag(i + 1);
      const bool same = ((f1 ^ f2) & 0x7f) == 0;
      ev = ev || (same && !(f2 & LGAR_FLAG_BOTTOM) && val(z1) > val(z2));   // passing
      ev = ev || (same && val(t1) <= val(t2));                                // dry over wet
      ev = ev || (val(z1) > val(cum_at(f1 & 0x7f)));                         // past its layer (or the domain) bottom
      z1 = z2; t1 = t2; f1 = f2;
    }
    return ev;
  }

  // dpLGAR.move_wetting_front, models/dpLGAR.py:340-367.  Returns the bottom-boundary flux.
  // wetting_front_cross_domain_boundary (Layer.py:1010-1053) cannot be reached in the reference without
  // crashing in the layer-boundary step first; here that case sets LGAR_ST_BOTTOM and the flux is 0.
  __device__ __forceinline__ S move_wetting_front(S infiltration, S &aet, S old_mass, int fdd) {
    move_sweep(infiltration, aet, old_mass, fdd);
    LGAR_MEASURE_POINT(CLK, 3)
    S bottom_flux = S(R(0.0));
    // (a per-lane decision: a column's results must not depend on which other columns share its wave)
    LGAR_MEASURE_POINT(DUP_EVENT)
    bool pending;
    if constexpr (M::fused_walk) pending = post_event;
    else pending = front_event_pending();
    if (__builtin_expect(pending, 0)) {
      post_mass_valid = false;
      psi_rewritten = false;
      for (int pass = 0; pass < 2; pass++) {
        merge_fronts();
        if (pass == 0) cross_layer_boundary();
      }
      if (G->bottom_mode != 0) bottom_flux = cross_domain_boundary();
      S mass_change = fix_dry_over_wet();
      if (ab(val(mass_change)) > R(1e-7)) aet = aet - mass_change;
      // the passes can leave psi inconsistent with theta (dry-over-wet in a deeper layer writes the psi of ANOTHER
      // layer's theta into the fronts above it, Layer.py:1117-1143): the reference's update_psi repairs that
      // ... every front a merge or a crossing touched carries psi = h(Se(theta)) already (each pass sets it); only that rewrite
      // needs the reference's full pass -- and a column with a near-saturated boundary front (below), whose bit may no longer
      // sit at the front's index after a deletion
      if constexpr (!M::literal) { if (psi_rewritten || near_sat_fronts != 0u) update_psi(); }
      if constexpr (M::top_step) top_table = is_top_table();  // (the passes delete fronts and change tags)
    } else if constexpr (!M::literal && M::f64) {
      // A layer's deepest front takes the psi of the front below and theta(psi) of its own layer (Layer.py:389-418); the
      // reference's update_psi then re-derives psi from that theta.  The round trip returns psi to ~eps / (alpha psi)^n
      // relative: nothing a decision can see (the tie rule of calc_wetting_front_free_drainage has rtol 1e-5, atol 1e-8)
      // unless the front is all but saturated -- (alpha psi)^n < 1e-6, psi below ~0.03 cm -- where the reference's psi is
      // the round trip's noise and its tie rule decides on that noise (fixture crash_bottom_three_layer_synth3: 1.77e-7 cm
      // comes back as 4.64e-6).  Those fronts, and only those, go through the same round trip here.
      if (__builtin_expect(near_sat_fronts != 0u, 0)) {
        for (int i = 0; i < nf - 1; i++)
          if (near_sat_fronts & (1u << i)) {
            const LayerK<S> lk = pick(P, F.layer(i));
            F.PS(i) = h_from_se<S, POL>(lk, se_from_theta(lk, F.TH(i)));
          }
      }
    }
    // update_psi (Layer.py:1157-1174) re-derives psi from theta for every front but the deepest.  After the sweep alone
    // every front already carries psi = h(Se(theta)) (in-layer and base-case fronts) or the psi its theta was computed
    // from (a layer's deepest front), so the pass only adds a theta -> psi -> theta round trip: MODE_LITERAL keeps it, MODE_FAST
    // runs it only after an event.
    if constexpr (M::literal) update_psi();
    LGAR_MEASURE_POINT(CLK, 4)
    LGAR_MEASURE_POINT(DUP_PSI)
    return bottom_flux;
  }

  // calc_dzdt, Layer.py:1176-1252 (calc_bottom_sum :1557-1582): one Geff per moving front
  // Every lane walks its OWN list of moving fronts: fronts that need no Geff (layer bottoms, delta_theta <= 0) are finished
  // on the way, and the k-th moving front of every column meets the others' k-th in one evaluation of the trapezoid --
  // columns whose moving fronts sit at different indices (one has crossed into the next layer, another has two fronts
  // above a boundary) would otherwise take turns.  The fronts' dz/dt do not depend on one another, so the order is free.
  // Cooperating lanes, groups of at least LGAR_COOP_PAIR_LANES: TWO moving fronts at a time.  A trapezoid's cost on a lone wave
  // is its dependent chains -- the two pows that open it, the 120 additions of its heads, the 120 of its sum -- not its nodes,
  // and most steps have two moving fronts: the lower half of the group takes one front, the upper half the other, through
  // the same instruction stream (each half with its own front's layer, thetas and psi as operands, its own row of the group's
  // LDS table, its lanes numbered from 0), and the halves then exchange Geff and the conductivities that rode along.  Every
  // value is computed exactly as the one-front path computes it.  Returns the index the one-front loop resumes after (it
  // finishes a last unpaired front, and everything when there is no pair).
  __device__ __forceinline__ int calc_dzdt_pairs(S h_p) {
    const int hl = share_lanes >> 1;
    const bool upper = coop_rank >= hl;
    const int r2 = upper ? coop_rank - hl : coop_rank;
    R *tab2 = xchg + (upper ? LGAR_COOP_TAB_ROW : 0);
    int i = -1;
    auto next_moving = [&]() {  // the one-front loop's scan: fronts that need no Geff are finished on the way
      while (++i < nf - 1) {
        if (F.bottom(i)) { F.DZ(i) = S(R(0.0)); continue; }
        const bool top = F.layer(i) == 0;
        if (top && val(F.TH(i + 1)) > val(F.TH(i))) status |= LGAR_ST_THETA_ORDER;  // Layer.py:1206-1208
        if (val(F.TH(i) - F.TH(i + 1)) > R(0.0)) return i;
        F.DZ(i) = S(R(0.0));
      }
      return -1;
    };
    for (;;) {
      const int ia = next_moving();
      if (ia < 0) return i;
      const int ib = next_moving();
      const int ka = F.layer(ia), kb = (ib >= 0) ? F.layer(ib) : 0;
      // no pair, or a half too small for a front's riders: the one-front loop takes over at front ia (the fronts behind it are
      // done; the scan's side effects beyond it are idempotent)
      if (ib < 0 || hl < 5 + ((ka > kb) ? ka : kb)) return ia - 1;
      const int im = upper ? ib : ia;
      const int k = upper ? kb : ka;
      const LayerK<S> lk = pick(P, k);
      const S theta_1 = F.TH(im + 1), theta_2 = F.TH(im);
      CoopRiders riders;
      {
        const int e = r2 - 5;  // my layer above (lanes 5 .. 5 + k - 1 of my half)
        LayerK<S> le = lk;
        S th_e = theta_2;
#pragma unroll
        for (int j = 0; j < NL - 1; j++) {
          const bool mine = (e == j) && (j < k);
          le.alpha = choose(mine, P.alpha[j], le.alpha); le.n = choose(mine, P.n[j], le.n); le.m = choose(mine, P.m[j], le.m);
          le.inv_m = choose(mine, P.inv_m[j], le.inv_m); le.ksat = choose(mine, P.ksat[j], le.ksat);
          le.te = choose(mine, P.te[j], le.te); le.tr = choose(mine, P.tr[j], le.tr);
        }
        if (ka > 0 || kb > 0) {
          const S tl = theta_from_h<S, POL>(le, F.PS(im));
          th_e = choose(e >= 0 && e < k, tl, th_e);
        }
        riders.n = 1 + k;
        riders.l = le;
        riders.se = se_from_theta(le, th_e);
#pragma unroll
        for (int q = 0; q < LGAR_LMAX; q++) riders.k[q] = R(1.0);
      }
      LGAR_COUNT_GEFF_CALL(1)
      LGAR_COUNT_GEFF_CALL(1)
      const S g_mine = geff_fused<S>(lk, theta_1, theta_2, G->nint, tab2, hl, r2, &riders);
      // the halves exchange what they found (every lane of a half stores the same values)
      tab2[0] = g_mine;
#pragma unroll
      for (int q = 0; q < NL; q++) tab2[1 + q] = riders.k[q];
      lds_exchange_point();
      S g2[2];
      R kk[2][NL];
#pragma unroll
      for (int h = 0; h < 2; h++) {
        g2[h] = xchg[h * LGAR_COOP_TAB_ROW];
#pragma unroll
        for (int q = 0; q < NL; q++) kk[h][q] = xchg[h * LGAR_COOP_TAB_ROW + 1 + q];
      }
      lds_exchange_point();
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int f = h ? ib : ia;
        const int kf = h ? kb : ka;
        const LayerK<S> lf = pick(P, kf);
        const S g = g2[h];
        S ki = kk[h][0];
        if (f == 0 && new_front_frozen) ki = ki * G->frozen;
        if (is_nan(val(g))) status |= LGAR_ST_NAN;
        const S delta_theta = F.TH(f) - F.TH(f + 1);
        S dzdt;
        if (kf == 0) {
          dzdt = dv<POL>(S(R(1.0)), delta_theta) * (dv<POL>(lf.ksat * (g + h_p), F.Z(f)) + ki);
        } else {
          S den = S(R(0.0)) + dv<POL>(F.Z(f) - cum_prev(kf), ki);
#pragma unroll
          for (int j = 0; j < NL - 1; j++)
            if (j < kf) {
              S pt = (j != 0) ? P.cum[(j > 0) ? j - 1 : 0] : S(R(0.0));
              den = den + dv<POL>(P.cum[j] - pt, S(kk[h][1 + j]));
            }
          dzdt = dv<POL>(S(R(1.0)), delta_theta) * (dv<POL>(F.Z(f), den) + dv<POL>(lf.ksat * (g + h_p), F.Z(f)));
        }
        F.DZ(f) = dzdt;
      }
    }
  }

  // ... and in the mixed-precision mode (MODE_MIXED_COOP): the halves of ANY group (the mixed trapezoid's ends are evaluated by every
  // lane, nothing rides along) take one moving front each -- its trapezoid (geff_mixed_heads, the half's lanes splitting its
  // four-node groups through the half's own 32 slots of the group's table row) and the conductivities of the layers above at
  // its psi -- and exchange Geff, K(theta) / Ksat of the wet end and those conductivities.
  __device__ __forceinline__ int calc_dzdt_pairs_mixed(S h_p) {
    const int hl = share_lanes >> 1;
    const bool upper = coop_rank >= hl;
    const int r2 = upper ? coop_rank - hl : coop_rank;
    R *tab2 = xchg + (upper ? 64 : 0);
    int i = -1;
    auto next_moving = [&]() {  // the one-front loop's scan: fronts that need no Geff are finished on the way
      while (++i < nf - 1) {
        if (F.bottom(i)) { F.DZ(i) = S(R(0.0)); continue; }
        const bool top = F.layer(i) == 0;
        if (top && val(F.TH(i + 1)) > val(F.TH(i))) status |= LGAR_ST_THETA_ORDER;  // Layer.py:1206-1208
        if (val(F.TH(i) - F.TH(i + 1)) > R(0.0)) return i;
        F.DZ(i) = S(R(0.0));
      }
      return -1;
    };
    for (;;) {
      const int ia = next_moving();
      if (ia < 0) return i;
      const int ib = next_moving();
      if (ib < 0) return ia - 1;  // no pair: the one-front loop takes over at front ia
      const int ka = F.layer(ia), kb = F.layer(ib);
      const int kmax = (ka > kb) ? ka : kb;
      const int im = upper ? ib : ia;
      const int k = upper ? kb : ka;
      const LayerK<S> lk = pick(P, k);
      LGAR_COUNT_GEFF_CALL(1)
      LGAR_COUNT_GEFF_CALL(1)
      double kr_mine;
      const S g_mine = geff_mixed_heads<true>(lk, F.TH(im + 1), F.TH(im), F.PS(im + 1), F.PS(im), G->nint, kr_mine, tab2, hl, r2);
      tab2[0] = g_mine;
      tab2[1] = kr_mine;
#pragma unroll
      for (int j = 0; j < NL - 1; j++)
        if (j < kmax) {  // (both halves, for the deeper of the two fronts: one instruction stream)
          const LayerK<S> lj = pick_static(P, j);
          const S tl = theta_from_h<S, POL>(lj, F.PS(im));
          tab2[2 + j] = k_from_se<S, POL>(lj, se_from_theta(lj, tl));
        }
      lds_exchange_point();
      S g2[2];
      R kr2[2], kk[2][NL];
#pragma unroll
      for (int h = 0; h < 2; h++) {
        g2[h] = xchg[h * 64];
        kr2[h] = xchg[h * 64 + 1];
#pragma unroll
        for (int j = 0; j < NL - 1; j++) kk[h][j] = xchg[h * 64 + 2 + j];
      }
      lds_exchange_point();
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int f = h ? ib : ia;
        const int kf = h ? kb : ka;
        const LayerK<S> lf = pick(P, kf);
        const S g = g2[h];
        S ki = lf.ksat * kr2[h];
        if (f == 0 && new_front_frozen) ki = ki * G->frozen;
        if (is_nan(val(g))) status |= LGAR_ST_NAN;
        const S delta_theta = F.TH(f) - F.TH(f + 1);
        S dzdt;
        if (kf == 0) {
          dzdt = dv<POL>(S(R(1.0)), delta_theta) * (dv<POL>(lf.ksat * (g + h_p), F.Z(f)) + ki);
        } else {
          S den = S(R(0.0)) + dv<POL>(F.Z(f) - cum_prev(kf), ki);
#pragma unroll
          for (int j = 0; j < NL - 1; j++)
            if (j < kf) {
              S pt = (j != 0) ? P.cum[(j > 0) ? j - 1 : 0] : S(R(0.0));
              den = den + dv<POL>(P.cum[j] - pt, S(kk[h][j]));
            }
          dzdt = dv<POL>(S(R(1.0)), delta_theta) * (dv<POL>(F.Z(f), den) + dv<POL>(lf.ksat * (g + h_p), F.Z(f)));
        }
        F.DZ(f) = dzdt;
      }
    }
  }

  // calc_dzdt of the kernels with the top-layer step (M::top_step: plain fp32, one lane per column): the loop below with a
  // wave-uniform `fast`.  Top-layer tables in every column of the wave (is_top_table): only the m = nf - NL fronts above the top
  // layer's boundary front can move, all of them in layer 0 -- the scan reads no flag, the layer's parameters are layer 0's
  // registers (no value-selects), the dz/dt formula is the top layer's, and the boundary fronts' dz/dt are zeroed after the
  // loop.  The trapezoid's one call site and the wave-level loop serve both kinds of wave: every Geff, every dz/dt is the same.
  // (A function of its own so that the other kernels' calc_dzdt stays the text -- and the instructions -- it was.)
  __device__ __forceinline__ void calc_dzdt_top_step(S h_p) {
    const bool fast = any_lane(!top_table) == 0ull;
    const int m = nf - NL;
    int i = -1;
    for (;;) {
      // advance to the next front that moves
      bool found = false;
      if (fast) {
        while (!found && ++i < m) {
          if (val(F.TH(i + 1)) > val(F.TH(i))) status |= LGAR_ST_THETA_ORDER;  // Layer.py:1206-1208
          if (val(F.TH(i) - F.TH(i + 1)) > R(0.0)) found = true;
          else F.DZ(i) = S(R(0.0));
        }
      } else {
        while (!found && ++i < nf - 1) {
          if (F.bottom(i)) { F.DZ(i) = S(R(0.0)); continue; }
          const bool top = F.layer(i) == 0;
          if (top && val(F.TH(i + 1)) > val(F.TH(i))) status |= LGAR_ST_THETA_ORDER;
          if (val(F.TH(i) - F.TH(i + 1)) > R(0.0)) found = true;
          else F.DZ(i) = S(R(0.0));
        }
      }
      if (any_lane(found) == 0ull) break;
      LGAR_MEASURE_POINT(CLK, 10)
      if (found) {
        int k = 0;
        LayerK<S> lk;
        if (fast) {
          lk = pick_static(P, 0);
        } else {
          k = F.layer(i);
          lk = pick(P, k);
        }
        S theta_1 = F.TH(i + 1), theta_2 = F.TH(i);
        S delta_theta = F.TH(i) - F.TH(i + 1);
        S g, ki;
        bool fronts_done = false;
        LGAR_MEASURE_POINT(F32_HEADS_FROM_PSI, lk, i, g, ki, fronts_done)
        if (!fronts_done) {
          g = capillary_drive(lk, theta_1, theta_2, 1);
          ki = front_k(i, lk);
#ifndef LGAR_NO_DZDT_MEMO
          // (see calc_dzdt; a top-layer table's moving fronts are all in layer 0: the first of the layer is front 0)
          if (same_bits(theta_2, lk.te) && (i == 0 || (!fast && F.layer(i - 1) != k))) { memo_theta = theta_1; memo_g = g; memo_layer = k; }
#endif
        }
        if (is_nan(val(g))) status |= LGAR_ST_NAN;
        S dzdt;
        if (fast || k == 0) {
          dzdt = dv<POL>(S(R(1.0)), delta_theta) * (dv<POL>(lk.ksat * (g + h_p), F.Z(i)) + ki);
        } else {
          S den = S(R(0.0)) + dv<POL>(F.Z(i) - cum_prev(k), ki);
#pragma unroll
          for (int j = 0; j < NL - 1; j++)
            if (j < k) {
              const LayerK<S> lj = pick_static(P, j);
              S tl = theta_from_h<S, POL>(lj, F.PS(i));
              S kl = k_from_se<S, POL>(lj, se_from_theta(lj, tl));
              S pt = (j != 0) ? P.cum[(j > 0) ? j - 1 : 0] : S(R(0.0));
              den = den + dv<POL>(P.cum[j] - pt, kl);
            }
          dzdt = dv<POL>(S(R(1.0)), delta_theta) * (dv<POL>(F.Z(i), den) + dv<POL>(lk.ksat * (g + h_p), F.Z(i)));
        }
        F.DZ(i) = dzdt;
        LGAR_MEASURE_POINT(CLK, 17)
      }
    }
    if (fast) {  // the boundary fronts but the domain's deepest (the generic scan zeroes them on its way)
#pragma unroll
      for (int j = 0; j < NL - 1; j++) F.DZ(m + j) = S(R(0.0));
    }
  }

  __device__ __forceinline__ void calc_dzdt(S h_p) {
    if constexpr (M::top_step) {
      calc_dzdt_top_step(h_p);
      return;
    }
    int i = -1;
    if constexpr (M::coop_f64 && M::mixed) {
      if (share_lanes >= 4 && !G->closed_form) i = calc_dzdt_pairs_mixed(h_p);
    }
    if constexpr (M::coop_f64 && !M::mixed) {
      // (a group of 8 or more lanes owns TWO rows of the exchange table: lgar_kernels_nl.hip)
      if (share_lanes >= LGAR_COOP_PAIR_LANES && !G->closed_form) i = calc_dzdt_pairs(h_p);
    }
    for (;;) {
      // advance to the next front that moves
      bool found = false;
      while (!found && ++i < nf - 1) {
        if (F.bottom(i)) { F.DZ(i) = S(R(0.0)); continue; }
        const bool top = F.layer(i) == 0;
        if (top && val(F.TH(i + 1)) > val(F.TH(i))) status |= LGAR_ST_THETA_ORDER;  // Layer.py:1206-1208
        if (val(F.TH(i) - F.TH(i + 1)) > R(0.0)) found = true;
        else F.DZ(i) = S(R(0.0));
      }
      if (any_lane(found) == 0ull) break;
      LGAR_MEASURE_POINT(CLK, 10)
      if (found) {
        const int k = F.layer(i);
        const LayerK<S> lk = pick(P, k);
        S theta_1 = F.TH(i + 1), theta_2 = F.TH(i);
        S delta_theta = F.TH(i) - F.TH(i + 1);
        S g, ki;
        bool fronts_done = false;
        if constexpr (M::mixed_f64) {
          if (!G->closed_form) {  // mixed precision: heads from the fronts' psi, K(theta_i) from the trapezoid's wet end node
            double kr_end;
            g = capillary_drive_fronts(lk, theta_1, theta_2, F.PS(i + 1), F.PS(i), kr_end);
            ki = lk.ksat * kr_end;
            if (i == 0 && new_front_frozen) ki = ki * G->frozen;
            fronts_done = true;
          }
        }
        CoopRiders riders;  // (cooperating lanes only)
        if constexpr (M::coop_f64 && !M::mixed) {
          // cooperating lanes: the front's own K(theta) and the K of the layers above at its psi (two pows each, after the
          // two of theta(psi)) ride along with the four evaluations that open the trapezoid -- see CoopRiders
          if (!G->closed_form && share_lanes >= 5 + k) {
            const int e = coop_rank - 5;  // my layer above (lanes 5 .. 5 + k - 1)
            LayerK<S> le = lk;
            S th_e = F.TH(i);
            if (k > 0) {
#pragma unroll
              for (int j = 0; j < NL - 1; j++) {
                const bool mine = (e == j) && (j < k);
                le.alpha = choose(mine, P.alpha[j], le.alpha); le.n = choose(mine, P.n[j], le.n); le.m = choose(mine, P.m[j], le.m);
                le.inv_m = choose(mine, P.inv_m[j], le.inv_m); le.ksat = choose(mine, P.ksat[j], le.ksat);
                le.te = choose(mine, P.te[j], le.te); le.tr = choose(mine, P.tr[j], le.tr);
              }
              const S tl = theta_from_h<S, POL>(le, F.PS(i));
              th_e = choose(e >= 0 && e < k, tl, th_e);
            }
            riders.n = 1 + k;
            riders.l = le;
            riders.se = se_from_theta(le, th_e);
#pragma unroll
            for (int q = 0; q < LGAR_LMAX; q++) riders.k[q] = R(1.0);
            g = capillary_drive(lk, theta_1, theta_2, 1, &riders);
            ki = riders.k[0];
            if (i == 0 && new_front_frozen) ki = ki * G->frozen;
            fronts_done = true;
          }
        }
        LGAR_MEASURE_POINT(F32_HEADS_FROM_PSI, lk, i, g, ki, fronts_done)
        if (!fronts_done) {
          g = capillary_drive(lk, theta_1, theta_2, 1);
          ki = front_k(i, lk);
#ifndef LGAR_NO_DZDT_MEMO
          if constexpr (M::plain_f32 && !M::literal) {
            // A SATURATED moving front that is the first of its layer: g is Geff(theta_{i+1} -> theta_e) of that layer, the very
            // value insert_water asks for at the start of the next sub-step when this layer holds the free-drainage front (its
            // theta_1 is the front after the layer's first).  Plain fp32 has one Geff function for all call sites, so the value
            // is the one insert_water would compute, bit for bit: it goes into insert_water's memo.  (Fronts further down the
            // layer are never that neighbour: they leave the memo alone.)
            if (same_bits(theta_2, lk.te) && (i == 0 || F.layer(i - 1) != k)) { memo_theta = theta_1; memo_g = g; memo_layer = k; }
          }
#endif
        }
        if (is_nan(val(g))) status |= LGAR_ST_NAN;
        S dzdt;
        if (k == 0) {
          dzdt = dv<POL>(S(R(1.0)), delta_theta) * (dv<POL>(lk.ksat * (g + h_p), F.Z(i)) + ki);
        } else {
          S den = S(R(0.0)) + dv<POL>(F.Z(i) - cum_prev(k), ki);
#pragma unroll
          for (int j = 0; j < NL - 1; j++)
            if (j < k) {
              const LayerK<S> lj = pick_static(P, j);
              S kl;
              bool rode = false;
              if constexpr (M::coop_f64 && !M::mixed) {
                if (riders.n > 0) { kl = riders.k[1 + j]; rode = true; }
              }
              if (!rode) {
                S tl = theta_from_h<S, POL>(lj, F.PS(i));
                kl = k_from_se<S, POL>(lj, se_from_theta(lj, tl));
              }
              S pt = (j != 0) ? P.cum[(j > 0) ? j - 1 : 0] : S(R(0.0));
              den = den + dv<POL>(P.cum[j] - pt, kl);
            }
          dzdt = dv<POL>(S(R(1.0)), delta_theta) * (dv<POL>(F.Z(i), den) + dv<POL>(lk.ksat * (g + h_p), F.Z(i)));
        }
        F.DZ(i) = dzdt;
        LGAR_MEASURE_POINT(CLK, 17)
      }
    }
  }

  // calc_dry_depth, Layer.py:1309-1334
  __device__ __forceinline__ S calc_dry_depth() {
    const LayerK<S> l0 = pick_static(P, 0);
    S delta_theta = l0.te - F.TH(0);
    S tau = G->dt_h * l0.ksat / delta_theta;
    S g = capillary_drive(l0, F.TH(0), l0.te, 2);
    if (is_nan(val(g))) status |= LGAR_ST_NAN;
    S dry = R(0.5) * (tau + sq(tau * tau + R(4.0) * tau * g));
    return mn(P.cum[0], dry);
  }

  // Layer.create_surficial_front, Layer.py:1336-1416
  __device__ __forceinline__ void create_surficial_front(S dry_depth, S &ponded, S &infiltration) {
    if (nf >= cap) { status |= LGAR_ST_OVERFLOW; return; }
    const LayerK<S> l0 = pick_static(P, 0);
    S cur_theta = F.TH(0);
    S delta_theta = l0.te - cur_theta;
    S theta_new;
    bool to_bottom = false;
    if (val(dry_depth * delta_theta) > val(ponded)) {
      infiltration = ponded;
      theta_new = mn((cur_theta + ponded / dry_depth), l0.te);
      ponded = S(R(0.0));
    } else {
      infiltration = dry_depth * delta_theta;
      ponded = ponded - (dry_depth * delta_theta);
      theta_new = l0.te;
      to_bottom = !(val(dry_depth) < val(P.cum[0]));
    }
    for (int j = nf; j > 0; j--) F.copy(j, j - 1);
    nf++;
    F.Z(0) = dry_depth;
    F.TH(0) = theta_new;
    F.set_flag(0, 0, to_bottom);
    F.PS(0) = h_from_se<S, POL>(l0, se_from_theta(l0, theta_new));
    new_front_frozen = true;
    F.DZ(0) = S(R(0.0));
  }

  // insert_water, Layer.py:1418-1536 (get_drainage_neighbors :1584-1607, calc_bottom_sum_f_p :1538-1555):
  // Green-Ampt infiltration capacity f_p and the infiltration / runoff / ponding split
  __device__ __forceinline__ void insert_water(int fdd, S precip, S &ponded, S &infiltration, S &runoff) {
    const R dt = G->dt_h;
    S h_p = (ponded - precip) * dt;
    if (val(h_p) < R(0.0)) h_p = S(R(0.0));
    const int kfp = F.layer(fdd);
    int lo, len;
    range_of(kfp, lo, len);
    const int nxt_i = lo + 1;  // the front after the FIRST front of the free-drainage front's layer (quirk)
    // reference: AttributeError (Layer.py:1606) when the free-drainage front is the lone front of the bottom layer.
    // With one front per layer no neighbour is needed (Geff = 0); bottom_mode 1 lets that case through.
    if (nxt_i >= nf && (nf != NL || G->bottom_mode == 0)) { status |= LGAR_ST_STRUCT; return; }
    const LayerK<S> lk = pick(P, kfp);
    S g = S(R(0.0));
    // quirk: with a fully saturated one-front top layer right after a layer crossing, nxt_i is a front of the
    // NEXT layer and Se > 1: the reference raises ValueError (negative pow base, physics/utils.py:25-27);
    // here the NaN is flagged and the IEEE min below drops it (all ponded water infiltrates).
    // Geff(theta_1 -> theta_e) is a pure function of theta_1 and the layer's parameters, and during a storm theta_1 -- the
    // front BEHIND the wetting front, usually the layer's untouched boundary front -- stays the same for many steps: the
    // value of the previous call is reused when its inputs are bit for bit the same (the whole trapezoid is skipped when
    // that holds for every column of the wavefront; same results either way).
    if (nf != NL) {
      const S theta_1 = F.TH(nxt_i < nf ? nxt_i : nf - 1);
      bool hit = memo_layer == kfp && same_bits(theta_1, memo_theta);
      if constexpr (M::dual) {
        // Dual numbers: same_bits compares the tangent as well, the only place where a branch could depend on it.  The W
        // lanes of a shared group (LgarDims.tangent_share) hold the same values and different tangents and must enter the
        // trapezoid TOGETHER (geff_shared_blocks exchanges nodes between them): when any lane's tangent alone says "miss",
        // every lane whose values match recomputes -- the same result as its memo, bit for bit.
        if (share_lanes >= 2) {
          const bool value_hit = memo_layer == kfp && val(theta_1) == val(memo_theta);
          if (any_lane(value_hit && !hit) != 0ull) hit = false;
        }
      }
      if (hit) {
        g = memo_g;
      } else {
        g = capillary_drive(lk, theta_1, lk.te, 3);
        memo_theta = theta_1; memo_g = g; memo_layer = kfp;
      }
    }
    if (is_nan(val(g))) status |= LGAR_ST_NAN | LGAR_ST_NEGBASE;
    S f_p;
    if (kfp == 0) {
      f_p = P.ksat[0] * (R(1.0) + dv<POL>(g + h_p, F.Z(fdd)));
    } else {
      S fd_ksat = lk.ksat * G->frozen;
      S bottom_sum = dv<POL>(F.Z(fdd) - cum_prev(kfp), fd_ksat);
      bottom_sum = bottom_sum + dv<POL>(P.cum[0] - R(0.0), P.ksat[0] * G->frozen);
#pragma unroll
      for (int j = 1; j < NL - 1; j++)
        if (j < kfp) {
          const LayerK<S> lj = pick_static(P, j);
          S tl = theta_from_h<S, POL>(lj, F.PS(fdd));
          S kl = k_from_se<S, POL>(lj, se_from_theta(lj, tl));
          bottom_sum = bottom_sum + dv<POL>(P.cum[j] - P.cum[j - 1], kl);
        }
      f_p = dv<POL>(F.Z(fdd), bottom_sum) + dv<POL>((g + h_p) * fd_ksat, F.Z(fdd));
    }
    S pond_temp = ponded - f_p * dt;
    if (val(pond_temp) < R(0.0)) pond_temp = S(R(0.0));
    S fp_cm = f_p * dt;
    if (G->pdm > R(0.0)) {
      if (val(pond_temp) < G->pdm) {
        infiltration = mn(ponded, fp_cm);
        ponded = ponded - infiltration;
      } else if (val(pond_temp) > G->pdm) {
        ponded = S(G->pdm);
        infiltration = fp_cm;
      }
      S r = pond_temp - G->pdm;
      runoff = (val(r) > R(0.0)) ? r : S(R(0.0));
    } else {
      infiltration = mn(ponded, fp_cm);
      S r = ponded - infiltration;
      ponded = S(G->pdm);
      runoff = (val(r) > R(0.0)) ? r : S(R(0.0));
    }
  }

  // dpLGAR.set_internal_states, models/dpLGAR.py:97-147
  __device__ __forceinline__ void init_state() {
    nf = NL;
    status = 0;
    new_front_frozen = false;
#pragma unroll
    for (int k = 0; k < NL; k++) {
      const LayerK<S> lk = pick_static(P, k);
      F.Z(k) = P.cum[k];
      F.TH(k) = theta_from_h<S, POL>(lk, S(G->initial_psi));
      F.PS(k) = S(G->initial_psi);
      if (k == NL - 1) k_deepest = k_from_se<S, POL>(lk, se_from_theta(lk, F.TH(k)));
      F.DZ(k) = S(R(0.0));
      F.set_flag(k, k, true);
    }
    ponded_water = previous_precip = S(R(0.0));
#pragma unroll
    for (int i = 0; i < LGAR_GMAX; i++) giuh_q[i] = S(R(0.0));
    ending_volume = mass_balance();
    drain();
  }

  __device__ __forceinline__ void drain() {
    a_precip = a_pet = a_aet = a_infil = a_runoff = a_perc = a_giuh = a_disch = S(R(0.0));
  }

  // dpLGAR.forward, models/dpLGAR.py:154-299: one forcing step = nsub sub-steps
  __device__ __forceinline__ void forward(S precip, S pet) {
    const R dt = G->dt_h;
    // a NaN in the forcing slips through the reference unnoticed (every comparison with it is false; the step's runoff comes
    // out NaN, the front table stays finite): flagged here, a data fault the caller should hear about
    if (is_nan(val(precip)) || is_nan(val(pet))) status |= LGAR_ST_NAN;
    S ending_volume_sub = ending_volume;
    for (int sub = 0; sub < G->nsub; sub++) {
      if (status & DEAD) return;  // dead column
      new_front_frozen = false;
      post_mass_valid = false;
      S precip_sub = precip * dt;
      S pet_sub = pet * dt;
      S ponded_depth_sub = precip_sub + ponded_water;
      S ponded_water_sub = S(R(0.0)), runoff_sub = S(R(0.0)), infiltration_sub = S(R(0.0)), AET_sub = S(R(0.0));
      // create_surficial_front predicate, models/dpLGAR.py:310-323
      const bool create = (val(previous_precip) == R(0.0)) && (val(precip_sub) > R(0.0)) && (val(ponded_water) == R(0.0));
      LGAR_MEASURE_POINT(CLK, 0)
      LGAR_MEASURE_POINT(DUP_FDD)
      const int fdd = free_drainage_front();
      const bool saturated = val(F.TH(0)) >= val(P.te[0]);  // Layer.is_saturated, Layer.py:785-793
      if (val(pet) > R(0.0)) {
        if (!aet_psi_wp_known) {  // four pows, once per column and launch instead of once per sub-step
          aet_psi_wp_memo = aet_psi_wp<S, POL>(pick_static(P, 0), G->wp_psi);
          aet_psi_wp_known = true;
        }
        AET_sub = aet_from_psi_wp<S, POL>(pet, dt, F.PS(0), aet_psi_wp_memo);
      }
      if constexpr (!M::late_forcing_sums) {
        a_precip = a_precip + precip_sub;
        a_pet = a_pet + ((val(pet_sub) > R(0.0)) ? pet_sub : S(R(0.0)));
      }
      // Single call site for the front move (models/dpLGAR.py:199-266 re-ordered, same data flow): columns
      // that create a surficial front move first with zero infiltration and then create it; the others
      // infiltrate (insert_water) and then move.  update_ponded_depth touches no front state, so doing it
      // after the move is equivalent.
      const bool inserting = !create && val(ponded_depth_sub) > R(0.0);
      LGAR_MEASURE_POINT(CLK, 1)
      if (inserting) {
        LGAR_ABLATABLE(INSERT, insert_water(fdd, precip_sub, ponded_depth_sub, infiltration_sub, runoff_sub);)
        a_infil = a_infil + infiltration_sub;
        a_runoff = a_runoff + runoff_sub;
        ponded_water_sub = ponded_depth_sub;
      }
      LGAR_MEASURE_POINT(CLK, 2)
      if (!create || !saturated) {
        S perc_sub = S(R(0.0));
        LGAR_ABLATABLE(MOVE, perc_sub = move_wetting_front(create ? S(R(0.0)) : infiltration_sub, AET_sub, ending_volume_sub, fdd);)
        if (!create) a_perc = a_perc + perc_sub;
      }
      if (__builtin_expect(create && !saturated, 0)) {
        S dry_depth = calc_dry_depth();
        create_surficial_front(dry_depth, ponded_depth_sub, infiltration_sub);
        a_infil = a_infil + infiltration_sub;
        post_mass_valid = false;
        if constexpr (M::top_step) top_table = is_top_table();  // (one more front, tagged as a boundary front if it fills the layer)
      }
      if (!inserting) {
        // update_ponded_depth, models/dpLGAR.py:369-382
        if (val(ponded_depth_sub) < G->pdm) {
          runoff_sub = S(R(0.0));
          ponded_water_sub = ponded_depth_sub;
          ponded_depth_sub = S(R(0.0));
        } else {
          runoff_sub = ponded_depth_sub - G->pdm;
          ponded_depth_sub = S(G->pdm);
          ponded_water_sub = ponded_depth_sub;
          a_runoff = a_runoff + runoff_sub;
        }
      }
      LGAR_MEASURE_POINT(CLK, 5)
      LGAR_ABLATABLE(DZDT, calc_dzdt(ponded_depth_sub);)
      LGAR_MEASURE_POINT(CLK, 6)
      LGAR_MEASURE_POINT(DUP_DZDT, ponded_depth_sub)
      LGAR_MEASURE_POINT(DUP_MB, ending_volume_sub)
      if constexpr (M::fused_walk) {
        // (calc_dzdt touches neither depth nor theta: the walk after the sweep is still the column's mass)
        if (__builtin_expect(!post_mass_valid, 0)) post_mass = mass_balance();
        ending_volume_sub = post_mass;
      } else {
        ending_volume_sub = mass_balance();
      }
      LGAR_MEASURE_POINT(CLK, 7)
      previous_precip = precip_sub;
      ending_volume = ending_volume_sub;
      if constexpr (M::late_forcing_sums) {
        a_precip = a_precip + precip_sub;
        a_pet = a_pet + ((val(pet_sub) > R(0.0)) ? pet_sub : S(R(0.0)));
      }
      a_aet = a_aet + AET_sub;
      ponded_water = ponded_water_sub;
      // GIUH, models/dpLGAR.py:292-298 and lgar/giuh.py:8-20
      // (queue entries from the ng-th on are zero and stay zero -- nothing is ever added to them and zeros shift in from above --
      // so the sum and the shift need no test against ng: the same values, eight adds and eight moves)
      if constexpr (M::giuh_mem) {
        if (giuh_live || val(runoff_sub) > R(0.0)) {
          const int ng = G->ng;
          S q[LGAR_GMAX];
#pragma unroll
          for (int i = 0; i < LGAR_GMAX; i++) q[i] = (i < ng) ? S(giuh_mem[(size_t)i * giuh_stride]) : S(R(0.0));
#pragma unroll
          for (int i = 0; i < LGAR_GMAX; i++) if (i < ng) q[i] = q[i] + (G->giuh[i] * runoff_sub);
          const S now = q[0];
          R qsum = R(0.0);
#pragma unroll
          for (int i = 0; i < LGAR_GMAX; i++) {
            const S shifted = (i + 1 < LGAR_GMAX) ? q[(i + 1 < LGAR_GMAX) ? i + 1 : i] : S(R(0.0));
            qsum += val(shifted);  // (the next sub-step's test, summed in its order)
            if (i < ng) giuh_mem[(size_t)i * giuh_stride] = val(shifted);
          }
          giuh_live = qsum > R(0.0);
          a_giuh = a_giuh + now;
          a_disch = a_disch + now;
        }
      } else {
      R qsum = R(0.0);
#pragma unroll
      for (int i = 0; i < LGAR_GMAX; i++) qsum += val(giuh_q[i]);
      if (qsum > R(0.0) || val(runoff_sub) > R(0.0)) {
#pragma unroll
        for (int i = 0; i < LGAR_GMAX; i++) if (i < G->ng) giuh_q[i] = giuh_q[i] + (G->giuh[i] * runoff_sub);
        S now = giuh_q[0];
#pragma unroll
        for (int i = 0; i < LGAR_GMAX - 1; i++) giuh_q[i] = giuh_q[i + 1];
        giuh_q[LGAR_GMAX - 1] = S(R(0.0));
        a_giuh = a_giuh + now;
        a_disch = a_disch + now;
      }
      }
      // NaN anywhere in the front table (the reference raises at the pow that produces it, physics/utils.py:17-27).
      // MODE_FAST: a NaN depth or theta reaches the column mass just computed, a NaN psi reaches a theta within a step.
      if constexpr (M::literal) {
        bool bad = false;
        for (int i = 0; i < nf; i++) bad = bad || is_nan(val(F.TH(i))) || is_nan(val(F.Z(i))) || is_nan(val(F.PS(i)));
        if (bad) status |= LGAR_ST_NAN;
      } else {
        if (is_nan(val(ending_volume_sub))) status |= LGAR_ST_NAN;
      }
      LGAR_MEASURE_POINT(CLK, 8)
    }
  }
};

}  // namespace lgar
