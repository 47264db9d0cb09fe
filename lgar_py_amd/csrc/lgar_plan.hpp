// lgar_plan.hpp -- what one call launches, and with which arguments: the argument blocks of the kernels and the
// front-capacity chain of a forward / tangent call.  Host-only and free of the HIP API, so the library's launchers
// (lgar_kernels_nl.hip, lgar_tangent_nl.hip) and the test-only device-code simulator (tests/devsim, -DLGAR_DEVSIM) walk the
// SAME plans with the SAME arguments; tests/test_launch_plan.py pins the plans themselves.  The tangent family's walk of its plan
// is shared too: tangent_chain, beside the argument blocks it fills (lgar_tangent_body.hpp).
#pragma once
#include "lgar_forward_body.hpp"

// The soil-layer counts the library is compiled for, as an X-macro: one translation unit per count and kernel family
// (lgar_launch.hpp), one case of the dispatch (lgar_kernels.hip), one instantiation of the simulator.  A build of fewer counts
// (build.py build_variant, tests/devsim) defines it on the command line; build.py's LAYERS is the Python-side list.
#ifndef LGAR_LAYERS
#define LGAR_LAYERS(X) X(2) X(3) X(4) X(5) X(6)
namespace lgar {
constexpr bool default_layers_span_lmin_lmax() {
  int want = LGAR_LMIN;
#define LGAR_X(n) if (n != want++) return false;
  LGAR_LAYERS(LGAR_X)
#undef LGAR_X
  return want == LGAR_LMAX + 1;
}
static_assert(default_layers_span_lmin_lmax(), "LGAR_LAYERS must list LGAR_LMIN .. LGAR_LMAX");
}  // namespace lgar
#endif

namespace lgar {

template <typename R> inline Glob<R> make_glob(const LgarDims *d) {
  Glob<R> G;
  G.dt_h = (R)d->dt_h;
  G.initial_psi = (R)d->initial_psi;
  G.pdm = (R)d->ponded_depth_max;
  G.wp_psi = (R)d->wilting_point_psi;
  G.frozen = (R)d->frozen_factor;
  for (int i = 0; i < LGAR_GMAX; i++) G.giuh[i] = (i < d->n_giuh) ? (R)d->giuh[i] : R(0);
  G.nint = d->nint;
  G.nsub = d->num_subcycles;
  G.ng = d->n_giuh;
  G.bottom_mode = d->bottom_mode;
  G.closed_form = d->use_closed_form_G;
  // literal searches (mode 0) are unbounded in the reference: generous cap.  In the fast modes the depth search needs a
  // few dozen iterations when it converges at all, so a diverging column (reference: endless loop) is cut off early.
  G.iter_cap = d->iter_cap > 0 ? d->iter_cap : (d->search_mode != 0 ? 5000LL : 2000000LL);
  return G;
}

inline int front_slots(const LgarDims *d) { return d->front_slots > 0 ? d->front_slots : LGAR_FMAX; }
inline int forcing_group(const LgarDims *d) { return d->forcing_group > 1 ? d->forcing_group : 1; }
inline int forcing_columns(const LgarDims *d) {
  return d->forcing_columns > 0 ? d->forcing_columns : d->n_columns / forcing_group(d);
}

inline int check_dims(const LgarDims *d) {
  if (!d) return LGAR_E_ARG;
  if (d->n_columns <= 0 || d->n_layers < LGAR_LMIN || d->n_layers > LGAR_LMAX) return LGAR_E_ARG;
  if (d->n_giuh < 0 || d->n_giuh > LGAR_GMAX) return LGAR_E_ARG;
  if (d->nint <= 0 || d->num_subcycles <= 0 || d->n_steps < 0 || d->n_steps >= (1 << 23)) return LGAR_E_ARG;
  if (d->search_mode < 0 || d->search_mode > 2) return LGAR_E_ARG;
  if (d->front_slots < 0 || d->front_slots > LGAR_FMAX || (d->front_slots > 0 && d->front_slots < d->n_layers + 1)) return LGAR_E_ARG;
  if (d->forcing_columns < 0 || d->forcing_group < 0 || d->n_columns % forcing_group(d) != 0) return LGAR_E_ARG;
  if (d->tangent_share != 0 && (d->tangent_share < 2 || d->tangent_share > 32 || d->n_columns % d->tangent_share != 0)) return LGAR_E_ARG;
  if (d->geff_mode < 0 || d->geff_mode > 1) return LGAR_E_ARG;
  if (d->forward_lanes < 0 || d->forward_lanes > 64 || d->forward_lanes == 2 || d->forward_lanes == 3) return LGAR_E_ARG;
  if (!(d->dt_h > 0.0)) return LGAR_E_ARG;
  return 0;
}

// The forcing layout of a call that READS forcing (lgar_forward, lgar_forward_tangent; check_dims has passed).  It depends on
// LgarForcing.column_map, so it is not check_dims' business: the entry points that read no forcing (lgar_state_init,
// lgar_soil_moisture ...) take whatever layout the last call left in the caller's LgarDims.  Without a map the forcing columns
// divide the groups of columns (broadcast); with one there are simply Nf >= 1 of them.
inline int check_forcing_layout(const LgarDims *d, const LgarForcing *f) {
  if (f != nullptr && f->column_map != nullptr) return d->forcing_columns >= 1 ? 0 : LGAR_E_ARG;
  if (d->forcing_columns > 0 && (d->n_columns / forcing_group(d)) % d->forcing_columns != 0) return LGAR_E_ARG;
  return 0;
}

// What lgar_forward_tangent and lgar_forward_tangent_window refuse alike.
inline int check_tangent_call(const LgarDims *d, const LgarParams *p, const LgarParams *dir, const LgarForcing *f, const void *grad_out,
                              const int32_t *status) {
  const int rc = check_dims(d);
  if (rc) return rc;
  if (!p || !dir || !f || !grad_out || !status) return LGAR_E_ARG;
  if (!p->alpha || !p->n || !p->ksat || !p->theta_e || !p->theta_r || !p->thickness) return LGAR_E_ARG;
  if (d->n_steps > 0 && (!f->precip || !f->pet)) return LGAR_E_ARG;
  return check_forcing_layout(d, f);
}

// What lgar_forward_tangent_window refuses beyond that (include/lgar.h).
inline int check_window(const LgarTangentWindow *w) {
  if (!w) return LGAR_E_ARG;
  if (w->dstate_in && !w->state_in) return LGAR_E_ARG;
  if ((w->state_out != nullptr) != (w->dstate_out != nullptr)) return LGAR_E_ARG;
  auto values = [](const LgarState *s) { return s->depth && s->theta && s->psi && s->k && s->dzdt && s->scalars; };
  auto table = [](const LgarState *s) { return s->flags && s->n_fronts; };
  if (w->state_in && !(values(w->state_in) && table(w->state_in))) return LGAR_E_ARG;
  if (w->dstate_in && !values(w->dstate_in)) return LGAR_E_ARG;
  if (w->state_out && !(values(w->state_out) && table(w->state_out) && values(w->dstate_out))) return LGAR_E_ARG;
  // an output state over an input's arrays: a handed-over column is redone from the input, which must still be there
  auto shares = [](const LgarState *o, const LgarState *i) {
    return o && i && (o->depth == i->depth || o->theta == i->theta || o->psi == i->psi || o->k == i->k || o->dzdt == i->dzdt ||
                      o->scalars == i->scalars || (o->flags && o->flags == i->flags) || (o->n_fronts && o->n_fronts == i->n_fronts));
  };
  if (shares(w->state_out, w->state_in) || shares(w->state_out, w->dstate_in) || shares(w->dstate_out, w->state_in) ||
      shares(w->dstate_out, w->dstate_in) || shares(w->dstate_out, w->state_out))
    return LGAR_E_ARG;
  return 0;
}

// What lgar_forward_tangent_forced refuses beyond that: the forcing tangents have the layout [n_steps][Nf][forcing_group], which
// the forcing's own column (layout or column_map) already indexes; a map of their own has no meaning.
inline int check_forcing_direction(const LgarForcing *df) {
  if (!df || df->column_map != nullptr) return LGAR_E_ARG;
  return 0;
}

// The forward / init kernels' argument block of one call: one kernel on its own, no work counter, one lane per column (the
// launchers set ticket and coop; chain_step the position in a chain).
template <typename R>
inline KArgs<R> make_args(const LgarDims *d, const LgarParams *p, LgarState *s, const LgarForcing *f, const LgarStepOut *o,
                          int32_t *status) {
  KArgs<R> a;
  a.N = d->n_columns;
  a.T = d->n_steps;
  a.F = front_slots(d);
  a.Nf = forcing_columns(d);
  a.Fg = forcing_group(d);
  a.coop = 1;
  a.ticket = nullptr;
  a.pending_in = nullptr;
  a.pending_out = nullptr;
  a.chain_first = a.chain_last = 1;
  a.alpha = (const R *)p->alpha; a.n = (const R *)p->n; a.ksat = (const R *)p->ksat;
  a.theta_e = (const R *)p->theta_e; a.theta_r = (const R *)p->theta_r; a.thick = (const R *)p->thickness;
  a.depth = (R *)s->depth; a.theta = (R *)s->theta; a.psi = (R *)s->psi; a.k = (R *)s->k; a.dzdt = (R *)s->dzdt;
  a.flags = s->flags;
  a.nf = s->n_fronts;
  a.scalars = (R *)s->scalars;
  a.totals = (R *)s->totals;
  a.precip = f ? (const R *)f->precip : nullptr;
  a.pet = f ? (const R *)f->pet : nullptr;
  a.fmap = f ? f->column_map : nullptr;
  for (int j = 0; j < LGAR_NACC; j++) a.series[j] = o ? (R *)o->series[j] : nullptr;
  a.basin = o ? o->basin : nullptr;
  a.basin_mask = o ? o->basin_mask : 0u;
  a.weights = o ? (const R *)o->weights : nullptr;
  a.counters = o ? (unsigned long long *)o->counters : nullptr;
  a.call_sums = o ? (R *)o->call_sums : nullptr;
  a.status = status;
  a.G = make_glob<R>(d);
  return a;
}

// lanes per column for this job: LgarDims.forward_lanes when given, else as many as keep the job within ONE wave per SIMD
// (ceil(n_columns / 1024) columns per wavefront, 64 / that lanes each) -- two such waves on a SIMD contend for its vector ALU
// in the trapezoid and the gain is gone (measured: 10 000 columns x 8 lanes = 1250 waves run slower than 157 plain ones; 6
// lanes = 1000 waves).  At most 16 columns per wavefront (that many LDS tables): 4..64 lanes; always 1 for fp32, closed-form
// G, the literal mode and more than 128 trapezoid intervals.  The rule is the same for the native double-precision trapezoid
// (MODE_COOP kernels) and the mixed-precision one (LgarDims.geff_mode = 1: MODE_MIXED_COOP kernels).
template <typename R> inline int cooperating_lanes(const LgarDims *dims, unsigned simds) {
  if (ScalarKind<R>::f32 || dims->search_mode == 0 || dims->use_closed_form_G) return 1;
  if (dims->nint > LGAR_COOP_TAB) return 1;  // the groups' LDS tables hold one head / node per trapezoid interval
  if (dims->forward_lanes > 0) return dims->forward_lanes;
  if (dims->search_mode == 2) return 1;      // the capacity chain was asked for (tests): plain kernels
  const size_t groups = ((size_t)dims->n_columns + simds - 1) / simds;  // columns a wavefront has to take
  return groups <= LGAR_COOP_GROUPS ? (int)(WAVE / groups) : 1;         // 64, 32, 21, 16, 12, 10, 9, 8, 7, 6, 5, 5, 4, 4, 4, 4
}

// The kernels of one lgar_forward call, in launch order (the front-capacity chain, see lgar_forward_body.hpp): their front
// capacities, and which kernel family runs them.  `simds`: the chip's SIMD count (one wave slot each).
struct ForwardPlan {
  bool literal;  // MODE_LITERAL: the reference's literal searches, verification mode, one kernel at the full capacity
  bool mixed;    // double precision with LgarDims.geff_mode = 1: the mixed-precision trapezoid (MODE_MIXED / MODE_MIXED_COOP)
  int coop;      // lanes per column (cooperating_lanes)
  int caps[3];
  int n;
};

template <typename R> inline ForwardPlan forward_plan(const LgarDims *dims, int NL, unsigned simds) {
  ForwardPlan p;
  p.literal = dims->search_mode == 0;
  p.mixed = ScalarKind<R>::f64 && !p.literal && dims->geff_mode == 1;
  p.coop = 1;
  p.n = 0;
  if (!p.literal) {
    const unsigned blocks = (unsigned)((dims->n_columns + WAVE - 1) / WAVE);
    const int slots = front_slots(dims);
    // smallest capacity that leaves room for a forcing step (one front per layer + one new front per sub-step + slack);
    // small jobs (under one wave per SIMD) gain nothing from occupancy and start at the full capacity
    const int need = NL + dims->num_subcycles + 2;
    // Jobs that cannot fill the chip (the reference's own use is ONE column, agents/DifferentiableLGAR.py:117-125): in double
    // precision every column gets 4..64 cooperating lanes that split the Geff trapezoid's nodes, the pows that open it and the
    // front sweep's independent evaluations (lgar_geff.hpp geff_nodes_cooperative / geff_ends_cooperative, lgar_column.hpp coop_sweep_thetas /
    // calc_dzdt_pairs).  Results are bit for bit those of one lane per column.  Such a job runs the 32-front kernel directly
    // (MODE_COOP: front table and exchange table once per GROUP of lanes, 34 KB of LDS per wave, one wave per SIMD): no capacity
    // chain, no hand-over.
    p.coop = cooperating_lanes<R>(dims, simds);
    const bool tiny = (blocks <= 1024u && dims->search_mode != 2) || p.coop > 1;  // search_mode 2: chain forced (tests)
    if (!tiny && need <= LGAR_CAP_SMALL && slots > LGAR_CAP_SMALL) p.caps[p.n++] = LGAR_CAP_SMALL;
    if (!tiny && need <= LGAR_CAP_MID && slots > LGAR_CAP_MID) p.caps[p.n++] = LGAR_CAP_MID;
  }
  p.caps[p.n++] = LGAR_FMAX;
  return p;
}

// A block of the tangent kernels = the columns of one wavefront: 64, or -- W lanes sharing a column (tangent_share) --
// floor(64 / W) groups of W.
__host__ __device__ inline unsigned columns_per_block(int share) { return share >= 2 ? (unsigned)((WAVE / share) * share) : (unsigned)WAVE; }

// The kernels of one lgar_forward_tangent call: values + tangents double the LDS per front, so the chain is LGAR_CAP_SMALL ->
// LGAR_FMAX (lgar_tangent_body.hpp).
struct TangentPlan {
  bool literal;
  int caps[2];
  int n;
  unsigned columns_per_block, blocks;
};

inline TangentPlan tangent_plan(const LgarDims *dims, int NL) {
  TangentPlan p;
  p.literal = dims->search_mode == 0;
  p.columns_per_block = columns_per_block(dims->tangent_share);
  p.blocks = ((unsigned)dims->n_columns + p.columns_per_block - 1) / p.columns_per_block;
  p.n = 0;
  const bool chain = (NL + dims->num_subcycles + 2 <= LGAR_CAP_SMALL) && (p.blocks > 1024u || dims->search_mode == 2);
  if (!p.literal && chain) p.caps[p.n++] = LGAR_CAP_SMALL;
  p.caps[p.n++] = LGAR_FMAX;
  return p;
}

// Kernel i of a chain of n: its position, where it finds the number of columns handed over to it and where it counts those
// it hands over (tickets[4..5]: by kernel 0, 1).  Returns the kernel's work counter (tickets[i]); all null without tickets.
template <typename A> inline unsigned *chain_step(A &a, int i, int n, unsigned *tickets) {
  a.chain_first = (i == 0);
  a.chain_last = (i == n - 1);
  a.pending_in = (tickets && i > 0) ? tickets + 4 + (i - 1) : nullptr;
  a.pending_out = (tickets && i < n - 1) ? tickets + 4 + i : nullptr;
  return tickets ? tickets + i : nullptr;
}

}  // namespace lgar
