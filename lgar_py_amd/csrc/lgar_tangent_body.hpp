// lgar_tangent_body.hpp -- what one lane of the forward-mode tangent kernels does (the differentiable path).
//
// Same device physics as the forward kernels, instantiated with Dual<R> (lgar_dual.hpp).  One launch integrates value +
// tangent for ONE parameter direction applied to every column's own parameters (columns are independent, so a one-hot
// direction over (alpha|n|Ksat, layer) yields every column's partial derivative at once) and contracts
// d runoff_t / d percolation_t with the caller's weights (the incoming gradient) on the fly: nothing is stored per step.
// A vector-Jacobian product over the 3 x L parameters is 3 x L such launches.
//
// Front capacity: values + tangents double the LDS per front, so the first kernel runs with LGAR_CAP_SMALL slots; a
// column that could outgrow them is flagged LGAR_ST_RESUME and the second kernel (LGAR_FMAX slots) integrates exactly
// those columns again from their fresh state (a tangent run always starts from set_internal_states).
//
// Window kernels (lgar_forward_tangent_window, lgar_tangent_window_kernel): tangent_lane<..., WINDOW = true> starts from a value
// state + tangent state (TWindow::in / din) instead of the fresh one, continues the fold of grad from grad_in, and the kernel
// that FINISHES a column stores both states (TWindow::out / dout).  A handed-over column is redone from in / din / grad_in, which
// nobody writes.  Everything about the window sits behind `if constexpr (WINDOW)`: the plain instantiations are what they were.
//
// Forced kernels (lgar_forward_tangent_forced, lgar_tangent_forced_kernel, lgar_tangent_forced_nl.hip): tangent_lane<..., WINDOW =
// true, FORCED = true> is the window lane whose forcing is a dual number too: step t runs forward(S(precip, dprecip), S(pet,
// dpet)) with the two tangents read from TForcing ([T][Nf][Fg]: every lane of a direction group has its own).  A forcing
// direction changes no value, so tangent_share, the capacity chain and the window are the window family's.  Everything about
// it sits behind `if constexpr (FORCED)`.
#pragma once
#include <type_traits>

#include "lgar_dual.hpp"
#include "lgar_plan.hpp"

namespace lgar {

template <typename R> struct TArgs {
  int N, T, Nf, Fg;  // Nf, Fg: columns of the forcing and weight arrays and group: column c reads column (c / Fg) % Nf
  int share;         // W = 2..32: each group of W consecutive columns is one soil column along W directions (LgarDims.tangent_share)
  int F;             // LgarDims.front_slots: the most fronts a column may hold, as in the forward kernels (same overflow flag)
  unsigned *ticket;  // null, or this launch's work counter (persistent waves)
  const unsigned *pending_in;  // null, or how many columns the first kernel of the chain handed over
  unsigned *pending_out;       // null, or where this kernel counts the columns it hands over
  int chain_first, chain_last;
  const R *alpha, *n, *ksat, *theta_e, *theta_r, *thick;  // [NL][N]
  const R *d_alpha, *d_n, *d_ksat;                        // [NL][N] or null
  const R *precip, *pet;                                  // [T][Nf]
  const R *w_runoff, *w_perc;                             // [T][Nf] or null; with fmap [T][N / Fg], column c reads c / Fg
  R *grad_out;                                            // [N]
  R *tangent_runoff;                                      // [T][N] or null
  int32_t *status;                                        // [N]
  Glob<R> G;
  const int32_t *fmap;                                    // null, or [N / Fg] (LgarForcing.column_map), as KArgs::fmap; last
};

// One per-front state as the window kernels see it: LgarState's arrays that carry a value (in, out) or a tangent (din, dout:
// flags and nf unused).  [F][N] / [N] / [LGAR_NSCAL][N], column fastest: a lane reads and writes its own column, coalesced.
template <typename Q, typename B, typename I> struct TStateP {
  Q *depth, *theta, *psi, *k, *dzdt;
  B *flags;
  I *nf;
  Q *scalars;
};
// the window block of one lgar_forward_tangent_window call; it follows TArgs in the window kernels' argument block
template <typename R> struct TWindow {
  TStateP<const R, const uint8_t, const int32_t> in, din;  // in.depth null: fresh state; din.depth null: zero tangents
  TStateP<R, uint8_t, int32_t> out, dout;                  // out.depth null: not wanted
  const R *grad_in;                                        // [N] or null = zeros
};
template <typename R> struct TWArgs {
  TArgs<R> a;
  TWindow<R> w;
};

// the forcing tangents of one lgar_forward_tangent_forced call; it follows the window block in the forced kernels' argument block
template <typename R> struct TForcing {
  const R *dprecip, *dpet;  // [T][Nf][Fg] or null = zeros: column c reads (t * Nf + cf) * Fg + c % Fg, cf its forcing column
};
template <typename R> struct TFArgs {
  TArgs<R> a;
  TWindow<R> w;
  TForcing<R> f;
};

template <typename Q, typename B, typename I> inline TStateP<Q, B, I> make_tstate(const LgarState *s) {
  TStateP<Q, B, I> t;
  t.depth = s ? (Q *)s->depth : nullptr; t.theta = s ? (Q *)s->theta : nullptr; t.psi = s ? (Q *)s->psi : nullptr;
  t.k = s ? (Q *)s->k : nullptr; t.dzdt = s ? (Q *)s->dzdt : nullptr;
  t.flags = s ? (B *)s->flags : nullptr;
  t.nf = s ? (I *)s->n_fronts : nullptr;
  t.scalars = s ? (Q *)s->scalars : nullptr;
  return t;
}

// the argument block of one lgar_forward_tangent call: one kernel on its own, no work counter (as make_args, lgar_plan.hpp)
template <typename R>
inline TArgs<R> make_targs(const LgarDims *d, const LgarParams *p, const LgarParams *dir, const LgarForcing *f, const void *w_runoff,
                           const void *w_perc, void *grad_out, void *tangent_runoff, int32_t *status) {
  TArgs<R> a;
  a.N = d->n_columns;
  a.T = d->n_steps;
  a.Nf = forcing_columns(d);
  a.Fg = forcing_group(d);
  a.share = d->tangent_share;
  a.F = front_slots(d);
  a.ticket = nullptr;
  a.pending_in = nullptr;
  a.pending_out = nullptr;
  a.chain_first = a.chain_last = 1;
  a.alpha = (const R *)p->alpha; a.n = (const R *)p->n; a.ksat = (const R *)p->ksat;
  a.theta_e = (const R *)p->theta_e; a.theta_r = (const R *)p->theta_r; a.thick = (const R *)p->thickness;
  a.d_alpha = (const R *)dir->alpha; a.d_n = (const R *)dir->n; a.d_ksat = (const R *)dir->ksat;
  a.precip = (const R *)f->precip;
  a.pet = (const R *)f->pet;
  a.fmap = f->column_map;
  a.w_runoff = (const R *)w_runoff;
  a.w_perc = (const R *)w_perc;
  a.grad_out = (R *)grad_out;
  a.tangent_runoff = (R *)tangent_runoff;
  a.status = status;
  a.G = make_glob<R>(d);
  return a;
}

// ... and of one lgar_forward_tangent_window call
template <typename R>
inline TWArgs<R> make_twargs(const LgarDims *d, const LgarParams *p, const LgarParams *dir, const LgarForcing *f, const void *w_runoff,
                             const void *w_perc, const LgarTangentWindow *win, void *grad_out, void *tangent_runoff, int32_t *status) {
  TWArgs<R> t;
  t.a = make_targs<R>(d, p, dir, f, w_runoff, w_perc, grad_out, tangent_runoff, status);
  t.w.in = make_tstate<const R, const uint8_t, const int32_t>(win->state_in);
  t.w.din = make_tstate<const R, const uint8_t, const int32_t>(win->dstate_in);
  t.w.out = make_tstate<R, uint8_t, int32_t>(win->state_out);
  t.w.dout = make_tstate<R, uint8_t, int32_t>(win->dstate_out);
  t.w.grad_in = (const R *)win->grad_in;
  return t;
}

// ... and of one lgar_forward_tangent_forced call
template <typename R>
inline TFArgs<R> make_tfargs(const LgarDims *d, const LgarParams *p, const LgarParams *dir, const LgarForcing *f, const LgarForcing *df,
                             const void *w_runoff, const void *w_perc, const LgarTangentWindow *win, void *grad_out,
                             void *tangent_runoff, int32_t *status) {
  const TWArgs<R> tw = make_twargs<R>(d, p, dir, f, w_runoff, w_perc, win, grad_out, tangent_runoff, status);
  TFArgs<R> t;
  t.a = tw.a;
  t.w = tw.w;
  t.f.dprecip = (const R *)df->precip;
  t.f.dpet = (const R *)df->pet;
  return t;
}

// the TArgs of any argument block: what the launch and the chain write (ticket, chain_step)
template <typename R> inline TArgs<R> &targs(TArgs<R> &a) { return a; }
template <typename R> inline TArgs<R> &targs(TWArgs<R> &a) { return a.a; }
template <typename R> inline TArgs<R> &targs(TFArgs<R> &a) { return a.a; }

// The walk of a tangent plan (lgar_plan.hpp), for both kernel families, the library's launcher and the host builds of the tests
// alike: kernel i's place in the chain goes into the block, then run(cap, mode, work counter) -- cap and mode as
// std::integral_constant -- runs kernel <CAP, MODE> on it and returns 0 or LGAR_E_*.  The first non-zero status ends the walk.
template <typename A, typename Run> inline int tangent_chain(A &a, const TangentPlan &plan, unsigned *tickets, Run run) {
  using Full = std::integral_constant<int, LGAR_FMAX>;
  using Small = std::integral_constant<int, LGAR_CAP_SMALL>;
  using Fast = std::integral_constant<int, MODE_FAST>;
  using Literal = std::integral_constant<int, MODE_LITERAL>;
  for (int i = 0; i < plan.n; i++) {
    unsigned *tk = chain_step(targs(a), i, plan.n, tickets);
    int rc;
    if (plan.literal) rc = run(Full(), Literal(), tk);
    else if (plan.caps[i] == LGAR_CAP_SMALL) rc = run(Small(), Fast(), tk);
    else rc = run(Full(), Fast(), tk);
    if (rc) return rc;
  }
  return 0;
}

template <typename R, int NL, int FMAX, int MODE, bool WINDOW = false, bool FORCED = false>
__device__ __forceinline__ void tangent_lane(const LGAR_KARG TArgs<R> *ap, size_t c, int lane, WaveLDS<Dual<R>, FMAX, 1> &lds,
                                             R *xchg = nullptr, const LGAR_KARG TWindow<R> *wp = nullptr,
                                             const LGAR_KARG TForcing<R> *fp = nullptr) {
  using S = Dual<R>;
  const LGAR_KARG TArgs<R> &a = *ap;
  const size_t N = (size_t)a.N;
  if (!a.chain_first) {
    const bool mine = (a.status[c] & LGAR_ST_RESUME) != 0;
    if (any_lane(mine) == 0ull) return;
    if (!mine) return;  // (the eight lanes of a shared group are handed over together: same values, same front counts)
  }
  ColParams<S, NL> P;
#pragma unroll
  for (int k = 0; k < NL; k++) {
    const size_t o = k * N + c;
    P.alpha[k] = S(a.alpha[o], a.d_alpha ? a.d_alpha[o] : R(0));
    P.n[k] = S(a.n[o], a.d_n ? a.d_n[o] : R(0));
    P.ksat[k] = S(a.ksat[o], a.d_ksat ? a.d_ksat[o] : R(0)) * a.G.frozen;  // models/dpLGAR.py:57
    P.te[k] = S(a.theta_e[o]);
    P.tr[k] = S(a.theta_r[o]);
    P.thick[k] = S(a.thick[o]);
    derive_layer(P.n[k], P.m[k], P.inv_m[k], P.inv_n[k]);
    P.cum[k] = (k == 0) ? P.thick[0] : P.cum[(k > 0) ? k - 1 : 0] + P.thick[k];
  }
  Column<S, NL, FMAX, MODE> col(P, &ap->G, make_view<S, FMAX>(&lds.f[0][0][0], &lds.fl[0][0], lane));
  col.share_lanes = (xchg != nullptr) ? a.share : 0;
  col.xchg = xchg;
  col.cap = FMAX < a.F ? FMAX : a.F;
  R grad = R(0);
  bool handed_over = false;
  if constexpr (WINDOW) {
    const LGAR_KARG TWindow<R> &w = *wp;
    if (w.in.depth != nullptr) {
      // state HBM -> LDS / registers, as forward_lane loads it (n_fronts clamped), each value with its tangent
      const bool dz = w.din.depth != nullptr;
      const int nf_stored = w.in.nf[c];
      const int nf = nf_stored < 0 ? 0 : (nf_stored > col.cap ? col.cap : nf_stored);
      col.nf = nf;
      col.status = (nf < NL) ? LGAR_ST_STRUCT : 0;  // not a state lgar_state_init / lgar_forward produced: column is skipped
      col.new_front_frozen = false;
      for (int i = 0; i < nf; i++) {
        const size_t o = (size_t)i * N + c;
        col.F.Z(i) = S(w.in.depth[o], dz ? w.din.depth[o] : R(0));
        col.F.TH(i) = S(w.in.theta[o], dz ? w.din.theta[o] : R(0));
        col.F.PS(i) = S(w.in.psi[o], dz ? w.din.psi[o] : R(0));
        col.F.DZ(i) = S(w.in.dzdt[o], dz ? w.din.dzdt[o] : R(0));
        col.F.flag(i) = w.in.flags[o];
      }
      col.ponded_water = S(w.in.scalars[0 * N + c], dz ? w.din.scalars[0 * N + c] : R(0));
      col.previous_precip = S(w.in.scalars[1 * N + c], dz ? w.din.scalars[1 * N + c] : R(0));
      col.ending_volume = S(w.in.scalars[2 * N + c], dz ? w.din.scalars[2 * N + c] : R(0));
#pragma unroll
      for (int i = 0; i < LGAR_GMAX; i++) col.giuh_q[i] = S(w.in.scalars[(3 + i) * N + c], dz ? w.din.scalars[(3 + i) * N + c] : R(0));
      col.k_deepest = S(R(0));
      if (nf > 0) col.k_deepest = S(w.in.k[(size_t)(nf - 1) * N + c], dz ? w.din.k[(size_t)(nf - 1) * N + c] : R(0));
      col.drain();
      if (nf_stored > col.cap) {
        // more fronts than this kernel can hold: the next kernel of the chain takes the column before its first row, or
        // (last kernel: more than the state arrays have rows) front overflow
        if (!a.chain_last) handed_over = true;
        else col.status |= LGAR_ST_OVERFLOW;
      }
    } else {
      col.init_state();
    }
    if (w.grad_in != nullptr) grad = w.grad_in[c];
  } else {
    col.init_state();
  }
  const size_t Nf = (size_t)a.Nf;
  // this column's forcing column: by the layout, or by the caller's index (read here, once, and clamped), as in forward_lane
  size_t cf;
  if (a.fmap != nullptr) {
    const int m = a.fmap[c / (size_t)a.Fg];
    cf = (size_t)(m < 0 ? 0 : (m < a.Nf ? m : a.Nf - 1));
  } else {
    cf = (Nf == N) ? c : (c / (size_t)a.Fg) % Nf;
  }
  // The weights: without a map they have the forcing's layout and ONE offset serves both (t * Nf + cf).  With a map they are
  // [T][N / Fg] and column c reads c / Fg: that offset is worked out where it is used, from values that are at hand anyway
  // (c, and N and Fg in the argument block), so the loop carries nothing new across a step in either case.
  // One wave per SIMD: nothing else covers a load's latency, so a step's forcing and weights are loaded one step AHEAD (four
  // values in registers across a step; they are taken into their registers before the step's optional store is issued --
  // loads and stores share one counter).
  R precip_ahead = R(0), pet_ahead = R(0), wr_ahead = R(0), wp_ahead = R(0);
  if (a.T > 0) {
    precip_ahead = a.precip[cf];
    pet_ahead = a.pet[cf];
    const size_t ow = (a.fmap != nullptr) ? (size_t)((unsigned)c / (unsigned)a.Fg) : cf;
    if (a.w_runoff) wr_ahead = a.w_runoff[ow];
    if (a.w_perc) wp_ahead = a.w_perc[ow];
  }
  // FORCED: the forcing's two tangents travel with the values: loaded one step ahead, settled with them, carried as they are.
  // Their offset is the values' times Fg plus this lane's place in its direction group (with Nf = N / Fg: t * N + c).
  [[maybe_unused]] R dprecip_ahead = R(0), dpet_ahead = R(0);
  [[maybe_unused]] size_t cg = 0;
  if constexpr (FORCED) {
    cg = (size_t)((unsigned)c % (unsigned)a.Fg);
    if (a.T > 0) {
      const size_t od = cf * (size_t)a.Fg + cg;
      if (fp->dprecip) dprecip_ahead = fp->dprecip[od];
      if (fp->dpet) dpet_ahead = fp->dpet[od];
    }
  }
  for (int t = 0; t < a.T; t++) {
    if constexpr (WINDOW) {
      if (handed_over) break;  // (handed over at load)
    }
    if (!a.chain_last && col.nf + a.G.nsub > FMAX) {
      handed_over = true;  // could outgrow this kernel's front capacity: the next kernel redoes this column
      break;
    }
    const R precip = precip_ahead, pet = pet_ahead, wr = wr_ahead, wp = wp_ahead;
    {
      const size_t tn = (size_t)((t + 1 < a.T) ? t + 1 : t);
      const size_t o = tn * Nf + cf;
      precip_ahead = a.precip[o];
      pet_ahead = a.pet[o];
      size_t ow = o;
      if (a.fmap != nullptr) ow = tn * (size_t)((unsigned)a.N / (unsigned)a.Fg) + (size_t)((unsigned)c / (unsigned)a.Fg);
      if (a.w_runoff) wr_ahead = a.w_runoff[ow];
      if (a.w_perc) wp_ahead = a.w_perc[ow];
    }
    if constexpr (FORCED) {
      const R dprecip = dprecip_ahead, dpet = dpet_ahead;
      const size_t tn = (size_t)((t + 1 < a.T) ? t + 1 : t);
      const size_t od = (tn * Nf + cf) * (size_t)a.Fg + cg;
      if (fp->dprecip) dprecip_ahead = fp->dprecip[od];
      if (fp->dpet) dpet_ahead = fp->dpet[od];
      col.forward(S(precip, dprecip), S(pet, dpet));
      settle_load(dprecip_ahead); settle_load(dpet_ahead);
    } else {
      col.forward(S(precip), S(pet));
    }
    settle_load(precip_ahead); settle_load(pet_ahead); settle_load(wr_ahead); settle_load(wp_ahead);
    if (a.w_runoff) grad += wr * col.a_runoff.d;
    if (a.w_perc) grad += wp * col.a_perc.d;
    if (a.tangent_runoff) a.tangent_runoff[(size_t)t * N + c] = col.a_runoff.d;
    col.drain();
  }
  if constexpr (WINDOW) {
    // only the kernel that finishes a column writes its results: grad_out may be grad_in, and the next kernel reads that
    if (!handed_over) {
      a.grad_out[c] = grad;
      const LGAR_KARG TWindow<R> &w = *wp;
      if (w.out.depth != nullptr) {
        // state LDS / registers -> HBM, as store_state writes it (rows [0, nf)), each value with its tangent
        const int rows = col.nf < a.F ? col.nf : a.F;
        for (int i = 0; i < rows; i++) {
          const size_t o = (size_t)i * N + c;
          const S kk = (i < col.nf - 1) ? col.front_k(i, pick(col.P, col.F.layer(i))) : col.k_deepest;
          w.out.depth[o] = col.F.Z(i).v; w.dout.depth[o] = col.F.Z(i).d;
          w.out.theta[o] = col.F.TH(i).v; w.dout.theta[o] = col.F.TH(i).d;
          w.out.psi[o] = col.F.PS(i).v; w.dout.psi[o] = col.F.PS(i).d;
          w.out.k[o] = kk.v; w.dout.k[o] = kk.d;
          w.out.dzdt[o] = col.F.DZ(i).v; w.dout.dzdt[o] = col.F.DZ(i).d;
          w.out.flags[o] = col.F.flag(i);
        }
        w.out.nf[c] = col.nf;
        w.out.scalars[0 * N + c] = col.ponded_water.v; w.dout.scalars[0 * N + c] = col.ponded_water.d;
        w.out.scalars[1 * N + c] = col.previous_precip.v; w.dout.scalars[1 * N + c] = col.previous_precip.d;
        w.out.scalars[2 * N + c] = col.ending_volume.v; w.dout.scalars[2 * N + c] = col.ending_volume.d;
#pragma unroll
        for (int i = 0; i < LGAR_GMAX; i++) {
          w.out.scalars[(3 + i) * N + c] = col.giuh_q[i].v;
          w.dout.scalars[(3 + i) * N + c] = col.giuh_q[i].d;
        }
      }
    }
  } else {
    a.grad_out[c] = handed_over ? R(0) : grad;
  }
  a.status[c] = handed_over ? (col.status | LGAR_ST_RESUME) : col.status;
  if (a.pending_out != nullptr) {
    const unsigned long long m = any_lane(handed_over);
    if (m != 0ull && first_active_lane()) atomic_add(a.pending_out, (unsigned)__builtin_popcountll(m));
  }
}

}  // namespace lgar
