/*
 * lgar.h -- C-ABI of the MI355X-native many-column LGAR engine (liblgar_hip.so).
 *
 * The reference (LGAR-py, "dpLGAR") has no FFI: its only seam is the Python object surface of
 * dpLGAR(nn.Module) (dpLGAR/models/dpLGAR.py:30-299) as driven by the agent
 * (dpLGAR/agents/DifferentiableLGAR.py:94-172) and drained by MassBalance
 * (dpLGAR/models/physics/MassBalance.py:31-53).  The entry points below are what a binding for that
 * path needs; each cites the reference interface it replaces.  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *  - Plain pointers + sizes; no torch types.  Every pointer is DEVICE memory owned by the caller
 *    (the library never allocates, frees or copies host<->device), valid on the given stream.
 *  - All arrays are struct-of-arrays, COLUMN-FASTEST: a per-layer quantity is [n_layers][n_columns],
 *    a per-front quantity [front_slots][n_columns], a forcing / per-step series [n_steps][n_columns].
 *  - dtype: LGAR_F32 or LGAR_F64 selects the element type of every `void*` array (float / double).
 *  - Return value: 0 ok; <0 argument / launch error (LGAR_E_*).  Physics faults never abort the
 *    launch: they set bits in status[column] (the reference raises Python exceptions instead:
 *    physics/utils.py:17-27,181-183; layers/Layer.py:1206-1208,1115,980).
 *  - Re-entrant, no globals; one in-flight call per state buffer.  `stream` is a hipStream_t (NULL =
 *    default stream).
 */
#ifndef LGAR_H
#define LGAR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Front capacity.  The reference's per-layer front lists are unbounded (layers/Layer.py:1336-1416; observed <= 8 on the
 * bundled cases).  The kernels keep a wave's front table in LDS and are compiled for three capacities; lgar_forward
 * starts with the smallest that fits and hands the (rare) columns that outgrow it to the next one in the same call, so a
 * column can hold up to LGAR_FMAX fronts (LGAR_ST_OVERFLOW beyond) while the common case runs at the occupancy of 8. */
#define LGAR_CAP_SMALL 8
#define LGAR_CAP_MID 16
#define LGAR_FMAX 32
#define LGAR_LMIN 2   /* the reference itself needs >= 2 layers (Layer.py:204) */
#define LGAR_LMAX 6   /* soil layers: kernels are compiled for 2 .. 6 (BASELINE configs: 3; the reference builds any number, Layer.py:77-89) */
#define LGAR_GMAX 8   /* GIUH ordinates */
#define LGAR_NSCAL (3 + LGAR_GMAX) /* scalars row count: ponded_water, previous_precip, ending_volume, giuh_queue[GMAX] */
#define LGAR_NACC 10  /* precip, PET, AET, infiltration, runoff, percolation, giuh_runoff, discharge, ponded_water, ending_volume */

#define LGAR_F32 0
#define LGAR_F64 1

#define LGAR_E_ARG (-1)     /* bad argument (null pointer, size out of range, unsupported n_layers) */
#define LGAR_E_LAUNCH (-2)  /* HIP launch error */
#define LGAR_E_NODEVICE (-3)

/* status bits, one int32 per column */
#define LGAR_ST_NAN 1
#define LGAR_ST_NEGBASE 2
#define LGAR_ST_THETA_ORDER 4
#define LGAR_ST_OVERFLOW 8
#define LGAR_ST_ITERCAP 16
#define LGAR_ST_BOTTOM 32
#define LGAR_ST_STRUCT 64
#define LGAR_ST_FAULT_MASK 0x7f
/* internal to a lgar_forward call (never set when it returns): the column was handed to the next kernel of the
 * front-capacity chain at the step index held in bits 8..31 */
#define LGAR_ST_RESUME 128
#define LGAR_ST_STEP_SHIFT 8
#define LGAR_NTICKETS 8   /* LgarState.tickets: [0..2] one work counter per kernel of a call's capacity chain; [4..5] columns
                             handed over by the first / second kernel (a next kernel with nothing to do exits at once) */
#define LGAR_NCOUNTERS 4  /* LgarStepOut.counters: [0] wave-level Geff evaluations of the launch; [1..3] reserved */

/* front flag byte: low 7 bits layer number, bit 7 = to_bottom (layers/WettingFront.py:39,49) */
#define LGAR_FLAG_BOTTOM 0x80

/* Run-time constants: the cfg keys dpLGAR(cfg) reads (models/dpLGAR.py:31-95, physics/GlobalParams.py:79-138). */
typedef struct {
  int32_t n_columns;      /* N */
  int32_t n_layers;       /* len(cfg.data.layer_thickness); LGAR_LMIN..LGAR_LMAX */
  int32_t n_steps;        /* T forcing rows processed by this call */
  int32_t num_subcycles;  /* cfg.models.num_subcycles */
  int32_t nint;           /* cfg.constants.nint (120) */
  int32_t n_giuh;         /* len(cfg.data.giuh_ordinates) <= LGAR_GMAX */
  int32_t search_mode;    /* 0 = the reference's literal line searches (Layer.py:275-317, 681-701) */
  int32_t bottom_mode;    /* 0 = reference behaviour: a front reaching the domain bottom sets LGAR_ST_BOTTOM and the
                             column stops (the reference crashes, Layer.py:980); 1 = LGAR-C intent: the bottom layer is
                             exempt from the layer-boundary step and wetting_front_cross_domain_boundary
                             (Layer.py:1010-1053) turns the overshoot into percolation.  Parity of mode 1 is unpinned. */
  int32_t use_closed_form_G; /* cfg.data.use_closed_form_G: Brooks-Corey closed-form capillary drive
                                (lgar/green_ampt.py:85-98) instead of the nint-interval trapezoid (:45-84) */
  int32_t front_slots;       /* rows of the per-front state arrays, 3 .. LGAR_FMAX (0 = LGAR_FMAX): the most fronts a
                                column can hold in this state buffer */
  double dt_h;               /* cfg.models.subcycle_length_h */
  double initial_psi;        /* cfg.data.initial_psi */
  double ponded_depth_max;   /* cfg.data.ponded_depth_max */
  double wilting_point_psi;  /* cfg.data.wilting_point_psi */
  double frozen_factor;      /* cfg.constants.frozen_factor */
  double giuh[LGAR_GMAX];    /* cfg.data.giuh_ordinates */
  int64_t iter_cap;          /* cap on the reference's unbounded line searches (0 = default) */
  int32_t forcing_columns;   /* columns of the forcing (and tangent-weight) arrays: 0 or n_columns = one forcing column per
                                soil column; a divisor Nf of n_columns = broadcast, soil column c reads forcing column c % Nf
                                (Nf = 1: one basin series for every column, the reference's Data yields exactly that,
                                data/Data.py:32-37; the differentiable path lays its parameter directions side by side this
                                way without replicating the forcing) */
  int32_t forcing_group;     /* 0 or 1: as above.  G > 1: G CONSECUTIVE soil columns share a forcing column -- column c reads
                                forcing column (c / G) % forcing_columns; n_columns must be a multiple of G * forcing_columns.
                                (The differentiable path puts the G parameter directions of one column in adjacent lanes:
                                they take the same branches, so a wavefront diverges over 64 / G columns instead of 64.) */
  int32_t tangent_share;     /* lgar_forward_tangent only.  0: every column stands alone.  W = 2..32: the caller guarantees that
                                each group of W consecutive columns is ONE soil column (identical parameters and forcing) with W
                                different directions; the W lanes then share the Geff trapezoid -- each evaluates every W-th node,
                                and the tangent of the whole sum comes from five direction-independent sums (fp64 fast modes;
                                ignored elsewhere).  n_columns must be a multiple of W; a wavefront carries floor(64 / W) such
                                groups (W = 9, the 3 x L parameters of a 3-layer column: 7 groups, one idle lane). */
  int32_t geff_mode;         /* 0: the Geff trapezoid (lgar/green_ampt.py:45-84) in the precision of `dtype`.  1 (LGAR_F64 fast
                                modes only; ignored elsewhere): mixed precision -- column state, branches and mass bookkeeping
                                stay fp64, the two heads and the two end nodes of the trapezoid stay fp64, its 119 interior
                                nodes use the fp32 hardware transcendentals and are summed in fp64 */
  int32_t forward_lanes;     /* lgar_forward, LGAR_F64 fast modes with the trapezoid, native (geff_mode 0) or mixed precision
                                (geff_mode 1) alike (ignored elsewhere).  0: the library decides -- jobs under one wave per SIMD
                                get 4..64 cooperating lanes per column, which split the nodes of the Geff trapezoid and the
                                front sweep's independent evaluations between them (results bit for bit those of one lane per
                                column in the same geff_mode); 1: one lane per column whatever the job size; 4 .. 64: that
                                many (64 / lanes columns per wavefront) */
  int32_t reserved4;
} LgarDims;

/* Per-column soil parameters, each [n_layers][n_columns].  Replaces dpLGAR.alpha/.n/.ksat
 * (models/dpLGAR.py:50-57), theta_e/theta_r from the soil table (data/utils.py:66-67) and
 * cfg.data.layer_thickness.  ksat is the value BEFORE frozen_factor is applied. */
typedef struct {
  const void *alpha, *n, *ksat, *theta_e, *theta_r, *thickness;
} LgarParams;

/* Per-column model state (caller-owned, updated in place).  Replaces the Layer/WettingFront object
 * graph (layers/Layer.py:62-90, layers/WettingFront.py:38-49) and the model attributes
 * ponded_water / previous_precip / ending_volume / giuh_runoff_queue (models/dpLGAR.py:128-147). */
typedef struct {
  void *depth, *theta, *psi, *k, *dzdt; /* each [front_slots][n_columns], fronts ordered top -> bottom; rows at and
                                           beyond n_fronts[column] are not meaningful */
  uint8_t *flags;                        /* [front_slots][n_columns] */
  int32_t *n_fronts;                     /* [n_columns] */
  void *scalars;                         /* [LGAR_NSCAL][n_columns] */
  void *totals;                          /* [LGAR_NACC][n_columns]: run totals, what MassBalance accumulates
                                            (physics/MassBalance.py:31-44); rows 8,9 hold the latest value */
  uint32_t *tickets;                     /* NULL or device uint32[LGAR_NTICKETS]: work counters of the persistent-wave
                                            schedule (the library zeroes them on the stream at every call).  With tickets the
                                            forward kernels run as ONE resident wave per wave slot of the chip, each pulling
                                            64-column blocks until none is left (no partially filled last round); without,
                                            one workgroup per block. */
} LgarState;

/* Forcing, each [n_steps][forcing_columns], cm/h (data/Data.py:32-37).
 *
 * column_map: NULL (the layouts of LgarDims.forcing_columns / forcing_group above, bit for bit), or a per-column forcing
 * index in device memory -- B catchments of unequal size, each with its own series, without a gathered [n_steps][n_columns]
 * copy.  With column_map != NULL:
 *  - G = forcing_group (>= 1, n_columns % G == 0 as ever); the map is int32[M], M = n_columns / G.
 *  - Nf = LgarDims.forcing_columns is the number of forcing columns: it must be >= 1 (else LGAR_E_ARG) and needs NO
 *    divisibility relation to n_columns; precip / pet are [n_steps][Nf].
 *  - soil column c reads forcing column m(c) = min(max(column_map[c / G], 0), Nf - 1) at every step.  The clamp is memory
 *    safety before meaning, as in lgar_catchment_sums: the library never reads device memory on the host, so a corrupt map
 *    cannot index out of bounds (what such a column computes is not meaningful).  The index is read ONCE per column, before
 *    the time loop.
 *  - lgar_forward_tangent reads precip / pet the same way; its weights w_runoff / w_perc are then [n_steps][M] and column c
 *    reads weight column c / G.  (Weights cannot go through the map: the gradient of a catchment sum with respect to a member
 *    column carries that column's own area weight, so it is [n_steps][n_columns] by nature -- lgar_catchment_spread produces
 *    exactly that.  Without a map the weights keep the forcing's [n_steps][Nf] layout.)  tangent_share = W: the caller's
 *    guarantee is unchanged; with a map it holds whenever G % W == 0, since all columns of a group index one map entry.
 *  - the result for column c is, bit for bit, that of an unmapped call with precip'[t][c] = precip[t][m(c)], pet' likewise,
 *    in every kernel family (fp32, fp64, mixed, cooperating lanes, literal, every capacity of the chain, the tangent). */
typedef struct {
  const void *precip, *pet;
  const int32_t *column_map;
} LgarForcing;

/* Optional per-step outputs.
 * series[j]: [n_steps][n_columns] or NULL: the model accumulators as they stand after forward() and before
 *   MassBalance.change_mass zeroes them (order = LGAR_NACC list).  series[4] (runoff) and series[5] (percolation)
 *   are forward()'s return pair (models/dpLGAR.py:299).
 * basin: [LGAR_NACC][n_steps] fp64 or NULL; for every bit j set in basin_mask,
 *   basin[j][t] += sum over this launch's columns of weight[c] * accumulator_j[t][c]
 *   (the caller zeroes it; what MassBalance.report_mass / the agent's y_hat aggregate over a basin).  Where series[j]
 *   is given as well, the sum is taken from the stored series by a second kernel on the same stream (one pass, fixed
 *   summation order: the same bits on every run; ~1 % of the launch).  Without series[j] it is reduced inside the forward
 *   kernels (wave reduction + one fp64 atomic per wave and step: no [n_steps][n_columns] array is needed, summation order
 *   across waves is not fixed, ~10 % of an fp32 launch on 1M columns).  Calls that add into the same basin block must
 *   be on one stream.
 * weights: [n_columns] (dtype) or NULL = 1: e.g. area fractions.
 * counters[0] += number of wave-level Geff evaluations (calc_geff, lgar/green_ampt.py:19-99) of the launch: what
 *   bench.py prices against the chip's measured transcendental issue rate. */
typedef struct {
  void *series[LGAR_NACC];
  double *basin;
  const void *weights;
  uint32_t basin_mask;
  uint32_t reserved;
  uint64_t *counters; /* NULL or device uint64[LGAR_NCOUNTERS], accumulated (caller zeroes): measurement only */
  void *call_sums;    /* NULL or [LGAR_NACC][n_columns] (dtype): rows 0..7 = the accumulators summed over THIS call's
                         steps (what the model attributes gain over a block of forward() calls, models/dpLGAR.py:271-298),
                         rows 8, 9 = latest ponded_water / ending_volume */
} LgarStepOut;

const char *lgar_version(void);
/* ABI revision of this header: bumped whenever a struct of this file changes size or layout or an entry point changes its
 * argument list (3: LgarDims.geff_mode / forward_lanes, lgar_forward_tangent's `tickets`; 4: LgarForcing.column_map -- a caller
 * built against 3 would pass a two-pointer LgarForcing and the library would read past it).  A caller compares it with the
 * LGAR_ABI_VERSION it was compiled against, and lgar_sizeof_dims() with its own sizeof(LgarDims), before the first call. */
#define LGAR_ABI_VERSION 4
int32_t lgar_abi_version(void);
int32_t lgar_sizeof_dims(void);
int32_t lgar_fmax(void);
int32_t lgar_lmax(void);
/* Lanes per column lgar_forward would use for these dims and dtype (LgarDims.forward_lanes = 0: the library's choice for jobs
 * under one wave per SIMD; 1 = every column its own lane).  A pure function of its arguments and of the device's CU count
 * (256 when no device is visible). */
int32_t lgar_cooperating_lanes(const LgarDims *dims, int32_t dtype);

/* dpLGAR.set_internal_states() (models/dpLGAR.py:97-147): one to_bottom front per layer at
 * psi = initial_psi, theta = theta(initial_psi); zero scalars/totals; status = 0. */
int32_t lgar_state_init(const LgarDims *dims, const LgarParams *params, LgarState *state, int32_t *status,
                        int32_t dtype, void *stream);

/* n_steps x dpLGAR.forward(x) (models/dpLGAR.py:154-299) for every column, each followed by the
 * MassBalance.change_mass drain (physics/MassBalance.py:31-53), i.e. the agent's inner loop
 * (agents/DifferentiableLGAR.py:117-125).  `out` may be NULL. */
int32_t lgar_forward(const LgarDims *dims, const LgarParams *params, LgarState *state, const LgarForcing *forcing,
                     const LgarStepOut *out, int32_t *status, int32_t dtype, void *stream);

/* Forward-mode tangent of lgar_forward (the differentiable path; replaces torch autograd through
 * forward(), agents/DifferentiableLGAR.py:119,163).  For a parameter direction (d_alpha, d_n, d_ksat,
 * each [n_layers][n_columns], NULL = 0) it integrates value and tangent together from a FRESH state
 * (set_internal_states) over n_steps and accumulates, per column,
 *     grad_out[column] = sum_t  w_runoff[t][column] * d runoff_t + w_perc[t][column] * d percolation_t
 * (w_* may be NULL).  Line-search offsets are constants w.r.t. the parameters, as in the reference
 * (Layer.py:277-288,683-696).  tangent_runoff ([n_steps][n_columns]) may be NULL.
 * tickets: NULL or device uint32[LGAR_NTICKETS] (zeroed by the library on the stream): with it the kernels run as one
 * resident wave per wave slot of the chip, each pulling blocks of columns until none is left. */
int32_t lgar_forward_tangent(const LgarDims *dims, const LgarParams *params, const LgarParams *direction,
                             const LgarForcing *forcing, const void *w_runoff, const void *w_perc,
                             void *grad_out, void *tangent_runoff, int32_t *status, int32_t dtype, void *stream,
                             uint32_t *tickets);

/* The resumable tangent: lgar_forward_tangent over a WINDOW of rows that may start from a carried state and hand its end
 * state back.  A state is a value state plus its tangent parts (the derivative of every stored value along `direction`).
 *  - Carry: a run cut into chunks -- state_out / dstate_out / grad_out of one call given as state_in / dstate_in / grad_in of
 *    the next -- leaves the bits of one call over all rows (grad_out, tangent_runoff, both end states).
 *  - Stop-gradient: the value state of a spun-up run (what lgar_forward left) with dstate_in = NULL gives the exact derivative,
 *    with respect to the parameters, of "lgar_forward from this fixed state over these rows".  Nothing flows into the spin-up.
 *  - state_in = NULL is lgar_forward_tangent itself, bit for bit.  A fresh start is NOT a zero tangent state: the fresh state
 *    depends on the parameters (theta(initial_psi; alpha, n), the deepest front's K).
 * Forcing layouts, column_map, forcing_group, tangent_share, tickets, dtype and layer counts are lgar_forward_tangent's.  With
 * tangent_share = W the caller guarantees in addition that the W columns of a group hold the same VALUE state.
 * grad_out[c] is grad_in[c] followed by this call's terms in row order (grad_out may be grad_in).  status is written, not read:
 * a column whose state_in has fewer fronts than layers gets LGAR_ST_STRUCT; n_fronts is clamped on load as in lgar_forward.
 * state_in / dstate_in are never written: a column handed over in the front-capacity chain is redone from them (a state that
 * arrives with more fronts than the first kernel holds is handed over before its first row), and only the kernel that finishes
 * a column writes its grad_out and end state.  state_out is written as lgar_forward's store writes it -- rows [0, n_fronts) of
 * the per-front arrays, n_fronts, scalars; totals and tickets are not touched -- so lgar_forward and lgar_soil_moisture accept
 * it.  n_steps = 0 copies state, tangent state and grad through.
 * LGAR_E_ARG: everything lgar_forward_tangent refuses; a null window; dstate_in without state_in; exactly one of state_out /
 * dstate_out; a given state with a null array among those read or written; an output state that shares an array with an input
 * state or with the other output state (the pointers are compared). */
typedef struct {
  const LgarState *state_in;    /* NULL: fresh state (set_internal_states), exactly lgar_forward_tangent's start */
  const LgarState *dstate_in;   /* tangent parts of state_in; NULL: zeros.  Read: depth, theta, psi, k, dzdt
                                   [front_slots][n_columns], scalars [LGAR_NSCAL][n_columns].  flags, n_fronts, totals,
                                   tickets are ignored.  Must be NULL when state_in is NULL. */
  LgarState *state_out;         /* NULL: not wanted.  Value state after the last row: a state lgar_forward accepts. */
  LgarState *dstate_out;        /* its tangent parts; given iff state_out is given */
  const void *grad_in;          /* [n_columns] (dtype) or NULL = zeros: the fold of grad continues from it */
} LgarTangentWindow;

int32_t lgar_forward_tangent_window(const LgarDims *dims, const LgarParams *params, const LgarParams *direction,
                                    const LgarForcing *forcing, const void *w_runoff, const void *w_perc,
                                    const LgarTangentWindow *window, void *grad_out, void *tangent_runoff, int32_t *status,
                                    int32_t dtype, void *stream, uint32_t *tickets);

/* The tangent along a direction of the FORCING as well: lgar_forward_tangent_window whose step t runs on (precip, precip') and
 * (pet, pet').  `dforcing` holds the two tangents: its precip / pet are arrays [n_steps][Nf][G] of dtype, G = forcing_group
 * (LgarDims) and Nf the number of forcing columns, either may be NULL = zeros; column c reads element
 * (t * Nf + cf) * G + c mod G, cf being the forcing column it reads its values from (by the layout or by
 * forcing->column_map).  So every lane of a direction group has a forcing tangent of its own (lanes that carry a parameter
 * direction read zeros), and with Nf = n_columns / G the read is t * n_columns + c.  A forcing direction changes no value:
 * the W columns of a tangent_share group still hold one value state.  With both tangents NULL or all zero every result has
 * the bits of lgar_forward_tangent_window.  Everything else -- window (a block of NULLs: fresh state), weights, tickets,
 * dtype, layer counts, the front-capacity chain -- is lgar_forward_tangent_window's.
 * LGAR_E_ARG: everything lgar_forward_tangent_window refuses; a null dforcing; a non-null dforcing->column_map. */
int32_t lgar_forward_tangent_forced(const LgarDims *dims, const LgarParams *params, const LgarParams *direction,
                                    const LgarForcing *forcing, const LgarForcing *dforcing, const void *w_runoff,
                                    const void *w_perc, const LgarTangentWindow *window, void *grad_out, void *tangent_runoff,
                                    int32_t *status, int32_t dtype, void *stream, uint32_t *tickets);

/* Soil-moisture output: the water the front table holds in depth bins (the product the reference reserves and never fills:
 * GlobalParams.soil_moisture_wetting_fronts, physics/GlobalParams.py:61; LGAR-C's soil_moisture_layers).  The theta profile
 * implied by a front table is piecewise constant: front j (depth d_j, water content theta_j, layer tag k_j) reaches up to
 * t_j = d_{j-1} when front j-1 carries the same layer tag, else to the top of layer k_j.  For bin i = [a, b]
 *     S_i = sum_j theta_j * (clip(d_j, a, b) - clip(t_j, a, b)),   clip(x, a, b) = min(max(x, a), b)
 * in front order, widths SIGNED (what Layer.mass_balance implies, layers/Layer.py:795-824: bins covering the column sum to
 * ending_volume also in the steps where the reference leaves depths transiently non-monotone).  All arithmetic is fp64 whatever
 * `dtype`, rounded once to it: a pure function of the stored state.
 * edges: device fp64[n_bins + 1], cm, strictly increasing (the CALLER guarantees it: the library never reads device memory on
 *   the host), 1 <= n_bins <= LGAR_MOIST_BINS; or NULL: the bins are each column's own soil layers and n_bins must equal
 *   n_layers.
 * what: 0 = mean volumetric water content S_i / w_i over the bin's in-column width w_i = clip(Z, a, b) - a (Z = the column's
 *   total thickness); NaN where w_i <= 0 (bin wholly below the column).  1 = storage S_i in cm (0 below the column).
 * out: [n_bins][n_columns] (dtype).
 * basin: NULL, or device fp64[n_bins]: basin[i] += sum_c weights[c] * out[i][c] (weights: [n_columns] (dtype) or NULL = 1), by
 *   the fixed-order pass LgarStepOut.basin uses for a stored series: the same bits on every run; the caller zeroes it.
 * Only state->depth, theta, flags, n_fronts and params->thickness are read; nothing of the state is written.  n_fronts is
 * clamped to the state's front_slots and layer tags to n_layers - 1, so the leftover state of a faulted column cannot index
 * out of bounds (its output is not meaningful). */
#define LGAR_MOIST_BINS 32
int32_t lgar_soil_moisture(const LgarDims *dims, const LgarParams *params, const LgarState *state, const double *edges,
                           int32_t n_bins, int32_t what, void *out, const void *weights, double *basin, int32_t dtype,
                           void *stream);

/* The tangent of the soil-moisture output: the derivative of lgar_soil_moisture's bins along the direction a tangent state was
 * integrated for (state_out / dstate_out of lgar_forward_tangent_window, passed as they are: `state` is the value state, `dstate`
 * its tangent parts; dims->n_columns = M is the number of lanes of that state).  With lgar_soil_moisture's notation and the
 * tangents d'_j, theta'_j, t'_j = d'_{j-1} (same layer tag) or +0.0 (a layer's top: thickness is not differentiated), bin
 * i = [a, b] has
 *     in(x) = x >= a && x < b
 *     S'_i  = sum_j  theta'_j * (clip(d_j, a, b) - clip(t_j, a, b))  +  (in(d_j) ? theta_j * d'_j : 0.0)  -  (in(t_j) ? theta_j * t'_j : 0.0)
 * in front order, per front acc = ((acc + first) + second) - third; fp64 whatever `dtype`; every decision is a select.
 * The tie rule: clip's two one-sided derivatives differ where a depth sits exactly on an edge.  `in` is half-open, so such a depth
 * lies in exactly one of two adjacent bins (the lower one, whose a it equals), and the bins that cover a column sum to the tangent
 * of the stored volume, sum_j theta'_j (d_j - t_j) + theta_j (d'_j - t'_j), also with a front on an edge; counting it in both
 * bins or in neither would break that closure.
 * what: 1 = storage: m'_i = S'_i.  0 = m'_i = w_i > 0 ? S'_i / w_i : +0.0, w_i being lgar_soil_moisture's in-column width, a
 *   constant: below the column the value is NaN, its tangent is zero.
 * Outputs, either or both:
 *   out: [n_bins][M] (dtype), m'_i rounded once; or NULL.
 *   cot, grad (both or neither): the contraction into the gradient a run of tangent windows carries.  cot: fp64 [n_bins][M / group];
 *     lane c reads column c / group (the forcing_group convention of the tangent launches).  acc = +0.0; for i ascending:
 *     acc = acc + (live_i ? cot_i * m'_i : 0.0) with the unrounded fp64 m'_i, live_i = w_i > 0 for what = 0 and true for what = 1 (a
 *     select: a NaN cotangent under a dead bin is discarded); then grad[c] = (dtype)((double)grad[c] + acc), in place: grad is
 *     [M] (dtype).
 * edges, n_bins: as in lgar_soil_moisture (NULL: each lane's own layers).  n_fronts is clamped to the state's front_slots and layer
 * tags to n_layers - 1 exactly as there; only state->depth, theta, flags, n_fronts, dstate->depth, theta and params->thickness
 * are read; nothing of either state is written.
 * LGAR_E_ARG: what lgar_soil_moisture refuses (but M = 0, which returns 0 without a launch); a null dstate, dstate->depth or
 * dstate->theta; neither out nor (cot and grad); exactly one of cot / grad; group < 1 or M not a multiple of group. */
int32_t lgar_soil_moisture_tangent(const LgarDims *dims, const LgarParams *params, const LgarState *state, const LgarState *dstate,
                                   const double *edges, int32_t n_bins, int32_t what, void *out, const double *cot, int32_t group,
                                   void *grad, int32_t dtype, void *stream);

/* Catchment sums: per-row sums of a stored series over MANY catchments, out[t][b] for B catchments at once (LgarStepOut.basin
 * is the one-catchment case; what a NextGen-style job compares with observations is the [T][B] matrix of catchment runoff).
 *
 * Catchment map (CSR).  offsets: int32[n_catchments + 1], non-decreasing, offsets[0] = 0.  order: int32[n_order] column
 * indices, n_order = offsets[n_catchments], or NULL: the members of catchment b are then the contiguous columns
 * offsets[b] .. offsets[b + 1] - 1.  A column belongs to at most one catchment and may belong to none.
 *
 * For row t and catchment b with n members c_0 .. c_{n-1} in map order:
 *   - the term is x_i = (double)w[c_i] * (double)series[t][c_i]; w = 1 when weights == NULL (the product is exact for fp32);
 *   - member i is SKIPPED ENTIRELY (no term, not 0 * NaN) when status != NULL and status[c_i] & LGAR_ST_FAULT_MASK is
 *     non-zero, and also when c_i is outside [0, n_columns);
 *   - there are 256 partials s_p, p = i mod 256, each accumulated from +0.0 in increasing i with plain fp64 adds (the library
 *     is built with -ffp-contract=off);
 *   - q_l = (s_l + s_{l+64}) + (s_{l+128} + s_{l+192}) for l = 0 .. 63;
 *   - then for off = 32, 16, 8, 4, 2, 1: q_l <- q_l + q_{l xor off} (every l at once);
 *   - out[t][b] = q_0; an empty catchment gives +0.0.
 * out[t][b] is WRITTEN, not added: exactly one wavefront owns it (lane l holds the partials l, l + 64, l + 128, l + 192), there
 * are no atomics and the caller zeroes nothing.  The result for catchment b is therefore a pure function of its own members'
 * values, weights and order: it does not depend on n_catchments, on the other catchments, on where the members sit in the
 * launch, or on the run.
 *
 * series: [n_rows][n_columns] (dtype), e.g. a stored LgarStepOut.series[j] or lgar_soil_moisture's [n_bins][n_columns].
 * weights: [n_columns] (dtype) or NULL.  status: int32[n_columns] or NULL.  out: fp64 [n_rows][n_catchments].
 * weight_sums: NULL, or fp64[n_catchments]: the same sum, in the same order and with the same skipping, over the terms
 *   (double)w[c_i] -- what turns a sum into a mean over the columns that are still valid.
 * Memory safety before meaning: offsets[b] and offsets[b + 1] are clamped into [0, len] (len = n_order, or n_columns without
 * `order`) before use and a catchment whose clamped end is not beyond its start is empty, so a corrupt map cannot index out of
 * bounds (its sums are not meaningful).  n_rows = 0 with weight_sums computes the weight sums alone. */
int32_t lgar_catchment_sums(const void *series, int32_t n_rows, int32_t n_columns, const int32_t *offsets, int32_t n_catchments,
                            const int32_t *order, int32_t n_order, const void *weights, const int32_t *status, double *out,
                            double *weight_sums, int32_t dtype, void *stream);

/* Spread, the adjoint of the catchment sums: from a [n_rows][n_catchments] fp64 gradient of the sums to the [n_rows][n_columns]
 * tangent weights lgar_forward_tangent takes (w_runoff / w_perc):
 *     out[t][c] = round_to_dtype(grad[t][catchment_of[c]] * (double)w[c])
 * and 0 where catchment_of[c] is outside [0, n_catchments) (-1: the column belongs to no catchment) or status[c] has a bit of
 * LGAR_ST_FAULT_MASK.  catchment_of: int32[n_columns]; weights ([n_columns], dtype) and status may be NULL. */
int32_t lgar_catchment_spread(const double *grad, int32_t n_rows, int32_t n_catchments, const int32_t *catchment_of,
                              int32_t n_columns, const void *weights, const int32_t *status, void *out, int32_t dtype,
                              void *stream);

/* Catchment routing: one unit hydrograph per catchment over a [n_rows][n_catchments] matrix of catchment sums (what a catchment
 * job compares with observations is routed runoff at the outlet).  Routing is linear, so it commutes with the catchment sum
 * and is applied after lgar_catchment_sums; the in-kernel GIUH of the forward kernels (LgarDims.giuh, one hydrograph shared by
 * every column, at most LGAR_GMAX ordinates; the reference's lgar/giuh.py:8-20) is not touched.
 *
 * All arrays are fp64, catchment fastest: x[T][B] the input, ordinates g[K][B] (per_catchment != 0) or g[K] (shared by all
 * catchments), 1 <= K <= LGAR_ROUTE_KMAX, queue_in / queue_out [K][B]: the carried queue, with the layout and meaning of the
 * reference's giuh_runoff_queue (queue_in == NULL: zeros; queue_out == NULL: not wanted).  For every catchment b independently,
 * for t = 0 .. T - 1:
 *     q[i] <- q[i] + g[i][b] * x[t][b]    i = 0 .. K - 1   (one rounded product, one rounded add: -ffp-contract=off)
 *     y[t][b] = q[0]
 *     q[i] <- q[i + 1] for i < K - 1;  q[K - 1] <- +0.0
 * and queue_out is q after row T - 1.  The kernels evaluate the equivalent statement without a dependence between rows (the
 * same bits: every y is the same chain of adds, oldest term first):
 *     y[t][b] starts from queue_in[t][b] if t < K, else from +0.0, and adds g[k][b] * x[t - k][b] for k = min(t, K - 1) down to 0;
 *     queue_out[i][b] is the same fold for the virtual row T + i over k = K - 1 .. i + 1 with T + i - k >= 0, starting from
 *     queue_in[T + i][b] when T + i < K.
 * There is NO skip test: the reference's `sum(queue) > 0 or runoff > 0` changes no value for non-negative input, and without
 * it the operator is plainly linear, which the adjoint needs.  T = 0 gives queue_out = queue_in; B = 0 is a no-op.  y and
 * queue_out are WRITTEN, not added to, and the caller zeroes nothing; the result for catchment b depends only on column b of
 * the inputs -- not on B, on the launch shape or on the run.
 * RESOLUTION: the operator works at the row resolution of the stored series.  With num_subcycles > 1 the in-kernel GIUH
 * shifts once per SUB-step, so this is then a different operator from the in-kernel one.
 *
 * reverse != 0: the same fold under t -> T - 1 - t on input and output, with a zero queue (queue_in and queue_out must be NULL):
 *     y[t][b] = the fold of g[k][b] * x[t + k][b] from k = min(K - 1, T - 1 - t) down to 0, starting at +0.0
 * which is the adjoint of the routing with respect to x (x holds the gradient of y, y receives the gradient of x).
 * K outside 1 .. LGAR_ROUTE_KMAX, negative sizes, or a null x (with T, B > 0), y (T, B > 0) or ordinates return LGAR_E_ARG. */
#define LGAR_ROUTE_KMAX 64
int32_t lgar_catchment_route(const double *x, int32_t n_rows, int32_t n_catchments, const double *ordinates,
                             int32_t n_ordinates, int32_t per_catchment, const double *queue_in, double *queue_out, double *y,
                             int32_t reverse, void *stream);

/* Gradient of the routing with respect to the ordinates, per catchment:
 *     g_out[k][b] = sum over t = k .. T - 1 of gy[t][b] * x[t - k][b]
 * from +0.0, in increasing t, with plain fp64 products and adds.  Rows before the call (the carried queue) are constants.
 * g_out: [n_ordinates][n_catchments], written; for shared ordinates the caller sums it over b. */
int32_t lgar_catchment_route_grad(const double *x, const double *gy, int32_t n_rows, int32_t n_catchments,
                                  int32_t n_ordinates, double *g_out, void *stream);

/* Catchment scores: per-catchment moments of a simulation against observations with gaps, and their adjoint (what a catchment
 * job compares with observations: every metric -- MSE, NSE, KGE, bias, correlation -- is a few operations on these [B] vectors).
 *
 * All arrays are fp64, catchment fastest: sim[T][B] the model rows (the output of the routing above, say), obs[To][B] the
 * observations, window = r >= 1 and T == To * r (r model rows under one observation row: 5-minute steps, hourly gauges).
 * A pair (j, b) is VALID iff obs[j][b] is finite: NaN, +inf and -inf all mark a gap.  Nothing about sim decides validity; a
 * NaN in sim on a valid row poisons that catchment's moments, as it should.  The aggregated simulation is
 *     s[j][b] = (((0.0 + sim[j r][b]) + sim[j r + 1][b]) + ... + sim[j r + r - 1][b]) / (double)r
 * THE GATED FOLD of a term x[j][b] over j: the rows are cut into blocks of LGAR_SCORE_BLOCK = 64 observation rows, block k =
 * rows 64 k .. min(64 k + 63, To - 1); a block partial starts at +0.0 and adds the terms of its valid rows in increasing j
 * (an invalid row adds NOTHING: not 0 * NaN, no term at all); the result starts at +0.0 and adds the block partials in
 * increasing k.  Plain fp64 adds and products (-ffp-contract=off).  The block size is a constant of the definition, not of the
 * launch, so the result for catchment b is a pure function of column b of the inputs -- not of B, the launch shape or the run.
 *
 * moments[LGAR_SCORE_NMOM = 7][B], WRITTEN, not added to:
 *     row 0  n   = the number of valid rows (exact, as a double)
 *     row 1  mo  = fold(o) / n
 *     row 2  ms  = fold(s) / n                      (IEEE divides: n = 0 gives NaN for both means)
 *     row 3  soo = fold((o - mo) * (o - mo))
 *     row 4  sss = fold((s - ms) * (s - ms))
 *     row 5  sos = fold((o - mo) * (s - ms))
 *     row 6  see = fold((s - o) * (s - o))
 * With no valid row, rows 3 .. 6 are +0.0.  To = 0 gives n = 0; B = 0 is a no-op.
 *
 * workspace: device scratch of lgar_catchment_moments_workspace(To, B) bytes, owned by the caller (the library allocates
 * nothing): it holds the block partials between the launches of a call and nothing between calls.  That function returns
 * LGAR_E_ARG for a negative size.
 * Negative sizes, window < 1, To * window beyond int32, a null pointer the sizes say will be read or written, or a null
 * workspace where the workspace function returns more than 0, return LGAR_E_ARG. */
#define LGAR_SCORE_BLOCK 64
#define LGAR_SCORE_NMOM 7
int64_t lgar_catchment_moments_workspace(int32_t n_obs_rows, int32_t n_catchments);
int32_t lgar_catchment_moments(const double *sim, const double *obs, int32_t n_obs_rows, int32_t n_catchments, int32_t window,
                               double *moments, void *workspace, void *stream);

/* The adjoint of the moments.  Every differentiable function F of them has, on the valid rows,
 *     dF / ds[j][b] = c0 / n + 2 c1 (s - ms) + c2 (o - mo) + 2 c3 (s - o),      c = dF / d(ms, sss, sos, see)
 * and 0 elsewhere (n, mo and soo do not depend on sim; the terms through the means cancel: the centred sums are stationary in
 * them).  coef[4][B] holds c, moments the result of lgar_catchment_moments on the same sim and obs.  s is recomputed and
 *     g = ((c0[b] / n[b] + (2.0 * c1[b]) * (s - ms)) + c2[b] * (o - mo)) + (2.0 * c3[b]) * (s - o)
 * evaluated in exactly that order; grad_sim[j r + i][b] = g / (double)r for i < r, and +0.0 on every row of an invalid j.
 * Elementwise: no reduction, nothing to zero; grad_sim[T][B] is written. */
int32_t lgar_catchment_moments_grad(const double *sim, const double *obs, int32_t n_obs_rows, int32_t n_catchments,
                                    int32_t window, const double *moments, const double *coef, double *grad_sim, void *stream);

/* Catchment network: linear Muskingum channel routing BETWEEN catchments.  A gauge at an outlet sees the catchment's own routed
 * runoff plus everything that arrives from the catchments upstream, delayed and attenuated by the channels; this is the stage
 * between lgar_catchment_route and lgar_catchment_moments.  One reach is the channel of one catchment.
 *
 * All floating-point arrays are fp64, catchment fastest: the lateral inflow x[T][B], the discharge y[T][B], the coefficients
 * coef[3][B] = c0, c1, c2 of every reach.  x and y do not overlap.
 * TOPOLOGY, int32.  On the device:
 *     down[B]                 the catchment b drains into, -1 for an outlet.  A forest: at most one downstream each, no cycles.
 *     up_ptr[B + 1], up_idx[E] CSR lists of the direct upstream catchments of every b, IN ASCENDING INDEX within a list;
 *                             E = n_edges = B minus the number of outlets.
 *     order[B]                the catchments sorted by (level, index); level(b) = 0 without upstream, else 1 + max level(u).
 * In HOST memory:
 *     level_ptr[n_levels + 1] delimits the levels inside order.  The library never reads DEVICE memory on the host; level_ptr
 *                             is host memory and the library reads it, on the host, to launch one kernel per level.
 *
 * FORWARD.  For every reach b, with Iprev, Oprev = state_in[0][b], state_in[1][b] (state_in == NULL: +0.0), for t = 0 .. T - 1:
 *     I = x[t][b];  for e = up_ptr[b] .. up_ptr[b + 1] - 1:  I = I + y[t][up_idx[e]]      (ascending e, one rounded add each)
 *     O = (c0[b] * I + c1[b] * Iprev) + c2[b] * Oprev                                    (exactly this association; -ffp-contract=off)
 *     y[t][b] = O;  Iprev = I;  Oprev = O
 * state_out[0][b], state_out[1][b] = Iprev, Oprev after row T - 1 (state_out == NULL: not wanted).  y and state_out are
 * WRITTEN, not added to; the caller zeroes nothing.  T = 0 copies the state (zeros when state_in is NULL); B = 0 is a no-op.
 * The result for b is a pure function of the columns of x and coef in its upstream closure -- not of B, of the other
 * catchments, of the launch or of the run.  coef = (1, 0, 0) is plain upstream accumulation, (0, 1, 0) a one-row lag per reach.
 * Muskingum with storage constant K and weight X: c0 = (dt/2 - K X) / D, c1 = (dt/2 + K X) / D, c2 = (K - K X - dt/2) / D,
 * D = K - K X + dt/2; the kernels take coefficients and do not restrict their sign.
 *
 * The levels run in ascending order, one launch each on `stream`; stream order is the only dependence between them.
 * Every index the kernels read from device memory is clamped into its array (order, up_idx, down to [0, B - 1]; up_ptr to
 * [0, n_edges]): a corrupt topology gives wrong numbers, never an access out of bounds.  Offsets are 64-bit.
 * Negative sizes, n_levels < 0, a level_ptr that does not start at 0, end at B and never decrease, or a null pointer the sizes
 * say will be read or written, return LGAR_E_ARG. */
int32_t lgar_network_route(const double *x, int32_t n_rows, int32_t n_catchments, const double *coef, const int32_t *up_ptr,
                           const int32_t *up_idx, int32_t n_edges, const int32_t *order, const int32_t *level_ptr, int32_t n_levels,
                           const double *state_in, double *state_out, double *y, void *stream);

/* The adjoint of the network routing with respect to x and, when gc != NULL, the gradient with respect to coef.  The levels run
 * in DESCENDING order, so gx[.][down[b]] is complete before b runs.  For each reach lam_next = +0.0 and, with gc wanted, three
 * accumulators gc0, gc1, gc2 = +0.0; for t = T - 1 .. 0:
 *     a = gy[t][b];  if down[b] >= 0:  a = a + gx[t][down[b]]
 *     lam = a + c2[b] * lam_next
 *     gx[t][b] = c0[b] * lam + c1[b] * lam_next
 *     gc0 = gc0 + lam * I[t];   gc1 = gc1 + lam * I[t - 1];   gc2 = gc2 + lam * y[t - 1][b]          (only when gc is wanted)
 *     lam_next = lam
 * I[t] is re-formed from x and the stored y (the result of lgar_network_route on the same x, coef, state_in) by the forward's own
 * fold, so it has the same bits; I[-1], y[-1] come from state_in, or are zeros.  The carried state is a constant: nothing flows
 * back into it.  gx[T][B] and gc[3][B] are WRITTEN.  gy and gx do not overlap.  gc == NULL: x, y, up_ptr, up_idx, state_in are
 * not read.  The refusals of lgar_network_route, and gc wanted without x, y, up_ptr, up_idx, return LGAR_E_ARG. */
int32_t lgar_network_route_grad(const double *gy, int32_t n_rows, int32_t n_catchments, const double *coef, const int32_t *down,
                                const int32_t *order, const int32_t *level_ptr, int32_t n_levels, double *gx, const double *x,
                                const double *y, const int32_t *up_ptr, const int32_t *up_idx, int32_t n_edges,
                                const double *state_in, double *gc, void *stream);

/* Catchment network with flow-dependent reaches (Muskingum-Cunge): the storage constant of a reach is a power law of the reach's
 * own previous discharge, K = kref (Oprev / qref)^(-beta), so a flood wave travels faster than low flow.  Everything is fp64,
 * catchment fastest.  The topology, order, the HOST level_ptr, state_in / state_out [2][B] = Iprev, Oprev and the inflow fold are
 * exactly lgar_network_route's.  par[4][B] = kref, beta, X, qref: kref the reach's travel time in hours at discharge qref, beta the
 * celerity exponent, X the Muskingum weight, qref in the unit of x.  Scalars dt_h (the row step in hours), rmin, rmax (the range
 * Oprev / qref is held to); half = 0.5 * dt_h, formed once.
 *
 * FORWARD.  For every reach b, with Iprev, Oprev = state_in[0][b], state_in[1][b] (NULL: +0.0), for t = 0 .. T - 1:
 *     I   = x[t][b];  for e = up_ptr[b] .. up_ptr[b + 1] - 1:  I = I + y[t][up_idx[e]]      (the linear walk's own fold)
 *     rho = Oprev / qref
 *     rc  = rho < rmin ? rmin : (rho > rmax ? rmax : rho)       (selects: a NaN stays a NaN; rho == rmin / rmax is not "clamped")
 *     L   = mc_ln(rc)
 *     tau = beta * L                                            (K = kref * rc^(-beta))
 *     ta  = tau < 0 ? -tau : tau;   tc = ta > LGAR_GW_ZMAX ? LGAR_GW_ZMAX : ta
 *     e   = gw_exp(tc)                                          (lgar_catchment_baseflow's, as it is)
 *     K   = tau > 0 ? kref / e : kref * e
 *     KX  = K * X;   u = K - KX;   D = u + half
 *     c0  = (half - KX) / D;   c1 = (half + KX) / D;   c2 = (u - half) / D
 *     O   = (c0 * I + c1 * Iprev) + c2 * Oprev
 *     y[t][b] = O;   Iprev = I;   Oprev = O
 * in exactly this association, without contraction (-ffp-contract=off), with IEEE divisions.  state_out = Iprev, Oprev after the
 * last row; y and state_out are WRITTEN, not added to; T = 0 copies the state (zeros when state_in is NULL); B = 0 is a no-op.  A
 * negative or zero Oprev is simply rho < rmin.  Parameter VALUES are not policed on the device, and the coefficients may come
 * out negative (they are non-negative iff 2 K X <= dt_h <= 2 K (1 - X)).  beta = 0 gives tau = 0, e = 1, K = kref exactly: the
 * linear route with the Muskingum coefficients of (kref, X, dt_h), bit for bit.  Variable-K Muskingum does not conserve volume
 * exactly in transients; a steady flow is kept (c0 + c1 + c2 = 1 up to rounding).
 *
 * mc_ln(x), x a positive normal double, uses no libm, no fma and no hardware reciprocal -- numpy restates it one operation for one:
 *     (m, k) = frexp(x)                     by integer operations on the bits, m in [0.5, 1)
 *     m < 0x1.6a09e667f3bcdp-1 ?            (fl(sqrt 1/2))   m = m + m, k = k - 1
 *     s = (m - 1.0) / (m + 1.0);  z = s * s
 *     p = sum_{j <= 10} z^j / (2 j + 1)     Horner from j = 10 down: p = p * z + c_j, one rounded multiply and one rounded add per
 *                                           step, c_j the correctly rounded 1 / (2 j + 1)
 *     L = k * LN2_HI + ((2.0 * s) * p + k * LN2_LO)          LN2_HI, LN2_LO: gw_exp's, so k * LN2_HI is exact
 * Its relative error is below gamma_9 + 7e-19 = 1.0e-15 (derived in csrc/lgar_network_mc.hpp).
 *
 * Everything lgar_network_route refuses is refused here, and so are a dt_h that is not finite or <= 0, rmin or rmax that are not
 * finite, rmin < 2^-60, rmax > 2^60, rmin > rmax and (B > 0) a null par: LGAR_E_ARG.  Indices read from device memory are clamped
 * as in lgar_network_route; one launch per non-empty level on `stream`; offsets are 64-bit. */
int32_t lgar_network_route_mc(const double *x, int32_t n_rows, int32_t n_catchments, const double *par, double dt_h, double rmin,
                              double rmax, const int32_t *up_ptr, const int32_t *up_idx, int32_t n_edges, const int32_t *order,
                              const int32_t *level_ptr, int32_t n_levels, const double *state_in, double *state_out, double *y,
                              void *stream);

/* The adjoint of the Muskingum-Cunge routing: from gy[T][B] the gradients with respect to x (gx[T][B]), to kref, beta and X
 * (gpar[3][B] = gkref, gbeta, gX; NULL: not wanted; qref is a constant) and to the initial state (gstate[2][B]; NULL: not wanted).
 * y is what lgar_network_route_mc stored for the same x, par, dt_h, rmin, rmax, state_in.  The levels run in DESCENDING order.
 * I[t] is re-formed by the forward's fold; L, K, D, c0, c1, c2 and the regime of row t come from the forward's own row function
 * with Oprev = y[t - 1][b] (row 0: state_in[1][b], or +0.0): the same bits.  inside = neither select of rc fired and not
 * ta > LGAR_GW_ZMAX; big = ta > LGAR_GW_ZMAX.  Per reach, with omx = 1.0 - X (once), pI = pO = +0.0 and three accumulators from
 * +0.0, for t = T - 1 .. 0, with Ip = I[t - 1], Op = y[t - 1][b] (row 0: state_in, or +0.0):
 *     a     = gy[t][b];  if down[b] >= 0:  a = a + gx[t][down[b]]
 *     lam   = a + pO
 *     gx[t][b] = c0 * lam + pI
 *     dK    = ((I * (-(X + c0 * omx)) + Ip * (X - c1 * omx)) + Op * (omx * (1.0 - c2))) / D;     GK = lam * dK
 *     dX    = ((I * (-(1.0 - c0)) + Ip * (1.0 + c1)) + Op * (-(1.0 - c2))) * (K / D)
 *     gkref = gkref + GK * (K / kref)
 *     gbeta = big ? gbeta : gbeta + GK * (-(K * L))
 *     gX    = gX + lam * dX
 *     pI    = c1 * lam
 *     pO    = inside ? c2 * lam + GK * ((-(beta * K)) / Op) : c2 * lam
 * and gstate[0][b], gstate[1][b] = pI, pO after row 0.  In real arithmetic this is lam_t = a_t + c2_{t+1} lam_{t+1} +
 * GK_{t+1} dK_{t+1}/dO_t and gx[t] = c0_t lam_t + c1_{t+1} lam_{t+1}, with dK/dOprev = -beta K / Oprev inside and 0 elsewhere.
 * The regimes are selects on the forward's values, so a tie belongs where the forward sent it; every accumulator receives its
 * terms in decreasing t, and one that receives no term in a row keeps its bits.  gx, gpar and gstate are WRITTEN; T = 0 writes
 * zeros.  The refusals of lgar_network_route_mc, and (T > 0) a null gy, gx, x, y, down, up_ptr, or a null up_idx with
 * n_edges > 0, return LGAR_E_ARG. */
int32_t lgar_network_route_mc_grad(const double *gy, int32_t n_rows, int32_t n_catchments, const double *par, double dt_h, double rmin,
                                   double rmax, const int32_t *down, const int32_t *order, const int32_t *level_ptr, int32_t n_levels,
                                   double *gx, const double *x, const double *y, const int32_t *up_ptr, const int32_t *up_idx,
                                   int32_t n_edges, const double *state_in, double *gpar, double *gstate, void *stream);

/* Catchment network with two node kinds: Muskingum-Cunge reaches (exactly lgar_network_route_mc's row) and level-pool reservoirs
 * (lakes): a pool stores what arrives, releases by a power law of its active storage, never below its dead storage s0, and spills
 * what does not fit below smax.  Everything is fp64, catchment fastest; the topology, the inflow fold, par_mc[4][B] (unread at a
 * pool), dt_h, rmin, rmax are lgar_network_route_mc's.  The KIND of a node is given by its place in `order`: inside every level
 * the reaches come first and the pools after them (each part by ascending index), and pool_ptr[n_levels] -- HOST memory, like
 * level_ptr -- gives the split: positions level_ptr[l] .. pool_ptr[l] - 1 are reaches, pool_ptr[l] .. level_ptr[l + 1] - 1 pools,
 * level_ptr[l] <= pool_ptr[l] <= level_ptr[l + 1].  A level gets up to two launches, one per kind; the order of the nodes inside
 * a level never affects a bit.  The pool data are compact over the P = n_pools pools: pool_slot[B] (int32, device) = the pool's
 * index 0 .. P - 1, -1 at a reach (clamped into 0 .. P - 1 when read at a pool); par_pool[5][P] = cq (the release at
 * a = sref, in the unit of x), m (the exponent), s0 (dead storage), sref (> 0), smax (>= s0; +inf: never spills), storages in
 * the unit of x times hours; storage[T][P] = S after every row (NULL: not wanted).  state_in / state_out [2][B] = (Iprev, Oprev)
 * at a reach, (Iprev, S) at a pool.  prmin, prmax: the range a / sref is held to, 2^-60 <= prmin <= prmax <= 2^60.
 *
 * FORWARD at a pool b of slot s, with Iprev, S = state_in[0][b], state_in[1][b] (NULL: +0.0), half = 0.5 * dt_h and
 * cap = smax - s0 formed once, for t = 0 .. T - 1:
 *     I    = x[t][b];  for e = up_ptr[b] .. up_ptr[b + 1] - 1:  I = I + y[t][up_idx[e]]
 *     vin  = half * (I + Iprev)
 *     a    = S - s0;   rho = a / sref
 *     lo   = rho < prmin;   hi = !lo && rho > prmax;   rc = lo ? prmin : (hi ? prmax : rho)
 *     L    = mc_ln(rc);   tau = m * L
 *     ta   = tau < 0 ? -tau : tau;   big = ta > LGAR_GW_ZMAX;   tc = big ? LGAR_GW_ZMAX : ta
 *     e    = gw_exp(tc)
 *     Ql   = tau > 0 ? cq * e : cq / e                        (the release law cq rc^m)
 *     av   = a + vin;   qa = av / dt_h
 *     free = Ql < qa;   Q = free ? Ql : qa                     (a NaN qa stays)
 *     empty = Q < 0;    Q = empty ? 0.0 : Q                    (a NaN Q stays)
 *     r    = av - dt_h * Q
 *     ex   = r - cap;   spill = ex > 0
 *     O    = spill ? Q + ex / dt_h : Q
 *     S    = (spill ? cap : r) + s0
 *     y[t][b] = O;   storage[t][s] = S;   Iprev = I
 * in exactly this association, without contraction, with IEEE divisions; every decision is a select and ties go where the selects
 * send them (rho == prmin / prmax is not clamped, Ql == qa is limited, ex == 0 does not spill).  m = 0 gives tau = 0, e = 1,
 * Ql = cq exactly.  In real arithmetic S_t - S_(t-1) = vin_t - dt_h O_t in every regime: volume is conserved.  The explicit
 * release can oscillate when cq dt_h is large against sref; that is not policed.  y, storage and state_out are WRITTEN; T = 0
 * copies the state; B = 0 is a no-op; P = 0 is allowed (then par_pool, pool_slot and storage may be NULL and no level may have a
 * pool segment) and is lgar_network_route_mc bit for bit.  |Ql - cq rc^m| <= (|tau| (1.0e-15 + u) + 4.56e-15 + u) cq rc^m for
 * |tau| <= LGAR_GW_ZMAX (derived in csrc/lgar_network_pool.hpp).
 *
 * Refused with LGAR_E_ARG, the scalars first: everything lgar_network_route_mc refuses; prmin, prmax outside
 * 2^-60 <= prmin <= prmax <= 2^60; n_pools < 0; a null pool_ptr with n_levels > 0; a pool_ptr[l] outside its level; a pool
 * segment with n_pools = 0; with n_pools > 0 a null par_pool or pool_slot. */
int32_t lgar_network_route_pool(const double *x, int32_t n_rows, int32_t n_catchments, const double *par_mc, const double *par_pool,
                                int32_t n_pools, double dt_h, double rmin, double rmax, double prmin, double prmax,
                                const int32_t *up_ptr, const int32_t *up_idx, int32_t n_edges, const int32_t *order,
                                const int32_t *level_ptr, const int32_t *pool_ptr, int32_t n_levels, const int32_t *pool_slot,
                                const double *state_in, double *state_out, double *y, double *storage, void *stream);

/* The adjoint of lgar_network_route_pool: from gy[T][B] the gradients with respect to x (gx[T][B]), the reach parameters
 * (gpar_mc[3][B], lgar_network_route_mc_grad's; +0.0 at a pool; NULL: not wanted), the pool parameters (gpool[4][P] = gcq, gm,
 * gs0, gsmax; sref is a constant; NULL: not wanted) and the initial state (gstate[2][B]; NULL: not wanted).  y and storage are
 * what the forward stored for the same arguments; storage is required when T > 0 and P > 0.  The levels run in DESCENDING order;
 * gx[t][down[b]] is the adjoint of the downstream node's total inflow at either kind.  A reach runs lgar_network_route_mc_grad's
 * rows.  A pool, with pI = pS = +0.0 and four accumulators from +0.0, for t = T - 1 .. 0, with Ip = I[t - 1],
 * Sp = storage[t - 1][s] (row 0: state_in, or +0.0), the flags and a, L, e, Ql of the forward's row from S = Sp and
 * vin = half * (I + Ip) (the same bits), inside = !lo && !hi && !big, and pw = tau > 0 ? e : 1.0 / e:
 *     lamO  = gy[t][b];  if down[b] >= 0:  lamO = lamO + gx[t][down[b]]
 *     lamS  = pS;   q = lamO / dt_h
 *     gr    = spill ? q : lamS;   gcap = lamS - q                        (gcap is used where spill)
 *     gQ    = empty ? 0.0 : lamO - dt_h * gr
 *     gav   = free ? gr : gr + gQ / dt_h
 *     ga    = free && inside ? gav + ((gQ * m) * Ql) / a : gav
 *     gcq   = free ? gcq + gQ * pw : gcq
 *     gm    = free && !big ? gm + (gQ * Ql) * L : gm
 *     gs0   = (gs0 + (spill ? lamS - gcap : lamS)) - ga
 *     gsmax = spill ? gsmax + gcap : gsmax
 *     hg    = half * gav;   gx[t][b] = hg + pI;   pI = hg;   pS = ga
 * and gstate[0][b], gstate[1][b] = pI, pS after row 0.  In real arithmetic: O = Q + (r - cap) / dt and S = smax where the pool
 * spills, S = r + s0 elsewhere; r = av - dt Q; Q = Ql where free, av / dt where limited, 0 where empty; dQl/dcq = rc^m,
 * dQl/dm = Ql ln rc unless big, dQl/da = m Ql / a inside; av = a + vin; a = S - s0.  The regimes are selects on the forward's own
 * values, so a tie belongs where the forward sent it; an accumulator that receives no term in a row keeps its bits; inside is a
 * select, not a multiply by zero.  Every output element is WRITTEN; T = 0 writes zeros.  Refused with LGAR_E_ARG: everything
 * lgar_network_route_mc_grad and lgar_network_route_pool refuse, and a null storage with T > 0 and n_pools > 0. */
int32_t lgar_network_route_pool_grad(const double *gy, int32_t n_rows, int32_t n_catchments, const double *par_mc, const double *par_pool,
                                     int32_t n_pools, double dt_h, double rmin, double rmax, double prmin, double prmax,
                                     const int32_t *down, const int32_t *order, const int32_t *level_ptr, const int32_t *pool_ptr,
                                     int32_t n_levels, const int32_t *pool_slot, double *gx, const double *x, const double *y,
                                     const double *storage, const int32_t *up_ptr, const int32_t *up_idx, int32_t n_edges,
                                     const double *state_in, double *gpar_mc, double *gpool, double *gstate, void *stream);

/* Catchment baseflow: a groundwater store per catchment, fed by the catchment sums of percolation, that returns water to the
 * channel through the exponential storage-discharge relation (the nonlinear reservoir coupled below this infiltration scheme in
 * NextGen / CFE).  Its result is added to the routed runoff ahead of lgar_network_route.
 *
 * All arrays are fp64, catchment fastest: the recharge r[T][B], the baseflow q[T][B], the storage s[T][B], the parameters
 * par[3][B] = cgw, expon, smax.  r, s, smax and the state share one depth unit (cm per row, or area-weighted cm); cgw is in that
 * unit per hour; dt_h is the row step in hours.
 *
 * FORWARD.  For every catchment b, with S = state_in[b] (state_in == NULL: +0.0), for t = 0 .. T - 1:
 *     A  = S + r[t][b]
 *     z  = expon[b] * (A / smax[b])
 *     zc = z < 0 ? 0 : (z > LGAR_GW_ZMAX ? LGAR_GW_ZMAX : z)                 (selects: a NaN stays a NaN)
 *     e  = gw_exp(zc)
 *     f  = (cgw[b] * dt_h) * (e - 1.0)
 *     qq = f > A ? A : f                                                    (the store cannot give more than it holds)
 *     qq = qq < 0 ? 0 : qq
 *     S  = A - qq
 *     q[t][b] = qq;   s[t][b] = S                                           (s == NULL: not wanted)
 * in exactly this association, without contraction (-ffp-contract=off).  state_out[b] = S after the last row (NULL: not wanted).
 * q, s and state_out are WRITTEN, not added to.  T = 0 copies the state (zeros when state_in is NULL); B = 0 is a no-op.  Mass
 * closes per catchment up to rounding: state_in + sum r = sum q + state_out.  The result for b is a pure function of column b
 * of r and par and of state_in[b]: a NaN in r[t][b] reaches q and s of catchment b from row t on and no other catchment.
 * Ties go where the selects send them: f == A is flux (qq = f), z == 0 and z == LGAR_GW_ZMAX are not clamped, qq == 0 is not
 * "clamped to 0".
 *
 * gw_exp(zc), 0 <= zc <= LGAR_GW_ZMAX, uses no libm, no fma and no hardware reciprocal -- numpy restates it one operation for one:
 *     k = rint(zc * LOG2E)                  computed as (zc * LOG2E + 1.5 * 2^52) - 1.5 * 2^52 (two rounded adds, ties to even)
 *     r = (zc - k * LN2_HI) - k * LN2_LO    LN2_HI = 0x1.62e42fee00000p-1 (32 trailing zero bits: k * LN2_HI is exact for
 *                                           k <= 58), LN2_LO = 0x1.a39ef35793c76p-33, LOG2E = 0x1.71547652b82fep+0
 *     p = sum_{j <= 13} r^j / j!            Horner from j = 13 down: p = p * r + c_j, one rounded multiply and one rounded add per
 *                                           step, c_j the correctly rounded 1 / j!
 *     e = ldexp(p, k)                       exact
 *
 * Negative sizes, a null pointer the sizes say will be read or written (T > 0: r, par, q), or a dt_h that is not finite or
 * <= 0, return LGAR_E_ARG.  Parameter VALUES are not policed: smax = 0 gives the IEEE result.  One launch on `stream`; offsets
 * are 64-bit. */
#define LGAR_GW_ZMAX 40.0
int32_t lgar_catchment_baseflow(const double *r, int32_t n_rows, int32_t n_catchments, const double *par, double dt_h,
                                const double *state_in, double *state_out, double *q, double *s, void *stream);

/* The adjoint of the baseflow store: from gq[T][B] and gs[T][B] (gs == NULL: zeros), the incoming gradients of q and s, the
 * gradients with respect to r (gr[T][B]), to the parameters (gpar[3][B] = gcgw, gexpon, gsmax; NULL: not wanted) and to the
 * initial storage (gstate[B]; NULL: not wanted).  s is the storage the forward stored for the same r, par, dt_h, state_in.  A of
 * row t is re-formed as s[t - 1][b] + r[t][b] (row 0: state_in[b], or +0.0), and z, zc, e, f and the regime of the row come from
 * the forward's own function: the same bits.  With lam = +0.0 and three accumulators from +0.0, for t = T - 1 .. 0:
 *     lam = lam + gs[t][b];   w = gq[t][b] - lam;   ce = (cgw[b] * dt_h) * e
 *     zero    ((f > A ? A : f) < 0: qq was clamped to 0):   dA = 0;  no parameter terms
 *     emptied (not zero, f > A: qq = A >= 0):               dA = 1;  no parameter terms
 *     flux    (neither), z < 0 or z > LGAR_GW_ZMAX:         dA = 0;  gcgw = gcgw + w * (dt_h * (e - 1.0))
 *     flux, 0 <= z <= LGAR_GW_ZMAX:                         dA = ce * (expon[b] / smax[b]);
 *                                                           gcgw   = gcgw   + w * (dt_h * (e - 1.0))
 *                                                           gexpon = gexpon + w * (ce * (A / smax[b]))
 *                                                           gsmax  = gsmax  + w * (-(ce * zc) / smax[b])
 *     gr[t][b] = lam + w * dA;   lam = gr[t][b]
 * gstate[b] = lam after row 0.  gr, gpar and gstate are WRITTEN; every accumulator receives its terms in decreasing t, and an
 * accumulator that receives no term in a row keeps its bits.  T = 0 writes zeros.  The refusals of lgar_catchment_baseflow
 * (T > 0: gq, r, s, par, gr), and so gpar or gstate wanted without s, return LGAR_E_ARG. */
int32_t lgar_catchment_baseflow_grad(const double *gq, const double *gs, const double *r, const double *s, int32_t n_rows,
                                     int32_t n_catchments, const double *par, double dt_h, const double *state_in, double *gr,
                                     double *gpar, double *gstate, void *stream);

/* Catchment snowpack: a temperature-index store per forcing cell AHEAD of the columns.  It takes precipitation and air
 * temperature and hands on rain plus melt: w is the [T][B] water input lgar_forward reads as `precip` through a column map.
 * Two states per cell, ice and held liquid water; a linear rain/snow transition, degree-day melt, refreezing of held liquid, a
 * liquid holding capacity (the classic HBV / SNOW-17 family of routines).
 *
 * All arrays are fp64, cell fastest: the precipitation rate p[T][B] (the unit of the engine's forcing: depth per hour), the air
 * temperature ta[T][B], the water input rate w[T][B], the pack ice[T][B], liq[T][B] (depth; both or neither: NULL = not wanted),
 * par[7][B] = tlo, thi, tm, sfcf, cfmax, cfr, cwh (tlo, thi, tm: temperatures; sfcf: snowfall correction; cfmax: depth per degree
 * per hour; cfr, cwh: fractions), state_in / state_out [2][B] = ice, liq; dt_h is the row step in hours.
 *
 * FORWARD.  For every cell b, with cd = cfmax[b] * dt_h, cr = cfr[b] * cd, span = thi[b] - tlo[b] (one rounding each, once) and
 * (ice, liq) = state_in[.][b] (state_in == NULL: +0.0), for t = 0 .. T - 1:
 *     Ta   = ta[t][b];   pd = p[t][b] * dt_h
 *     lo   = Ta <= tlo;  hi = !lo && Ta >= thi
 *     fr   = lo ? 0.0 : (hi ? 1.0 : (Ta - tlo) / span)                   (tlo == thi: the quotient is never selected)
 *     rain = pd * fr;    dry = pd - rain;   snow = sfcf * dry
 *     d    = Ta - tm;    warm = d > 0
 *     ice1 = ice + snow
 *     pm   = cd * d;     ml = pm > ice1
 *     melt = warm ? (ml ? ice1 : pm) : 0.0
 *     pr   = cr * (-d);  rl = pr > liq
 *     refr = warm ? 0.0 : (rl ? liq : pr)
 *     ice2 = (ice1 - melt) + refr
 *     liq1 = ((liq + rain) + melt) - refr
 *     cap  = cwh * ice2; over = liq1 > cap
 *     out  = over ? liq1 - cap : 0.0
 *     liq  = over ? cap : liq1;   ice = ice2
 *     w[t][b] = out / dt_h;   ice[t][b] = ice;   liq[t][b] = liq
 * in exactly this association, without contraction (-ffp-contract=off), IEEE divisions, no libm.  state_out = (ice, liq) after
 * the last row (NULL: not wanted).  Every output is WRITTEN, not added to.  Every decision is a select, and ties go where the
 * selects send them: Ta == tlo is lo, Ta == thi is hi, d == 0 is not warm, pm == ice1 melts pm, pr == liq refreezes pr,
 * liq1 == cap holds.
 *   Mass balance, in real arithmetic: ice_T + liq_T + dt_h sum w = ice_0 + liq_0 + dt_h sum (fr + sfcf (1 - fr)) p.
 *   Empty store: T = 0 copies the state (zeros when state_in is NULL); B = 0 is a no-op.
 *   Independence: the result for b is a pure function of column b of p, ta and par and of state_in[.][b].  A NaN fails every
 *     comparison and takes the last alternative: a NaN in p[t][b] or ta[t][b] is in ice and liq of cell b from row t on and in no
 *     other cell (out's last alternative is the constant 0.0: w of such a row is +0.0 -- the pack carries the NaN).
 *   Warm identity: with a zero state, every Ta > max(thi, tm) and dt_h a power of two, w has the bits of p where p > 0 and is
 *     +0.0 where p == 0.
 * Refused with LGAR_E_ARG: negative sizes, a dt_h that is not finite or <= 0, exactly one of ice / liq given, a null pointer
 * the sizes say will be read or written (T > 0: p, ta, par, w).  Parameter VALUES are not policed (a negative p, a negative
 * initial liq, tlo > thi give the IEEE result).  One launch on `stream`; offsets are 64-bit. */
int32_t lgar_catchment_snow(const double *p, const double *ta, int32_t n_rows, int32_t n_cells, const double *par, double dt_h,
                            const double *state_in, double *state_out, double *w, double *ice, double *liq, void *stream);

/* The adjoint of the snowpack: from gw[T][B], gice[T][B], gliq[T][B] (gice, gliq == NULL: zeros), the incoming gradients of w,
 * ice and liq, the gradients with respect to p (gp[T][B]), to ta (gta[T][B]; NULL: not wanted), to the parameters (gpar[7][B] in
 * par's order; NULL: not wanted) and to the initial state (gstate[2][B]; NULL: not wanted).  ice and liq are the pack the forward
 * stored for the same p, ta, par, dt_h, state_in.  Row t is re-formed from ice[t - 1][b], liq[t - 1][b] (row 0: state_in, or
 * +0.0) through the forward's own row function: every flag and value below has the forward's bits.  With li = ll = +0.0 and
 * the accumulators gtlo, gthi, gtm, gsfcf, gcd, gcr, gcwh from +0.0, mid = !lo && !hi, for t = T - 1 .. 0:
 *     li    = li + gice[t][b];   ll = ll + gliq[t][b];   go = gw[t][b] / dt_h
 *     dl1   = over ? go : ll;    dcap = over ? ll - go : 0.0
 *     di2   = li + cwh * dcap;   gcwh = over ? gcwh + dcap * ice2 : gcwh
 *     dmelt = dl1 - di2;         drefr = di2 - dl1
 *     wm = warm && ml;   wf = warm && !ml;   cl = !warm && rl;   cf = !warm && !rl
 *     di1   = wm ? di2 + dmelt : di2;       dliq = cl ? dl1 + drefr : dl1
 *     gcd   = wf ? gcd + dmelt * d : gcd;   gcr  = cf ? gcr + drefr * (-d) : gcr
 *     gd    = wf ? dmelt * cd : (cf ? -(drefr * cr) : 0.0)
 *     gtm   = wf || cf ? gtm - gd : gtm
 *     gsfcf = gsfcf + di1 * dry
 *     sd    = sfcf * di1;   drain = dl1 - sd;   dpd = sd + drain * fr;   dfr = drain * pd
 *     gTa   = mid ? gd + dfr / span : gd
 *     gtlo  = mid ? gtlo + (dfr * (Ta - thi)) / (span * span) : gtlo
 *     gthi  = mid ? gthi - (dfr * (Ta - tlo)) / (span * span) : gthi
 *     gp[t][b] = dpd * dt_h;   gta[t][b] = gTa;   li = di1;   ll = dliq
 * and after row 0: gcfmax = dt_h * (gcd + cfr * gcr), gcfr = cd * gcr, gstate = (li, ll).  The regimes are selects on the
 * forward's own values, so a tie belongs where the forward sent it; an accumulator that receives no term in a row keeps its bits
 * (a select of the accumulator, not an added zero); a quotient by span is formed only inside a select that discards it outside
 * mid.  Every output element is WRITTEN; T = 0 writes zeros.  Refused with LGAR_E_ARG: what lgar_catchment_snow refuses (T > 0:
 * gw, p, ta, par, gp), and a null ice / liq with T > 0. */
int32_t lgar_catchment_snow_grad(const double *gw, const double *gice, const double *gliq, const double *p, const double *ta,
                                 const double *ice, const double *liq, int32_t n_rows, int32_t n_cells, const double *par,
                                 double dt_h, const double *state_in, double *gp, double *gta, double *gpar, double *gstate,
                                 void *stream);

/* Forward-mode tangent of lgar_catchment_snow along n_dirs = D directions at once: one lane per (cell, direction), everything
 * fp64.  p, ta, par, dt_h, state_in are the forward's; the value recurrence is the forward's own, so every decision has its
 * bits.  Input tangents, NULL = zeros: dp, dta [D][n_rows][n_cells]; dpar [D][7][n_cells]; dstate_in [D][2][n_cells].
 * Outputs: dw(t, b, k) = d w[t][b] along direction k, stored at dw[(t * n_cells + b) * ld + k0 + k] with ld >= k0 + D, so the
 * call writes straight into the [n_steps][Nf][G] block of forcing tangents lgar_forward_tangent_forced reads (G = ld); the other
 * elements of a row of ld are not touched.  Optional dice, dliq [D][n_rows][n_cells] (both or neither) and dstate_out
 * [D][2][n_cells].  Ties go where the forward's selects send them (the adjoint's conventions); n_rows = 0 copies dstate.
 * lgar_snow.hpp has the recurrence.  Refused with LGAR_E_ARG: negative sizes or k0, ld < k0 + D, a dt_h that is not finite or
 * <= 0, exactly one of dice / dliq, and (n_rows, n_cells, D > 0) a null p, ta, par or dw. */
int32_t lgar_catchment_snow_tangent(const double *p, const double *ta, int32_t n_rows, int32_t n_cells, const double *par, double dt_h,
                                    const double *state_in, int32_t n_dirs, const double *dp, const double *dta, const double *dpar,
                                    const double *dstate_in, double *dw, int32_t ld, int32_t k0, double *dice, double *dliq,
                                    double *dstate_out, void *stream);

/* Catchment canopy: an interception store per forcing cell AHEAD of the snowpack and the columns.  All
 * arrays fp64, cell fastest: the precipitation rate p[T][B] and the PET rate e[T][B] (the engine's forcing unit), the relative leaf
 * area lai[T][B] (NULL: 1, and then cap = cmax is formed once with no multiplication), par[3][B] = cmax (the depth the canopy
 * holds per unit lai), fe (the wet-canopy evaporation factor), cover (the vegetated fraction), state_in[1][B] = s, the depth held
 * (NULL: +0.0).  T = n_rows, B = n_cells.  Outputs: the throughfall rate w[T][B], the PET left to the columns pet_out[T][B], and
 * optionally (both or neither) store[T][B], the depth held behind each row, and evap[T][B], the wet-canopy evaporation rate.  One
 * cell b, with fc = fe * cover (once), for t = 0 .. T - 1:
 *     pd   = p[t][b] * dt_h;      ed = e[t][b] * dt_h
 *     hit  = cover * pd;          direct = pd - hit
 *     cap  = cmax * lai[t][b]
 *     s1   = s + hit;             full = s1 > cap
 *     drip = full ? s1 - cap : 0.0
 *     s2   = full ? cap : s1
 *     dem  = fc * ed;             lim = dem > s2
 *     ei   = lim ? s2 : dem
 *     s    = s2 - ei
 *     neg  = ei > ed
 *     r    = neg ? 0.0 : ed - ei
 *     w[t][b] = (direct + drip) / dt_h;   pet_out[t][b] = r / dt_h;   store[t][b] = s;   evap[t][b] = ei / dt_h
 * in exactly this association, without contraction (-ffp-contract=off), IEEE divisions, no libm.  state_out = s after the last
 * row (NULL: not wanted).  Every output is WRITTEN, not added to.  Every decision is a select, and ties go where the selects send
 * them: s1 == cap holds (no drip), dem == s2 is demand-limited (ei = dem), ei == ed leaves r = ed - ei = +0.0.
 *   Water balance, in real arithmetic: dt_h sum p = dt_h sum w + dt_h sum evap + s_T - s_0.
 *   Empty store: T = 0 copies the state (zeros when state_in is NULL); B = 0 is a no-op.
 *   Independence: the result for b is a pure function of column b of p, e, lai and par and of state_in[0][b].  A NaN fails every
 *     comparison and takes the last alternative.  A NaN in p[t][b]: w of row t is NaN, evap and pet_out of row t are clean (ei =
 *     dem), store is NaN from row t on; in the later rows drip = 0.0 and ei = dem, so w = direct / dt_h, evap and pet_out are clean
 *     -- the store carries the NaN.  A NaN in e[t][b]: evap and pet_out of row t are NaN, w of row t is clean, store is NaN from
 *     row t on.  A NaN in lai[t][b]: full is false, the row holds all that hit it, and the NaN is gone.  No other cell sees any.
 *   Bare ground: with cover = 0, a zero state and dt_h a power of two, w has p's bits and pet_out has e's bits.
 * Refused with LGAR_E_ARG: negative sizes, a dt_h that is not finite or <= 0, exactly one of store / evap given, a null pointer
 * the sizes say will be read or written (T > 0: p, e, par, w, pet_out).  Parameter VALUES are not policed.  One launch on
 * `stream`; offsets are 64-bit. */
int32_t lgar_catchment_canopy(const double *p, const double *e, const double *lai, int32_t n_rows, int32_t n_cells, const double *par,
                              double dt_h, const double *state_in, double *state_out, double *w, double *pet_out, double *store,
                              double *evap, void *stream);

/* The adjoint of the canopy: from gw[T][B], gpet[T][B] and gstore[T][B], gevap[T][B] (each NULL: zeros), the incoming gradients of
 * w, pet_out, store and evap, the gradients with respect to p (gp[T][B]), to e (ge[T][B]), to lai (glai[T][B]; NULL: not wanted),
 * to the parameters (gpar[3][B] in par's order; NULL: not wanted) and to the initial state (gstate[1][B]; NULL: not wanted).
 * store is the series the forward stored for the same p, e, lai, par, dt_h, state_in.  Row t is re-formed from store[t - 1][b]
 * (row 0: state_in, or +0.0) through the forward's own row function: every flag below has the forward's bits.  With ls = +0.0
 * and the accumulators gcmax, gfc, gcover from +0.0, lai = lai[t][b] (NULL: 1.0), for t = T - 1 .. 0:
 *     ls   = ls + gstore[t][b];  gtf = gw[t][b] / dt_h;  gr = gpet[t][b] / dt_h;  gei = gevap[t][b] / dt_h
 *     dr   = neg ? 0.0 : gr;          dei  = (gei - dr) - ls
 *     ds2  = lim ? ls + dei : ls;     ddem = lim ? 0.0 : dei
 *     gfc  = lim ? gfc : gfc + ddem * ed;          ged = dr + ddem * fc
 *     ds1  = full ? gtf : ds2;        dcap = full ? ds2 - gtf : 0.0
 *     gcmax = full ? gcmax + dcap * lai : gcmax;   glai[t][b] = dcap * cmax
 *     dhit = ds1 - gtf;               gcover = gcover + dhit * pd
 *     gp[t][b] = (gtf + dhit * cover) * dt_h;      ge[t][b] = ged * dt_h;      ls = ds1
 * and after row 0: gfe = gfc * cover, gcover = gcover + gfc * fe, gstate = ls.  The regimes are selects on the forward's own
 * flags, so a tie belongs where the forward sent it; an accumulator that receives no term in a row keeps its bits (a select of the
 * accumulator, not an added zero).  Every output element is WRITTEN; T = 0 writes zeros.  Refused with LGAR_E_ARG: negative sizes,
 * a dt_h that is not finite or <= 0, and (T, B > 0) a null gw, gpet, p, e, store, par, gp or ge. */
int32_t lgar_catchment_canopy_grad(const double *gw, const double *gpet, const double *gstore, const double *gevap, const double *p,
                                   const double *e, const double *lai, const double *store, int32_t n_rows, int32_t n_cells,
                                   const double *par, double dt_h, const double *state_in, double *gp, double *ge, double *glai,
                                   double *gpar, double *gstate, void *stream);

/* Forward-mode tangent of lgar_catchment_canopy along n_dirs = D directions at once: one lane per (cell, direction), lane
 * k * B + b, everything fp64.  p, e, lai, par, dt_h, state_in are the forward's; the value recurrence is the forward's own, so
 * every decision has its bits.  Input tangents, NULL = zeros: dp, de, dlai [D][T][B]; dpar [D][3][B]; dstate_in [D][B].  Once per
 * lane fc' = fe' * cover + fe * cover', and per row, with s' from dstate_in, lai = lai[t][b] (NULL: 1.0), lai' = dlai[k][t][b]:
 *     pd'   = dp[k][t][b] * dt_h;           ed' = de[k][t][b] * dt_h
 *     hit'  = cover' * pd + cover * pd';    direct' = pd' - hit'
 *     cap'  = cmax' * lai + cmax * lai'
 *     s1'   = s' + hit';   drip' = full ? s1' - cap' : 0.0;   s2' = full ? cap' : s1'
 *     dem'  = fc' * ed + fc * ed';          ei' = lim ? s2' : dem'
 *     s'    = s2' - ei';   r' = neg ? 0.0 : ed' - ei'
 * Outputs: dw(t, b, k) = (direct' + drip') / dt_h at dw[(t * B + b) * ld + k0 + k] and dpet(t, b, k) = r' / dt_h at the same
 * offset of dpet (NULL: not wanted), with ld >= k0 + D, so the call writes straight into the two [n_steps][Nf][G] blocks of forcing
 * tangents lgar_forward_tangent_forced reads (G = ld); the other elements of a row of ld are not touched.  Optional dstore
 * (s') and devap (ei' / dt_h) [D][T][B] (both or neither) and dstate_out [D][B].  T = 0 copies dstate.  Refused with LGAR_E_ARG:
 * negative sizes or k0, ld < k0 + D, a dt_h that is not finite or <= 0, exactly one of dstore / devap, and (T, B, D > 0) a null
 * p, e, par or dw. */
int32_t lgar_catchment_canopy_tangent(const double *p, const double *e, const double *lai, int32_t n_rows, int32_t n_cells,
                                      const double *par, double dt_h, const double *state_in, int32_t n_dirs, const double *dp,
                                      const double *de, const double *dlai, const double *dpar, const double *dstate_in, double *dw,
                                      double *dpet, int32_t ld, int32_t k0, double *dstore, double *devap, double *dstate_out,
                                      void *stream);

/* Run totals of a run cut into several lgar_forward calls.  lgar_forward sums a call's accumulators step by step from zero
 * and adds that sum to LgarState.totals, so a chunked run adds several partial sums where one call adds one: the same numbers in
 * another order, equal to the last bits only.  This replays the one-call order over series the chunks stored: for every j < 7
 * with stored->series[j] != NULL ([n_rows][n_columns], dtype; only `series` of `stored` is read)
 *     running[j][c] = (..((running[j][c] + series[j][0][c]) + series[j][1][c]) + ..) + series[j][n_rows - 1][c]
 * running: [8][n_columns] (dtype), zeroed by the caller before the first chunk and carried from chunk to chunk; after the last
 * one totals[j] = totals_before_the_run[j] + running[j] (j = 7, discharge, takes running[6]; percolation is not summed in
 * bottom_mode 0) is what ONE call over all rows leaves, bit for bit, for every column that stayed in one kernel of the
 * front-capacity chain (a hand-over inside a call splits that call's sum as well).  Rows a chunk did not write must read zero. */
int32_t lgar_totals_replay(const LgarDims *dims, const LgarStepOut *stored, int32_t n_rows, void *running, int32_t dtype,
                           void *stream);

/* Leaf kernels (known-answer tests on the GPU), element-wise over n items:
 * op 0 theta_from_h(x), 1 se_from_h(x), 2 k_from_se(x), 3 h_from_se(x)      (physics/utils.py:35-174)
 * op 4 geff(theta1 = x, theta2 = y)                                        (lgar/green_ampt.py:45-84)
 * op 6 the same trapezoid evaluated operation by operation like the reference (4 pow + sqrt per node, running h)
 * op 5 aet(psi = x, pet = y, dt_h = z)                                      (lgar/aet.py:17-51)
 * op 7 log2(x), 8 exp2(x) as the Geff trapezoid evaluates them, 9 pow(x, y) as the fast modes evaluate torch.pow
 *      (accuracy of the device arithmetic on the real hardware; soil parameters unused but required)
 * op 10 geff(theta1 = x, theta2 = y) by the mixed-precision trapezoid of LgarDims.geff_mode = 1 (LGAR_F64; LGAR_F32: op 4)
 * op 11 x / y as the fast modes divide (LGAR_F64: reciprocal + Newton + correction, within an ulp of the IEEE quotient)
 * op 12 pow(x, y), 13 log2(x), 14 exp2(x) as the mixed-precision kernels evaluate them (polynomial terms combined pairwise)
 * LGAR_F32 only (LGAR_F64: LGAR_E_ARG) -- the arithmetic of the fp32 fast mode, which ops 0-3 and 5 (IEEE divide) do not run:
 * op 15 x / y as x * v_rcp_f32(y), 16 sqrt(x) as v_sqrt_f32
 * op 17 theta_from_h(x), 18 se_from_h(x), 19 k_from_se(x), 20 h_from_se(x), 21 aet(psi = x, pet = y, dt_h = z) with that
 *      quotient and the v_log_f32 / v_exp_f32 pow
 * op 22 the fp32 trapezoid between two heads h_i = x, h_f = y (calc_dzdt's site: the heads are the fronts' own psi)
 * op 23 the closed-form Geff(theta1 = x, theta2 = y)                        (lgar/green_ampt.py:85-98)
 * (LGAR_F32: ops 7 and 8 are the raw v_log_f32 and v_exp_f32, op 9 the pow made of them)
 * alpha, n, ksat, theta_e, theta_r: [n] per-item soil parameters. */
int32_t lgar_leaf_batch(int32_t op, int32_t n_items, const void *x, const void *y, double z, const void *alpha,
                        const void *n, const void *ksat, const void *theta_e, const void *theta_r, int32_t nint,
                        double wilting_point_psi, void *out, int32_t dtype, void *stream);

/* Tangent leaf kernels (known-answer tests of the dual-number arithmetic of the tangent kernels), element-wise over n items: the
 * leaf's value and ONE directional derivative, along the seeds d_alpha, d_n, d_ksat, d_theta_e, d_theta_r, d_x, d_y ([n] each; a
 * null pointer is a seed of 0).  m = 1 - 1/n, 1/m and 1/n are formed in dual numbers as the tangent kernels form them.
 * policy: 0 POL_LEAN (the fast tangent kernels), 1 POL_LIBRARY (the verification kernels) -- read by ops 0-3, 5, 23, 24.
 * op numbers are lgar_leaf_batch's where the op exists there:
 * op 0 theta_from_h(x), 1 se_from_h(x), 2 k_from_se(x), 3 h_from_se(x), 5 aet(psi = x, pet = y, dt_h = z),
 * op 23 the closed-form Geff(theta1 = x, theta2 = y), 24 se_from_theta(x)
 * op 4 geff(theta1 = x, theta2 = y): the fused trapezoid with its hand-derived node tangent
 * op 6 the same trapezoid operation by operation, POL_LIBRARY
 * primitives of the dual numbers (soil parameters unused but required; seeds d_x, d_y):
 * op 7 lg2p(x), 8 ex2p(x), 9 pw(x, y), 11 dv<POL_LEAN>(x, y), 16 sq(x), 25 pwx<true>(x, y) (the library pow),
 * op 26 dv<POL_LEAN>(x, real y), 27 dv<POL_LEAN>(real x, y), 28 x / y (operator/), 29 lg2(x), 30 ex2(x), 31 mn(x, y), 32 ab(x)
 * share = W in 2 .. 32 (op 4, LGAR_F64 only; 0: every lane on its own): the trapezoid shared by W lanes as the tangent kernels
 * share it (LgarDims.tangent_share) -- one-wave workgroups, floor(64 / W) groups of W adjacent lanes, one item per group, lane r of
 * a group along direction r: the seeds and both outputs are then [n][W]. */
int32_t lgar_leaf_tangent_batch(int32_t op, int32_t policy, int32_t share, int32_t n_items, const void *x, const void *y, double z,
                                const void *alpha, const void *n, const void *ksat, const void *theta_e, const void *theta_r,
                                const void *d_alpha, const void *d_n, const void *d_ksat, const void *d_theta_e,
                                const void *d_theta_r, const void *d_x, const void *d_y, int32_t nint, double wilting_point_psi,
                                void *out_value, void *out_tangent, int32_t dtype, void *stream);

/* Measurement only (no reference counterpart): vector-ALU issue-rate probe, the compute-side roof bench.py prices the
 * path against (the path is VALU-bound: ~10^3 flop per algorithmic byte).  Launches n_workgroups one-wave workgroups,
 * each running `iters` iterations of lgar_valu_probe_insts(op) instructions of kind `op`; lds_bytes_per_workgroup sets the resident waves
 * per SIMD (160 KiB / (4 k) => k).  sink: device float[n_workgroups * 64] (never written in practice).  The caller
 * times the launch on `stream`. */
#define LGAR_PROBE_EXP 0      /* v_exp_f32, 8 independent chains */
#define LGAR_PROBE_LOG 1      /* v_log_f32 */
#define LGAR_PROBE_RCP 2      /* v_rcp_f32 */
#define LGAR_PROBE_SQRT 3     /* v_sqrt_f32 */
#define LGAR_PROBE_FMA 4      /* v_fma_f32 */
#define LGAR_PROBE_MUL 5      /* v_mul_f32 */
#define LGAR_PROBE_PK_FMA 6   /* v_pk_fma_f32 */
#define LGAR_PROBE_PK_MUL 7   /* v_pk_mul_f32 */
#define LGAR_PROBE_CNDMASK 8  /* v_cndmask_b32 */
#define LGAR_PROBE_CMP 9      /* v_cmp_lt_f32 */
#define LGAR_PROBE_EXP_DEP 10 /* v_exp_f32, ONE dependent chain (latency) */
#define LGAR_PROBE_FMA_DEP 11 /* v_fma_f32, ONE dependent chain */
#define LGAR_PROBE_FMA64 12   /* v_fma_f64 */
#define LGAR_PROBE_MUL64 13   /* v_mul_f64 */
#define LGAR_PROBE_ADD64 14   /* v_add_f64 */
#define LGAR_PROBE_RCP64 15   /* v_rcp_f64 */
#define LGAR_PROBE_GEFF_MIX 16 /* the instruction stream of the lean fp32 Geff loop: per node pair 4 v_log, 4 v_exp, 10 packed */
#define LGAR_PROBE_CNDMASK_SGPR 17 /* v_cndmask_b32 with an SGPR-pair mask */
#define LGAR_PROBE_BFI 18      /* v_bfi_b32 (bitwise select on a vector mask) */
#define LGAR_PROBE_CMP_CNDMASK 19 /* v_cmp_lt_f32 + v_cndmask_b32 pairs */
#define LGAR_PROBE_ADD 20      /* v_add_f32 */
#define LGAR_PROBE_READLANE 21 /* v_readlane_b32 (what an SGPR spill reload costs) */
#define LGAR_PROBE_DS_READ 22  /* ds_read_b32, lane-contiguous */
#define LGAR_PROBE_MIN 23      /* v_min_f32 */
#define LGAR_PROBE_LDEXP64 24       /* v_ldexp_f64 */
#define LGAR_PROBE_FREXP_EXP64 25   /* v_frexp_exp_i32_f64 */
#define LGAR_PROBE_RNDNE64 26       /* v_rndne_f64 */
#define LGAR_PROBE_CVT_I32_F64 27   /* v_cvt_i32_f64 */
#define LGAR_PROBE_CVT_F64_I32 28   /* v_cvt_f64_i32 */
#define LGAR_PROBE_ADD_U32 29       /* v_add_u32 */
int32_t lgar_valu_probe_insts(int32_t op); /* wave-instructions per probe iteration: 64 (72 for LGAR_PROBE_GEFF_MIX) */
int32_t lgar_valu_probe(int32_t op, int32_t n_workgroups, int32_t lds_bytes_per_workgroup, int32_t iters, void *sink,
                        void *stream);

#ifdef __cplusplus
}
#endif
#endif
