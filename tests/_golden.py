"""TEST INFRASTRUCTURE ONLY: what the fixtures under tests/golden demand of an engine -- the bars, the checks and the runners
that the simulator's suite (test_devsim_golden.py) and the GPU's (test_gpu_parity.py, test_gpu_mixed.py, test_gpu_autograd.py)
share.  The checks are pure functions of numpy arrays and the opened fixture and raise AssertionError with the quantity, the
place, the observed value and the bar spelled out (tests/test_golden_checks.py feeds them the reference's own data, moved by
0.3 and by 3 bars).  The runners drive any engine built by a `make_engine(g, ncol, **kw)` callable."""
import os

import numpy as np

from conftest import GOLDEN, check_fault_kind, golden_names

TRAJ = [n for n in golden_names() if not n.startswith("grad_")]
GRADS = [n for n in golden_names() if n.startswith("grad_")]

# ---- the bars ----------------------------------------------------------------------------------------------------------
REL_FLOOR = 1e-6      # relative errors are taken against max(|reference|, floor): below 1e-6 cm a flux is rounding noise
NATIVE = 1e-6         # north_star: fp64 within 1e-6 relative per step, every accumulator, depth, theta, run totals (observed <= 5e-8)
LITERAL = 1e-7        # search_mode 0 repeats the reference's own operations: ten times tighter (observed <= 2e-9)
INIT_VOLUME = 1e-9    # absolute, cm: the initial state is a handful of fp64 operations
DERIVED = 1e-5        # psi, K, dz/dt of the last table are functions of theta: one digit looser than theta itself
PSI_FLOOR, K_FLOOR, DZDT_FLOOR = 1e-3, 1e-12, 1e-9  # cm, cm/h, cm/h (K: the deepest front keeps its initial K(theta))
# Mixed-precision Geff (LgarDims.geff_mode = 1: fp64 state, fp32 hardware transcendentals in the trapezoid's interior nodes).
# What it reaches against the reference: a Geff value carries a RANDOM relative error of ~1e-8 (<= 2e-7),
# which the column dynamics pass on to the fluxes 1:1 except at front events, where one step's infiltration can move by up to
# ~50x that -- and a runoff that is the small difference of rainfall and infiltration moves by the same ABSOLUTE amount.
MIXED_FLUX = 2e-5     # per-step outputs against max(rain + ponding of the step, |value|, 1e-3 cm) (observed 1.3e-5 on the hardware)
MIXED_TOTAL = 2e-6    # run totals against max(|total|, total rain, 1e-2 cm)
MIXED_STEP_BACKSTOP = 1e-3  # relative, every single per-step value (observed 1.7e-4 on a 1.1e-3 cm runoff off by 2e-7 cm)
# The every-step front table, (bar, usual): every step within `bar`, all but max(1, T // 50) steps within `usual` (observed:
# 4e-10 fast, 2e-9 literal).  The mixed mode holds `usual` except in the step of a front event (one step of two_layer_synth1
# at 7e-6, 8e-8 elsewhere), where its bar on per-step fluxes applies; `usual` is 1e-6 on the simulator (the host's log2f /
# exp2f) and 2e-6 on the GPU (the hardware's v_log_f32 / v_exp_f32).
STEPWISE_NATIVE, STEPWISE_LITERAL = (NATIVE, NATIVE), (LITERAL, LITERAL)
STEPWISE_MIXED_SIM, STEPWISE_MIXED_GPU = (MIXED_FLUX, 1e-6), (MIXED_FLUX, 2e-6)
STEPWISE_LITERAL_STEPS = 600  # the literal line searches take ~100x the evaluations: the head of the long fixtures
GRADIENT, GRADIENT_LOSS = 1e-6, 1e-9  # |got - ref| against max |ref| of the parameter kind; the loss, relative
ORACLE_TOTAL_FLOOR = 1e-3  # cm: run totals of an ensemble column against the oracle's


# ---- fixtures ----------------------------------------------------------------------------------------------------------
def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def engine_keywords(g):
    """LgarEngine's keyword settings for the run a golden fixture (an opened .npz) records."""
    return dict(dt_h=float(g["dt_h"]), num_subcycles=int(g["num_subcycles"]), ponded_depth_max=float(g["pdm"]),
                initial_psi=float(g["initial_psi"]), wilting_point_psi=float(g["wilting_point_psi"]),
                frozen_factor=float(g["frozen_factor"]), nint=int(g["nint"]), giuh_ordinates=tuple(g["giuh_ordinates"]),
                use_closed_form_G=bool(g["closed_form"]) if "closed_form" in g.files else False)


def soil(g):
    """LgarEngine's positional arguments: a column of the fixture's soil."""
    return tuple(g[k] for k in ("alpha", "n", "ksat", "theta_e", "theta_r", "thickness"))


def steps_before_crash(g, cap=None):
    """(crash, T): the step at which the reference raised (-1: it did not) and the steps it completed (at most `cap`)."""
    crash = int(g["crash_step"])
    T = crash if crash >= 0 else g["forcing"].shape[0]
    return crash, T if cap is None else min(T, cap)


def rel(a, b, floor=REL_FLOOR):
    return np.abs(a - b) / np.maximum(np.abs(b), floor)


def to_numpy(x):
    """An engine's tensors (one, or the dict / tuple forward() / tangent() return) as numpy arrays for the checks."""
    if isinstance(x, dict):
        return {k: to_numpy(v) for k, v in x.items()}
    if isinstance(x, tuple):
        return tuple(to_numpy(v) for v in x)
    return x if x is None or isinstance(x, np.ndarray) else x.cpu().numpy()


def replicated_forcing(g, ncol, sl=slice(None), device=None):
    """The fixture's forcing rows `sl` for ncol identical columns: (precip, pet), contiguous [T, ncol] fp64 tensors."""
    import torch
    f = torch.tensor(g["forcing"][sl], device=device)
    T = f.shape[0]
    return f[:, 0:1].expand(T, ncol).contiguous(), f[:, 1:2].expand(T, ncol).contiguous()


def reference_gradients(g):
    """{kind: d loss / d kind [L]} in the engine's convention: None in the reference (no dependence, stored as NaN) is 0, and
    d_ksat is scaled by frozen_factor -- the reference's Parameter is Ksat x frozen_factor (models/dpLGAR.py:57), the engine's
    input is Ksat."""
    ref = {k: np.nan_to_num(g["d_" + k], nan=0.0) for k in ("alpha", "n", "ksat")}
    ref["ksat"] = ref["ksat"] * float(g["frozen_factor"])
    return ref


# ---- checks ------------------------------------------------------------------------------------------------------------
def _within(what, err, bar):
    """err <= bar everywhere (a NaN fails), or an AssertionError naming the worst element."""
    err = np.asarray(err, dtype=np.float64)
    if not (err <= bar).all():
        i = np.unravel_index(int(np.argmax(np.where(np.isnan(err), np.inf, err))), err.shape)
        raise AssertionError("%s: %.3e at index %s exceeds the bar %.1e" % (what, err[i], tuple(int(j) for j in i), bar))


def _same(what, got, want):
    """got == want element by element, or an AssertionError naming the first difference."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        raise AssertionError("%s: shape %s, expected %s" % (what, got.shape, want.shape))
    bad = ~(got == want)
    if bad.any():
        i = tuple(int(j) for j in np.argwhere(bad)[0])
        raise AssertionError("%s: %r at index %s, expected %r (%d of %d differ)" % (what, got[i], i, want[i], bad.sum(), bad.size))


def check_accumulators(g, acc, T, bar=NATIVE):
    """acc [T, NACC]: a column's per-step accumulators against the reference's."""
    _within("per-step accumulators [step, accumulator]", rel(acc, g["acc"][:T]), bar)


def check_replicated(what, x, axis=1):
    """Replicated columns (along `axis`) must be bit-identical."""
    x = np.asarray(x)
    _same(what + ": replicated columns", x, np.broadcast_to(np.take(x, [0], axis), x.shape))


def check_clean(status):
    _same("status", status, np.zeros_like(status))


def check_initial_volume(g, volume):
    _within("initial volume (absolute, cm)", abs(float(volume) - float(g["init_volume"])), INIT_VOLUME)


def check_last_front_table(g, fr, T, derived=True):
    """fr: LgarEngine.fronts() after step T - 1.  Front count in every column; depth, theta, layer tags and to_bottom of column
    0 -- and psi, K, dz/dt unless derived=False (the mixed mode's bars cover depth, theta and the tags only)."""
    nf = int(g["nfronts"][T - 1])
    _same("n_fronts after step %d" % (T - 1), fr["n_fronts"], np.full_like(fr["n_fronts"], nf))
    ref = g["fronts"][T - 1, :nf]
    for j, (key, floor, bar) in enumerate((("depth", REL_FLOOR, NATIVE), ("theta", REL_FLOOR, NATIVE), ("psi", PSI_FLOOR, DERIVED),
                                           ("k", K_FLOOR, DERIVED), ("dzdt", DZDT_FLOOR, DERIVED))):
        if j < 2 or derived:
            _within("last front table, %s [front]" % key, rel(fr[key][:nf, 0], ref[:, j], floor), bar)
    _same("last front table, layer", fr["layer"][:nf, 0], g["front_layer"][T - 1, :nf])
    _same("last front table, to_bottom", fr["to_bottom"][:nf, 0], g["front_bottom"][T - 1, :nf])


def check_totals(g, totals, T, call_sums=None):
    """Rows 0-7 of a column's run totals (what MassBalance accumulates) -- and of the per-call sums the model surface reads."""
    ref = g["acc"][:T, :8].sum(0)
    _within("run totals [accumulator]", rel(totals[:8], ref), NATIVE)
    if call_sums is not None:
        _within("call_sums [accumulator]", rel(call_sums[:8], ref), NATIVE)


def mixed_totals_error(tot, ref):
    """Rows 0-7 of the mixed mode's run totals ([8] or [8, N]) against the column's water input."""
    return np.abs(tot[:8] - ref[:8]) / np.maximum(np.maximum(np.abs(ref[:8]), ref[0:1]), 1e-2)


def mixed_mode_check(acc, ref, T):
    """acc, ref: [T, NACC] per-step outputs of the mixed mode and of the reference"""
    scale = np.maximum(np.maximum(ref[:, 0:1] + ref[:, 8:9], np.abs(ref)), 1e-3)
    _within("mixed mode, per-step outputs against the step's water [step, accumulator]", np.abs(acc - ref) / scale, MIXED_FLUX)
    _within("mixed mode, per-step backstop [step, accumulator]", rel(acc, ref), MIXED_STEP_BACKSTOP)
    _within("mixed mode, run totals [accumulator]", mixed_totals_error(acc[:, :8].sum(0), ref[:, :8].sum(0)), MIXED_TOTAL)


def check_native_trajectory(g, run):
    """Everything a native fp64 run_trajectory() result owes the fixture."""
    T = run["T"]
    check_initial_volume(g, run["init_volume"])
    check_accumulators(g, run["acc"][:, 0], T)
    check_replicated("per-step accumulators", run["acc"])
    check_clean(run["status"])
    check_last_front_table(g, run["fronts"], T)
    check_totals(g, run["totals"][:, 0], T, None if run["call_sums"] is None else run["call_sums"][:, 0])


def check_mixed_trajectory(g, run):
    T = run["T"]
    check_replicated("per-step accumulators", run["acc"])
    mixed_mode_check(run["acc"][:, 0], g["acc"][:T], T)
    check_clean(run["status"])
    check_last_front_table(g, run["fronts"], T, derived=False)


def check_crash_step(g, status, raised=True):
    """After the row at which the reference raised: every column flagged with the fault kind of what it raised, and
    forward(check=True) raised LgarStatusError."""
    status = np.asarray(status)
    if (status == 0).any():
        raise AssertionError("crash step %d: column %d of %d is not flagged" % (int(g["crash_step"]), int(np.argmin(status != 0)), status.size))
    check_fault_kind(g, status)
    if not raised:
        raise AssertionError("crash step %d: forward() did not raise LgarStatusError" % int(g["crash_step"]))


def check_front_table_at_every_step(g, rec, T, bar, usual):
    """rec: run_row_by_row()'s recording of column 0 -- depth / theta / flags [T, F], n_fronts [T] -- with the final status and
    the final depth / theta of all columns.  Front count, layer tags and to_bottom exact at every step; depth and theta within
    `bar` at every step and within `usual` at all but max(1, T // 50) of them; status 0; replicated columns bit-equal."""
    check_clean(rec["status"])
    check_replicated("final depth", rec["final_depth"])
    check_replicated("final theta", rec["final_theta"])
    Z, TH, FL, NF = rec["depth"], rec["theta"], rec["flags"], rec["n_fronts"]
    _same("n_fronts [step]", NF, g["nfronts"][:T])
    frec = min(g["fronts"].shape[1], Z.shape[1])
    live = np.arange(frec)[None, :] < np.minimum(NF, frec)[:, None]
    _same("layer tags [step, front]", np.where(live, FL[:, :frec] & 0x7F, 0), np.where(live, g["front_layer"][:T, :frec], 0))
    _same("to_bottom [step, front]", np.where(live, FL[:, :frec] >> 7, 0), np.where(live, g["front_bottom"][:T, :frec], 0))
    err = np.maximum(rel(Z[:, :frec], g["fronts"][:T, :frec, 0]), rel(TH[:, :frec], g["fronts"][:T, :frec, 1]))
    _within("front table depth / theta [step, front]", np.where(live, err, 0.0), bar)
    above = np.nonzero(np.where(live, err, 0.0).max(axis=1) > usual)[0]
    if len(above) > max(1, T // 50):
        raise AssertionError("front table: %d of %d steps above the usual %.1e (allowed: %d); the first is step %d"
                             % (len(above), T, usual, max(1, T // 50), int(above[0])))


def check_oracle_agreement(o, status, runoff=None, totals=None, bar=NATIVE, cols=None, flips=None, scale=None, mixed=False):
    """An engine against oracle_ensemble()'s results o.  Same columns flagged (flips: a set of columns that may differ; None:
    flags are not compared); per-step runoff [T, N] within bar * scale (default max(1, max |oracle runoff|)) and rows 0-7 of
    the totals [NACC, N] within `bar`, relative with a 1e-3 cm floor, on the columns `cols` (default: the ones the oracle
    finishes).  mixed: the mixed mode's bars and its totals scale instead."""
    st = o["st"]
    if flips is not None:
        differ = set(int(i) for i in np.nonzero((st != 0) != (np.asarray(status) != 0))[0])
        if not differ <= set(flips):
            raise AssertionError("fault flags differ from the oracle's on columns %s" % sorted(differ - set(flips))[:20])
    ok = st == 0 if cols is None else cols
    if runoff is not None:
        scale = max(1.0, np.abs(o["ro"]).max()) if scale is None else scale
        _within("runoff against the oracle [step, valid column]", np.abs(runoff - o["ro"])[:, ok] / scale, MIXED_FLUX if mixed else bar)
    if totals is not None and mixed:
        _within("run totals against the oracle [accumulator, valid column]", mixed_totals_error(totals, o["acc"])[:, ok], MIXED_TOTAL)
    elif totals is not None:
        _within("run totals against the oracle [accumulator, valid column]",
                rel(totals[:8], o["acc"][:8], ORACLE_TOTAL_FLOOR)[:, ok], bar)


def check_gradients(g, loss, grads):
    """loss = mean(runoff^2) and {kind: d loss / d kind [L]} against the reference's own loss.backward()."""
    _within("loss (absolute)", abs(float(loss) - float(g["loss"])), GRADIENT_LOSS * float(g["loss"]))
    for kind, ref in reference_gradients(g).items():
        _within("d loss / d %s (absolute) [layer]" % kind, np.abs(grads[kind] - ref), GRADIENT * np.abs(ref).max())


def check_bit_identical(a, b, fields=None, label=""):
    """Two engines' outputs and state (dicts of arrays, see outputs_and_state) bit for bit over `fields` (default: all of a's)."""
    for f in a if fields is None else fields:
        _same(label + f, b[f], a[f])


# ---- runners -----------------------------------------------------------------------------------------------------------
def outputs_and_state(eng, out, fields):
    """forward()'s result and the named state tensors of the engine in one dict of numpy arrays."""
    return dict(to_numpy(out), **{f: to_numpy(getattr(eng, f)) for f in fields})


def run_trajectory(make_engine, g, ncol, call_sums=False, **kw):
    """ncol replicated columns over the steps the reference completed, one launch.  acc: [T, ncol, NACC]."""
    from lgar_py_amd import ACC_NAMES
    crash, T = steps_before_crash(g)
    eng = make_engine(g, ncol, **kw)
    init_volume = float(eng.ending_volume[0])
    pr, pe = replicated_forcing(g, ncol, slice(0, T))
    out = to_numpy(eng.forward(pr, pe, series=ACC_NAMES, **(dict(call_sums=True) if call_sums else {})))
    return dict(eng=eng, T=T, crash=crash, init_volume=init_volume, acc=np.stack([out[nm] for nm in ACC_NAMES], 2),
                call_sums=out.get("call_sums"), status=to_numpy(eng.status), fronts=eng.fronts(), totals=to_numpy(eng.totals))


def run_crash_row(eng, g, ncol):
    """The row at which the reference raised, with forward()'s own check on: (status, whether LgarStatusError was raised)."""
    from lgar_py_amd import LgarStatusError
    T = int(g["crash_step"])
    pr, pe = replicated_forcing(g, ncol, slice(T, T + 1))
    try:
        eng.forward(pr, pe, check=True)
    except LgarStatusError:
        return to_numpy(eng.status), True
    return to_numpy(eng.status), False


def trajectory_vs_reference(make_engine, name, ncol, check, **kw):
    """The contract of a trajectory fixture: run_trajectory() passes `check` (check_native_trajectory or
    check_mixed_trajectory), and if the reference raised at the next row, every column faults there too."""
    g = load(name)
    run = run_trajectory(make_engine, g, ncol, **kw)
    check(g, run)
    if run["crash"] >= 0:
        check_crash_step(g, *run_crash_row(run["eng"], g, ncol))


def run_row_by_row(make_engine, g, ncol, T, **kw):
    """The engine stepped ONE forcing row per call; the whole front table of column 0 after every step is recorded into
    preallocated tensors on the engine's device and brought to the host once, at the end (no host synchronisation per step)."""
    import torch
    eng = make_engine(g, ncol, **kw)
    dev = eng.device
    pr, pe = replicated_forcing(g, ncol, slice(0, T), device=dev)
    F = eng.depth.shape[0]
    Z = torch.empty(T, F, dtype=torch.float64, device=dev)
    TH = torch.empty(T, F, dtype=torch.float64, device=dev)
    FL = torch.empty(T, F, dtype=torch.uint8, device=dev)
    NF = torch.empty(T, dtype=torch.int32, device=dev)
    for t in range(T):
        eng.forward(pr[t:t + 1], pe[t:t + 1], series=(), check=False)
        Z[t], TH[t], FL[t], NF[t] = eng.depth[:, 0], eng.theta[:, 0], eng.flags[:, 0], eng.n_fronts[0]
    return to_numpy(dict(depth=Z, theta=TH, flags=FL, n_fronts=NF, status=eng.status, final_depth=eng.depth, final_theta=eng.theta))


def run_lanes_pair(make_engine, g, ncol, lanes, fields, **kw):
    """The fixture's whole run with one lane per column and with `lanes` cooperating lanes: two outputs_and_state() dicts."""
    from lgar_py_amd import ACC_NAMES
    res = []
    for k in (1, lanes):
        eng = make_engine(g, ncol, forward_lanes=k, **kw)
        pr, pe = replicated_forcing(g, ncol)
        res.append(outputs_and_state(eng, eng.forward(pr, pe, series=ACC_NAMES, check=False), fields))
    return res


def oracle_ensemble(N, seed, scale=None, wide=False, hourly_steps=0):
    """N columns -- W.perturbed_columns(N, seed), or W.ensemble_columns(N, seed) if wide -- under the synth_1 storm (5-minute
    steps, no ponding, no PET) or, with hourly_steps, under that many rows of phil_hourly_3000 (hourly, 2 cm ponding, PET), the
    rain of every column scaled by W.forcing_scale(N, *scale), and what the oracle makes of them: dict with cols (the engine's
    positional arguments), kw (its dt_h / ponded_depth_max), pr, pe [T, N], and the oracle's ro [T, N], acc [NACC, N], st [N]."""
    from lgar_py_amd import workloads as W
    from oracle import lgar_oracle as O
    P = (W.ensemble_columns if wide else W.perturbed_columns)(N, seed=seed)
    sc = np.ones(N) if scale is None else W.forcing_scale(N, *scale[:-1], seed=scale[-1])
    f, dt_h, pdm = (load("phil_hourly_3000")["forcing"][:hourly_steps], 1.0, 2.0) if hourly_steps else (W.synth1_forcing(), 300.0 / 3600.0, 0.0)
    pr = f[:, 0:1] * sc[None, :]
    pe = f[:, 1:2] * np.ones((1, N)) if hourly_steps else np.zeros_like(pr)
    cols = tuple(P[k] for k in ("alpha", "n", "ksat", "theta_e", "theta_r", "thickness"))
    ro, pc, acc, st = O.run_columns(*cols, pr, pe, pdm=pdm, dt_h=dt_h)
    return dict(cols=cols, kw=dict(dt_h=dt_h, ponded_depth_max=pdm), pr=pr, pe=pe, ro=ro, acc=acc, st=st)
