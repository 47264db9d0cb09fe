"""TEST INFRASTRUCTURE ONLY: the host build of the snowpack's forward-mode tangent (lgar_catchment_snow_tangent: sn_walk_tangent of
lgar_py_amd/csrc/lgar_snow.hpp under -DLGAR_DEVSIM) as a library and as a stand-alone program (also built with AddressSanitizer +
UBSan), the numpy statement of the recurrence (snow_tangent_ref; `absolute`: the same recurrence on absolute values, every
difference a sum, which bounds what rounding can do; `variant`: the WRONG tangents the bound must refuse) and SimSnow: the product's
CatchmentSnow over the two host builds.  The forward, the adjoint, the data and the regimes are tests/snow_host's.  Never imported
by the product package."""
import ctypes as C
import os

import numpy as np

import _hostbuild
import snow_host as SH
from _hostbuild import f64, out, same_bits  # noqa: F401
from lgar_py_amd.snow import CatchmentSnow

_HERE = os.path.dirname(os.path.abspath(__file__))
UNIT = _hostbuild.HostUnit(_HERE, "snow_tangent_host", "snowtanhost", ["lgar_snow.hpp"], "snow-tangent")


def library():
    i32, vp, dbl = C.c_int32, C.c_void_p, C.c_double
    return UNIT.library({"catchment_snow_tangent": [vp, vp, i32, i32, vp, dbl, vp, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp]})


def snow_tangent_ref(p, ta, par, dt_h, state, D, dp=None, dta=None, dpar=None, dstate=None, absolute=False, variant=None):
    """(dw [T, B, D], dice [D, T, B], dliq [D, T, B], dstate_out [D, 2, B]): the recurrence of lgar_snow.hpp, one numpy operation
    for one of the header's, the directions and cells side by side.  absolute: inputs by their absolute values, every difference a
    sum, the values' factors by their absolute values.  variant: "no_cwh_ice2" (cwh * ice2' dropped from cap'), "refr_sign" (refr'
    enters ice2' and liq1' with the wrong sign), "no_fr" (fr' = 0)."""
    p, ta = np.asarray(p, dtype=np.float64), np.asarray(ta, dtype=np.float64)
    T, B = p.shape
    dt = np.float64(dt_h)
    A = np.abs if absolute else (lambda x: x)
    sub = (lambda x, y: x + y) if absolute else (lambda x, y: x - y)
    z = lambda x, shape: np.zeros(shape) if x is None else A(np.asarray(x, dtype=np.float64))
    dp, dta, dpar, dstate = z(dp, (D, T, B)), z(dta, (D, T, B)), z(dpar, (D, 7, B)), z(dstate, (D, 2, B))
    c, ice, liq = SH._start(par, dt_h, state, B)
    dtlo, dthi, dtm, dsfcf, dcfmax, dcfr, dcwh = (dpar[:, j] for j in range(7))
    dice, dliq = dstate[:, 0].copy(), dstate[:, 1].copy()
    dw, si, sl = np.zeros((T, B, D)), np.zeros((D, T, B)), np.zeros((D, T, B))
    with np.errstate(all="ignore"):
        dcd = dcfmax * dt
        dcr = dcfr * A(c["cd"]) + A(c["cfr"]) * dcd
        dspan = sub(dthi, dtlo)
        for t in range(T):
            pd = p[t] * dt
            o = SH._step(ice, liq, pd, ta[t], c)
            mid = ~o["lo"] & ~o["hi"]
            dpd = dp[:, t] * dt
            q = sub(sub(dta[:, t], dtlo), A(o["fr"]) * dspan) / A(c["span"])
            dfr = np.zeros_like(q) if variant == "no_fr" else np.where(mid, q, 0.0)
            drain = dpd * A(o["fr"]) + A(pd) * dfr
            ddry = sub(dpd, drain)
            dsnow = dsfcf * A(o["dry"]) + A(c["sfcf"]) * ddry
            dd = sub(dta[:, t], dtm)
            dice1 = dice + dsnow
            dpm = dcd * A(o["d"]) + A(c["cd"]) * dd
            dmelt = np.where(o["warm"], np.where(o["ml"], dice1, dpm), 0.0)
            dpr = sub(dcr * A(-o["d"]), A(c["cr"]) * dd)
            drefr = np.where(o["warm"], 0.0, np.where(o["rl"], dliq, dpr))
            if variant == "refr_sign":
                dice2, dliq1 = (dice1 - dmelt) - drefr, ((dliq + drain) + dmelt) + drefr
            else:
                dice2, dliq1 = sub(dice1, dmelt) + drefr, sub((dliq + drain) + dmelt, drefr)
            dcap = (dcwh * A(o["ice2"]) if variant == "no_cwh_ice2" else dcwh * A(o["ice2"]) + A(c["cwh"]) * dice2)
            dout = np.where(o["over"], sub(dliq1, dcap), 0.0)
            dliq = np.where(o["over"], dcap, dliq1)
            dice = dice2
            ice, liq = o["ice"], o["liq"]
            dw[t] = (dout / dt).T
            si[:, t], sl[:, t] = dice, dliq
    return dw, si, sl, np.stack([dice, dliq], axis=1)


def call(p, ta, par, dt_h, state, D, dp=None, dta=None, dpar=None, dstate=None, ld=None, k0=0, want_pack=True, want_state=True, fill=7.5):
    """The host library on numpy arrays: (rc, dw block [T, B, ld] that held `fill` everywhere before, dice, dliq, dstate_out)."""
    T, B = np.asarray(p).shape
    ld = k0 + D if ld is None else ld
    keep = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (p, ta, par, state, dp, dta, dpar, dstate)]
    dw = np.full((T, B, ld), fill)
    dice, dliq = (np.full((D, T, B), np.nan), np.full((D, T, B), np.nan)) if want_pack else (None, None)
    dso = np.full((D, 2, B), np.nan) if want_state else None
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data
    rc = library().snowtanhost_catchment_snow_tangent(ptr(keep[0]), ptr(keep[1]), T, B, ptr(keep[2]), float(dt_h), ptr(keep[3]), D, ptr(keep[4]),
                                                      ptr(keep[5]), ptr(keep[6]), ptr(keep[7]), ptr(dw), ld, k0, ptr(dice), ptr(dliq), ptr(dso))
    return rc, dw, dice, dliq, dso


def run_program(cases, sanitize=False):
    """ONE run of the stand-alone program over (p, ta, par, dt_h, state, D, dp, dta, dpar, dstate, ld, k0) cases: [(dw, dice, dliq,
    dstate_out)]; dw starts as zeros."""
    calls, results = [], []
    for p, ta, par, dt_h, state, D, dp, dta, dpar, dstate, ld, k0 in cases:
        T, B = np.asarray(p).shape
        dw = _hostbuild.Out(np.float64, T, B, ld, start=np.zeros((T, B, ld)))
        o = (dw, out(True, D, T, B), out(True, D, T, B), out(True, D, 2, B))
        calls.append((0, (T, B, D, ld, k0), (dt_h,), (f64(p), f64(ta), f64(par), f64(state), f64(dp), f64(dta), f64(dpar), f64(dstate)) + o))
        results.append(o)
    UNIT.run_calls(calls, sanitize)
    return [_hostbuild.values(r) for r in results]


class SimSnow(CatchmentSnow):
    """lgar_py_amd.snow.CatchmentSnow (device="cpu") over the host builds: the tangent on this package's, the rest on snow_host's."""

    def __init__(self, tlo, thi, tm, sfcf, cfmax, cfr, cwh, dt_h, n_catchments=None, device="cpu"):
        super().__init__(tlo, thi, tm, sfcf, cfmax, cfr, cwh, dt_h, device="cpu", n_catchments=n_catchments)

    @classmethod
    def _open(cls, device):
        return _hostbuild.AsHipLibrary(("catchment_snow_tangent", "snowtanhost", library), ("", "snowhost", SH.library))


# ---- the bodies the host suite and the GPU suite share --------------------------------------------------------------------
SHAPE_B, SHAPE_T, SHAPE_D = (1, 2, 63, 64, 65, 257), (0, 1, 9, 17), (1, 3, 7)
LAYOUTS = ((0, 0), (3, 2))  # (ld - D, k0): the block is exactly the directions, or wider with the directions inside it


def directions(rng, D, T, B):
    """dp, dta [D, T, B], dpar [D, 7, B], dstate [D, 2, B] of mixed signs and magnitudes"""
    mixed = lambda *shape: (rng.random(shape) - 0.4) * 10.0 ** rng.integers(-2, 2, shape)
    return mixed(D, T, B), mixed(D, T, B), mixed(D, 7, B), mixed(D, 2, B)


def statement_product(call, B, seed=2018):
    """For one B: T in {0, 1, 9, 17} x D in {1, 3, 7} x EVERY combination of (dp, dta, dpar, dstate_in NULL or given) x (pack
    wanted or not) x (end state wanted or not) x both (ld, k0) -- (D, 0) and (D + 3, 2) -- and, crossed with all of it, the
    value state given or NULL: 12 x 64 x 2 x 2 calls of `call` (ST.call's arguments and results), each bit for bit against
    snow_tangent_ref (evaluated once per shape, input combination and state); the elements of dw outside k0 .. k0 + D keep what
    they held; T = 0 copies dstate.  Section 19's cell mix (snow_host.case_data).  Returns (calls made, rows per regime, rows
    per tie) of the data used, for the caller to hold."""
    import itertools
    rng = np.random.default_rng(seed + B)
    calls, reg_total, tie_total = 0, dict.fromkeys(SH.REGIMES, 0), dict.fromkeys(SH.TIES, 0)
    for T, D in itertools.product(SHAPE_T, SHAPE_D):
        p, ta, _, _, _, par, state, dt = SH.case_data(rng, T, B)
        reg, tie, _, _ = SH.regimes(p, ta, par, dt, state)
        for k in reg:
            reg_total[k] += reg[k]
        for k in tie:
            tie_total[k] += tie[k]
        dirs = directions(rng, D, T, B)
        for st in (state, None):
            for use in itertools.product((0, 1), repeat=4):
                given = [d if u else None for d, u in zip(dirs, use)]
                want = snow_tangent_ref(p, ta, par, dt, st, D, *given)
                for pack, end, (extra, k0) in itertools.product((False, True), (False, True), LAYOUTS):
                    ld = D + extra
                    rc, dw, dice, dliq, dso = call(p, ta, par, dt, st, D, *given, ld=ld, k0=k0, want_pack=pack, want_state=end)
                    calls += 1
                    where = (B, T, D, use, st is None, pack, end, ld, k0)
                    assert rc == 0 and same_bits(dw[:, :, k0:k0 + D], want[0]), where
                    assert (dw[:, :, :k0] == 7.5).all() and (dw[:, :, k0 + D:] == 7.5).all(), where
                    assert (dice is None) == (not pack) and (dso is None) == (not end), where
                    if pack:
                        assert same_bits(dice, want[1]) and same_bits(dliq, want[2]), where
                    if end:
                        assert same_bits(dso, want[3]), where
                        if T == 0:
                            assert same_bits(dso, np.zeros((D, 2, B)) if given[3] is None else given[3]), where
    return calls, reg_total, tie_total


def nan_confinement(call, which):
    """A NaN in one input tangent of (direction 1, cell 5) (row 4 for the series) reaches nothing of another cell or another
    direction, and nothing of its own lane before its row; a NaN in dp or dstate stays in its own lane's pack tangent (one in
    Ta' or a parameter's tangent may be discarded by the row's selects, as in the forward)."""
    rng = np.random.default_rng(9)
    B, T, D = 9, 12, 3
    p, ta, _, _, _, par, state, dt = SH.case_data(rng, T, B)
    dirs = list(directions(rng, D, T, B))
    clean = call(p, ta, par, dt, state, D, *dirs)
    i = ["dp", "dta", "dpar", "dstate"].index(which)
    dirs[i] = dirs[i].copy()
    if i < 2:
        dirs[i][1, 4, 5] = np.nan
    else:
        dirs[i][1, :, 5] = np.nan
    rc, dw, dice, dliq, dso = call(p, ta, par, dt, state, D, *dirs)
    own = np.zeros((D, T, B), dtype=bool)
    own[1, (4 if i < 2 else 0):, 5] = True
    assert same_bits(dice[~own], clean[2][~own]) and same_bits(dliq[~own], clean[3][~own])
    assert same_bits(dw.transpose(2, 0, 1)[~own], clean[1].transpose(2, 0, 1)[~own])
    if which in ("dp", "dstate"):
        assert np.isnan(dice[own] + dliq[own]).any()
