"""TEST INFRASTRUCTURE ONLY: the host build of the catchment-snowpack header (lgar_py_amd/csrc/lgar_snow.hpp, compiled for the host
with -DLGAR_DEVSIM) and its front-end.  snow_host.hpp holds the host-side launchers of the two entry points; snow_host.cpp is the
stand-alone program around them (run() below; also built with AddressSanitizer + UBSan), libsnowhost.so the same header as a
shared library (library(): what SimCatchmentSnow puts behind the product's calling surface).  The numpy statement of the
definition (include/lgar.h, lgar_catchment_snow / lgar_catchment_snow_grad) -- snow_ref, snow_grad_ref and
regimes: plain loops over rows, the cells side by side -- and the data of the tests' cases live here too.
The build, the program's call records (tests/_hostprog.hpp) and same_bits are tests/_hostbuild.py's: UNIT below.
Never imported by the product package.
"""
import ctypes as C
import os

import numpy as np

import _hostbuild
from _hostbuild import f64, out, same_bits  # noqa: F401
from lgar_py_amd.snow import CatchmentSnow

_HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE_B = (1, 2, 63, 64, 65, 257)
SHAPE_T = (0, 1, 2, 7, 8, 9, 17)  # around the row chunk of 8
TLO, THI, TM, SFCF, CFMAX, CFR, CWH = range(7)  # the rows of par
REGIMES = ("lo", "mid", "hi", "melt_limited", "melt_free", "refreeze_limited", "refreeze_free", "over", "hold", "step")
TIES = ("Ta==tlo", "Ta==thi", "d==0", "pm==ice1", "pr==liq", "liq1==cap")
TIE_CELLS = {name: 16 + k for k, name in enumerate(TIES)}  # the cells case_data plants the ties in (row 0, with the state given)


# ---- the definition, in numpy ----------------------------------------------------------------------------------------------
def _start(par, dt_h, state, B):
    """the parameters as the rows use them (cd, cr and span rounded once), and the pack before row 0"""
    par = np.asarray(par, dtype=np.float64)
    c = dict(tlo=par[TLO], thi=par[THI], tm=par[TM], sfcf=par[SFCF], cfr=par[CFR], cwh=par[CWH])
    c["cd"] = par[CFMAX] * np.float64(dt_h)
    c["cr"] = c["cfr"] * c["cd"]
    c["span"] = c["thi"] - c["tlo"]
    if state is None:
        return c, np.zeros(B), np.zeros(B)
    state = np.asarray(state, dtype=np.float64)
    return c, state[0].copy(), state[1].copy()


def _step(ice, liq, pd, Ta, c):
    """One row of the definition, one numpy operation for one of the header's: a dict of every value and flag."""
    lo = Ta <= c["tlo"]
    hi = ~lo & (Ta >= c["thi"])
    fr = np.where(lo, 0.0, np.where(hi, 1.0, (Ta - c["tlo"]) / c["span"]))
    rain = pd * fr
    dry = pd - rain
    snow = c["sfcf"] * dry
    d = Ta - c["tm"]
    warm = d > 0.0
    ice1 = ice + snow
    pm = c["cd"] * d
    ml = pm > ice1
    melt = np.where(warm, np.where(ml, ice1, pm), 0.0)
    pr = c["cr"] * (-d)
    rl = pr > liq
    refr = np.where(warm, 0.0, np.where(rl, liq, pr))
    ice2 = (ice1 - melt) + refr
    liq1 = ((liq + rain) + melt) - refr
    cap = c["cwh"] * ice2
    over = liq1 > cap
    out = np.where(over, liq1 - cap, 0.0)
    return dict(lo=lo, hi=hi, fr=fr, rain=rain, dry=dry, d=d, warm=warm, ice1=ice1, pm=pm, ml=ml, pr=pr, rl=rl, ice2=ice2, liq1=liq1,
                cap=cap, over=over, out=out, ice=ice2, liq=np.where(over, cap, liq1), liq_in=liq)


def snow_ref(p, ta, par, dt_h, state=None):
    """(w [T, B], ice [T, B], liq [T, B], state_out [2, B]): the rows in ascending order."""
    p, ta = np.asarray(p, dtype=np.float64), np.asarray(ta, dtype=np.float64)
    T, B = p.shape
    dt = np.float64(dt_h)
    c, ice, liq = _start(par, dt_h, state, B)
    w, si, sl = np.zeros((T, B)), np.zeros((T, B)), np.zeros((T, B))
    with np.errstate(all="ignore"):
        for t in range(T):
            o = _step(ice, liq, p[t] * dt, ta[t], c)
            w[t], si[t], sl[t] = o["out"] / dt, o["ice"], o["liq"]
            ice, liq = o["ice"], o["liq"]
    return w, si, sl, np.stack([ice, liq])


def regimes(p, ta, par, dt_h, state=None):
    """(rows per regime, rows per exact tie, [T, B] bool maps of both) of a run.  The regimes: lo / mid / hi of the rain-snow
    transition; melt limited by the ice or free (warm rows); refreeze limited by the held liquid or free (the other rows); over
    (water leaves) or hold; step = a row of a cell with tlo == thi.  A tie counts where it decides: pm == ice1 in a warm row,
    pr == liq in a row that is not warm."""
    p, ta = np.asarray(p, dtype=np.float64), np.asarray(ta, dtype=np.float64)
    T, B = p.shape
    c, ice, liq = _start(par, dt_h, state, B)
    reg = {k: np.zeros((T, B), dtype=bool) for k in REGIMES}
    tie = {k: np.zeros((T, B), dtype=bool) for k in TIES}
    with np.errstate(all="ignore"):
        for t in range(T):
            o = _step(ice, liq, p[t] * np.float64(dt_h), ta[t], c)
            mid = ~o["lo"] & ~o["hi"]
            for k, v in (("lo", o["lo"]), ("mid", mid), ("hi", o["hi"]), ("melt_limited", o["warm"] & o["ml"]), ("melt_free", o["warm"] & ~o["ml"]),
                         ("refreeze_limited", ~o["warm"] & o["rl"]), ("refreeze_free", ~o["warm"] & ~o["rl"]), ("over", o["over"]),
                         ("hold", ~o["over"]), ("step", c["span"] == 0.0)):
                reg[k][t] = v
            for k, v in (("Ta==tlo", ta[t] == c["tlo"]), ("Ta==thi", ta[t] == c["thi"]), ("d==0", o["d"] == 0.0), ("pm==ice1", o["warm"] & (o["pm"] == o["ice1"])),
                         ("pr==liq", ~o["warm"] & (o["pr"] == o["liq_in"])), ("liq1==cap", o["liq1"] == o["cap"])):
                tie[k][t] = v
            ice, liq = o["ice"], o["liq"]
    return {k: int(v.sum()) for k, v in reg.items()}, {k: int(v.sum()) for k, v in tie.items()}, reg, tie


def snow_grad_ref(gw, gice, gliq, p, ta, ice, liq, par, dt_h, state=None, variant=None):
    """(gp [T, B], gta [T, B], gpar [7, B], gstate [2, B]): the rows in descending order, each re-formed from the stored pack of
    the row before; every accumulator from +0.0, left as it is in a row that gives it no term.  variant: one of the WRONG adjoints
    the bound test must refuse -- "no_dcap" (dcap dropped from di2), "refr_sign" (the refreeze cotangent with the wrong sign:
    drefr = dl1 - di2), "gice_late" (gice added after the row instead of before), "no_mid" (the mid quotient missing from gta)."""
    gw, p, ta, ice, liq = (np.asarray(a, dtype=np.float64) for a in (gw, p, ta, ice, liq))
    T, B = p.shape
    gice = np.zeros((T, B)) if gice is None else np.asarray(gice, dtype=np.float64)
    gliq = np.zeros((T, B)) if gliq is None else np.asarray(gliq, dtype=np.float64)
    dt = np.float64(dt_h)
    c, ice0, liq0 = _start(par, dt_h, state, B)
    gp, gta = np.zeros((T, B)), np.zeros((T, B))
    li, ll = np.zeros(B), np.zeros(B)
    gtlo, gthi, gtm, gsfcf, gcd, gcr, gcwh = (np.zeros(B) for _ in range(7))
    gcfmax, gcfr = np.zeros(B), np.zeros(B)
    with np.errstate(all="ignore"):
        span2 = c["span"] * c["span"]
        for t in range(T - 1, -1, -1):
            Ta, pd = ta[t], p[t] * dt
            o = _step(ice[t - 1] if t > 0 else ice0, liq[t - 1] if t > 0 else liq0, pd, Ta, c)
            mid = ~o["lo"] & ~o["hi"]
            wm, wf, cl, cf = o["warm"] & o["ml"], o["warm"] & ~o["ml"], ~o["warm"] & o["rl"], ~o["warm"] & ~o["rl"]
            if variant != "gice_late":
                li = li + gice[t]
            ll = ll + gliq[t]
            go = gw[t] / dt
            dl1 = np.where(o["over"], go, ll)
            dcap = np.where(o["over"], ll - go, 0.0)
            di2 = li if variant == "no_dcap" else li + c["cwh"] * dcap
            dmelt = dl1 - di2
            drefr = dl1 - di2 if variant == "refr_sign" else di2 - dl1
            di1 = np.where(wm, di2 + dmelt, di2)
            dliq = np.where(cl, dl1 + drefr, dl1)
            gd = np.where(wf, dmelt * c["cd"], np.where(cf, -(drefr * c["cr"]), 0.0))
            sd = c["sfcf"] * di1
            drain = dl1 - sd
            dpd = sd + drain * o["fr"]
            dfr = drain * pd
            gcwh = np.where(o["over"], gcwh + dcap * o["ice2"], gcwh)
            gcd = np.where(wf, gcd + dmelt * o["d"], gcd)
            gcr = np.where(cf, gcr + drefr * (-o["d"]), gcr)
            gtm = np.where(wf | cf, gtm - gd, gtm)
            gsfcf = gsfcf + di1 * o["dry"]
            gtlo = np.where(mid, gtlo + (dfr * (Ta - c["thi"])) / span2, gtlo)
            gthi = np.where(mid, gthi - (dfr * (Ta - c["tlo"])) / span2, gthi)
            gp[t] = dpd * dt
            gta[t] = gd if variant == "no_mid" else np.where(mid, gd + dfr / c["span"], gd)
            li, ll = di1, dliq
            if variant == "gice_late":
                li = li + gice[t]
        if T > 0:
            gcfmax = dt * (gcd + c["cfr"] * gcr)
            gcfr = c["cd"] * gcr
    return gp, gta, np.stack([gtlo, gthi, gtm, gsfcf, gcfmax, gcfr, gcwh]), np.stack([li, ll])


# ---- data ------------------------------------------------------------------------------------------------------------------
def case_data(rng, T, B):
    """p, ta, gw, gice, gliq [T, B], par [7, B], state [2, B], dt_h.  The cells take turns (b mod 8) so that every branch of the
    walk is taken somewhere: 0, 1 ordinary packs under a temperature that oscillates around the thresholds; 2 tlo == thi; 3 a
    large cfmax (melt limited by the ice); 4 a large cfr (refreeze limited by the held liquid); 5 cwh = 0; 6 a pack that never
    melts; 7 a NEGATIVE p in some rows and a negative initial liq, which only the raw entry points take.  A -0.0 stands in p.
    Cells 16 .. 21 (where B has them) hold in row 0, for the given state, the exact ties of TIES in this order."""
    kind = np.arange(B) % 8
    n = lambda k: int((kind == k).sum())
    dt = float(rng.choice([1.0, 0.25, 24.0]))
    tlo = rng.uniform(-2.0, 0.0, B)
    thi = tlo + rng.uniform(0.5, 3.0, B)
    tm = rng.uniform(-0.5, 1.0, B)
    sfcf = rng.uniform(0.8, 1.3, B)
    cfmax = rng.uniform(0.05, 0.3, B) / dt
    cfr = rng.uniform(0.02, 0.1, B)
    cwh = rng.uniform(0.02, 0.15, B)
    phase = rng.uniform(0.0, 6.28, B)
    ta = 4.0 * np.sin(phase[None, :] + 0.9 * np.arange(T)[:, None]) + rng.normal(0.0, 1.0, (T, B))
    p = rng.random((T, B)) * (rng.random((T, B)) < 0.6) * 10.0 ** rng.integers(-1, 1, (T, B)) / dt
    state = np.stack([rng.random(B) * 5.0, rng.random(B) * 0.3])
    thi[kind == 2] = tlo[kind == 2]
    cfmax[kind == 3] = rng.uniform(20.0, 50.0, n(3)) / dt
    cfr[kind == 4] = rng.uniform(5.0, 20.0, n(4))
    cwh[kind == 5] = 0.0
    ta[:, kind == 6] = -8.0 - 5.0 * rng.random((T, n(6)))
    p[:, kind == 7] = (rng.random((T, n(7))) - 0.3) / dt
    state[1, kind == 7] = -rng.random(n(7)) * 0.2
    if T:
        p[0, B // 2] = -0.0
        p[T - 1, 0] = -0.0
    if T and B > max(TIE_CELLS.values()):
        b = TIE_CELLS
        for k in b.values():  # plain cells: tlo = -1, thi = 2, tm = 0.5, cd = 2 dt, cr = dt (both exact), cwh = 0.5, a dry row 0
            tlo[k], thi[k], tm[k], sfcf[k], cfmax[k], cfr[k], cwh[k] = -1.0, 2.0, 0.5, 1.0, 2.0, 0.5, 0.5
            p[0, k], ta[0, k], state[0, k], state[1, k] = 0.0, -3.0, 4.0 * dt, dt
        ta[0, b["Ta==tlo"]], p[0, b["Ta==tlo"]] = -1.0, 1.0 / dt
        ta[0, b["Ta==thi"]], p[0, b["Ta==thi"]] = 2.0, 1.0 / dt
        ta[0, b["d==0"]] = 0.5
        ta[0, b["pm==ice1"]] = 2.5                                     # d = 2, pm = cd d = 4 dt = ice1
        ta[0, b["pr==liq"]] = -0.5                                     # d = -1, pr = cr = dt = liq
        cfr[b["liq1==cap"]], state[1, b["liq1==cap"]] = 0.0, 2.0 * dt  # no refreeze: liq1 = 2 dt = cwh ice2 = 0.5 * 4 dt
    mixed = lambda *shape: (rng.random(shape) - 0.4) * 10.0 ** rng.integers(-2, 2, shape)
    return p, ta, mixed(T, B), mixed(T, B), mixed(T, B), np.stack([tlo, thi, tm, sfcf, cfmax, cfr, cwh]), state, dt


# ---- the host build --------------------------------------------------------------------------------------------------------
UNIT = _hostbuild.HostUnit(_HERE, "snow_host", "snowhost", ["lgar_snow.hpp"], "catchment-snowpack")


def library():
    """libsnowhost.so: snowhost_<entry point>(the arguments of include/lgar.h without the stream), loaded once."""
    i32, vp, dbl = C.c_int32, C.c_void_p, C.c_double
    return UNIT.library({"catchment_snow": [vp, vp, i32, i32, vp, dbl, vp, vp, vp, vp, vp],
                         "catchment_snow_grad": [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, dbl, vp, vp, vp, vp, vp]})


def run(cases, sanitize=False):
    """ONE run of the host program over every case:
    ("fwd", p, ta, par, dt_h, state_in or None, want_pack, want_state) gives (w, ice or None, liq or None, state_out or None);
    ("grad", gw, gice or None, gliq or None, p, ta, ice, liq, par, dt_h, state_in or None, want_gta, want_gpar, want_gstate) gives
    (gp, gta or None, gpar or None, gstate or None).  gice and gliq come together."""
    calls, results = [], []
    for case in cases:
        if case[0] == "fwd":
            p, ta, par, dt_h, state, want_pack, want_state = case[1:]
            T, B = np.asarray(p).shape
            assert np.asarray(par).shape == (7, B) and np.asarray(ta).shape == (T, B)
            # (an array of no elements is a null pointer: with T = 0 or B = 0 a wanted pack is "neither", which the entry point takes)
            w, ice, liq, state_out = out(True, T, B), out(want_pack, T, B), out(want_pack, T, B), out(want_state, 2, B)
            calls.append((0, (T, B), (dt_h,), (f64(p), f64(ta), f64(par), f64(state), state_out, w, ice, liq)))
            results.append((w, ice, liq, state_out))
        else:
            assert case[0] == "grad"
            gw, gice, gliq, p, ta, ice, liq, par, dt_h, state, want_ta, want_par, want_state = case[1:]
            T, B = np.asarray(p).shape
            assert (gice is None) == (gliq is None) and np.asarray(par).shape == (7, B)
            assert all(np.asarray(a).shape == (T, B) for a in (gw, ta, ice, liq))
            gp, gta, gpar, gstate = out(True, T, B), out(want_ta, T, B), out(want_par, 7, B), out(want_state, 2, B)
            calls.append((1, (T, B), (dt_h,), (f64(gw), f64(gice), f64(gliq), f64(p), f64(ta), f64(ice), f64(liq), f64(par), f64(state),
                                               gp, gta, gpar, gstate)))
            results.append((gp, gta, gpar, gstate))
    UNIT.run_calls(calls, sanitize)
    return [_hostbuild.values(r) for r in results]


class SimCatchmentSnow(CatchmentSnow):
    """lgar_py_amd.snow.CatchmentSnow (device="cpu") with the host build of the snow kernels in the library's place;
    SimCatchmentSnow.function is catchment_snow on that build."""

    def __init__(self, tlo, thi, tm, sfcf, cfmax, cfr, cwh, dt_h, n_catchments=None):
        super().__init__(tlo, thi, tm, sfcf, cfmax, cfr, cwh, dt_h, device="cpu", n_catchments=n_catchments)

    @classmethod
    def _open(cls, device):
        return _hostbuild.AsHipLibrary(("", "snowhost", library))
