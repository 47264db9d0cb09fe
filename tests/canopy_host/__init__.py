"""TEST INFRASTRUCTURE ONLY: the host build of the catchment-canopy header (lgar_py_amd/csrc/lgar_canopy.hpp, compiled for the host
with -DLGAR_DEVSIM) and its front-end.  canopy_host.hpp holds the host-side launchers of the three entry points; canopy_host.cpp is
the stand-alone program around them (run() below; also built with AddressSanitizer + UBSan), libcanopyhost.so the same header as a
shared library (library(): what SimCatchmentCanopy puts behind the product's calling surface, and what host_call() calls on numpy
arrays).  The numpy statement of the definition (include/lgar.h, lgar_catchment_canopy / _grad / _tangent)
-- canopy_ref, canopy_grad_ref, canopy_tangent_ref and regimes: plain loops over rows, the cells side by side -- the data of the
tests' cases and the case grid the host suite and the GPU suite share live here too.
The build, the program's call records (tests/_hostprog.hpp) and same_bits are tests/_hostbuild.py's: UNIT below.
Never imported by the product package.
"""
import ctypes as C
import itertools
import os

import numpy as np

import _hostbuild
from _hostbuild import f64, out, same_bits  # noqa: F401
from lgar_py_amd.canopy import CatchmentCanopy

_HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE_B = (1, 2, 63, 64, 65, 257)
SHAPE_T = (0, 1, 9, 17)  # none, one, one more than the row chunk of 8, one more than two chunks
SHAPE_D = (1, 3)
LAYOUTS = ((0, 0), (3, 2))  # (ld - D, k0): the block is exactly the directions, or wider with the directions inside it
CMAX, FE, COVER = range(3)  # the rows of par
REGIMES = ("full", "hold", "lim", "free", "neg", "pos")
TIES = ("s1==cap", "dem==s2", "ei==ed")
TIE_CELLS = {name: 16 + k for k, name in enumerate(TIES)}  # the cells case_data plants the ties in (row 0, with the state given)


# ---- the definition, in numpy ----------------------------------------------------------------------------------------------
def _start(par, state, B):
    """the parameters as the rows use them (fc rounded once), and the store before row 0"""
    par = np.asarray(par, dtype=np.float64)
    c = dict(cmax=par[CMAX], fe=par[FE], cover=par[COVER])
    c["fc"] = c["fe"] * c["cover"]
    return c, (np.zeros(B) if state is None else np.asarray(state, dtype=np.float64)[0].copy())


def _cap(c, lai, t):
    """cmax * lai[t], or cmax itself (no multiplication) without leaf area"""
    return c["cmax"] if lai is None else c["cmax"] * lai[t]


def _step(s, pd, ed, cap, c):
    """One row of the definition, one numpy operation for one of the header's: a dict of every value and flag."""
    hit = c["cover"] * pd
    direct = pd - hit
    s1 = s + hit
    full = s1 > cap
    drip = np.where(full, s1 - cap, 0.0)
    s2 = np.where(full, cap, s1)
    dem = c["fc"] * ed
    lim = dem > s2
    ei = np.where(lim, s2, dem)
    s_new = s2 - ei
    neg = ei > ed
    r = np.where(neg, 0.0, ed - ei)
    return dict(hit=hit, direct=direct, s1=s1, cap=cap, full=full, drip=drip, s2=s2, dem=dem, lim=lim, ei=ei, s=s_new, neg=neg, r=r,
                tf=direct + drip, ed=ed, pd=pd)


def _series(*arrays):
    return tuple(None if a is None else np.asarray(a, dtype=np.float64) for a in arrays)


def canopy_ref(p, e, lai, par, dt_h, state=None):
    """(w, pet_out, store, evap [T, B] each, state_out [1, B]): the rows in ascending order."""
    p, e, lai = _series(p, e, lai)
    T, B = p.shape
    dt = np.float64(dt_h)
    c, s = _start(par, state, B)
    w, pet, st, ev = (np.zeros((T, B)) for _ in range(4))
    with np.errstate(all="ignore"):
        for t in range(T):
            o = _step(s, p[t] * dt, e[t] * dt, _cap(c, lai, t), c)
            w[t], pet[t], st[t], ev[t] = o["tf"] / dt, o["r"] / dt, o["s"], o["ei"] / dt
            s = o["s"]
    return w, pet, st, ev, s[None, :].copy()


def regimes(p, e, lai, par, dt_h, state=None):
    """(rows per regime, rows per exact tie, [T, B] bool maps of both, the smallest relative distance of a row from a switch) of a
    run.  The regimes: full (the store spills) / hold; lim (the evaporation takes all that is held) / free (demand-limited); neg
    (the evaporation exceeds PET: none is left) / pos (a residual >= 0 is left)."""
    p, e, lai = _series(p, e, lai)
    T, B = p.shape
    c, s = _start(par, state, B)
    reg = {k: np.zeros((T, B), dtype=bool) for k in REGIMES}
    tie = {k: np.zeros((T, B), dtype=bool) for k in TIES}
    margin = np.inf
    with np.errstate(all="ignore"):
        for t in range(T):
            o = _step(s, p[t] * np.float64(dt_h), e[t] * np.float64(dt_h), _cap(c, lai, t), c)
            for k, v in (("full", o["full"]), ("hold", ~o["full"]), ("lim", o["lim"]), ("free", ~o["lim"]), ("neg", o["neg"]), ("pos", ~o["neg"])):
                reg[k][t] = v
            for k, a, b in (("s1==cap", o["s1"], o["cap"]), ("dem==s2", o["dem"], o["s2"]), ("ei==ed", o["ei"], o["ed"])):
                tie[k][t] = a == b
                rel = np.abs(a - b) / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)
                margin = min(margin, float(np.nanmin(rel))) if rel.size else margin
            s = o["s"]
    return {k: int(v.sum()) for k, v in reg.items()}, {k: int(v.sum()) for k, v in tie.items()}, reg, tie, margin


def canopy_grad_ref(gw, gpet, gstore, gevap, p, e, lai, store, par, dt_h, state=None, absolute=False):
    """(gp, ge, glai [T, B] each, gpar [3, B], gstate [1, B]): the rows in descending order, each re-formed from the stored depth of
    the row before; every accumulator from +0.0, left as it is in a row that gives it no term.  absolute: the same adjoint on
    absolute values, every difference a sum (what rounding can do is relative to it)."""
    gw, gpet, gstore, gevap, p, e, lai, store = _series(gw, gpet, gstore, gevap, p, e, lai, store)
    T, B = p.shape
    A = np.abs if absolute else (lambda x: x)
    sub = (lambda x, y: x + y) if absolute else (lambda x, y: x - y)
    gstore = np.zeros((T, B)) if gstore is None else gstore
    gevap = np.zeros((T, B)) if gevap is None else gevap
    dt = np.float64(dt_h)
    c, s0 = _start(par, state, B)
    gp, ge, glai = np.zeros((T, B)), np.zeros((T, B)), np.zeros((T, B))
    ls, gcmax, gfc, gcover, gfe = (np.zeros(B) for _ in range(5))
    one = np.ones(B)
    with np.errstate(all="ignore"):
        for t in range(T - 1, -1, -1):
            pd, ed = p[t] * dt, e[t] * dt
            o = _step(store[t - 1] if t > 0 else s0, pd, ed, _cap(c, lai, t), c)
            lv = one if lai is None else lai[t]
            ls = ls + A(gstore[t])
            gtf, gr, gei = A(gw[t]) / dt, A(gpet[t]) / dt, A(gevap[t]) / dt
            dr = np.where(o["neg"], 0.0, gr)
            dei = sub(sub(gei, dr), ls)
            ds2 = np.where(o["lim"], ls + dei, ls)
            ddem = np.where(o["lim"], 0.0, dei)
            gfc = np.where(o["lim"], gfc, gfc + ddem * A(ed))
            ged = dr + ddem * A(c["fc"])
            ds1 = np.where(o["full"], gtf, ds2)
            dcap = np.where(o["full"], sub(ds2, gtf), 0.0)
            gcmax = np.where(o["full"], gcmax + dcap * A(lv), gcmax)
            glai[t] = dcap * A(c["cmax"])
            dhit = sub(ds1, gtf)
            gcover = gcover + dhit * A(pd)
            gp[t] = (gtf + dhit * A(c["cover"])) * dt
            ge[t] = ged * dt
            ls = ds1
        if T > 0:
            gfe = gfc * A(c["cover"])
            gcover = gcover + gfc * A(c["fe"])
    return gp, ge, glai, np.stack([gcmax, gfe, gcover]), ls[None, :].copy()


def canopy_tangent_ref(p, e, lai, par, dt_h, state, D, dp=None, de=None, dlai=None, dpar=None, dstate=None, absolute=False, variant=None):
    """(dw [T, B, D], dpet [T, B, D], dstore [D, T, B], devap [D, T, B], dstate_out [D, B]): the recurrence of lgar_canopy.hpp, one
    numpy operation for one of the header's, the directions and cells side by side.  absolute: inputs by their absolute values, every
    difference a sum, the values' factors by their absolute values.  variant: one of the WRONG tangents the bound must refuse --
    "no_cmax_dlai" (cmax * lai' dropped from cap'), "ei_sign" (s' = s2' + ei'), "no_dfc" (fc' = 0)."""
    p, e, lai = _series(p, e, lai)
    T, B = p.shape
    dt = np.float64(dt_h)
    A = np.abs if absolute else (lambda x: x)
    sub = (lambda x, y: x + y) if absolute else (lambda x, y: x - y)
    z = lambda x, shape: np.zeros(shape) if x is None else A(np.asarray(x, dtype=np.float64))
    dp, de, dlai, dpar, dstate = z(dp, (D, T, B)), z(de, (D, T, B)), z(dlai, (D, T, B)), z(dpar, (D, 3, B)), z(dstate, (D, B))
    c, s = _start(par, state, B)
    dcmax, dfe, dcover = (dpar[:, j] for j in range(3))
    ds = dstate.copy()
    dw, dpet, dst, dev = np.zeros((T, B, D)), np.zeros((T, B, D)), np.zeros((D, T, B)), np.zeros((D, T, B))
    one = np.ones(B)
    with np.errstate(all="ignore"):
        dfc = np.zeros((D, B)) if variant == "no_dfc" else dfe * A(c["cover"]) + A(c["fe"]) * dcover
        for t in range(T):
            pd, ed = p[t] * dt, e[t] * dt
            o = _step(s, pd, ed, _cap(c, lai, t), c)
            lv = one if lai is None else lai[t]
            dpd, ded = dp[:, t] * dt, de[:, t] * dt
            dhit = dcover * A(pd) + A(c["cover"]) * dpd
            ddirect = sub(dpd, dhit)
            dcap = dcmax * A(lv) if variant == "no_cmax_dlai" else dcmax * A(lv) + A(c["cmax"]) * dlai[:, t]
            ds1 = ds + dhit
            ddrip = np.where(o["full"], sub(ds1, dcap), 0.0)
            ds2 = np.where(o["full"], dcap, ds1)
            ddem = dfc * A(ed) + A(c["fc"]) * ded
            dei = np.where(o["lim"], ds2, ddem)
            ds = ds2 + dei if variant == "ei_sign" else sub(ds2, dei)
            dr = np.where(o["neg"], 0.0, sub(ded, dei))
            s = o["s"]
            dw[t], dpet[t] = ((ddirect + ddrip) / dt).T, (dr / dt).T
            dst[:, t], dev[:, t] = ds, dei / dt
    return dw, dpet, dst, dev, ds.copy()


# ---- data ------------------------------------------------------------------------------------------------------------------
def case_data(rng, T, B, dt=None):
    """p, e, lai [T, B], par [3, B], state [1, B], dt_h.  cmax in [0, 0.2], fe in [0, 2.5], cover in [0, 1], lai in [0.5, 4.5], half
    the rows dry, depths per row of the order of the capacity: rows that spill and hold, evaporation that empties the store and
    that is demand-limited, fc > 1 (more evaporates than PET: no residual) and fc < 1 all occur.  Every eighth cell (b mod 8 == 7)
    has a NEGATIVE p in some rows and a negative initial store, which only the raw entry points take; b mod 8 == 5 has cmax = 0
    and b mod 8 == 6 cover = 0.  A -0.0 stands in p.  Cells 16 .. 18 (where B has them) hold in row 0, for the given state, the
    exact ties of TIES in this order (a dry row; lai = 1 there, so the tie holds with and without leaf area)."""
    kind = np.arange(B) % 8
    n = lambda k: int((kind == k).sum())
    dt = float(rng.choice([0.25, 1.0, 24.0])) if dt is None else float(dt)
    cmax, fe, cover = rng.uniform(0.0, 0.2, B), rng.uniform(0.0, 2.5, B), rng.uniform(0.0, 1.0, B)
    lai = rng.uniform(0.5, 4.5, (T, B))
    p = rng.random((T, B)) * 2.0 * (rng.random((T, B)) < 0.5) / dt
    e = rng.random((T, B)) * 0.4 / dt
    state = rng.random((1, B)) * 0.3
    cmax[kind == 5] = 0.0
    cover[kind == 6] = 0.0
    p[:, kind == 7] = (rng.random((T, n(7))) - 0.3) / dt
    state[0, kind == 7] = -rng.random(n(7)) * 0.2
    if T:
        p[0, B // 2] = -0.0
        p[T - 1, 0] = -0.0
    if T and B > max(TIE_CELLS.values()):
        b = TIE_CELLS
        for k in b.values():  # a dry row 0 under a unit leaf area; cmax = 0.125
            cmax[k], p[0, k], lai[0, k], e[0, k] = 0.125, 0.0, 1.0, 0.0625 / dt
        ed = np.float64(e[0, 16]) * np.float64(dt)                        # the row's PET depth as the walk forms it
        fe[b["s1==cap"]], cover[b["s1==cap"]], state[0, b["s1==cap"]] = 0.5, 0.5, 0.125        # s1 = s = cap: holds
        fe[b["dem==s2"]], cover[b["dem==s2"]], state[0, b["dem==s2"]] = 1.0, 0.5, 0.5 * ed      # dem = 0.5 ed = s2: demand-limited
        fe[b["ei==ed"]], cover[b["ei==ed"]], state[0, b["ei==ed"]] = 2.0, 0.5, 0.125            # fc = 1: ei = dem = ed <= s2
        assert 0.5 * ed < 0.125 and ed <= 0.125
    return p, e, lai, np.stack([cmax, fe, cover]), state, dt


def mixed(rng, *shape):
    """cotangents and directions of mixed signs and magnitudes"""
    return (rng.random(shape) - 0.4) * 10.0 ** rng.integers(-2, 2, shape)


# ---- the host build --------------------------------------------------------------------------------------------------------
UNIT = _hostbuild.HostUnit(_HERE, "canopy_host", "canopyhost", ["lgar_canopy.hpp"], "catchment-canopy")


def library():
    """libcanopyhost.so: canopyhost_<entry point>(the arguments of include/lgar.h without the stream), loaded once."""
    i32, vp, dbl = C.c_int32, C.c_void_p, C.c_double
    return UNIT.library({"catchment_canopy": [vp, vp, vp, i32, i32, vp, dbl, vp, vp, vp, vp, vp, vp],
                         "catchment_canopy_grad": [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, dbl, vp, vp, vp, vp, vp, vp],
                         "catchment_canopy_tangent": [vp, vp, vp, i32, i32, vp, dbl, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp]})


# A case is a tuple; what it gives is a tuple of arrays, None where the case asks for none:
#   ("fwd", p, e, lai or None, par, dt_h, state_in or None, want_store, want_state) -> (w, pet_out, store, evap, state_out)
#   ("grad", gw, gpet, gstore or None, gevap or None, p, e, lai or None, store, par, dt_h, state_in or None, want_glai, want_gpar,
#    want_gstate) -> (gp, ge, glai, gpar, gstate)
#   ("tan", p, e, lai or None, par, dt_h, state_in or None, D, dp, de, dlai, dpar, dstate (each or None), ld, k0, want_pet,
#    want_store, want_state) -> (dw block [T, B, ld], dpet block or None, dstore, devap, dstate_out); the two blocks hold FILL
#    everywhere before the call
FILL = 7.5


def _records(case):
    """(operation, ints, doubles, arrays, outputs) of a case for the stand-alone program"""
    kind = case[0]
    if kind == "fwd":
        p, e, lai, par, dt_h, state, want_store, want_state = case[1:]
        T, B = np.asarray(p).shape
        o = (out(True, T, B), out(True, T, B), out(want_store, T, B), out(want_store, T, B), out(want_state, 1, B))
        return 0, (T, B), (dt_h,), (f64(p), f64(e), f64(lai), f64(par), f64(state), o[4], o[0], o[1], o[2], o[3]), o
    if kind == "grad":
        gw, gpet, gstore, gevap, p, e, lai, store, par, dt_h, state, want_lai, want_par, want_state = case[1:]
        T, B = np.asarray(p).shape
        o = (out(True, T, B), out(True, T, B), out(want_lai, T, B), out(want_par, 3, B), out(want_state, 1, B))
        return 1, (T, B), (dt_h,), (f64(gw), f64(gpet), f64(gstore), f64(gevap), f64(p), f64(e), f64(lai), f64(store), f64(par), f64(state)) + o, o
    assert kind == "tan"
    p, e, lai, par, dt_h, state, D, dp, de, dlai, dpar, dstate, ld, k0, want_pet, want_store, want_state = case[1:]
    T, B = np.asarray(p).shape
    blk = lambda want: _hostbuild.Out(np.float64, T, B, ld, start=np.full((T, B, ld), FILL)) if want else None
    o = (blk(True), blk(want_pet), out(want_store, D, T, B), out(want_store, D, T, B), out(want_state, D, B))
    return 2, (T, B, D, ld, k0), (dt_h,), (f64(p), f64(e), f64(lai), f64(par), f64(state), f64(dp), f64(de), f64(dlai), f64(dpar), f64(dstate)) + o, o


def run(cases, sanitize=False):
    """ONE run of the host program over every case."""
    calls, results = [], []
    for case in cases:
        op, ints, doubles, arrays, outs = _records(case)
        calls.append((op, ints, doubles, arrays))
        results.append(outs)
    UNIT.run_calls(calls, sanitize)
    return [_hostbuild.values(r) for r in results]


def call(case, launch):
    """One case on numpy arrays through launch(name, arguments of include/lgar.h without the stream, arrays as numpy or None,
    outputs included) -> rc.  Returns (rc, the case's outputs).  Every wanted output starts as NaN (the blocks as FILL)."""
    kind = case[0]
    nan = lambda want, *shape: np.full(shape, np.nan) if want else None
    if kind == "fwd":
        p, e, lai, par, dt_h, state, want_store, want_state = case[1:]
        T, B = np.asarray(p).shape
        o = (nan(True, T, B), nan(True, T, B), nan(want_store, T, B), nan(want_store, T, B), nan(want_state, 1, B))
        rc = launch("catchment_canopy", f64(p), f64(e), f64(lai), T, B, f64(par), float(dt_h), f64(state), o[4], o[0], o[1], o[2], o[3])
    elif kind == "grad":
        gw, gpet, gstore, gevap, p, e, lai, store, par, dt_h, state, want_lai, want_par, want_state = case[1:]
        T, B = np.asarray(p).shape
        o = (nan(True, T, B), nan(True, T, B), nan(want_lai, T, B), nan(want_par, 3, B), nan(want_state, 1, B))
        rc = launch("catchment_canopy_grad", f64(gw), f64(gpet), f64(gstore), f64(gevap), f64(p), f64(e), f64(lai), f64(store), T, B, f64(par),
                    float(dt_h), f64(state), *o)
    else:
        p, e, lai, par, dt_h, state, D, dp, de, dlai, dpar, dstate, ld, k0, want_pet, want_store, want_state = case[1:]
        T, B = np.asarray(p).shape
        o = (np.full((T, B, ld), FILL), np.full((T, B, ld), FILL) if want_pet else None, nan(want_store, D, T, B), nan(want_store, D, T, B),
             nan(want_state, D, B))
        rc = launch("catchment_canopy_tangent", f64(p), f64(e), f64(lai), T, B, f64(par), float(dt_h), f64(state), D, f64(dp), f64(de), f64(dlai),
                    f64(dpar), f64(dstate), o[0], o[1], ld, k0, o[2], o[3], o[4])
    return rc, o


# where the outputs stand among the arguments launch() of call() is given
OUTPUT_ARGS = {"catchment_canopy": (8, 9, 10, 11, 12), "catchment_canopy_grad": (13, 14, 15, 16, 17),
               "catchment_canopy_tangent": (14, 15, 18, 19, 20)}


def host_launch(name, *args):
    """`launch` of call() on the host library (an array of no elements is a null pointer)"""
    ptr = lambda a: (None if a.size == 0 else a.ctypes.data) if isinstance(a, np.ndarray) else a
    return getattr(library(), "canopyhost_" + name)(*[ptr(a) for a in args])


def host_call(case):
    rc, o = call(case, host_launch)
    assert rc == 0, (rc, case[0])
    return o


def reference(case):
    """What the numpy statement gives for a case, shaped as the case's outputs."""
    kind = case[0]
    if kind == "fwd":
        p, e, lai, par, dt_h, state, want_store, want_state = case[1:]
        w, pet, st, ev, so = canopy_ref(p, e, lai, par, dt_h, state)
        return w, pet, st if want_store else None, ev if want_store else None, so if want_state else None
    if kind == "grad":
        *ins, want_lai, want_par, want_state = case[1:]
        gp, ge, glai, gpar, gstate = canopy_grad_ref(*ins)
        return gp, ge, glai if want_lai else None, gpar if want_par else None, gstate if want_state else None
    p, e, lai, par, dt_h, state, D, dp, de, dlai, dpar, dstate, ld, k0, want_pet, want_store, want_state = case[1:]
    return _blocks(np.asarray(p).shape, D, ld, k0, canopy_tangent_ref(p, e, lai, par, dt_h, state, D, dp, de, dlai, dpar, dstate),
                   want_pet, want_store, want_state)


def _blocks(shape, D, ld, k0, ref, want_pet, want_store, want_state):
    """the tangent statement's (dw, dpet, dstore, devap, dstate_out) as a case gives them: inside [T, B, ld] blocks of FILL"""
    def blk(a):
        full = np.full(shape + (ld,), FILL)
        full[:, :, k0:k0 + D] = a
        return full
    return (blk(ref[0]), blk(ref[1]) if want_pet else None, ref[2] if want_store else None, ref[3] if want_store else None,
            ref[4] if want_state else None)


def check(case, want, got):
    """a case's outputs against the statement's, bit for bit (an output of no elements is not there at all: the host program
    hands a null pointer for it)"""
    where = (case[0], np.asarray(case[5] if case[0] == "grad" else case[1]).shape)
    assert len(want) == len(got)
    for w, g in zip(want, got):
        assert (w is None or w.size == 0) == (g is None or g.size == 0), where
        assert w is None or w.size == 0 or same_bits(g, w), where


FWD_WANTS = tuple(itertools.product((True, False), repeat=2))   # store / evap, state_out
GRAD_WANTS = tuple(itertools.product((True, False), repeat=5))  # gstore given, gevap given, glai, gpar, gstate
TAN_GIVEN = tuple(itertools.product((True, False), repeat=5))   # dp, de, dlai, dpar, dstate_in given
TAN_WANTS = tuple(itertools.product((True, False), repeat=3))   # dpet, dstore / devap, dstate_out
TAN_PAIRS = tuple(itertools.product(SHAPE_D, LAYOUTS))          # (D, (ld - D, k0))


def grid_data(B, seed=21):
    """The data of grid(B), per T: (T, p, e, lai, par, state, dt_h, (gw, gpet, gstore, gevap), {D: (dp, de, dlai, dpar, dstate)})"""
    rng = np.random.default_rng(seed + B)
    for T in SHAPE_T:
        p, e, lai, par, state, dt = case_data(rng, T, B)
        cots = tuple(mixed(rng, T, B) for _ in range(4))
        dirs = {D: (mixed(rng, D, T, B), mixed(rng, D, T, B), mixed(rng, D, T, B), mixed(rng, D, 3, B), mixed(rng, D, B)) for D in SHAPE_D}
        yield T, p, e, lai, par, state, dt, cots, dirs


def grid(B, seed=21, tangent_every=1):
    """For one B: T in SHAPE_T x state present / NULL x lai present / NULL; at each of these 16 points
      the forward with every combination of store / evap and state_out wanted (4),
      the adjoint with every combination of gstore and gevap given and glai, gpar, gstate wanted (32),
      the tangent with every combination of dp, de, dlai, dpar, dstate_in given (32) x every combination of dpet, dstore / devap,
        dstate_out wanted (8); D in {1, 3} and the two (ld, k0) rotate with the combination and the point, so that every
        combination of given inputs meets all four at every point and every combination of wanted outputs meets all four at
        every B.  tangent_every = n keeps every n-th tangent case, the phase rotating with the point (the points of all B
        counted on): over the six B every one of the 256 combinations stays in.
    Yields (case, reference); the references of a point are evaluated once."""
    point = 16 * SHAPE_B.index(B) if B in SHAPE_B else 0
    for T, p, e, lai_all, par, state_all, dt, (gw, gpet, gstore, gevap), dirs in grid_data(B, seed):
        for state, lai in itertools.product((state_all, None), (lai_all, None)):
            w, pet, st, ev, so = canopy_ref(p, e, lai, par, dt, state)
            for want_store, want_state in FWD_WANTS:
                yield (("fwd", p, e, lai, par, dt, state, want_store, want_state),
                       (w, pet, st if want_store else None, ev if want_store else None, so if want_state else None))
            for gs, gv in itertools.product((gstore, None), (gevap, None)):
                ref = canopy_grad_ref(gw, gpet, gs, gv, p, e, lai, st, par, dt, state)
                for want_lai, want_par, want_state in itertools.product((True, False), repeat=3):
                    yield (("grad", gw, gpet, gs, gv, p, e, lai, st, par, dt, state, want_lai, want_par, want_state),
                           (ref[0], ref[1], ref[2] if want_lai else None, ref[3] if want_par else None, ref[4] if want_state else None))
            n = 0
            for gi, given in enumerate(TAN_GIVEN):
                refs = {}
                for wi, (want_pet, want_store, want_state) in enumerate(TAN_WANTS):
                    n += 1
                    if (n + point) % tangent_every:
                        continue
                    D, (extra, k0) = TAN_PAIRS[(wi + gi + point) % len(TAN_PAIRS)]
                    ins = [d if g else None for d, g in zip(dirs[D], given)]
                    if D not in refs:
                        refs[D] = canopy_tangent_ref(p, e, lai, par, dt, state, D, *ins)
                    yield (("tan", p, e, lai, par, dt, state, D, *ins, D + extra, k0, want_pet, want_store, want_state),
                           _blocks((T, B), D, D + extra, k0, refs[D], want_pet, want_store, want_state))
            point += 1


def grid_counts(B, seed=21):
    """(rows per regime, rows per exact tie) over the data of grid(B), with the state and the leaf area present"""
    rows, ties = dict.fromkeys(REGIMES, 0), dict.fromkeys(TIES, 0)
    for T, p, e, lai, par, state, dt, _, _ in grid_data(B, seed):
        r, t, _, _, _ = regimes(p, e, lai, par, dt, state)
        for k in rows:
            rows[k] += r[k]
        for k in ties:
            ties[k] += t[k]
    return rows, ties


def nan_confinement(do, which):
    """A NaN in one input (row 4 of cell 17 for the series) reaches no other cell: every other cell has the clean run's bits, and
    cell 17 has them before its row.  What the cell itself shows is what the header says: p -> w of the row and the store from the
    row on; e -> evap and pet_out of the row and the store from the row on; lai -> nothing at all (full is false: the row holds
    what hit it); state -> the store of every row."""
    rng = np.random.default_rng(41)
    T, B, t0, b = 9, 65, 4, 17
    p, e, lai, par, state, dt = case_data(rng, T, B)
    par[:, b], lai[t0, b] = (0.1, 0.5, 0.5), 2.0  # an ordinary cell
    clean = do(("fwd", p, e, lai, par, dt, state, True, True))
    arrays = dict(p=p, e=e, lai=lai, state=state)
    arrays[which] = arrays[which].copy()
    if which == "state":
        arrays[which][0, b] = np.nan
    else:
        arrays[which][t0, b] = np.nan
    case = ("fwd", arrays["p"], arrays["e"], arrays["lai"], par, dt, arrays["state"], True, True)
    got = do(case)
    check(case, reference(case), got)
    own = np.zeros((T, B), dtype=bool)
    own[(0 if which == "state" else t0):, b] = True
    for have, was in zip(got[:4], clean[:4]):
        assert same_bits(have[~own], was[~own])
    others = np.arange(B) != b
    assert same_bits(got[4][:, others], clean[4][:, others])
    w, pet, st, ev = (np.isnan(a) for a in got[:4])
    row = np.zeros((T, B), dtype=bool)
    row[t0, b] = True
    none = np.zeros((T, B), dtype=bool)
    want = dict(p=(row, none, own, none), e=(none, row, own, row), lai=(none, none, none, none), state=(none, none, own, none))[which]
    for have, should in zip((w, pet, st, ev), want):
        assert (have == should).all(), which
    assert bool(np.isnan(got[4][0, b])) == (which != "lai")


def refusals(entry, buf):
    """The refusals of the C-ABI (include/lgar.h): LGAR_E_ARG = -1 for negative sizes or k0, ld < k0 + D, a dt_h that is not finite
    or <= 0, exactly one of store / evap (and of their tangents), a null pointer the sizes say will be read or written; B = 0,
    D = 0 and T = 0 return 0 without touching anything, unless a state output is wanted.  entry(name): the entry point with the
    arguments of include/lgar.h without the stream; buf: 1024 doubles, all 1.0, where the entry points read and write them --
    .address, .get(lo, hi) -> list, .set(lo, hi, values)."""
    a = buf.address
    at = lambda k: a + 8 * 64 * k
    T, B = 2, 4
    fwd = (("p", a), ("e", a), ("lai", a), ("T", T), ("B", B), ("par", a), ("dt", 1.0), ("state_in", None), ("state_out", at(1)), ("w", at(2)),
           ("pet", at(3)), ("store", at(4)), ("evap", at(5)))
    run = lambda **kw: entry("catchment_canopy")(*[kw.get(k, d) for k, d in fwd])
    assert run() == 0
    for bad in (dict(T=-1), dict(B=-1), dict(p=None), dict(e=None), dict(par=None), dict(w=None), dict(pet=None), dict(store=None), dict(evap=None),
                dict(dt=0.0), dict(dt=-1.0), dict(dt=float("nan")), dict(dt=float("inf")), dict(B=0, dt=0.0), dict(B=0, store=None), dict(T=0, evap=None)):
        assert run(**bad) == -1, bad
    assert run(store=None, evap=None) == 0 and run(state_out=None) == 0 and run(state_in=a) == 0 and run(lai=None) == 0
    assert run(B=0, p=None, e=None, par=None, w=None, pet=None) == 0 and run(T=0, p=None, e=None, par=None, w=None, pet=None) == 0
    buf.set(64, 68, 7.0)
    assert run(T=0, p=None, e=None, lai=None, par=None, w=None, pet=None, store=None, evap=None) == 0 and buf.get(64, 68) == [0.0] * 4
    buf.set(64, 68, 7.0)
    assert run(T=0, state_out=None) == 0 and run(B=0) == 0 and buf.get(64, 68) == [7.0] * 4
    grd = (("gw", a), ("gpet", a), ("gstore", a), ("gevap", a), ("p", a), ("e", a), ("lai", a), ("store", a), ("T", T), ("B", B), ("par", a),
           ("dt", 1.0), ("state_in", None), ("gp", at(1)), ("ge", at(2)), ("glai", at(3)), ("gpar", at(4)), ("gstate", at(5)))
    grad = lambda **kw: entry("catchment_canopy_grad")(*[kw.get(k, d) for k, d in grd])
    assert grad() == 0
    for bad in (dict(T=-1), dict(B=-1), dict(gw=None), dict(gpet=None), dict(p=None), dict(e=None), dict(store=None), dict(par=None), dict(gp=None),
                dict(ge=None), dict(dt=0.0), dict(dt=float("nan")), dict(dt=float("-inf"))):
        assert grad(**bad) == -1, bad
    assert grad(gstore=None) == 0 and grad(gevap=None) == 0 and grad(gstore=None, gevap=None) == 0 and grad(lai=None) == 0
    assert grad(glai=None) == 0 and grad(gpar=None) == 0 and grad(gstate=None) == 0 and grad(glai=None, gpar=None, gstate=None) == 0
    assert grad(B=0, gw=None, gpet=None, p=None, e=None, store=None, par=None, gp=None, ge=None) == 0
    buf.set(256, 268, 7.0)
    buf.set(320, 324, 7.0)
    assert grad(T=0, gw=None, gpet=None, gstore=None, gevap=None, p=None, e=None, lai=None, store=None, par=None, gp=None, ge=None, glai=None) == 0
    assert buf.get(256, 268) == [0.0] * 12 and buf.get(320, 324) == [0.0] * 4  # T = 0: gpar and gstate are zeros
    assert grad(T=0, gpar=None, gstate=None, gw=None, store=None) == 0
    D = 2
    tan = (("p", a), ("e", a), ("lai", a), ("T", T), ("B", B), ("par", a), ("dt", 1.0), ("state_in", None), ("D", D), ("dp", a), ("de", a),
           ("dlai", a), ("dpar", a), ("dstate_in", a), ("dw", at(1)), ("dpet", at(2)), ("ld", 3), ("k0", 1), ("dstore", at(3)), ("devap", at(4)),
           ("dstate_out", at(5)))
    tang = lambda **kw: entry("catchment_canopy_tangent")(*[kw.get(k, d) for k, d in tan])
    assert tang() == 0
    for bad in (dict(T=-1), dict(B=-1), dict(D=-1), dict(k0=-1), dict(ld=2), dict(k0=2), dict(p=None), dict(e=None), dict(par=None), dict(dw=None),
                dict(dstore=None), dict(devap=None), dict(dt=0.0), dict(dt=float("nan")), dict(dt=float("inf")), dict(D=0, ld=0), dict(B=0, dstore=None)):
        assert tang(**bad) == -1, bad
    assert tang(dpet=None) == 0 and tang(dstore=None, devap=None) == 0 and tang(dstate_out=None) == 0 and tang(lai=None, dlai=None) == 0
    assert tang(dp=None, de=None, dlai=None, dpar=None, dstate_in=None) == 0
    buf.set(64, 128, 7.0)
    buf.set(320, 328, 7.0)
    assert tang(B=0, p=None, dw=None) == 0 and tang(D=0, p=None, dw=None) == 0 and tang(T=0, dstate_out=None, p=None, dw=None) == 0
    assert buf.get(64, 128) == [7.0] * (128 - 64) and buf.get(320, 328) == [7.0] * (328 - 320)
    buf.set(0, 8, np.arange(8.0))
    assert tang(T=0, p=None, e=None, par=None, dw=None) == 0 and buf.get(320, 328) == list(np.arange(8.0))  # T = 0 copies dstate


class SimCatchmentCanopy(CatchmentCanopy):
    """lgar_py_amd.canopy.CatchmentCanopy (device="cpu") with the host build of the canopy kernels in the library's place;
    SimCatchmentCanopy.function is catchment_canopy on that build."""

    def __init__(self, cmax, fe, cover, dt_h, n_catchments=None, device="cpu"):
        super().__init__(cmax, fe, cover, dt_h, device="cpu", n_catchments=n_catchments)

    @classmethod
    def _open(cls, device):
        return _hostbuild.AsHipLibrary(("", "canopyhost", library))
