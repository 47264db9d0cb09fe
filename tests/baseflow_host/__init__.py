"""TEST INFRASTRUCTURE ONLY: the host build of the catchment-baseflow header (lgar_py_amd/csrc/lgar_baseflow.hpp, compiled for the
host with -DLGAR_DEVSIM) and its front-end.  baseflow_host.hpp holds the host-side launchers of the two entry points;
baseflow_host.cpp is the stand-alone program around them (run() below; also built with AddressSanitizer + UBSan),
libbaseflowhost.so the same header as a shared library (library(): what SimCatchmentBaseflow puts behind the product's calling
surface).  The numpy statement of the definition (include/lgar.h, lgar_catchment_baseflow / lgar_catchment_baseflow_grad;
DESIGN.md section 15) -- gw_exp_ref, baseflow_ref, baseflow_grad_ref and regimes: plain loops over rows, the catchments side by
side -- and the data of the tests' cases live here too.
The build, the program's call records (tests/_hostprog.hpp) and same_bits are tests/_hostbuild.py's: UNIT below.
Never imported by the product package.
"""
import ctypes as C
import math
import os
from fractions import Fraction

import numpy as np

import _hostbuild
from _hostbuild import f64, out, same_bits  # noqa: F401
from lgar_py_amd.baseflow import CatchmentBaseflow

_HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE_B = (1, 2, 63, 64, 65, 257)
SHAPE_T = (0, 1, 2, 7, 8, 9, 17)  # around the row chunk of 8

ZMAX = 40.0  # LGAR_GW_ZMAX
LOG2E = float.fromhex("0x1.71547652b82fep+0")
LN2_HI = float.fromhex("0x1.62e42fee00000p-1")  # 32 trailing zero bits
LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")
MAGIC = 1.5 * 2.0 ** 52
COEF = [float(Fraction(1, math.factorial(j))) for j in range(14)]  # Fraction -> float rounds correctly
ZERO, EMPTIED, FLUX = 0, 1, 2  # the regime of a row


# ---- the definition, in numpy ----------------------------------------------------------------------------------------------
def gw_exp_ref(zc):
    """exp(zc) on [0, ZMAX] by the header's operations, one for one."""
    zc = np.asarray(zc, dtype=np.float64)
    with np.errstate(all="ignore"):
        k = (zc * LOG2E + MAGIC) - MAGIC
        r = (zc - k * LN2_HI) - k * LN2_LO
        p = np.full(zc.shape, COEF[13])
        for j in range(12, -1, -1):
            p = p * r
            p = p + COEF[j]
        ki = np.where((k >= 0.0) & (k <= 58.0), k, 0.0).astype(np.int32)
        return np.ldexp(p, ki)


def _step(A, cd, expon, smax):
    """z, zc, e, f, pre, qq, S of one row from A"""
    z = expon * (A / smax)
    zc = np.where(z < 0.0, 0.0, np.where(z > ZMAX, ZMAX, z))
    e = gw_exp_ref(zc)
    f = cd * (e - 1.0)
    pre = np.where(f > A, A, f)
    qq = np.where(pre < 0.0, 0.0, pre)
    return z, zc, e, f, pre, qq, A - qq


def _start(par, dt_h, state, B):
    par = np.asarray(par, dtype=np.float64)
    S = np.zeros(B) if state is None else np.array(state, dtype=np.float64)
    return par[0] * np.float64(dt_h), par[1], par[2], S


def baseflow_ref(r, par, dt_h, state=None):
    """(q [T, B], s [T, B], state_out [B]): the rows in ascending order."""
    r = np.asarray(r, dtype=np.float64)
    T, B = r.shape
    cd, expon, smax, S = _start(par, dt_h, state, B)
    q, s = np.zeros((T, B)), np.zeros((T, B))
    with np.errstate(all="ignore"):
        for t in range(T):
            q[t], s[t] = _step(S + r[t], cd, expon, smax)[5:]
            S = s[t]
    return q, s, S.copy()


def regimes(r, par, dt_h, state=None):
    """(regime [T, B] in ZERO / EMPTIED / FLUX, clamp [T, B] in -1 (z < 0) / 0 / +1 (z > ZMAX)) of every row."""
    r = np.asarray(r, dtype=np.float64)
    T, B = r.shape
    cd, expon, smax, S = _start(par, dt_h, state, B)
    reg, clamp = np.zeros((T, B), dtype=np.int64), np.zeros((T, B), dtype=np.int64)
    with np.errstate(all="ignore"):
        for t in range(T):
            A = S + r[t]
            z, _, _, f, pre, _, S = _step(A, cd, expon, smax)
            reg[t] = np.where(pre < 0.0, ZERO, np.where(f > A, EMPTIED, FLUX))
            clamp[t] = np.where(z < 0.0, -1, np.where(z > ZMAX, 1, 0))
    return reg, clamp


def baseflow_grad_ref(gq, gs, r, s, par, dt_h, state=None, variant=None):
    """(gr [T, B], gpar [3, B], gstate [B]): the rows in descending order, A re-formed from the stored s; every accumulator from
    +0.0, left as it is in a row that gives it no term.  variant: one of the WRONG adjoints the bound test must refuse --
    "no_e" (dA without the factor e), "gs_late" (gs added after w instead of before), "gsmax_sign"."""
    gq, r, s = (np.asarray(a, dtype=np.float64) for a in (gq, r, s))
    T, B = r.shape
    gs = np.zeros((T, B)) if gs is None else np.asarray(gs, dtype=np.float64)
    dt = np.float64(dt_h)
    cd, expon, smax, S0 = _start(par, dt_h, state, B)
    gr, lam = np.zeros((T, B)), np.zeros(B)
    g0, g1, g2 = np.zeros(B), np.zeros(B), np.zeros(B)
    with np.errstate(all="ignore"):
        slope = expon / smax
        for t in range(T - 1, -1, -1):
            A = (s[t - 1] if t > 0 else S0) + r[t]
            z, zc, e, f, pre, _, _ = _step(A, cd, expon, smax)
            zero = pre < 0.0
            emptied = ~zero & (f > A)
            flux = ~zero & ~(f > A)
            inside = flux & ~(z < 0.0) & ~(z > ZMAX)
            if variant == "gs_late":
                w = gq[t] - lam
                lam = lam + gs[t]
            else:
                lam = lam + gs[t]
                w = gq[t] - lam
            ce = cd * e
            dA = np.where(zero, 0.0, np.where(emptied, 1.0, np.where(inside, (cd if variant == "no_e" else ce) * slope, 0.0)))
            g0 = np.where(flux, g0 + w * (dt * (e - 1.0)), g0)
            g1 = np.where(inside, g1 + w * (ce * (A / smax)), g1)
            g2 = np.where(inside, g2 + w * (((ce * zc) if variant == "gsmax_sign" else -(ce * zc)) / smax), g2)
            lam = lam + w * dA
            gr[t] = lam
    return gr, np.stack([g0, g1, g2]), lam.copy()


# ---- data ------------------------------------------------------------------------------------------------------------------
def case_data(rng, T, B):
    """r, gq, gs [T, B], par [3, B], state [B], dt_h.  The catchments take turns (b mod 8) so that every branch of the walk is
    taken somewhere: 0 - 3 ordinary stores (flux, now and then emptied by a small store); 4 a tiny cgw under a large expon
    (flux with z > ZMAX); 5 a large cgw (emptied); 6 a negative initial storage and negative recharge (z < 0, qq clamped to 0);
    7 a NEGATIVE expon, which only the raw entry points take (flux with z < 0 under a positive A)."""
    kind = np.arange(B) % 8
    cgw = 10.0 ** rng.uniform(-3.0, -0.5, B)
    expon = rng.uniform(1.0, 8.0, B)
    smax = rng.uniform(5.0, 50.0, B)
    r = rng.random((T, B)) * 10.0 ** rng.integers(-2, 2, (T, B))
    state = rng.random(B) * smax
    cgw[kind == 4], expon[kind == 4] = 1e-25, rng.uniform(50.0, 90.0, int((kind == 4).sum()))
    cgw[kind == 5] = rng.uniform(2.0, 20.0, int((kind == 5).sum()))
    state[kind == 6] = -rng.random(int((kind == 6).sum())) * 3.0
    r[:, kind == 6] = (rng.random((T, int((kind == 6).sum()))) - 0.6) * 2.0
    expon[kind == 7] = -expon[kind == 7]
    if T:
        r[0, B // 2] = -0.0
        r[T - 1, 0] = -0.0
    mixed = lambda *shape: (rng.random(shape) - 0.4) * 10.0 ** rng.integers(-3, 3, shape)
    return r, mixed(T, B), mixed(T, B), np.stack([cgw, expon, smax]), state, float(rng.choice([1.0, 0.25, 24.0]))


# ---- the host build --------------------------------------------------------------------------------------------------------
UNIT = _hostbuild.HostUnit(_HERE, "baseflow_host", "baseflowhost", ["lgar_baseflow.hpp"], "catchment-baseflow")


def library():
    """libbaseflowhost.so: baseflowhost_<entry point>(the arguments of include/lgar.h without the stream), loaded once."""
    i32, vp, dbl = C.c_int32, C.c_void_p, C.c_double
    return UNIT.library({"catchment_baseflow": [vp, i32, i32, vp, dbl, vp, vp, vp, vp],
                         "catchment_baseflow_grad": [vp, vp, vp, vp, i32, i32, vp, dbl, vp, vp, vp, vp], "gw_exp": [vp, i32, vp]}, {"gw_exp": None})


def run(cases, sanitize=False):
    """ONE run of the host program over every case:
    ("fwd", r, par, dt_h, state_in or None, want_s, want_state) gives (q, s or None, state_out or None);
    ("grad", gq, gs or None, r, s, par, dt_h, state_in or None, want_gpar, want_gstate) gives (gr, gpar or None, gstate or None);
    ("exp", z) gives (gw_exp(z),)."""
    calls, results = [], []
    for case in cases:
        op = case[0]
        if op == "fwd":
            r, par, dt_h, state, want_s, want_state = case[1:]
            T, B = np.asarray(r).shape
            assert np.asarray(par).shape == (3, B)
            q, s, state_out = out(True, T, B), out(want_s, T, B), out(want_state, B)
            calls.append((0, (T, B), (dt_h,), (f64(r), f64(par), f64(state), state_out, q, s)))
            results.append((q, s, state_out))
        elif op == "grad":
            gq, gs, r, s, par, dt_h, state, want_par, want_state = case[1:]
            T, B = np.asarray(r).shape
            assert np.asarray(par).shape == (3, B) and np.asarray(s).shape == (T, B) and np.asarray(gq).shape == (T, B)
            gr, gpar, gstate = out(True, T, B), out(want_par, 3, B), out(want_state, B)
            calls.append((1, (T, B), (dt_h,), (f64(gq), f64(gs), f64(r), f64(s), f64(par), f64(state), gr, gpar, gstate)))
            results.append((gr, gpar, gstate))
        else:
            assert op == "exp"
            z = np.asarray(case[1], dtype=np.float64).ravel()
            e = out(True, len(z))
            calls.append((2, (len(z),), (), (z, e)))
            results.append((e,))
    UNIT.run_calls(calls, sanitize)
    return [_hostbuild.values(r) for r in results]


class SimCatchmentBaseflow(CatchmentBaseflow):
    """lgar_py_amd.baseflow.CatchmentBaseflow (device="cpu") with the host build of the baseflow kernels in the library's
    place; SimCatchmentBaseflow.function is catchment_baseflow on that build."""

    def __init__(self, cgw, expon, smax, dt_h, n_catchments=None):
        super().__init__(cgw, expon, smax, dt_h, device="cpu", n_catchments=n_catchments)

    @classmethod
    def _open(cls, device):
        return _hostbuild.AsHipLibrary(("", "baseflowhost", library))
