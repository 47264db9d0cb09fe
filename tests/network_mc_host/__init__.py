"""TEST INFRASTRUCTURE ONLY: the host build of the Muskingum-Cunge network header (lgar_py_amd/csrc/lgar_network_mc.hpp, compiled
for the host with -DLGAR_DEVSIM) and its front-end.  network_mc_host.hpp holds the host-side launchers of the two entry points;
network_mc_host.cpp is the stand-alone program around them (run() below; also built with AddressSanitizer + UBSan),
libnetworkmchost.so the same header as a shared library (library(): what SimCatchmentNetworkMC puts behind the product's calling
surface).  The numpy statement of the definition (include/lgar.h, lgar_network_route_mc / lgar_network_route_mc_grad; DESIGN.md
section 17) -- mc_ln_ref, route_mc_ref, route_mc_grad_ref and regimes: plain loops over rows and over the reaches in `order`, a
level's reaches side by side -- and the data of the tests' cases live here too; the topologies and the inflow fold are
tests/network_host's, gw_exp_ref is tests/baseflow_host's.
The build, the program's call records (tests/_hostprog.hpp) and same_bits are tests/_hostbuild.py's: UNIT below.
Never imported by the product package.
"""
import ctypes as C
import os
from fractions import Fraction

import numpy as np

import _hostbuild
import network_host as NH
from _hostbuild import f64, i32, out
from baseflow_host import LN2_HI, LN2_LO, ZMAX, gw_exp_ref
from lgar_py_amd.network import CatchmentNetwork
from network_host import Topology, same_bits  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE_T = (0, 1, 2, 7, 8, 9, 17)  # around the row chunk of 8
SQRT_HALF = float.fromhex("0x1.6a09e667f3bcdp-1")
COEF = [float(Fraction(1, 2 * j + 1)) for j in range(11)]  # Fraction -> float rounds correctly
NARROW, WIDE = (1.0 / 64.0, 64.0), (2.0 ** -60, 2.0 ** 60)  # rmin, rmax: the Python layer's default, and the widest allowed


# ---- the definition, in numpy ----------------------------------------------------------------------------------------------
def mc_ln_ref(x):
    """ln(x) for positive normal doubles by the header's operations, one for one."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    bits = x.view(np.uint64)
    k0 = ((bits >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64) - 1022
    m0 = ((bits & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(1022 << 52)).view(np.float64)
    with np.errstate(all="ignore"):
        low = m0 < SQRT_HALF
        m = np.where(low, m0 + m0, m0)
        k = np.where(low, k0 - 1, k0).astype(np.float64)
        s = (m - 1.0) / (m + 1.0)
        z = s * s
        p = np.full(x.shape, COEF[10])
        for j in range(9, -1, -1):
            p = p * z
            p = p + COEF[j]
        t = (2.0 * s) * p
        return k * LN2_HI + (t + k * LN2_LO)


def _row(Oprev, kref, beta, X, qref, half, rmin, rmax):
    """rho, L, tau, K, D, c0, c1, c2 and the regime flags lo, hi, big, inside of one row from Oprev"""
    rho = Oprev / qref
    lo = rho < rmin
    hi = ~lo & (rho > rmax)
    rc = np.where(lo, rmin, np.where(hi, rmax, rho))
    L = mc_ln_ref(rc)
    tau = beta * L
    ta = np.where(tau < 0.0, -tau, tau)
    big = ta > ZMAX
    e = gw_exp_ref(np.where(big, ZMAX, ta))
    K = np.where(tau > 0.0, kref / e, kref * e)
    KX = K * X
    u = K - KX
    D = u + half
    return dict(rho=rho, L=L, tau=tau, K=K, D=D, c0=(half - KX) / D, c1=(half + KX) / D, c2=(u - half) / D, lo=lo, hi=hi, big=big,
                inside=~lo & ~hi & ~big)


def _walk(topo, x, par, dt_h, rmin, rmax, state, rows=None):
    x, par = np.asarray(x, dtype=np.float64), np.asarray(par, dtype=np.float64)
    T, B = x.shape
    half, rmin, rmax = 0.5 * np.float64(dt_h), np.float64(rmin), np.float64(rmax)
    y = np.zeros((T, B))
    out = np.zeros((2, B)) if state is None else np.array(state, dtype=np.float64)
    with np.errstate(all="ignore"):
        for l in range(topo.n_levels):
            bs = topo.order[topo.level_ptr[l]:topo.level_ptr[l + 1]].astype(np.int64)
            kref, beta, X, qref = par[0, bs], par[1, bs], par[2, bs], par[3, bs]
            I = NH._inflow(topo, x, y, bs)
            Iprev, Oprev = out[0, bs], out[1, bs]
            for t in range(T):
                r = _row(Oprev, kref, beta, X, qref, half, rmin, rmax)
                if rows is not None:
                    for k, v in rows.items():
                        v[t, bs] = Oprev if k == "Oprev" else r[k]
                O = (r["c0"] * I[t] + r["c1"] * Iprev) + r["c2"] * Oprev
                y[t, bs] = O
                Iprev, Oprev = I[t], O
            out[0, bs], out[1, bs] = Iprev, Oprev
    return y, out


def route_mc_ref(topo, x, par, dt_h, rmin, rmax, state=None):
    """(y [T, B], state_out [2, B]): the levels in ascending order, the rows in ascending order."""
    return _walk(topo, x, par, dt_h, rmin, rmax, state)


def regimes(topo, x, par, dt_h, rmin, rmax, state=None):
    """The count of rows per regime of the walk: inside, low (rho < rmin), low_negative (of them: Oprev < 0), high (rho > rmax),
    tau_pos, tau_neg, big (ta > ZMAX), tie_low (rho == rmin), tie_high (rho == rmax)."""
    T, B = np.asarray(x).shape
    rows = {k: np.zeros((T, B), dtype=(bool if k in ("lo", "hi", "big", "inside") else np.float64)) for k in
            ("rho", "tau", "lo", "hi", "big", "inside", "Oprev")}
    _walk(topo, x, par, dt_h, rmin, rmax, state, rows)
    return dict(inside=int(rows["inside"].sum()), low=int(rows["lo"].sum()), low_negative=int((rows["lo"] & (rows["Oprev"] < 0)).sum()),
                high=int(rows["hi"].sum()), tau_pos=int((rows["tau"] > 0).sum()), tau_neg=int((rows["tau"] < 0).sum()),
                big=int(rows["big"].sum()), tie_low=int((rows["rho"] == rmin).sum()), tie_high=int((rows["rho"] == rmax).sum()))


def route_mc_grad_ref(topo, gy, x, y, par, dt_h, rmin, rmax, state=None, variant=None):
    """(gx [T, B], gpar [3, B], gstate [2, B]): the levels in descending order, the rows in descending order, the row's K, the
    coefficients and the regime re-formed from the stored y; every accumulator from +0.0, left as it is in a row that gives it
    no term.  variant: one of the WRONG adjoints the bound test must refuse -- "no_gk" (the GK dK/dOprev term dropped),
    "c1_now" (c1 of row t where c1 of row t + 1 belongs in gx), "gbeta_sign"."""
    gy, x, y, par = (np.asarray(a, dtype=np.float64) for a in (gy, x, y, par))
    T, B = gy.shape
    half, rmin, rmax = 0.5 * np.float64(dt_h), np.float64(rmin), np.float64(rmax)
    gx, gpar, gstate = np.zeros((T, B)), np.zeros((3, B)), np.zeros((2, B))
    st = np.zeros((2, B)) if state is None else np.asarray(state, dtype=np.float64)
    with np.errstate(all="ignore"):
        for l in range(topo.n_levels - 1, -1, -1):
            bs = topo.order[topo.level_ptr[l]:topo.level_ptr[l + 1]].astype(np.int64)
            n = len(bs)
            kref, beta, X, qref = par[0, bs], par[1, bs], par[2, bs], par[3, bs]
            omx = 1.0 - X
            d = topo.down[bs].astype(np.int64)
            has = d >= 0
            a = gy[:, bs].copy()
            a[:, has] = a[:, has] + gx[:, d[has]]
            I = np.concatenate([st[0:1, bs], NH._inflow(topo, x, y, bs)])  # I[t + 1] = the inflow of row t; I[0] = I[-1]
            yb = np.concatenate([st[1:2, bs], y[:, bs]])
            pI, pO, g0, g1, g2, lam_next = (np.zeros(n) for _ in range(6))
            for t in range(T - 1, -1, -1):
                It, Ip, Op = I[t + 1], I[t], yb[t]
                r = _row(Op, kref, beta, X, qref, half, rmin, rmax)
                c0, c1, c2, K, D = r["c0"], r["c1"], r["c2"], r["K"], r["D"]
                lam = a[t] + pO
                gx[t, bs] = c0 * lam + (c1 * lam_next if variant == "c1_now" else pI)
                dK = ((It * (-(X + c0 * omx)) + Ip * (X - c1 * omx)) + Op * (omx * (1.0 - c2))) / D
                GK = lam * dK
                dX = ((It * (-(1.0 - c0)) + Ip * (1.0 + c1)) + Op * (-(1.0 - c2))) * (K / D)
                g0 = g0 + GK * (K / kref)
                g1 = np.where(r["big"], g1, g1 + GK * ((K * r["L"]) if variant == "gbeta_sign" else -(K * r["L"])))
                g2 = g2 + lam * dX
                c2l = c2 * lam
                pI = c1 * lam
                pO = c2l if variant == "no_gk" else np.where(r["inside"], c2l + GK * ((-(beta * K)) / Op), c2l)
                lam_next = lam
            gpar[0, bs], gpar[1, bs], gpar[2, bs] = g0, g1, g2
            gstate[0, bs], gstate[1, bs] = pI, pO
    return gx, gpar, gstate


# ---- data ------------------------------------------------------------------------------------------------------------------
def case_data(rng, T, B, wide=False):
    """x, gy [T, B] (x with -0.0), par [4, B], state [2, B], dt_h, (rmin, rmax).  The reaches take turns (b mod 8) so that every
    regime of the row is taken somewhere: 0 - 3 ordinary reaches (inside, tau of either sign); 4 a large qref (rho < rmin); 5 a
    tiny qref (rho > rmax); 6 lateral inflow of mixed sign (a negative Oprev: rho < rmin); 7 a large beta (ta > ZMAX).  Reaches
    0 and 1 start at Oprev = rmin qref and rmax qref with qref a power of two: the exact ties.  wide: the widest range the entry
    points take, where only a zero or negative Oprev and huge sums leave it."""
    rmin, rmax = WIDE if wide else NARROW
    kind = np.arange(B) % 8
    kref = rng.uniform(0.5, 6.0, B)
    beta = rng.uniform(0.1, 0.9, B)
    X = rng.uniform(0.0, 0.5, B)
    qref = 10.0 ** rng.uniform(-0.5, 0.5, B)
    x = rng.random((T, B)) * 10.0 ** rng.integers(-1, 2, (T, B))
    state = rng.random((2, B)) * 3.0 + 0.05
    qref[kind == 4], qref[kind == 5] = 1e4, 1e-4
    n6 = int((kind == 6).sum())
    x[:, kind == 6] = NH.mixed(rng, T, n6)
    state[1, kind == 6] = -state[1, kind == 6]
    beta[kind == 7] = rng.uniform(40.0, 90.0, int((kind == 7).sum()))
    qref[0] = 2.0
    state[1, 0] = rmin * 2.0
    if B > 1:
        qref[1] = 0.5
        state[1, 1] = rmax * 0.5
    if T:
        x[0, B // 2] = -0.0
        x[T - 1, 0] = -0.0
    return x, NH.mixed(rng, T, B), np.stack([kref, beta, X, qref]), state, float(rng.choice([1.0, 0.25, 24.0])), (rmin, rmax)


def embed(rng, topo, M):
    """(down [M], slots [topo.B]): topo under an ORDER-PRESERVING relabelling b -> slots[b] (increasing) into a larger network
    whose other catchments form a forest of their own.  Only order-preserving: the inflow fold adds the upstream discharges in
    ascending index."""
    slots = np.sort(rng.permutation(M)[:topo.B])
    others = np.setdiff1d(np.arange(M), slots)
    down = np.full(M, -1, dtype=np.int64)
    down[slots] = np.where(topo.down >= 0, slots[np.maximum(topo.down, 0)], -1)
    for i, o in enumerate(others[1:], 1):
        down[o] = others[rng.integers(0, i)] if rng.random() > 0.2 else -1
    return down, slots


# ---- the host build --------------------------------------------------------------------------------------------------------
UNIT = _hostbuild.HostUnit(_HERE, "network_mc_host", "networkmchost", ["lgar_network_mc.hpp", "lgar_network.hpp", "lgar_baseflow.hpp"],
                           "Muskingum-Cunge network")


def library():
    """libnetworkmchost.so: networkmchost_<entry point>(the arguments of include/lgar.h without the stream), loaded once."""
    i32, vp, dbl = C.c_int32, C.c_void_p, C.c_double
    return UNIT.library({"network_route_mc": [vp, i32, i32, vp, dbl, dbl, dbl, vp, vp, i32, vp, vp, i32, vp, vp, vp],
                         "network_route_mc_grad": [vp, i32, i32, vp, dbl, dbl, dbl, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp],
                         "mc_ln": [vp, i32, vp]}, {"mc_ln": None})


def run(cases, sanitize=False):
    """ONE run of the host program over every case:
    ("route", topo, x, par, dt_h, (rmin, rmax), state_in or None, want_state) gives (y, state_out or None);
    ("grad", topo, gy, x, y, par, dt_h, (rmin, rmax), state_in or None, want_gpar, want_gstate) gives (gx, gpar or None, gstate or None);
    ("ln", x) gives (mc_ln(x),).
    topo: anything with the attributes of Topology (the arrays go to the program as they are: a test may corrupt them)."""
    calls, results = [], []
    for case in cases:
        op = case[0]
        if op == "ln":
            v = np.asarray(case[1], dtype=np.float64).ravel()
            results.append((out(True, len(v)),))
            calls.append((2, (len(v),), (), (v, results[-1][0])))
            continue
        topo = case[1]
        T, B = np.asarray(case[2]).shape
        assert B == topo.B and op in ("route", "grad")
        ints = (T, B, len(topo.up_idx), topo.n_levels)
        if op == "route":
            x, par, dt_h, (rmin, rmax), state, want = case[2:]
            assert np.asarray(par).shape == (4, B)
            y, state_out = out(True, T, B), out(want, 2, B)
            calls.append((0, ints, (dt_h, rmin, rmax), (f64(x), f64(par), i32(topo.up_ptr), i32(topo.up_idx), i32(topo.order), i32(topo.level_ptr),
                                                        f64(state), state_out, y)))
            results.append((y, state_out))
        else:
            gy, x, y, par, dt_h, (rmin, rmax), state, want_par, want_state = case[2:]
            assert np.asarray(par).shape == (4, B) and np.asarray(x).shape == (T, B) and np.asarray(y).shape == (T, B)
            gx, gpar, gstate = out(True, T, B), out(want_par, 3, B), out(want_state, 2, B)
            calls.append((1, ints, (dt_h, rmin, rmax), (f64(gy), f64(par), i32(topo.down), i32(topo.order), i32(topo.level_ptr), gx, f64(x), f64(y),
                                                        i32(topo.up_ptr), i32(topo.up_idx), f64(state), gpar, gstate)))
            results.append((gx, gpar, gstate))
    UNIT.run_calls(calls, sanitize)
    return [_hostbuild.values(r) for r in results]


def hip_library(*first):
    """The network host libraries under the HIP library's names (_hostbuild.AsHipLibrary): `first`, then this unit's for
    network_route_mc*, then tests/network_host's for the linear route."""
    return _hostbuild.AsHipLibrary(*first, ("network_route_mc", "networkmchost", library), ("", "networkhost", NH.library))


class SimCatchmentNetworkMC(CatchmentNetwork):
    """lgar_py_amd.network.CatchmentNetwork (device="cpu") with the host builds of the network kernels in the library's place:
    _open() is the only thing overridden."""

    def __init__(self, downstream):
        super().__init__(downstream, device="cpu")

    def _open(self):
        return hip_library()
