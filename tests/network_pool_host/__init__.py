"""TEST INFRASTRUCTURE ONLY: the host build of the reach-and-pool network header (lgar_py_amd/csrc/lgar_network_pool.hpp, compiled
for the host with -DLGAR_DEVSIM) and its front-end.  network_pool_host.hpp holds the host-side launchers of the two entry points;
network_pool_host.cpp is the stand-alone program around them (run() below; also built with AddressSanitizer + UBSan),
libnetworkpoolhost.so the same header as a shared library (library(): what SimCatchmentNetworkPool puts behind the product's
calling surface).  The numpy statement of the definition (include/lgar.h, lgar_network_route_pool / lgar_network_route_pool_grad;
DESIGN.md section 18) -- route_pool_ref, route_pool_grad_ref and pool_regimes: plain loops over rows and over the nodes in the
pool-aware `order`, a level's reaches side by side and then its pools side by side -- and the data of the tests' cases live here
too; the topologies and the inflow fold are tests/network_host's, the reach row (_row), mc_ln_ref and the reach data are
tests/network_mc_host's, gw_exp_ref is tests/baseflow_host's.
The build, the program's call records (tests/_hostprog.hpp) and same_bits are tests/_hostbuild.py's: UNIT below.
Never imported by the product package.
"""
import ctypes as C
import os

import numpy as np

import _hostbuild
import network_host as NH
import network_mc_host as MH
from _hostbuild import f64, i32, out
from baseflow_host import ZMAX, gw_exp_ref
from lgar_py_amd.network import CatchmentNetwork
from network_host import Topology, same_bits  # noqa: F401
from network_mc_host import mc_ln_ref

_HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE_T = (0, 1, 2, 7, 8, 9, 17)  # around the row chunk of 8
PNARROW, PWIDE = (2.0 ** -20, 2.0 ** 20), (2.0 ** -60, 2.0 ** 60)  # prmin, prmax: the Python layer's default, and the widest allowed
PLACEMENTS = ("none", "all", "outlets", "headwaters", "alternate", "random10", "level64", "level65", "poollevel")
POOL_REGIMES = ("inside", "lo", "hi", "big", "free", "limited", "empty", "empty_dry", "spill", "no_spill_inf", "tie_lo", "tie_hi", "tie_free",
                "tie_ex")


# ---- which nodes are pools -------------------------------------------------------------------------------------------------
class PoolTopology:
    """A Topology and the pools on it, built by plain loops (independently of lgar_py_amd.network.NetworkPools): every attribute
    of the Topology, but `order` sorted by (level, is_pool, index); pool_ptr[n_levels]; pool_slot[B]; nodes[P]; is_pool[B]."""

    def __init__(self, topo, nodes):
        self.__dict__.update({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in topo.__dict__.items()})
        self.base = topo
        self.nodes = np.asarray(nodes, dtype=np.int32).reshape(-1)
        self.P = len(self.nodes)
        self.is_pool = np.zeros(self.B, dtype=bool)
        self.pool_slot = np.full(self.B, -1, dtype=np.int32)
        for s, b in enumerate(self.nodes):
            assert not self.is_pool[b]
            self.is_pool[b], self.pool_slot[b] = True, s
        self.order = np.array(sorted(range(self.B), key=lambda b: (self.level[b], self.is_pool[b], b)), dtype=np.int32)
        self.pool_ptr = np.array([int(self.level_ptr[l]) + int(((self.level == l) & ~self.is_pool).sum()) for l in range(self.n_levels)],
                                 dtype=np.int32)

    @classmethod
    def of_pools(cls, pools):
        """The arrays a NetworkPools built (test_network_pool_host.py holds them to the loops above): for networks too large for
        those loops."""
        t = cls.__new__(cls)
        t.__dict__.update(Topology.of_network(pools.network).__dict__)
        t.base, t.nodes, t.P, t.is_pool = None, pools.nodes_host, pools.P, pools.is_pool
        t.order, t.pool_ptr, t.pool_slot = pools.order_host, pools.pool_ptr, pools.pool_slot_host
        return t

    def copy(self):
        t = PoolTopology.__new__(PoolTopology)
        t.__dict__ = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self.__dict__.items()}
        return t

    def reaches(self, l):
        return self.order[self.level_ptr[l]:self.pool_ptr[l]].astype(np.int64)

    def pools(self, l):
        return self.order[self.pool_ptr[l]:self.level_ptr[l + 1]].astype(np.int64)


def placement(topo, kind, rng):
    """The pools (catchment ids, in an order that is NOT ascending: slots and catchments do not run alike) of one placement:
    none; all; outlets only; headwaters only; every other level; a random 10 % (at least one); the first 64 / 65 nodes of the
    widest level (as many as it has); every node of the widest level with more than one level below the top, or of level 0."""
    B, level = topo.B, topo.level
    widest = int(np.argmax(np.diff(topo.level_ptr))) if B else 0
    if kind == "none":
        nodes = np.zeros(0, dtype=np.int64)
    elif kind == "all":
        nodes = np.arange(B)
    elif kind == "outlets":
        nodes = np.nonzero(topo.down < 0)[0]
    elif kind == "headwaters":
        nodes = np.nonzero(level == 0)[0]
    elif kind == "alternate":
        nodes = np.nonzero(level % 2 == 1)[0] if topo.n_levels > 1 else np.arange(B)
    elif kind == "random10":
        nodes = rng.permutation(B)[:max(1, B // 10)]
    elif kind in ("level64", "level65"):
        nodes = np.nonzero(level == widest)[0][:int(kind[5:])]
    else:
        assert kind == "poollevel"
        nodes = np.nonzero(level == (widest if widest > 0 else min(1, topo.n_levels - 1)))[0]
    return rng.permutation(np.asarray(nodes, dtype=np.int64))


# ---- the definition, in numpy ----------------------------------------------------------------------------------------------
def _pool_row(S, vin, cq, m, s0, sref, cap, dt, prmin, prmax):
    """One pool row from S and the volume in: a, rho, L, tau, e, Ql, qa, ex, O, S and the flags"""
    a = S - s0
    rho = a / sref
    lo = rho < prmin
    hi = ~lo & (rho > prmax)
    rc = np.where(lo, prmin, np.where(hi, prmax, rho))
    L = mc_ln_ref(rc)
    tau = m * L
    ta = np.where(tau < 0.0, -tau, tau)
    big = ta > ZMAX
    e = gw_exp_ref(np.where(big, ZMAX, ta))
    up = tau > 0.0
    Ql = np.where(up, cq * e, cq / e)
    av = a + vin
    qa = av / dt
    free = Ql < qa
    Q0 = np.where(free, Ql, qa)
    empty = Q0 < 0.0
    Q = np.where(empty, 0.0, Q0)
    r = av - dt * Q
    ex = r - cap
    spill = ex > 0.0
    O = np.where(spill, Q + ex / dt, Q)
    Snew = np.where(spill, cap, r) + s0
    return dict(a=a, rho=rho, L=L, tau=tau, e=e, up=up, Ql=Ql, qa=qa, av=av, ex=ex, O=O, S=Snew, lo=lo, hi=hi, big=big, free=free, empty=empty,
                spill=spill, inside=~lo & ~hi & ~big)


def _walk(pt, x, par_mc, par_pool, dt_h, rr, prr, state, rows=None):
    x, par_mc, par_pool = (np.asarray(a, dtype=np.float64) for a in (x, par_mc, par_pool))
    T, B = x.shape
    dt = np.float64(dt_h)
    half, rmin, rmax, prmin, prmax = 0.5 * dt, np.float64(rr[0]), np.float64(rr[1]), np.float64(prr[0]), np.float64(prr[1])
    y, storage = np.zeros((T, B)), np.zeros((T, pt.P))
    out = np.zeros((2, B)) if state is None else np.array(state, dtype=np.float64)
    with np.errstate(all="ignore"):
        for l in range(pt.n_levels):
            bs = pt.reaches(l)  # the reach row of tests/network_mc_host, as it is
            if len(bs):
                kref, beta, X, qref = par_mc[0, bs], par_mc[1, bs], par_mc[2, bs], par_mc[3, bs]
                I = NH._inflow(pt, x, y, bs)
                Iprev, Oprev = out[0, bs], out[1, bs]
                for t in range(T):
                    r = MH._row(Oprev, kref, beta, X, qref, half, rmin, rmax)
                    O = (r["c0"] * I[t] + r["c1"] * Iprev) + r["c2"] * Oprev
                    y[t, bs] = O
                    Iprev, Oprev = I[t], O
                out[0, bs], out[1, bs] = Iprev, Oprev
            bs = pt.pools(l)
            if len(bs):
                sl = pt.pool_slot[bs].astype(np.int64)
                cq, m, s0, sref = par_pool[0, sl], par_pool[1, sl], par_pool[2, sl], par_pool[3, sl]
                cap = par_pool[4, sl] - s0
                I = NH._inflow(pt, x, y, bs)
                Iprev, S = out[0, bs], out[1, bs]
                for t in range(T):
                    r = _pool_row(S, half * (I[t] + Iprev), cq, m, s0, sref, cap, dt, prmin, prmax)
                    if rows is not None:
                        for k, v in rows.items():
                            v[t, sl] = I[t] if k == "I" else (Iprev if k == "Iprev" else (S if k == "Sprev" else r[k]))
                    y[t, bs], storage[t, sl] = r["O"], r["S"]
                    Iprev, S = I[t], r["S"]
                out[0, bs], out[1, bs] = Iprev, S
    return y, out, storage


def route_pool_ref(pt, x, par_mc, par_pool, dt_h, rr, prr, state=None):
    """(y [T, B], state_out [2, B], storage [T, P]): the levels in ascending order, a level's reaches and then its pools, the rows
    in ascending order."""
    return _walk(pt, x, par_mc, par_pool, dt_h, rr, prr, state)


_ROW_KEYS = ("rho", "Ql", "qa", "ex", "a", "av", "tau", "I", "Iprev", "Sprev", "lo", "hi", "big", "inside", "free", "empty", "spill")


def pool_rows(pt, x, par_mc, par_pool, dt_h, rr, prr, state=None, keys=_ROW_KEYS):
    """name -> [T, P]: the row's values and flags at every pool, by slot."""
    T = np.asarray(x).shape[0]
    rows = {k: np.zeros((T, pt.P), dtype=(bool if k in ("lo", "hi", "big", "inside", "free", "empty", "spill") else np.float64)) for k in keys}
    _walk(pt, x, par_mc, par_pool, dt_h, rr, prr, state, rows)
    return rows


def _regimes(r, par_pool, prr, P):
    inf = np.isinf(np.asarray(par_pool)[4])[None, :] & np.ones(r["lo"].shape, dtype=bool) if P else r["lo"]
    n = lambda m: int(np.sum(m))
    return dict(inside=n(r["inside"]), lo=n(r["lo"]), hi=n(r["hi"]), big=n(r["big"]), free=n(r["free"] & ~r["empty"]),
                limited=n(~r["free"] & ~r["empty"] & ~np.isnan(r["qa"])), empty=n(r["empty"]), empty_dry=n(r["empty"] & (r["a"] < 0)),
                spill=n(r["spill"]), no_spill_inf=n(inf), tie_lo=n(r["rho"] == prr[0]), tie_hi=n(r["rho"] == prr[1]), tie_free=n(r["Ql"] == r["qa"]),
                tie_ex=n(r["ex"] == 0.0))


def pool_regimes(pt, x, par_mc, par_pool, dt_h, rr, prr, state=None):
    """The count of pool rows per regime: inside; lo (rho < prmin); hi; big (|tau| > ZMAX); free (the release law, not cut to
    zero); limited (what would drain the pool to s0, not cut to zero); empty (cut to zero), of them empty_dry (a < 0: S below s0);
    spill; no_spill_inf (smax = +inf); the exact ties rho == prmin, rho == prmax, Ql == qa, ex == 0."""
    return _regimes(pool_rows(pt, x, par_mc, par_pool, dt_h, rr, prr, state), par_pool, prr, pt.P)


def route_pool_ref_and_regimes(pt, x, par_mc, par_pool, dt_h, rr, prr, state=None):
    """route_pool_ref and pool_regimes from ONE walk: (y, state_out, storage, regimes)."""
    T = np.asarray(x).shape[0]
    rows = {k: np.zeros((T, pt.P), dtype=(bool if k in ("lo", "hi", "big", "inside", "free", "empty", "spill") else np.float64)) for k in _ROW_KEYS}
    y, out, storage = _walk(pt, x, par_mc, par_pool, dt_h, rr, prr, state, rows)
    return y, out, storage, _regimes(rows, par_pool, prr, pt.P)


def route_pool_grad_ref(pt, gy, x, y, storage, par_mc, par_pool, dt_h, rr, prr, state=None, variant=None):
    """(gx [T, B], gpar_mc [3, B], gpool [4, P], gstate [2, B]): the levels in descending order, the rows in descending order; a
    reach by the rows of tests/network_mc_host.route_mc_grad_ref, a pool by the rows of include/lgar.h with the regime re-formed
    from the stored storage; every accumulator from +0.0, left as it is in a row that gives it no term.  variant: one of the
    WRONG pool adjoints the bound test must refuse -- "no_dqda" (the gQ m Ql / a term dropped), "no_limited" (the limited branch's
    gQ / dt dropped), "gcap_sign" (gcap with the wrong sign), "pI_row" (the row's own half gav where the row above's belongs)."""
    gy, x, y, storage, par_mc, par_pool = (np.asarray(a, dtype=np.float64) for a in (gy, x, y, storage, par_mc, par_pool))
    T, B = gy.shape
    dt = np.float64(dt_h)
    half, rmin, rmax, prmin, prmax = 0.5 * dt, np.float64(rr[0]), np.float64(rr[1]), np.float64(prr[0]), np.float64(prr[1])
    gx, gpar, gpool, gstate = np.zeros((T, B)), np.zeros((3, B)), np.zeros((4, pt.P)), np.zeros((2, B))
    st = np.zeros((2, B)) if state is None else np.asarray(state, dtype=np.float64)
    with np.errstate(all="ignore"):
        for l in range(pt.n_levels - 1, -1, -1):
            for pools in (False, True):
                bs = pt.pools(l) if pools else pt.reaches(l)
                n = len(bs)
                if not n:
                    continue
                d = pt.down[bs].astype(np.int64)
                has = d >= 0
                a = gy[:, bs].copy()
                a[:, has] = a[:, has] + gx[:, d[has]]
                I = np.concatenate([st[0:1, bs], NH._inflow(pt, x, y, bs)])  # I[t + 1] = the inflow of row t; I[0] = I[-1]
                if not pools:
                    kref, beta, X, qref = par_mc[0, bs], par_mc[1, bs], par_mc[2, bs], par_mc[3, bs]
                    omx = 1.0 - X
                    yb = np.concatenate([st[1:2, bs], y[:, bs]])
                    pI, pO, g0, g1, g2 = (np.zeros(n) for _ in range(5))
                    for t in range(T - 1, -1, -1):
                        It, Ip, Op = I[t + 1], I[t], yb[t]
                        r = MH._row(Op, kref, beta, X, qref, half, rmin, rmax)
                        c0, c1, c2, K, D = r["c0"], r["c1"], r["c2"], r["K"], r["D"]
                        lam = a[t] + pO
                        gx[t, bs] = c0 * lam + pI
                        dK = ((It * (-(X + c0 * omx)) + Ip * (X - c1 * omx)) + Op * (omx * (1.0 - c2))) / D
                        GK = lam * dK
                        dX = ((It * (-(1.0 - c0)) + Ip * (1.0 + c1)) + Op * (-(1.0 - c2))) * (K / D)
                        g0 = g0 + GK * (K / kref)
                        g1 = np.where(r["big"], g1, g1 + GK * (-(K * r["L"])))
                        g2 = g2 + lam * dX
                        c2l = c2 * lam
                        pI = c1 * lam
                        pO = np.where(r["inside"], c2l + GK * ((-(beta * K)) / Op), c2l)
                    gpar[0, bs], gpar[1, bs], gpar[2, bs] = g0, g1, g2
                    gstate[0, bs], gstate[1, bs] = pI, pO
                    continue
                sl = pt.pool_slot[bs].astype(np.int64)
                cq, m, s0, sref = par_pool[0, sl], par_pool[1, sl], par_pool[2, sl], par_pool[3, sl]
                cap = par_pool[4, sl] - s0
                sb = np.concatenate([st[1:2, bs], storage[:, sl]])
                pI, pS, g0, g1, g2, g3 = (np.zeros(n) for _ in range(6))
                for t in range(T - 1, -1, -1):
                    r = _pool_row(sb[t], half * (I[t + 1] + I[t]), cq, m, s0, sref, cap, dt, prmin, prmax)
                    lamO, lamS = a[t], pS
                    q = lamO / dt
                    gr = np.where(r["spill"], q, lamS)
                    gcap = (q - lamS) if variant == "gcap_sign" else (lamS - q)
                    gQ = np.where(r["empty"], 0.0, lamO - dt * gr)
                    gav = gr if variant == "no_limited" else np.where(r["free"], gr, gr + gQ / dt)
                    ga = gav if variant == "no_dqda" else np.where(r["free"] & r["inside"], gav + ((gQ * m) * r["Ql"]) / r["a"], gav)
                    pw = np.where(r["up"], r["e"], 1.0 / r["e"])
                    g0 = np.where(r["free"], g0 + gQ * pw, g0)
                    g1 = np.where(r["free"] & ~r["big"], g1 + (gQ * r["Ql"]) * r["L"], g1)
                    g2 = (g2 + np.where(r["spill"], lamS - gcap, lamS)) - ga
                    g3 = np.where(r["spill"], g3 + gcap, g3)
                    hg = half * gav
                    gx[t, bs] = hg + (hg if variant == "pI_row" else pI)
                    pI, pS = hg, ga
                gpool[0, sl], gpool[1, sl], gpool[2, sl], gpool[3, sl] = g0, g1, g2, g3
                gstate[0, bs], gstate[1, bs] = pI, pS
    return gx, gpar, gpool, gstate


# ---- data ------------------------------------------------------------------------------------------------------------------
def case_data(rng, pt, T, wide=False):
    """x, gy [T, B], par_mc [4, B], par_pool [5, P], state [2, B], dt_h, (rmin, rmax), (prmin, prmax).  The reach data are
    tests/network_mc_host.case_data's.  The pools take turns (slot mod 8) so that every regime of the pool row is taken
    somewhere: 0 an ordinary pool that fills and spills; 1 smax = +inf; 2 a huge sref (rho < prmin); 3 a tiny sref (rho > prmax);
    4 an m of 4.5 - 6 far from rc = 1 (|tau| > ZMAX: only the raw entry points are handed that); 5 lateral inflow of mixed sign
    and S below s0 at the start (empty); 6 a huge cq (limited: the pool drains to s0 every row); 7 the exact ties, by
    (slot // 8) mod 4: rho == prmin and rho == prmax at row 0 (sref a power of two, s0 = 0), Ql == qa at row 0 (m = 0, cq set
    to the row's own qa) and ex == 0 at row 0 (cq = 0, smax set to the row's own r); the last two take the inflow of row 0
    from a first walk -- it does not depend on the pool's own parameters."""
    B, P = pt.B, pt.P
    x, gy, par_mc, state, dt, rr = MH.case_data(rng, T, B, wide)
    prr = PWIDE if wide else PNARROW
    kind = np.arange(P) % 8
    sub = (np.arange(P) // 8) % 4
    nodes = pt.nodes.astype(np.int64)
    cq, m = rng.uniform(0.1, 2.0, P), rng.uniform(0.5, 2.5, P)
    s0, sref = rng.uniform(0.0, 2.0, P), 10.0 ** rng.uniform(-0.5, 0.5, P)
    smax = s0 + rng.uniform(2.0, 8.0, P)
    S = s0 + rng.random(P) * 3.0 + 0.05
    smax[kind == 1] = np.inf
    sref[kind == 2], sref[kind == 3] = 1e9, 1e-9
    m[kind == 4], sref[kind == 4] = rng.uniform(4.5, 6.0, int((kind == 4).sum())), 1e-4
    x[:, nodes[kind == 5]] = NH.mixed(rng, T, int((kind == 5).sum()))
    S[kind == 5] = s0[kind == 5] - rng.random(int((kind == 5).sum())) - 0.1
    cq[kind == 6] = 1e3
    tie = kind == 7
    s0[tie] = 0.0
    sref[tie & (sub == 0)], sref[tie & (sub == 1)] = 2.0, 0.5
    S[tie & (sub == 0)], S[tie & (sub == 1)] = prr[0] * 2.0, prr[1] * 0.5
    smax[tie & (sub == 1)] = np.inf
    m[tie & (sub == 2)], cq[tie & (sub == 3)] = 0.0, 0.0
    smax[tie & (sub == 2)] = np.inf
    state[1, nodes] = S
    par_pool = np.stack([cq, m, s0, sref, smax])
    late = tie & (sub >= 2)
    if T and late.any():
        first = pool_rows(pt, x[:1], par_mc, par_pool, dt, rr, prr, state, keys=("I", "Iprev"))
        with np.errstate(all="ignore"):
            av = (S - s0) + (0.5 * np.float64(dt)) * (first["I"][0] + first["Iprev"][0])  # a + vin of row 0, the row's own operations
        ok = late & np.isfinite(av) & (av > 0.0)
        par_pool[0, ok & (sub == 2)] = (av / np.float64(dt))[ok & (sub == 2)]
        par_pool[4, ok & (sub == 3)] = av[ok & (sub == 3)]  # cap = smax - 0 = r = av - dt * 0
    return x, gy, par_mc, par_pool, state, dt, rr, prr


# ---- the host build --------------------------------------------------------------------------------------------------------
UNIT = _hostbuild.HostUnit(_HERE, "network_pool_host", "networkpoolhost",
                           ["lgar_network_pool.hpp", "lgar_network_mc.hpp", "lgar_network.hpp", "lgar_baseflow.hpp"], "reach-and-pool network")


def library():
    """libnetworkpoolhost.so: networkpoolhost_<entry point>(the arguments of include/lgar.h without the stream), loaded once."""
    i32, vp, dbl = C.c_int32, C.c_void_p, C.c_double
    return UNIT.library({"network_route_pool": [vp, i32, i32, vp, vp, i32, dbl, dbl, dbl, dbl, dbl, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp],
                         "network_route_pool_grad": [vp, i32, i32, vp, vp, i32, dbl, dbl, dbl, dbl, dbl, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp,
                                                     vp, i32, vp, vp, vp, vp],
                         "release": [vp, vp, i32, dbl, dbl, vp]}, {"release": None})


def run(cases, sanitize=False):
    """ONE run of the host program over every case:
    ("route", pt, x, par_mc, par_pool, dt_h, rr, prr, state_in or None, want_state, want_storage) gives (y, state_out or None,
        storage or None);
    ("grad", pt, gy, x, y, storage, par_mc, par_pool, dt_h, rr, prr, state_in or None, want_gpar, want_gpool, want_gstate) gives
        (gx, gpar_mc or None, gpool or None, gstate or None);
    ("release", rc, m, prr) gives (the row's Ql for cq = 1,).
    pt: anything with the attributes of PoolTopology (the arrays go to the program as they are: a test may corrupt them)."""
    calls, results = [], []
    for case in cases:
        op = case[0]
        if op == "release":
            v, m, prr = (np.asarray(case[1], dtype=np.float64).ravel(), np.asarray(case[2], dtype=np.float64).ravel(), case[3])
            assert len(v) == len(m)
            results.append((out(True, len(v)),))
            calls.append((2, (len(v),), tuple(prr), (v, m, results[-1][0])))
            continue
        pt = case[1]
        T, B = np.asarray(case[2]).shape
        P = pt.P
        assert B == pt.B and op in ("route", "grad")
        ints, slot = (T, B, len(pt.up_idx), pt.n_levels, P), i32(pt.pool_slot) if P else None
        if op == "route":
            x, par_mc, par_pool, dt_h, rr, prr, state, want_state, want_storage = case[2:]
            assert np.asarray(par_mc).shape == (4, B) and np.asarray(par_pool).shape == (5, P)
            y, state_out, storage = out(True, T, B), out(want_state, 2, B), out(want_storage, T, P)
            calls.append((0, ints, (dt_h, *rr, *prr), (f64(x), f64(par_mc), f64(par_pool), i32(pt.up_ptr), i32(pt.up_idx), i32(pt.order),
                                                       i32(pt.level_ptr), i32(pt.pool_ptr), slot, f64(state), state_out, y, storage)))
            results.append((y, state_out, storage))
        else:
            gy, x, y, storage, par_mc, par_pool, dt_h, rr, prr, state, want_par, want_pool, want_state = case[2:]
            assert np.asarray(par_mc).shape == (4, B) and np.asarray(par_pool).shape == (5, P) and np.asarray(x).shape == (T, B)
            assert np.asarray(y).shape == (T, B) and np.asarray(storage).shape == (T, P)
            gx, gpar, gpool, gstate = out(True, T, B), out(want_par, 3, B), out(want_pool, 4, P), out(want_state, 2, B)
            calls.append((1, ints, (dt_h, *rr, *prr), (f64(gy), f64(par_mc), f64(par_pool), i32(pt.down), i32(pt.order), i32(pt.level_ptr),
                                                       i32(pt.pool_ptr), slot, gx, f64(x), f64(y), f64(storage), i32(pt.up_ptr), i32(pt.up_idx),
                                                       f64(state), gpar, gpool, gstate)))
            results.append((gx, gpar, gpool, gstate))
    UNIT.run_calls(calls, sanitize)
    return [_hostbuild.values(r) for r in results]


class SimCatchmentNetworkPool(CatchmentNetwork):
    """lgar_py_amd.network.CatchmentNetwork (device="cpu") with the host builds of the network kernels in the library's place:
    _open() is the only thing overridden."""

    def __init__(self, downstream):
        super().__init__(downstream, device="cpu")

    def _open(self):
        return MH.hip_library(("network_route_pool", "networkpoolhost", library))
