"""TEST INFRASTRUCTURE ONLY: the host build of the catchment-network header (lgar_py_amd/csrc/lgar_network.hpp, compiled for the
host with -DLGAR_DEVSIM) and its front-end.  network_host.hpp holds the host-side launchers of the two entry points;
network_host.cpp is the stand-alone program around them (run() below; also built with AddressSanitizer + UBSan),
libnetworkhost.so the same header as a shared library (library(): what SimCatchmentNetwork puts behind the product's calling
surface).  The numpy statement of the definition (include/lgar.h, lgar_network_route / lgar_network_route_grad; DESIGN.md section
14) -- route_ref, adjoint_ref and coef_grad_ref: plain loops over rows and over the reaches in `order`, a level's reaches side by
side -- the topology builders and the data of the tests' cases live here too.
The build, the program's call records (tests/_hostprog.hpp) and same_bits are tests/_hostbuild.py's: UNIT below.
Never imported by the product package.
"""
import ctypes as C
import os

import numpy as np

import _hostbuild
from _hostbuild import f64, i32, out, same_bits  # noqa: F401
from lgar_py_amd.network import CatchmentNetwork

_HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE_T = (0, 1, 2, 7, 8, 9, 17)  # around the row chunk of 8
COEFS = ("muskingum", "accumulate", "lag", "mixed")


class Topology:
    """The arrays of include/lgar.h for a `down` array, built by plain loops (independently of lgar_py_amd.network): level,
    order (by level, then index), level_ptr, up_ptr / up_idx (ascending within a list)."""

    def __init__(self, down):
        down = np.asarray(down, dtype=np.int32)
        B = len(down)
        ups = [[] for _ in range(B)]
        for b in range(B):  # ascending b: every list ascending
            if down[b] >= 0:
                ups[down[b]].append(b)
        level = np.full(B, -1, dtype=np.int64)
        for _ in range(B + 1):  # a level is known once every upstream level is
            todo = [b for b in range(B) if level[b] < 0 and all(level[u] >= 0 for u in ups[b])]
            for b in todo:
                level[b] = 1 + max((level[u] for u in ups[b]), default=-1)
            if not todo:
                break
        assert (level >= 0).all(), "not a forest"
        self.B, self.down, self.level = B, down, level
        self.n_levels = int(level.max()) + 1 if B else 0
        self.order = np.array(sorted(range(B), key=lambda b: (level[b], b)), dtype=np.int32)
        self.level_ptr = np.array([0] + [int((level <= l).sum()) for l in range(self.n_levels)], dtype=np.int32)
        self.up_ptr = np.array([0] + list(np.cumsum([len(u) for u in ups])), dtype=np.int32)
        self.up_idx = np.array([u for lst in ups for u in lst], dtype=np.int32)
        self.E = len(self.up_idx)
        self.ups = ups

    @classmethod
    def of_network(cls, net):
        """The arrays a CatchmentNetwork built (test_network_host.py holds them to the loops above): for networks too large for
        those loops."""
        t = cls.__new__(cls)
        t.B, t.E, t.n_levels, t.down, t.level = net.B, net.n_edges, net.n_levels, net.downstream_host, net.levels.astype(np.int64)
        t.order, t.level_ptr, t.up_ptr, t.up_idx = net.order_host, net.level_ptr, net.up_ptr_host, net.up_idx_host
        return t

    def copy(self):
        t = Topology.__new__(Topology)
        t.__dict__ = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in self.__dict__.items()}
        return t

    def closure(self):
        """R[b, a] = True iff a is b or upstream of b: (1 + A) multiplied with itself, as booleans, until it stops changing."""
        R = np.eye(self.B, dtype=bool)
        for b in range(self.B):
            if self.down[b] >= 0:
                R[self.down[b], b] = True
        while True:
            R2 = (R.astype(np.int64) @ R.astype(np.int64)) > 0
            if (R2 == R).all():
                return R
            R = R2


def single():
    return [-1]


def two():
    return [1, -1]


def chain(n):
    """0 -> 1 -> ... -> n - 1: n levels of one reach."""
    return list(range(1, n)) + [-1]


def star(n):
    """n - 1 headwaters into reach n // 2: one reach of in-degree n - 1, its upstream indices on both sides of its own."""
    return [n // 2 if b != n // 2 else -1 for b in range(n)]


def binary_tree(n):
    """A full binary tree in heap numbering (n = 2^k - 1), the outlet first: down[b] is below b."""
    return [-1] + [(b - 1) // 2 for b in range(1, n)]


def forest(n):
    """Three outlets with a tree each (catchments 8 ..), and catchments 3 .. 7 isolated: outlets without upstream."""
    down = [-1] * n
    for b in range(8, n):
        down[b] = b % 3 if b < 14 else 8 + (b * 7) % (b - 8)
    return down


def random_forest(n, seed, roots=0.05):
    """A random forest (catchment i drains into a random earlier one, or is an outlet with probability `roots`), renumbered
    at random: down[b] is both above and below b and `order` is not the identity."""
    rng = np.random.default_rng(seed)
    down = [-1] + [int(rng.integers(0, i)) if rng.random() >= roots else -1 for i in range(1, n)]
    perm = rng.permutation(n)
    out = np.full(n, -1, dtype=np.int64)
    for i in range(n):
        out[perm[i]] = perm[down[i]] if down[i] >= 0 else -1
    return out.tolist()


def wide(width, mids=3):
    """One level exactly `width` wide: `width` headwaters into `mids` reaches that drain into one outlet."""
    return [width + b % mids for b in range(width)] + [width + mids] * mids + [-1]


def topologies():
    """name -> down, every topology of the grid."""
    t = {"single": single(), "two": two(), "chain65": chain(65), "star257": star(257), "tree63": binary_tree(63),
         "tree127": binary_tree(127), "forest64": forest(64), "forest65": forest(65), "wide64": wide(64), "wide65": wide(65)}
    for n in (63, 64, 65, 257):
        t["random%d" % n] = random_forest(n, n)
    return t


# ---- the definition, in numpy ----------------------------------------------------------------------------------------------
def _inflow(topo, x, y, bs):
    """I[:, i] = x[:, bs[i]], then + y[:, up] for the upstream lists of bs in ascending entry, one rounded add each."""
    I = x[:, bs].copy()
    deg = topo.up_ptr[bs + 1] - topo.up_ptr[bs]
    for k in range(int(deg.max()) if len(bs) else 0):
        sel = deg > k
        I[:, sel] = I[:, sel] + y[:, topo.up_idx[topo.up_ptr[bs[sel]] + k]]
    return I


def route_ref(topo, x, coef, state=None):
    """(y [T, B], state_out [2, B]): the levels in ascending order, the rows in ascending order."""
    x, coef = np.asarray(x, dtype=np.float64), np.asarray(coef, dtype=np.float64)
    T, B = x.shape
    y = np.zeros((T, B))
    out = np.zeros((2, B)) if state is None else np.array(state, dtype=np.float64)
    with np.errstate(all="ignore"):
        for l in range(topo.n_levels):
            bs = topo.order[topo.level_ptr[l]:topo.level_ptr[l + 1]].astype(np.int64)
            c0, c1, c2 = coef[0, bs], coef[1, bs], coef[2, bs]
            I = _inflow(topo, x, y, bs)
            Iprev, Oprev = out[0, bs], out[1, bs]
            for t in range(T):
                O = (c0 * I[t] + c1 * Iprev) + c2 * Oprev
                y[t, bs] = O
                Iprev, Oprev = I[t], O
            out[0, bs], out[1, bs] = Iprev, Oprev
    return y, out


def _back(topo, gy, coef, x=None, y=None, state=None):
    gy, coef = np.asarray(gy, dtype=np.float64), np.asarray(coef, dtype=np.float64)
    T, B = gy.shape
    gx = np.zeros((T, B))
    gc = np.zeros((3, B)) if x is not None else None
    st = np.zeros((2, B)) if state is None else np.asarray(state, dtype=np.float64)
    with np.errstate(all="ignore"):
        for l in range(topo.n_levels - 1, -1, -1):
            bs = topo.order[topo.level_ptr[l]:topo.level_ptr[l + 1]].astype(np.int64)
            c0, c1, c2 = coef[0, bs], coef[1, bs], coef[2, bs]
            d = topo.down[bs].astype(np.int64)
            has = d >= 0
            a = gy[:, bs].copy()
            a[:, has] = a[:, has] + gx[:, d[has]]
            if gc is not None:
                I = np.concatenate([st[0:1, bs], _inflow(topo, x, y, bs)])   # I[t + 1] = the inflow of row t; I[0] = I[-1]
                yb = np.concatenate([st[1:2, bs], y[:, bs]])
                g0, g1, g2 = np.zeros(len(bs)), np.zeros(len(bs)), np.zeros(len(bs))
            lam_next = np.zeros(len(bs))
            for t in range(T - 1, -1, -1):
                lam = a[t] + c2 * lam_next
                gx[t, bs] = c0 * lam + c1 * lam_next
                if gc is not None:
                    g0, g1, g2 = g0 + lam * I[t + 1], g1 + lam * I[t], g2 + lam * yb[t]
                lam_next = lam
            if gc is not None:
                gc[0, bs], gc[1, bs], gc[2, bs] = g0, g1, g2
    return gx, gc


def adjoint_ref(topo, gy, coef):
    """gx [T, B]: the levels in descending order, the rows in descending order."""
    return _back(topo, gy, coef)[0]


def coef_grad_ref(topo, x, y, gy, coef, state=None):
    """gc [3, B], each accumulator from +0.0 in decreasing t; I re-formed from x and y by the forward's fold."""
    return _back(topo, gy, coef, np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), state)[1]


# ---- data ------------------------------------------------------------------------------------------------------------------
def mixed(rng, *shape):
    """Mixed signs over several decades."""
    return (rng.random(shape) - 0.4) * 10.0 ** rng.integers(-3, 3, shape)


def muskingum_np(K, X, dt):
    """c0, c1, c2 of the header's formula, in numpy."""
    K, X = np.asarray(K, dtype=np.float64), np.asarray(X, dtype=np.float64)
    D = K - K * X + 0.5 * dt
    return np.stack([(0.5 * dt - K * X) / D, (0.5 * dt + K * X) / D, (K - K * X - 0.5 * dt) / D])


def coefficients(rng, kind, B):
    if kind == "muskingum":
        return muskingum_np(0.5 + 5.0 * rng.random(B), 0.5 * rng.random(B), 1.0)
    if kind == "accumulate":
        return np.stack([np.ones(B), np.zeros(B), np.zeros(B)])
    if kind == "lag":
        return np.stack([np.zeros(B), np.ones(B), np.zeros(B)])
    assert kind == "mixed"
    return rng.standard_normal((3, B)) * 0.8


def case_data(rng, T, B, kind):
    """x, gy [T, B] (x with -0.0), coef [3, B], state [2, B]"""
    x, gy, state = mixed(rng, T, B), mixed(rng, T, B), mixed(rng, 2, B)
    if T:
        x[0, B // 2] = -0.0
        x[T - 1, 0] = -0.0
    return x, gy, coefficients(rng, kind, B), state


# ---- the host build --------------------------------------------------------------------------------------------------------
UNIT = _hostbuild.HostUnit(_HERE, "network_host", "networkhost", ["lgar_network.hpp"], "catchment-network")


def library():
    """libnetworkhost.so: networkhost_<entry point>(the arguments of include/lgar.h without the stream), loaded once."""
    i32, vp = C.c_int32, C.c_void_p
    return UNIT.library({"network_route": [vp, i32, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp],
                         "network_route_grad": [vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp]})


def run(cases, sanitize=False):
    """ONE run of the host program over every case:
    ("route", topo, x, coef, state_in or None, want_state) gives (y, state_out or None);
    ("grad", topo, gy, coef, x, y, state_in) -- x = y = None: no coefficient gradient -- gives (gx, gc or None).
    topo: anything with the attributes of Topology (the arrays go to the program as they are: a test may corrupt them)."""
    calls, results = [], []
    for case in cases:
        op, topo, z, coef = case[:4]
        T, B = np.asarray(z).shape
        assert B == topo.B and np.asarray(coef).shape == (3, B) and op in ("route", "grad")
        ints = (T, B, len(topo.up_idx), topo.n_levels)
        if op == "route":
            y, state_out = out(True, T, B), out(case[5], 2, B)
            calls.append((0, ints, (), (f64(z), f64(coef), i32(topo.up_ptr), i32(topo.up_idx), i32(topo.order), i32(topo.level_ptr), f64(case[4]),
                                        state_out, y)))
            results.append((y, state_out))
        else:
            x, y, state = case[4], case[5], case[6]
            gx, gc = out(True, T, B), out(x is not None, 3, B)
            more = (f64(x), f64(y), i32(topo.up_ptr), i32(topo.up_idx), f64(state)) if x is not None else (None,) * 5
            calls.append((1, ints, (), (f64(z), f64(coef), i32(topo.down), i32(topo.order), i32(topo.level_ptr), gx, *more, gc)))
            results.append((gx, gc))
    UNIT.run_calls(calls, sanitize)
    return [_hostbuild.values(r) for r in results]


class SimCatchmentNetwork(CatchmentNetwork):
    """lgar_py_amd.network.CatchmentNetwork (device="cpu") with the host build of the network kernels in the library's place."""

    def __init__(self, downstream):
        super().__init__(downstream, device="cpu")

    def _open(self):
        return _hostbuild.AsHipLibrary(("", "networkhost", library))
