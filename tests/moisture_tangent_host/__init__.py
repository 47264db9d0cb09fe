"""TEST INFRASTRUCTURE ONLY: the host build of the soil-moisture tangent (lgar_py_amd/csrc/lgar_moisture_tangent.hpp, compiled for
the host with -DLGAR_DEVSIM) and its front-end.  moisture_tangent_host.hpp holds the host-side launcher of the entry point;
moisture_tangent_host.cpp is the stand-alone program around it (run() below; also built with AddressSanitizer + UBSan),
libmthost.so the same header as a shared library (library(): what MoistureTangentSimEngine puts behind the product's calling
surface, and what host_call() calls on numpy arrays).  The numpy statement of the definition (include/lgar.h,
lgar_soil_moisture_tangent) -- profile_tangent_ref and contraction_ref, with post_host.moisture.profile_ref
as the model -- the lanes of the tests' cases, the planted ties and the case grid the host suite and the GPU suite share live
here too.  Never imported by the product package.
"""
import ctypes as C
import itertools
import os

import numpy as np

import _hostbuild
import forced_host
from _hostbuild import Out, same_bits  # noqa: F401
from lgar_py_amd import _capi
from lgar_py_amd._capi import F32, F64, MOIST_WHAT, LgarDims, LgarParams, LgarState

_HERE = os.path.dirname(os.path.abspath(__file__))
SHAPE_M = (1, 2, 63, 64, 65, 257)  # columns; a case has M * group lanes
GROUPS = (1, 3, 9)
MODES = ("out", "cot", "both")
BASES = ("grad_synth0_12h", "grad_manyfronts_60")
SEVEN = (0.0, 5.0, 10.0, 30.0, 60.0, 100.0, 250.0, 300.0)  # its last bin lies wholly below a 200 cm column
BIN_SETS = ("layers", 1, 7, 9, 17, 32)  # the layers; one bin; SEVEN; one past each unroll capacity (8, 16) and the cap


# ---- the definition, in numpy ----------------------------------------------------------------------------------------------
def _clip(x, a, b):
    x = np.where(x < a, a, x)
    return np.where(x > b, b, x)


def profile_tangent_ref(depth, theta, flags, n_fronts, ddepth, dtheta, thickness, edges=None, what="theta"):
    """The definition as a numpy loop over a tangent state laid out as the engine lays it out: depth / theta / ddepth / dtheta
    [F, M], flags uint8 [F, M], n_fronts [M], thickness [L, M]; edges [D + 1], or None for each lane's own layers.  Returns
    (m' fp64 [D, M], unrounded; live bool [D, M]): front by front, bin by bin, plain fp64 multiplies and adds in the kernel's
    order, every decision a select; n_fronts clamped to [0, F] and layer tags to L - 1 as the kernel clamps them."""
    depth, theta, ddepth, dtheta, thickness = (np.asarray(a).astype(np.float64) for a in (depth, theta, ddepth, dtheta, thickness))
    F, M = depth.shape
    L = thickness.shape[0]
    cols = np.arange(M)
    top = np.zeros((L + 1, M))
    for l in range(L):
        top[l + 1] = top[l] + thickness[l]
    E = top if edges is None else np.repeat(np.asarray(edges, dtype=np.float64)[:, None], M, axis=1)
    D = E.shape[0] - 1
    nf = np.clip(np.asarray(n_fronts).astype(np.int64), 0, F)
    S, prev_d, prev_dd, prev_k = np.zeros((D, M)), np.zeros(M), np.zeros(M), np.full(M, -1)
    with np.errstate(all="ignore"):
        for j in range(int(nf.max(initial=0))):
            live = j < nf
            k = np.minimum(np.asarray(flags[j]).astype(np.int64) & 0x7F, L - 1)
            same = k == prev_k
            t = np.where(same, prev_d, top[k, cols])
            dt = np.where(same, prev_dd, 0.0)
            d, dd = depth[j], ddepth[j]
            at_d, at_t = theta[j] * dd, theta[j] * dt
            for i in range(D):
                a, b = E[i], E[i + 1]
                first = dtheta[j] * (_clip(d, a, b) - _clip(t, a, b))
                second = np.where((d >= a) & (d < b), at_d, 0.0)
                third = np.where((t >= a) & (t < b), at_t, 0.0)
                S[i] = np.where(live, ((S[i] + first) + second) - third, S[i])
            prev_d, prev_dd, prev_k = np.where(live, d, prev_d), np.where(live, dd, prev_dd), np.where(live, k, prev_k)
        if what == "storage":
            return S, np.ones((D, M), dtype=bool)
        w = _clip(top[L][None, :], E[:-1], E[1:]) - E[:-1]
        return np.where(w > 0, S / np.where(w > 0, w, 1.0), 0.0), w > 0


def contraction_ref(m, live, cot, group, grad):
    """grad [M] (its dtype kept) + the contraction of the unrounded fp64 bin tangents with cot [D, M // group], in the stated order:
    acc from +0.0, bins ascending, a dead bin's product discarded by a select, one add into grad rounded once."""
    lane = np.arange(m.shape[1]) // group
    acc = np.zeros(m.shape[1])
    with np.errstate(all="ignore"):
        for i in range(m.shape[0]):
            acc = acc + np.where(live[i], cot[i, lane] * m[i], 0.0)
        return (grad.astype(np.float64) + acc).astype(grad.dtype)


# ---- the host build --------------------------------------------------------------------------------------------------------
UNIT = _hostbuild.HostUnit(_HERE, "moisture_tangent_host", "mthost", ["lgar_moisture_tangent.hpp", "lgar_moisture.hpp"], "soil-moisture tangent")
_ARGTYPES = [C.POINTER(LgarDims), C.POINTER(LgarParams), C.POINTER(LgarState), C.POINTER(LgarState), C.c_void_p, C.c_int32, C.c_int32,
             C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]


def library():
    """libmthost.so: mthost_soil_moisture_tangent(the arguments of include/lgar.h without the stream), loaded once."""
    return UNIT.library({"soil_moisture_tangent": _ARGTYPES})


class MoistureTangentSimEngine(forced_host.ForcedSimEngine):
    """The product's LgarEngine over the device-code simulator and the window / forced host builds (window_host.WindowSimEngine,
    forced_host.ForcedSimEngine), with lgar_soil_moisture_tangent on the host build above: everything else about
    soil_moisture_tangent is the product's own code."""

    def _call(self, name, *args, counters=None):
        if name != "soil_moisture_tangent":
            return super()._call(name, *args, counters=counters)
        _capi.check(library().mthost_soil_moisture_tangent(*args, self._dt), "moisture_tangent_host: lgar_" + name)


def install():
    """Put MoistureTangentSimEngine behind the autograd functions (in THIS process); returns what to put back."""
    import lgar_py_amd.autograd as A
    before = A.LgarEngine
    A.LgarEngine = MoistureTangentSimEngine
    return before


# ---- cases -----------------------------------------------------------------------------------------------------------------
# A case is a dict: depth, theta, ddepth, dtheta [F, lanes] (float32 or float64: the case's dtype), flags uint8 [F, lanes], n_fronts
# int32 [lanes], thickness [L, lanes] (dtype), edges ([D + 1] or None), what, mode ("out" | "cot" | "both"), group, cot fp64
# [D, lanes // group], grad [lanes] (dtype): what grad holds before the call.  It gives (out [D, lanes] or None, grad or None).
def n_bins(c):
    return c["thickness"].shape[0] if c["edges"] is None else len(c["edges"]) - 1


def reference(c):
    m, live = profile_tangent_ref(c["depth"], c["theta"], c["flags"], c["n_fronts"], c["ddepth"], c["dtheta"], c["thickness"], c["edges"], c["what"])
    dt = c["depth"].dtype
    return (m.astype(dt) if c["mode"] != "cot" else None,
            contraction_ref(m, live, c["cot"], c["group"], c["grad"]) if c["mode"] != "out" else None)


def _arrays(c):
    dt = c["depth"].dtype
    return [np.ascontiguousarray(c[k], dtype=typ) for k, typ in (("thickness", dt), ("depth", dt), ("theta", dt), ("flags", np.uint8),
                                                                  ("n_fronts", np.int32), ("ddepth", dt), ("dtheta", dt))]


def host_call(c, entry=None):
    """One case on numpy arrays through the host library (or `entry`, a function with its argument list): (rc, out, grad)."""
    entry = entry or library().mthost_soil_moisture_tangent
    dt = c["depth"].dtype
    F, lanes = c["depth"].shape
    thick, depth, theta, flags, nf, dd, dth = keep = _arrays(c)
    dims = LgarDims()
    dims.n_columns, dims.n_layers, dims.front_slots = lanes, thick.shape[0], F
    p = LgarParams()
    p.thickness = thick.ctypes.data
    s, ds = LgarState(), LgarState()
    s.depth, s.theta, s.flags, s.n_fronts = depth.ctypes.data, theta.ctypes.data, flags.ctypes.data, nf.ctypes.data
    ds.depth, ds.theta = dd.ctypes.data, dth.ctypes.data
    D = n_bins(c)
    edges = None if c["edges"] is None else np.ascontiguousarray(c["edges"], dtype=np.float64)
    out = np.full((D, lanes), np.nan, dtype=dt) if c["mode"] != "cot" else None
    cot = np.ascontiguousarray(c["cot"], dtype=np.float64) if c["mode"] != "out" else None
    grad = np.array(c["grad"], dtype=dt) if c["mode"] != "out" else None
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = entry(C.byref(dims), C.byref(p), C.byref(s), C.byref(ds), ptr(edges), D, MOIST_WHAT[c["what"]], ptr(out), ptr(cot), c["group"],
               ptr(grad), F64 if dt == np.float64 else F32)
    del keep
    return rc, out, grad


def run(cases, sanitize=False):
    """ONE run of the stand-alone program over every case: [(out or None, grad or None)]."""
    calls, results = [], []
    for c in cases:
        dt = c["depth"].dtype
        F, lanes = c["depth"].shape
        D = n_bins(c)
        out = Out(dt, D, lanes) if c["mode"] != "cot" else None
        grad = Out(dt, lanes, start=c["grad"]) if c["mode"] != "out" else None
        cot = np.ascontiguousarray(c["cot"], dtype=np.float64) if c["mode"] != "out" else None
        edges = None if c["edges"] is None else np.ascontiguousarray(c["edges"], dtype=np.float64)
        ints = [F64 if dt == np.float64 else F32, c["thickness"].shape[0], F, lanes, D, MOIST_WHAT[c["what"]], c["group"]]
        calls.append((0, ints, (), _arrays(c) + [edges, out, cot, grad]))
        results.append((out, grad))
    UNIT.run_calls(calls, sanitize)
    return [_hostbuild.values(r) for r in results]


def check(c, got, where=""):
    want = reference(c)
    for name, w, g in zip(("out", "grad"), want, got):
        assert (w is None) == (g is None), (where, name)
        assert w is None or same_bits(g, w), (where, name, c["mode"], c["what"], c["group"], n_bins(c), c["depth"].shape)


def base_state(engine, g, direction_seed=0):
    """The end TangentState of ONE column of a gradient fixture along a fixed mixed direction, as a dict of numpy arrays (fp64):
    depth, theta, ddepth, dtheta [F, 1], flags [F, 1], n_fronts [1], thickness [L, 1].  engine: an engine of one column over the
    fixture's soil (the simulator's, or the library's on the GPU)."""
    import torch
    rng = np.random.default_rng(7 + direction_seed)
    L = engine.L
    direction = {k: torch.tensor(rng.uniform(0.5, 1.5, (L, 1)) * s) for k, s in (("alpha", 0.01), ("n", 1.0), ("ksat", 1.0))}
    f = torch.tensor(g["forcing"])
    _, _, st, end = engine.tangent_window(direction, f[:, 0:1].contiguous(), f[:, 1:2].contiguous())
    assert int(st[0]) == 0
    v, t = end.value, end.tangent
    n = lambda x: x.cpu().numpy().copy()
    return dict(depth=n(v.depth), theta=n(v.theta), flags=n(v.flags), n_fronts=n(v.n_fronts), ddepth=n(t["depth"]), dtheta=n(t["theta"]),
                thickness=n(engine.thickness))


def lanes_of(base, lanes, dtype, seed):
    """`lanes` lanes from a one-column base state: replicated, every depth, content and tangent moved by its own random factor
    (depths by up to 2 %, so fronts move across edges and past each other now and then: signed widths), n_fronts cut for a third
    of the lanes (a wave's lanes end their row loop at different rows), in `dtype`."""
    rng = np.random.default_rng(seed)
    F = base["depth"].shape[0]
    rep = lambda a: np.repeat(a, lanes, axis=-1)
    c = dict(depth=rep(base["depth"]) * rng.uniform(0.98, 1.02, (F, lanes)), theta=rep(base["theta"]) * rng.uniform(0.97, 1.03, (F, lanes)),
             ddepth=rep(base["ddepth"]) * rng.uniform(0.5, 1.5, (F, lanes)), dtheta=rep(base["dtheta"]) * rng.uniform(0.5, 1.5, (F, lanes)),
             flags=rep(base["flags"]).copy(), thickness=rep(base["thickness"]).copy())
    nf = rep(base["n_fronts"]).astype(np.int32)
    cut = rng.random(lanes) < 1.0 / 3.0
    c["n_fronts"] = np.where(cut, np.maximum(1, nf - rng.integers(1, 4, lanes)), nf).astype(np.int32)
    for k in ("depth", "theta", "ddepth", "dtheta", "thickness"):
        c[k] = np.ascontiguousarray(c[k].astype(dtype))
    return c


def edges_of(which, Z):
    """A bin set of BIN_SETS for a column Z cm deep: None (the layers) or the fp64 edges"""
    if which == "layers":
        return None
    if which == 1:
        return np.array([0.0, 60.0])
    if which == 7:
        return np.array(SEVEN)
    return np.linspace(0.0, Z + 20.0, which + 1)


def with_call(c, edges, what, mode, group, seed):
    """The case of a state `c` (lanes_of) for one call: bins, `what`, the outputs wanted, the group and random cot / grad."""
    rng = np.random.default_rng(seed)
    lanes = c["depth"].shape[1]
    assert lanes % group == 0
    c = dict(c, edges=edges, what=what, mode=mode, group=group)
    c["cot"] = (rng.random((n_bins(c), lanes // group)) - 0.4) * 10.0 ** rng.integers(-2, 2, (n_bins(c), lanes // group))
    c["grad"] = ((rng.random(lanes) - 0.5) * 3.0).astype(c["depth"].dtype)
    return c


def grid(bases, shapes=SHAPE_M, keep_every=1, dtypes=(np.float64, np.float32)):
    """The bit-for-bit grid: base state x dtype x what x bin set x M, and at each of these points the three modes, the group
    rotating with the point and the mode so that every (mode, group) pair meets every bin set, dtype and `what`.  bases:
    {name: base_state()}.  keep_every = n keeps every n-th case; dtypes: the part of the grid in these.  Yields (label, case)."""
    n = 0
    for pi, (name, dtype, what, which, M) in enumerate(itertools.product(sorted(bases), (np.float64, np.float32), ("theta", "storage"), BIN_SETS, shapes)):
        if dtype not in dtypes:
            continue
        base = bases[name]
        Z = float(base["thickness"].astype(np.float64).sum())
        for mi, mode in enumerate(MODES):
            n += 1
            if n % keep_every:
                continue
            group = GROUPS[(pi + mi) % len(GROUPS)]
            state = lanes_of(base, M * group, dtype, seed=1000 * pi + mi)
            yield "%s %s %s bins=%s M=%d %s group=%d" % (name, np.dtype(dtype).name, what, which, M, mode, group), \
                with_call(state, edges_of(which, Z), what, mode, group, seed=pi)


def _hand_table(dtype, rows, thickness=(44.0, 131.0, 25.0), F=8):
    """One lane from rows of (depth, theta, layer tag, d', theta')"""
    c = dict(depth=np.zeros((F, 1), dtype), theta=np.zeros((F, 1), dtype), ddepth=np.zeros((F, 1), dtype), dtheta=np.zeros((F, 1), dtype),
             flags=np.zeros((F, 1), np.uint8), n_fronts=np.array([len(rows)], np.int32), thickness=np.array(thickness, dtype)[:, None])
    for j, (d, th, k, dd, dth) in enumerate(rows):
        c["depth"][j], c["theta"][j], c["flags"][j], c["ddepth"][j], c["dtheta"][j] = d, th, k, dd, dth
    return c


def ties(dtype=np.float64):
    """The planted ties, each with the side it must take: [(label, case, {(output, bin): exact expected value})].  Storage, the
    edges of SEVEN, one lane, cot = 1 under every bin (and NaN under the dead one where the case says so), grad = 0."""
    f = lambda x: dtype(x).astype(np.float64)  # the value as the state holds it
    out = []
    # front 0 sits exactly on the interior edge 10 with d' = 2; front 1 (same layer) therefore has its top t = 10 on that edge,
    # with t' = 2: both belong to the bin [10, 30) (x >= a) and neither to [5, 10) (x < b fails)
    rows = [(10.0, 0.3, 0, 2.0, 0.0), (44.0, 0.2, 0, 0.0, 0.0), (175.0, 0.25, 1, 0.0, 0.0), (200.0, 0.35, 2, 0.0, 0.0)]
    c = with_call(_hand_table(dtype, rows), np.array(SEVEN), "storage", "both", 1, seed=1)
    c["cot"], c["grad"] = np.ones_like(c["cot"]), np.zeros_like(c["grad"])
    lower = ((0.0 + 0.0) + f(0.3) * f(2.0)) - 0.0            # front 0: second
    lower = ((lower + 0.0) + 0.0) - f(0.2) * f(2.0)          # front 1: third
    out.append(("a front and a top exactly on an interior edge", c, {("out", 1): 0.0, ("out", 2): lower}))
    # theta: the bin [250, 300] lies wholly below the 200 cm column: its tangent is +0.0 and a NaN cotangent under it is discarded
    rows = [(7.0, 0.3, 0, 1.5, 0.01), (44.0, 0.2, 0, 0.0, 0.02), (175.0, 0.25, 1, 0.0, 0.0), (200.0, 0.35, 2, 0.0, 0.0)]
    c = with_call(_hand_table(dtype, rows), np.array(SEVEN), "theta", "both", 1, seed=2)
    c["cot"][6] = np.nan
    out.append(("a bin wholly below the column under a NaN cotangent", c, {("out", 6): 0.0}))
    # a front above its predecessor (signed widths): front 1 at 20 cm under front 0 at 35 cm, same layer
    rows = [(35.0, 0.3, 0, 1.0, 0.01), (20.0, 0.28, 0, 0.5, 0.02), (44.0, 0.2, 0, 0.0, 0.0), (175.0, 0.25, 1, 0.0, 0.0), (200.0, 0.35, 2, 0.0, 0.0)]
    out.append(("a non-monotone table", with_call(_hand_table(dtype, rows), np.array(SEVEN), "storage", "both", 1, seed=3), {}))
    return out


def corrupt(base, dtype=np.float64, lanes=66):
    """A corrupt table: n_fronts far out of range on both sides and layer tags beyond the layers, in every other lane.  The
    kernel clamps both and must stay in bounds (the program allocates every array at its exact size)."""
    c = lanes_of(base, lanes, dtype, seed=99)
    c["n_fronts"][0::4] = 1000
    c["n_fronts"][1::4] = -3
    c["n_fronts"][2::4] = np.iinfo(np.int32).max
    c["flags"][:, ::2] = 0xFF
    return [with_call(c, e, what, "both", 3, seed=5) for e in (None, np.array(SEVEN)) for what in ("theta", "storage")]


# ---- reference parity ------------------------------------------------------------------------------------------------------
KINDS = ("alpha", "n", "ksat")


def mgrad(name):
    """An opened fixture of tests/golden/make_moisture_grad_golden.py"""
    return np.load(os.path.join(_hostbuild.ROOT, "tests", "golden", "moisture_grad", "mgrad_" + name + ".npz"))


def reference_parity(make_engine, name, mode, share_group=False):
    """One column of a fixture along its 3 L one-hot directions, side by side, through tangent_window from a fresh state to every
    recorded row; the storage tangent of both bin sets against the reference's J, their sum over the covering bins against its dV, per kind against
    GRADIENT * max over the fixture's rows and bins of |J| of that kind; the front count of every end state.  share_group: the
    nine lanes read ONE forcing column (forcing_group), as the backward pass lays them out.  Returns the worst ratio."""
    import torch

    import _golden as G
    g, m = G.load(name), mgrad(name)
    L = g["alpha"].shape[0]
    D = 3 * L
    eng = make_engine(name, D, search_mode=mode)
    dev = eng.device
    f = torch.tensor(g["forcing"], device=dev)
    assert np.array_equal(m["forcing"], g["forcing"])
    cols = 1 if share_group else D
    pr, pe = f[:, 0:1].expand(-1, cols).contiguous(), f[:, 1:2].expand(-1, cols).contiguous()
    direction = {k: torch.zeros(L, D, dtype=torch.float64, device=dev) for k in KINDS}
    for ki, k in enumerate(KINDS):
        for l in range(L):
            direction[k][l, ki * L + l] = 1.0
    ff = float(g["frozen_factor"])
    scale = np.array([1.0, 1.0, ff])[None, None, :, None]  # the reference's Parameter is Ksat x frozen_factor, the engine's input Ksat
    sets = {"fixed": m["edges_fixed"], "layers": None}
    J = {key: m["J_" + key] * scale for key in sets}
    bars = {key: G.GRADIENT * np.abs(J[key]).max(axis=(0, 1, 3)) for key in sets}  # per kind
    assert all((b > 0).all() for b in bars.values())
    worst = 0.0
    for r, row in enumerate(m["rows"]):
        hi = int(row) + 1
        _, _, st, state = eng.tangent_window(direction, pr[:hi], pe[:hi], forcing_group=D if share_group else 1)
        assert int(st.abs().max()) == 0
        assert (state.value.n_fronts.cpu().numpy() == m["n_fronts"][r]).all(), (name, row)
        for key, edges in sets.items():
            got = eng.soil_moisture_tangent(state, edges, "storage").cpu().numpy().reshape(-1, 3, L)  # [bins, kind, layer]
            for ki in range(3):
                err = np.abs(got[:, ki] - J[key][r][:, ki]).max() / bars[key][ki]
                closure = np.abs(got[:, ki].sum(0) - m["dV"][r, ki] * scale[0, 0, ki, 0]).max() / bars[key][ki]
                worst = max(worst, err, closure)
                assert err <= 1.0 and closure <= 1.0, (name, mode, int(row), key, KINDS[ki], err, closure)
    print("%s mode %d%s: worst |got - J| or closure miss = %.3g of the bar" % (name, mode, " (shared group)" if share_group else "", worst))
    return worst
