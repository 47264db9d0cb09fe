"""GPU (-m gpu): the Muskingum-Cunge catchment network -- lgar_network_route_mc / lgar_network_route_mc_grad through
network.CatchmentNetwork.route_mc and network.network_route_mc (autograd).

y[.][b] is a pure function of the columns of x and par in the upstream closure of b (include/lgar.h), so the
kernels are held BIT FOR BIT to the numpy statement of the definition (tests/network_mc_host: route_mc_ref, route_mc_grad_ref)
and to the host build of the same header -- and tests/test_network_mc_host.py holds the definition itself to statements that do
not come from it: mc_ln to mpmath.log, beta = 0 to the linear route, the adjoint to derivatives of the real-arithmetic statement."""
import os

import numpy as np
import pytest

from _golden import engine_keywords
from conftest import GOLDEN

import network_host as NH
import network_mc_host as MH

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GRID_CAP = 4096  # LGAR_NET_GRID_CAP (csrc/lgar_network_mc.hip): workgroups of a launch; the rest by stride
GPU_T = (0, 1, 9, 17)
TOPOLOGIES = NH.topologies()
REGIMES = ("inside", "low", "low_negative", "high", "tau_pos", "tau_neg", "big", "tie_low", "tie_high")


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return None if t is None else t.cpu().numpy()


def _network(topo):
    from lgar_py_amd.network import CatchmentNetwork
    net = CatchmentNetwork(topo.down)
    assert (net.order_host == topo.order).all() and (net.level_ptr == topo.level_ptr).all() and (net.up_idx_host == topo.up_idx).all()
    return net


@pytest.mark.parametrize("name", sorted(TOPOLOGIES))
def test_kernels_equal_the_numpy_definition_and_the_host_build_bit_for_bit(name):
    """Every topology of the grid x T in {0, 1, 9, 17} x the default and the widest range x state_in present or NULL: the forward
    with and without state_out, the adjoint with gpar and gstate / gpar / gstate / neither, through the raw entry points (the
    parameters include a beta the regime ta > ZMAX needs).  Against the numpy statement and against ONE run of the host program
    over the same cases.  Every regime of the row is taken (star257 and the forests; counted over this topology's cases where it
    has the reaches for it)."""
    topo = NH.Topology(TOPOLOGIES[name])
    net = _network(topo)
    rng = np.random.default_rng(1700 + topo.B)
    count = dict.fromkeys(REGIMES, 0)
    host_cases, got = [], []
    for T in GPU_T:
        for wide in (False, True):
            x, gy, par, state, dt, rr = MH.case_data(rng, T, topo.B, wide)
            dx, dgy, dpar = _cuda(x), _cuda(gy), _cuda(par)
            for st in (None, state):
                what = (name, T, wide, st is not None)
                dst = _cuda(st)
                y_ref, so_ref = MH.route_mc_ref(topo, x, par, dt, *rr, st)
                for k, v in MH.regimes(topo, x, par, dt, *rr, st).items():
                    count[k] += v
                y, so = net._forward_mc(dx, dpar, dt, *rr, dst, True)
                assert MH.same_bits(_np(y), y_ref) and MH.same_bits(_np(so), so_ref), what
                y2, so2 = net._forward_mc(dx, dpar, dt, *rr, dst, False)
                assert MH.same_bits(_np(y2), y_ref) and so2 is None, what
                host_cases.append(("route", topo, x, par, dt, rr, st, True))
                got.append((_np(y), _np(so)))
                ref = MH.route_mc_grad_ref(topo, gy, x, y_ref, par, dt, *rr, st)
                for want_par, want_state in ((True, True), (True, False), (False, True), (False, False)):
                    gx, gpar, gstate = net._backward_mc(dgy, dx, y, dpar, dt, *rr, dst, want_par, want_state)
                    assert MH.same_bits(_np(gx), ref[0]), what
                    assert (gpar is None) == (not want_par) and (gpar is None or MH.same_bits(_np(gpar), ref[1])), what
                    assert (gstate is None) == (not want_state) and (gstate is None or MH.same_bits(_np(gstate), ref[2])), what
                    if want_par and want_state:
                        host_cases.append(("grad", topo, gy, x, y_ref, par, dt, rr, st, True, True))
                        got.append((_np(gx), _np(gpar), _np(gstate)))
    for c, mine, theirs in zip(host_cases, got, MH.run(host_cases)):
        assert all(MH.same_bits(a, b) for a, b in zip(mine, theirs)), (name, c[0], np.asarray(c[2]).shape)
    print(name, count)
    if topo.B >= 8:
        assert all(count[k] > 0 for k in REGIMES), count
    else:
        assert count["low"] > 0 and count["tie_low"] > 0


def test_the_capped_grid_strides():
    """A launch has at most 4096 workgroups of 256 lanes.  One level of 256 x 4096 + 65 reaches, T = 9: the lanes stride over the
    level.  Forward and adjoint with every output against the numpy definition, bit for bit."""
    from lgar_py_amd.network import CatchmentNetwork
    width, T = 256 * GRID_CAP + 65, 9
    net = CatchmentNetwork(np.array(NH.wide(width), dtype=np.int32))
    topo = NH.Topology.of_network(net)
    assert int(np.diff(topo.level_ptr).max()) == width
    rng = np.random.default_rng(8)
    x, gy, par, state, dt, rr = MH.case_data(rng, T, topo.B)
    y_ref, so_ref = MH.route_mc_ref(topo, x, par, dt, *rr, state)
    dx, dpar, dst = _cuda(x), _cuda(par), _cuda(state)
    y, so = net._forward_mc(dx, dpar, dt, *rr, dst, True)
    assert MH.same_bits(_np(y), y_ref) and MH.same_bits(_np(so), so_ref)
    ref = MH.route_mc_grad_ref(topo, gy, x, y_ref, par, dt, *rr, state)
    got = net._backward_mc(_cuda(gy), dx, y, dpar, dt, *rr, dst, True, True)
    assert all(MH.same_bits(_np(a), b) for a, b in zip(got, ref))


@pytest.mark.parametrize("name", sorted(TOPOLOGIES))
def test_beta_zero_is_the_linear_route(name):
    """beta = 0: tau = 0, e = 1, K = kref exactly, and the row's coefficient formulas have the association of
    network.muskingum_coefficients: y equals lgar_network_route with muskingum_coefficients(kref, X, dt_h) computed by torch on the
    CPU, bit for bit -- a statement that does not come from the Muskingum-Cunge definition."""
    from lgar_py_amd.network import muskingum_coefficients
    topo = NH.Topology(TOPOLOGIES[name])
    net = _network(topo)
    rng = np.random.default_rng(2900 + topo.B)
    for T in (9, 17):
        x, _, par, state, dt, rr = MH.case_data(rng, T, topo.B)
        par[1] = 0.0
        coef = muskingum_coefficients(torch.from_numpy(par[0]), torch.from_numpy(par[2]), dt).cuda()
        for st in (None, state):
            want = net.route(_cuda(x), coef, carry=False, state=_cuda(st))
            got = net.route_mc(_cuda(x), _cuda(par[0]), 0.0, _cuda(par[2]), _cuda(par[3]), dt, carry=False, state=_cuda(st))
            assert torch.equal(got, want) and MH.same_bits(_np(got), NH.route_ref(topo, x, coef.cpu().numpy(), st)[0]), (name, T)


def test_chunked_repeated_and_relabelled_calls_give_the_same_bits():
    """route_mc(carry=True) cut at 1 row, at T - 1 rows and in the middle against one call, from zeros and from a given state; a
    repeated call; an order-preserving relabelling of the catchments gives the relabelled bits."""
    from lgar_py_amd.network import CatchmentNetwork
    topo = NH.Topology(TOPOLOGIES["random257"])
    net = _network(topo)
    rng = np.random.default_rng(23)
    T = 17
    x, gy, par, state, dt, rr = MH.case_data(rng, T, topo.B)
    par[1] = np.minimum(par[1], 0.9)
    dx, dp = _cuda(x), [_cuda(p) for p in par]
    for st in (None, state):
        want, want_state = MH.route_mc_ref(topo, x, par, dt, *rr, st)
        y = net.route_mc(dx, *dp, dt, carry=False, state=_cuda(st))
        assert MH.same_bits(_np(y), want) and net.mc_state_of() is None
        assert torch.equal(net.route_mc(dx, *dp, dt, carry=False, state=_cuda(st)), y)
        for cut in (1, T - 1, T // 2):
            key = (cut, st is None)
            a = net.route_mc(dx[:cut], *dp, dt, key=key, state=_cuda(st))
            b = net.route_mc(dx[cut:], *dp, dt, key=key)
            assert torch.equal(torch.cat([a, b]), y) and MH.same_bits(_np(net.mc_state_of(key)), want_state), cut
    assert net.state_of((1, True)) is None  # a key space of its own
    net.reset()
    assert net.mc_state_of((1, True)) is None
    # the whole network under an order-preserving relabelling into a larger network
    M = 300
    down2, slots = MH.embed(rng, topo, M)
    x2, gy2, par2, state2, _, _ = MH.case_data(rng, T, M)
    x2[:, slots], gy2[:, slots], par2[:, slots], state2[:, slots] = x, gy, par, state
    net2 = CatchmentNetwork(down2)
    y2, so2 = net2._forward_mc(_cuda(x2), _cuda(par2), dt, *rr, _cuda(state2), True)
    want, want_state = MH.route_mc_ref(topo, x, par, dt, *rr, state)
    assert MH.same_bits(_np(y2)[:, slots], want) and MH.same_bits(_np(so2)[:, slots], want_state)
    g2 = net2._backward_mc(_cuda(gy2), _cuda(x2), y2, _cuda(par2), dt, *rr, _cuda(state2), True, True)
    ref = MH.route_mc_grad_ref(topo, gy, x, want, par, dt, *rr, state)
    assert all(MH.same_bits(_np(a)[:, slots], b) for a, b in zip(g2, ref))


def test_a_nan_reaches_exactly_the_downstream_closure_from_its_row_on():
    topo = NH.Topology(TOPOLOGIES["random65"])
    net = _network(topo)
    rng = np.random.default_rng(41)
    T = 9
    x, _, par, state, dt, rr = MH.case_data(rng, T, topo.B)
    clean, _ = MH.route_mc_ref(topo, x, par, dt, *rr, state)
    t0, b = 4, int(np.nonzero(topo.level == 0)[0][3])
    x[t0, b] = np.nan
    y, so = net._forward_mc(_cuda(x), _cuda(par), dt, *rr, _cuda(state), True)
    hit = np.zeros((T, topo.B), dtype=bool)
    hit[t0:, topo.closure()[:, b]] = True  # every catchment b is upstream of (or is)
    assert hit[:, b].sum() == T - t0 and hit.sum() > T - t0
    assert (np.isnan(_np(y)) == hit).all() and MH.same_bits(_np(y)[~hit], clean[~hit])
    assert (np.isnan(_np(so)[1]) == hit[-1]).all()


def test_entry_points_refuse_bad_arguments():
    """LGAR_E_ARG from the library itself: everything lgar_network_route refuses, a dt_h that is not finite or <= 0, rmin / rmax not
    finite or outside 2^-60 <= rmin <= rmax <= 2^60, a null par, the adjoint's null x, y, up_ptr, gx, down, or a null up_idx with
    E > 0.  Nothing is launched by a refused call."""
    from lgar_py_amd import _capi
    lib = _capi.load()
    buf = torch.zeros(1024, dtype=torch.float64, device="cuda")
    ibuf = torch.zeros(64, dtype=torch.int32, device="cuda")
    p, q = buf.data_ptr(), ibuf.data_ptr()
    level_ptr = np.array([0, 4], dtype=np.int32)
    bad_levels = np.array([0, 3], dtype=np.int32)
    fwd = (("x", p), ("T", 2), ("B", 4), ("par", p), ("dt", 1.0), ("rmin", 1 / 64), ("rmax", 64.0), ("up_ptr", q), ("up_idx", q), ("E", 1),
           ("order", q), ("level_ptr", level_ptr.ctypes.data), ("L", 1), ("state_in", None), ("state_out", p + 2048), ("y", p + 4096))
    run = lambda **kw: lib.lgar_network_route_mc(*[kw.get(k, d) for k, d in fwd], None)
    nan, inf = float("nan"), float("inf")
    scalars = (dict(dt=0.0), dict(dt=-1.0), dict(dt=nan), dict(dt=inf), dict(rmin=nan), dict(rmax=nan), dict(rmax=inf), dict(rmin=-inf),
               dict(rmin=2.0 ** -61), dict(rmax=2.0 ** 61), dict(rmin=65.0), dict(rmin=0.0), dict(B=0, dt=0.0))
    for bad in (dict(T=-1), dict(B=-1), dict(E=-1), dict(L=-1), dict(x=None), dict(par=None), dict(T=0, par=None), dict(y=None), dict(up_ptr=None), dict(up_idx=None),
                dict(order=None), dict(level_ptr=None), dict(level_ptr=bad_levels.ctypes.data)) + scalars:
        assert run(**bad) == -1, bad
    grd = (("gy", p), ("T", 2), ("B", 4), ("par", p), ("dt", 1.0), ("rmin", 1 / 64), ("rmax", 64.0), ("down", q), ("order", q),
           ("level_ptr", level_ptr.ctypes.data), ("L", 1), ("gx", p + 2048), ("x", p), ("y", p), ("up_ptr", q), ("up_idx", q), ("E", 1),
           ("state_in", None), ("gpar", p + 4096), ("gstate", p + 6144))
    grad = lambda **kw: lib.lgar_network_route_mc_grad(*[kw.get(k, d) for k, d in grd], None)
    for bad in (dict(T=-1), dict(B=-1), dict(E=-1), dict(L=-1), dict(gy=None), dict(par=None), dict(T=0, par=None), dict(down=None), dict(order=None), dict(gx=None),
                dict(x=None), dict(y=None), dict(up_ptr=None), dict(up_idx=None), dict(level_ptr=None), dict(level_ptr=bad_levels.ctypes.data),
                dict(x=None, gpar=None, gstate=None)) + scalars:
        assert grad(**bad) == -1, bad
    torch.cuda.synchronize()
    assert not buf.any()
    # accepted: nothing to do, or a launch over zeros (qref = 0: the selects carry the NaN -- parameter values are not policed)
    assert run(B=0, x=None, par=None, y=None, level_ptr=None) == 0 and run(T=0, state_out=None, x=None, y=None) == 0
    assert run(E=0, up_idx=None) == 0 and run() == 0 and run(state_in=p, state_out=None) == 0 and run(T=0, x=None, y=None) == 0
    assert grad(B=0, gy=None, gx=None, level_ptr=None) == 0 and grad(T=0, gpar=None, gstate=None, gy=None, x=None) == 0
    assert grad() == 0 and grad(gpar=None) == 0 and grad(gstate=None) == 0 and grad(gpar=None, gstate=None) == 0 and grad(E=0, up_idx=None) == 0
    assert grad(T=0, gy=None, gx=None, x=None, y=None) == 0
    torch.cuda.synchronize()


def test_gradients_end_to_end():
    """lgar_series -> catchment_sum -> catchment_route -> network_route_mc -> catchment_moments -> loss("nse"): 24 columns of
    synth1_phil's soil in 3 catchments that form a chain (0 -> 1 -> 2); observations = the same chain on a perturbed parameter
    set.  The loss and the gradients to the soil parameters and to kref, beta, X are finite and non-zero; the routing node hands
    back the definition's bits (gx, gpar of route_mc_grad_ref for the gy it received)."""
    import lgar_py_amd as lg
    from lgar_py_amd import workloads as W
    from lgar_py_amd.autograd import lgar_series
    from lgar_py_amd.catchments import CatchmentMap, CatchmentRouting, catchment_route, catchment_sum
    from lgar_py_amd.network import network_route_mc
    from lgar_py_amd.scores import catchment_moments
    g = np.load(os.path.join(GOLDEN, "synth1_phil.npz"))
    n, B, K = 24, 3, 5
    base = {k: g[k] for k in W.PARAM_KEYS + ("thickness",)}
    Pn = W.perturbed_columns(n, frac=0.05, seed=21, base=base)
    Pobs = W.perturbed_columns(n, frac=0.05, seed=22, base=base)
    f = torch.tensor(g["forcing"], device="cuda")
    Tn = f.shape[0]
    pr, pe = f[:, 0:1].expand(Tn, n).contiguous(), f[:, 1:2].expand(Tn, n).contiguous()
    ekw = dict(engine_keywords(g), dtype=torch.float64)
    dt = float(ekw["dt_h"])
    ids = np.array([0] * 9 + [2] * 5 + [-1] + [1] * 9)[np.random.default_rng(1).permutation(n)]
    cmap = CatchmentMap(ids, weights=np.random.default_rng(2).random(n) + 0.5)
    rng = np.random.default_rng(3)
    routing = CatchmentRouting(g["giuh_ordinates"][None, :] * (1.0 + 0.2 * rng.random((B, K))))
    net = lg.CatchmentNetwork([1, 2, -1])
    topo = NH.Topology([1, 2, -1])
    leaf = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda", requires_grad=True)
    kref, beta, X = leaf([2.0, 3.0, 1.5]), leaf([0.4, 0.3, 0.5]), leaf([0.2, 0.1, 0.3])
    state0 = torch.tensor([[0.02, 0.05, 0.1], [0.02, 0.06, 0.1]], dtype=torch.float64, device="cuda")

    def discharge_of(Pdict, grad, qref):
        P = {k: torch.tensor(val, device="cuda") for k, val in Pdict.items()}
        for k in ("alpha", "n", "ksat"):
            P[k].requires_grad_(grad)
        statuses = []
        runoff, _ = lgar_series(P["alpha"], P["n"], P["ksat"], P["theta_e"], P["theta_r"], P["thickness"], pr, pe, check=False,
                                status_out=statuses, **ekw)
        lateral = catchment_route(catchment_sum(runoff, cmap, statuses[0]), routing)
        if grad:
            lateral.retain_grad()
        q = network_route_mc(lateral, net, kref, beta, X, qref, dt, state=state0)
        if grad:
            q.retain_grad()
        return P, lateral, q

    with torch.no_grad():
        lat0 = discharge_of(Pobs, False, 1.0)[1]
        qref = torch.clamp(lat0.mean(dim=0) * torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64, device="cuda"), min=1e-6)
        obs = discharge_of(Pobs, False, qref)[2].clone()
    assert tuple(obs.shape) == (Tn, B) and float(obs.abs().max()) > 0
    score = lg.CatchmentScore(obs)
    P, lateral, q = discharge_of(Pn, True, qref)
    loss = score.loss(catchment_moments(q, score), "nse")
    loss.backward()
    assert np.isfinite(float(loss.detach())) and float(loss.detach()) > 0
    par_np = np.stack([_np(kref.detach()), _np(beta.detach()), _np(X.detach()), _np(qref)])
    x_np = _np(lateral.detach())
    y_ref, _ = MH.route_mc_ref(topo, x_np, par_np, dt, 1.0 / 64.0, 64.0, _np(state0))
    assert MH.same_bits(_np(q.detach()), y_ref)
    reg = MH.regimes(topo, x_np, par_np, dt, 1.0 / 64.0, 64.0, _np(state0))
    assert reg["inside"] > 0
    gx_ref, gpar_ref, _ = MH.route_mc_grad_ref(topo, _np(q.grad), x_np, y_ref, par_np, dt, 1.0 / 64.0, 64.0, _np(state0))
    assert MH.same_bits(_np(lateral.grad), gx_ref) and float(np.abs(gx_ref).max()) > 0
    assert MH.same_bits(np.stack([_np(kref.grad), _np(beta.grad), _np(X.grad)]), gpar_ref)
    for name, t in (("kref", kref), ("beta", beta), ("X", X)):
        assert bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().min()) > 0, name
    for kind in ("alpha", "n", "ksat"):
        assert bool(torch.isfinite(P[kind].grad).all()) and float(P[kind].grad.abs().max()) > 0, kind
