"""GPU (-m gpu): the catchment network with reaches and level-pool reservoirs -- lgar_network_route_pool /
lgar_network_route_pool_grad through network.CatchmentNetwork.route_pool and network.network_route_pool (autograd).

y[.][b] is a pure function of the columns of x and of the parameters in the upstream closure of b (include/lgar.h; DESIGN.md
section 18), so the kernels are held BIT FOR BIT to the numpy statement of the definition (tests/network_pool_host:
route_pool_ref, route_pool_grad_ref) and to the host build of the same header -- and tests/test_network_pool_host.py holds the
definition itself to statements that do not come from it."""
import os

import numpy as np
import pytest

from _golden import engine_keywords
from conftest import GOLDEN

import network_host as NH
import network_mc_host as MH
import network_pool_host as PH

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GRID_CAP = 4096  # LGAR_NET_GRID_CAP (csrc/lgar_network_pool.hip): workgroups of a launch; the rest by stride
GPU_T = (0, 1, 9, 17)
TOPOLOGIES = NH.topologies()


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return None if t is None else t.cpu().numpy()


def _network(pt):
    """(CatchmentNetwork, NetworkPools) of pt, their arrays held to pt's."""
    from lgar_py_amd.network import CatchmentNetwork, NetworkPools
    net = CatchmentNetwork(pt.down)
    pools = NetworkPools(net, pt.nodes)
    assert (pools.order_host == pt.order).all() and (pools.pool_ptr == pt.pool_ptr).all() and (pools.pool_slot_host == pt.pool_slot).all()
    assert (net.level_ptr == pt.level_ptr).all() and (net.up_idx_host == pt.up_idx).all()
    return net, pools


def _scalars(dt, rr, prr):
    return (dt, rr[0], rr[1], prr[0], prr[1])


GRID = [(name, part) for name in sorted(TOPOLOGIES) for part in range(3)]  # a topology's nine placements, three at a time
COUNT = dict.fromkeys(PH.POOL_REGIMES, 0)  # pool rows per regime over the grid cases that have run
RAN = set()


@pytest.mark.parametrize("name,part", GRID)
def test_kernels_equal_the_numpy_definition_and_the_host_build_bit_for_bit(name, part):
    """One topology of the grid x three of the nine pool placements x T in {0, 1, 9, 17} x the default and the widest ranges x
    state_in present or NULL, in full: the forward with state_out and storage wanted or not (all four), the adjoint with gpar_mc,
    gpool and gstate wanted or not (all eight).  Through the raw entry points (the parameters include the m the regime
    |tau| > ZMAX needs).  Against the numpy statement and against ONE run of the host program over the same cases.  Where a
    placement of the case has 32 pools or more (every kind of pool and every tie of the data, tests/network_pool_host.case_data)
    every regime of the pool row is counted and asserted here; the counts of all cases are asserted once more, together, by
    test_every_regime_of_the_pool_row_was_taken."""
    topo = NH.Topology(TOPOLOGIES[name])
    rng = np.random.default_rng(1800 + 3 * topo.B + part)
    count = dict.fromkeys(PH.POOL_REGIMES, 0)
    host_cases, got = [], []
    most = 0
    for kind in PH.PLACEMENTS[part::3]:
        pt = PH.PoolTopology(topo, PH.placement(topo, kind, rng))
        net, pools = _network(pt)
        most = max(most, pt.P)
        for T in GPU_T:
            for wide in (False, True):
                x, gy, pm, pp, state, dt, rr, prr = PH.case_data(rng, pt, T, wide)
                sc = _scalars(dt, rr, prr)
                dx, dgy, dpm, dpp = _cuda(x), _cuda(gy), _cuda(pm), _cuda(pp)
                for st in (None, state):
                    what = (name, kind, T, wide, st is not None)
                    dst = _cuda(st)
                    y_ref, so_ref, sg_ref, regimes = PH.route_pool_ref_and_regimes(pt, x, pm, pp, dt, rr, prr, st)
                    for key, v in regimes.items():
                        count[key] += v
                    for want_state in (True, False):
                        for want_storage in (True, False):
                            y, so, sg = net._forward_pool(dx, pools, dpm, dpp, sc, dst, want_state, want_storage)
                            assert PH.same_bits(_np(y), y_ref), what
                            assert (so is None) == (not want_state) and (so is None or PH.same_bits(_np(so), so_ref)), what
                            assert (sg is None) == (not want_storage) and (sg is None or PH.same_bits(_np(sg), sg_ref)), what
                    y, so, sg = net._forward_pool(dx, pools, dpm, dpp, sc, dst, True, True)
                    host_cases.append(("route", pt, x, pm, pp, dt, rr, prr, st, True, True))
                    got.append((_np(y), _np(so), _np(sg)))
                    ref = PH.route_pool_grad_ref(pt, gy, x, y_ref, sg_ref, pm, pp, dt, rr, prr, st)
                    for wants in range(8):
                        wp, wl, wt = bool(wants & 1), bool(wants & 2), bool(wants & 4)
                        gx, gpar, gpool, gstate = net._backward_pool(dgy, dx, y, sg, pools, dpm, dpp, sc, dst, wp, wl, wt)
                        assert PH.same_bits(_np(gx), ref[0]), what
                        for have, want, wanted in ((gpar, ref[1], wp), (gpool, ref[2], wl), (gstate, ref[3], wt)):
                            assert (have is None) == (not wanted) and (have is None or PH.same_bits(_np(have), want)), (what, wants)
                        if wants == 7:
                            host_cases.append(("grad", pt, gy, x, y_ref, sg_ref, pm, pp, dt, rr, prr, st, True, True, True))
                            got.append((_np(gx), _np(gpar), _np(gpool), _np(gstate)))
    for c, mine, theirs in zip(host_cases, got, PH.run(host_cases)):
        assert all(PH.same_bits(a, b) for a, b in zip(mine, theirs)), (name, c[0], c[1].P, np.asarray(c[2]).shape)
    print(name, part, count)
    if most >= 32:
        assert all(count[key] > 0 for key in PH.POOL_REGIMES), count
    for key, v in count.items():
        COUNT[key] += v
    RAN.add((name, part))


def test_every_regime_of_the_pool_row_was_taken():
    """Over all the cases of the grid above together, every regime of the pool row is taken on the GPU: inside, lo, hi, big, free,
    limited, empty (from mixed-sign x and from S < s0), spill, smax = +inf and the four exact ties.  (Counted by the grid cases
    as they run; a run that selects only some of them has nothing to assert here.)"""
    if RAN == set(GRID):
        print(COUNT)
        assert all(COUNT[key] > 0 for key in PH.POOL_REGIMES), COUNT


def test_the_capped_grid_strides():
    """A launch has at most 4096 workgroups of 256 lanes.  One level of 256 x 4096 + 65 headwaters, every other one a pool, T = 9:
    the lanes of both kernels stride over their part of the level.  Forward and adjoint with every output against the numpy
    definition, bit for bit."""
    from lgar_py_amd.network import CatchmentNetwork, NetworkPools
    width, T = 256 * GRID_CAP + 65, 9
    net = CatchmentNetwork(np.array(NH.wide(width), dtype=np.int32))
    pools = NetworkPools(net, np.arange(0, width, 2)[::-1].copy())
    pt = PH.PoolTopology.of_pools(pools)
    assert int(np.diff(pt.level_ptr).max()) == width and pt.P == (width + 1) // 2 and int(pt.pool_ptr[0]) == width // 2
    rng = np.random.default_rng(8)
    x, gy, pm, pp, state, dt, rr, prr = PH.case_data(rng, pt, T)
    sc = _scalars(dt, rr, prr)
    y_ref, so_ref, sg_ref = PH.route_pool_ref(pt, x, pm, pp, dt, rr, prr, state)
    dx, dpm, dpp, dst = _cuda(x), _cuda(pm), _cuda(pp), _cuda(state)
    y, so, sg = net._forward_pool(dx, pools, dpm, dpp, sc, dst, True, True)
    assert PH.same_bits(_np(y), y_ref) and PH.same_bits(_np(so), so_ref) and PH.same_bits(_np(sg), sg_ref)
    ref = PH.route_pool_grad_ref(pt, gy, x, y_ref, sg_ref, pm, pp, dt, rr, prr, state)
    got = net._backward_pool(_cuda(gy), dx, y, sg, pools, dpm, dpp, sc, dst, True, True, True)
    assert all(PH.same_bits(_np(a), b) for a, b in zip(got, ref))


def test_without_pools_it_is_the_muskingum_cunge_route():
    """P = 0 on every topology: y, state_out, gx, gpar_mc and gstate equal lgar_network_route_mc's and its adjoint's, kernel
    against kernel, bit for bit (and the numpy statement of the Muskingum-Cunge route)."""
    from lgar_py_amd.network import CatchmentNetwork, NetworkPools
    for name in sorted(TOPOLOGIES):
        topo = NH.Topology(TOPOLOGIES[name])
        net = CatchmentNetwork(topo.down)
        pools = NetworkPools(net, [])
        assert (pools.order_host == net.order_host).all() and (pools.pool_ptr == net.level_ptr[1:]).all()
        rng = np.random.default_rng(3100 + topo.B)
        none = torch.zeros(5, 0, dtype=torch.float64, device="cuda")
        for T in (0, 9, 17):
            x, gy, par, state, dt, rr = MH.case_data(rng, T, topo.B, wide=(T == 17))
            dx, dgy, dpar = _cuda(x), _cuda(gy), _cuda(par)
            sc = _scalars(dt, rr, PH.PNARROW)
            for st in (None, state):
                dst = _cuda(st)
                y, so, sg = net._forward_pool(dx, pools, dpar, none, sc, dst, True, False)
                y_mc, so_mc = net._forward_mc(dx, dpar, dt, *rr, dst, True)
                assert torch.equal(y, y_mc) and torch.equal(so, so_mc) and sg is None, (name, T)
                assert PH.same_bits(_np(y), MH.route_mc_ref(topo, x, par, dt, *rr, st)[0]), (name, T)
                gx, gpar, gpool, gstate = net._backward_pool(dgy, dx, y, torch.zeros(T, 0, dtype=torch.float64, device="cuda"), pools, dpar, none, sc,
                                                             dst, True, False, True)
                mc = net._backward_mc(dgy, dx, y_mc, dpar, dt, *rr, dst, True, True)
                assert gpool is None and all(PH.same_bits(_np(a), _np(b)) for a, b in zip((gx, gpar, gstate), mc)), (name, T)


def test_chunked_repeated_and_relabelled_calls_give_the_same_bits():
    """route_pool(carry=True) cut at 1 row, at T - 1 rows and in the middle against one call, from zeros and from a given state; a
    repeated call; an order-preserving relabelling of the catchments into a larger network gives the relabelled bits."""
    topo = NH.Topology(TOPOLOGIES["random257"])
    rng = np.random.default_rng(23)
    pt = PH.PoolTopology(topo, rng.permutation(topo.B)[:60])
    net, pools = _network(pt)
    T = 17
    x, gy, pm, pp, state, dt, rr, prr = PH.case_data(rng, pt, T)
    pm[1] = np.minimum(pm[1], 0.9)
    dx, reach, pool = _cuda(x), tuple(_cuda(p) for p in pm), tuple(_cuda(p) for p in pp)
    for st in (None, state):
        want, want_state, want_storage = PH.route_pool_ref(pt, x, pm, pp, dt, rr, prr, st)
        y, sg = net.route_pool(dx, pools, reach, pool, dt, carry=False, state=_cuda(st), return_storage=True)
        assert PH.same_bits(_np(y), want) and PH.same_bits(_np(sg), want_storage) and net.pool_state_of() is None
        assert torch.equal(net.route_pool(dx, pools, reach, pool, dt, carry=False, state=_cuda(st)), y)
        for cut in (1, T - 1, T // 2):
            key = (cut, st is None)
            a = net.route_pool(dx[:cut], pools, reach, pool, dt, key=key, state=_cuda(st))
            b = net.route_pool(dx[cut:], pools, reach, pool, dt, key=key)
            assert torch.equal(torch.cat([a, b]), y) and PH.same_bits(_np(net.pool_state_of(key)), want_state), cut
    assert net.state_of((1, True)) is None and net.mc_state_of((1, True)) is None  # a key space of its own
    net.reset()
    assert net.pool_state_of((1, True)) is None
    M = 300
    down2, slots = MH.embed(rng, topo, M)
    topo2 = NH.Topology(down2)
    extra = np.setdiff1d(np.arange(M), slots)[:5]
    pt2 = PH.PoolTopology(topo2, np.concatenate([extra, slots[pt.nodes]]))
    net2, pools2 = _network(pt2)
    x2, gy2, pm2, pp2, state2, _, _, _ = PH.case_data(rng, pt2, T)
    x2[:, slots], gy2[:, slots], pm2[:, slots], state2[:, slots], pp2[:, 5:] = x, gy, pm, state, pp
    sc = _scalars(dt, rr, prr)
    y2, so2, sg2 = net2._forward_pool(_cuda(x2), pools2, _cuda(pm2), _cuda(pp2), sc, _cuda(state2), True, True)
    want, want_state, want_storage = PH.route_pool_ref(pt, x, pm, pp, dt, rr, prr, state)
    assert PH.same_bits(_np(y2)[:, slots], want) and PH.same_bits(_np(so2)[:, slots], want_state) and PH.same_bits(_np(sg2)[:, 5:], want_storage)
    g2 = net2._backward_pool(_cuda(gy2), _cuda(x2), y2, sg2, pools2, _cuda(pm2), _cuda(pp2), sc, _cuda(state2), True, True, True)
    ref = PH.route_pool_grad_ref(pt, gy, x, want, want_storage, pm, pp, dt, rr, prr, state)
    assert PH.same_bits(_np(g2[0])[:, slots], ref[0]) and PH.same_bits(_np(g2[1])[:, slots], ref[1]) and PH.same_bits(_np(g2[3])[:, slots], ref[3])
    assert PH.same_bits(_np(g2[2])[:, 5:], ref[2])


@pytest.mark.parametrize("at_pool", (True, False))
def test_a_nan_reaches_exactly_the_downstream_closure_from_its_row_on(at_pool):
    """A NaN in x[t0][b], b a pool / b a reach above a pool."""
    rng = np.random.default_rng(41)
    topo = NH.Topology(TOPOLOGIES["random65"])
    b = int(np.nonzero(topo.level == 0)[0][3])
    while topo.down[b] < 0 or topo.down[topo.down[b]] < 0:
        b = int(np.nonzero(topo.level == 0)[0][list(np.nonzero(topo.level == 0)[0]).index(b) + 1])
    below = int(topo.down[b])
    nodes = [n for n in rng.permutation(65)[:20] if n not in (b, below)] + ([b] if at_pool else [below])
    pt = PH.PoolTopology(topo, nodes)
    net, pools = _network(pt)
    T = 9
    x, _, pm, pp, state, dt, rr, prr = PH.case_data(rng, pt, T)
    clean, _, clean_sg = PH.route_pool_ref(pt, x, pm, pp, dt, rr, prr, state)
    t0 = 4
    x[t0, b] = np.nan
    y, so, sg = net._forward_pool(_cuda(x), pools, _cuda(pm), _cuda(pp), _scalars(dt, rr, prr), _cuda(state), True, True)
    hit = np.zeros((T, topo.B), dtype=bool)
    hit[t0:, topo.closure()[:, b]] = True
    assert hit[:, b].sum() == T - t0 and hit[t0].sum() >= 3
    assert (np.isnan(_np(y)) == hit).all() and PH.same_bits(_np(y)[~hit], clean[~hit])
    assert (np.isnan(_np(sg)) == hit[:, pt.nodes]).all() and PH.same_bits(_np(sg)[~hit[:, pt.nodes]], clean_sg[~hit[:, pt.nodes]])
    assert (np.isnan(_np(so)[1]) == hit[-1]).all()


def test_entry_points_refuse_bad_arguments():
    """LGAR_E_ARG from the library itself: everything lgar_network_route_mc(_grad) refuses, prmin / prmax outside
    2^-60 <= prmin <= prmax <= 2^60, P < 0, a null pool_ptr with n_levels > 0, a pool_ptr[l] outside its level, a pool segment with
    P = 0, with P > 0 a null par_pool or pool_slot, the adjoint's null storage with T > 0 and P > 0.  Nothing is launched by a
    refused call."""
    from lgar_py_amd import _capi
    lib = _capi.load()
    buf = torch.zeros(1024, dtype=torch.float64, device="cuda")
    ibuf = torch.zeros(64, dtype=torch.int32, device="cuda")
    p, q = buf.data_ptr(), ibuf.data_ptr()
    arr = lambda *v: np.array(v, dtype=np.int32)
    level_ptr, bad_levels, pool_ptr, no_pools, below, above = arr(0, 4), arr(0, 3), arr(2), arr(4), arr(-1), arr(5)
    fwd = (("x", p), ("T", 2), ("B", 4), ("par", p), ("par_pool", p), ("P", 2), ("dt", 1.0), ("rmin", 1 / 64), ("rmax", 64.0), ("prmin", 2.0 ** -20),
           ("prmax", 2.0 ** 20), ("up_ptr", q), ("up_idx", q), ("E", 1), ("order", q), ("level_ptr", level_ptr.ctypes.data),
           ("pool_ptr", pool_ptr.ctypes.data), ("L", 1), ("pool_slot", q), ("state_in", None), ("state_out", p + 2048), ("y", p + 4096),
           ("storage", p + 6144))
    run = lambda **kw: lib.lgar_network_route_pool(*[kw.get(k, d) for k, d in fwd], None)
    nan, inf = float("nan"), float("inf")
    scalars = (dict(dt=0.0), dict(dt=-1.0), dict(dt=nan), dict(dt=inf), dict(rmin=nan), dict(rmax=inf), dict(rmin=2.0 ** -61), dict(rmin=65.0),
               dict(prmin=nan), dict(prmax=nan), dict(prmax=inf), dict(prmin=-inf), dict(prmin=2.0 ** -61), dict(prmax=2.0 ** 61),
               dict(prmin=2.0 ** 21), dict(prmin=0.0), dict(B=0, prmin=0.0), dict(B=0, dt=0.0))
    pool_args = (dict(P=-1), dict(B=0, P=-1), dict(pool_ptr=None), dict(pool_ptr=below.ctypes.data), dict(pool_ptr=above.ctypes.data),
                 dict(P=0), dict(P=0, par_pool=None, pool_slot=None), dict(par_pool=None), dict(pool_slot=None))
    for bad in (dict(T=-1), dict(B=-1), dict(E=-1), dict(L=-1), dict(x=None), dict(par=None), dict(T=0, par=None), dict(y=None), dict(up_ptr=None),
                dict(up_idx=None), dict(order=None), dict(level_ptr=None), dict(level_ptr=bad_levels.ctypes.data)) + scalars + pool_args:
        assert run(**bad) == -1, bad
    grd = (("gy", p), ("T", 2), ("B", 4), ("par", p), ("par_pool", p), ("P", 2), ("dt", 1.0), ("rmin", 1 / 64), ("rmax", 64.0), ("prmin", 2.0 ** -20),
           ("prmax", 2.0 ** 20), ("down", q), ("order", q), ("level_ptr", level_ptr.ctypes.data), ("pool_ptr", pool_ptr.ctypes.data), ("L", 1),
           ("pool_slot", q), ("gx", p + 2048), ("x", p), ("y", p), ("storage", p), ("up_ptr", q), ("up_idx", q), ("E", 1), ("state_in", None),
           ("gpar", p + 4096), ("gpool", p + 5120), ("gstate", p + 6144))
    grad = lambda **kw: lib.lgar_network_route_pool_grad(*[kw.get(k, d) for k, d in grd], None)
    for bad in (dict(T=-1), dict(B=-1), dict(E=-1), dict(L=-1), dict(gy=None), dict(par=None), dict(T=0, par=None), dict(down=None), dict(order=None),
                dict(gx=None), dict(x=None), dict(y=None), dict(up_ptr=None), dict(up_idx=None), dict(level_ptr=None),
                dict(level_ptr=bad_levels.ctypes.data), dict(x=None, gpar=None, gpool=None, gstate=None), dict(storage=None)) + scalars + pool_args:
        assert grad(**bad) == -1, bad
    torch.cuda.synchronize()
    assert not buf.any()
    # accepted: nothing to do, or a launch over zeros (sref = 0: the selects carry the NaN -- parameter values are not policed)
    assert run(B=0, x=None, par=None, y=None, level_ptr=None, pool_ptr=None) == 0 and run(T=0, state_out=None, x=None, y=None) == 0
    assert run(E=0, up_idx=None) == 0 and run() == 0 and run(state_in=p, state_out=None) == 0 and run(T=0, x=None, y=None) == 0 and run(storage=None) == 0
    assert run(P=0, par_pool=None, pool_slot=None, storage=None, pool_ptr=no_pools.ctypes.data) == 0
    assert grad(B=0, gy=None, gx=None, level_ptr=None, pool_ptr=None) == 0 and grad(T=0, gpar=None, gpool=None, gstate=None, gy=None, x=None) == 0
    assert grad() == 0 and grad(gpar=None) == 0 and grad(gpool=None) == 0 and grad(gstate=None) == 0 and grad(gpar=None, gpool=None, gstate=None) == 0
    assert grad(E=0, up_idx=None) == 0 and grad(T=0, gy=None, gx=None, x=None, y=None, storage=None) == 0
    assert grad(P=0, par_pool=None, pool_slot=None, storage=None, gpool=None, pool_ptr=no_pools.ctypes.data) == 0
    torch.cuda.synchronize()


def test_gradients_end_to_end():
    """lgar_series -> catchment_sum -> catchment_route -> network_route_pool -> catchment_moments -> loss("nse"): 24 columns of
    synth1_phil's soil in 3 catchments that form a chain (0 -> 1 -> 2), the middle one a pool; observations = the same chain on a
    perturbed parameter set.  The loss and the gradients to the soil parameters, to kref, beta, X and to cq, m, s0, smax are
    finite and non-zero; the routing node hands back the definition's bits (gx, gpool of route_pool_grad_ref for the gy it
    received)."""
    import lgar_py_amd as lg
    from lgar_py_amd import workloads as W
    from lgar_py_amd.autograd import lgar_series
    from lgar_py_amd.catchments import CatchmentMap, CatchmentRouting, catchment_route, catchment_sum
    from lgar_py_amd.network import network_route_pool
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
    pools = lg.NetworkPools(net, [1])
    pt = PH.PoolTopology(NH.Topology([1, 2, -1]), [1])
    leaf = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda", requires_grad=True)
    kref, beta, X = leaf([2.0, 3.0, 1.5]), leaf([0.4, 0.3, 0.5]), leaf([0.2, 0.1, 0.3])

    def discharge_of(Pdict, grad, qref, pool, state):
        P = {k: torch.tensor(val, device="cuda") for k, val in Pdict.items()}
        for k in ("alpha", "n", "ksat"):
            P[k].requires_grad_(grad)
        statuses = []
        runoff, _ = lgar_series(P["alpha"], P["n"], P["ksat"], P["theta_e"], P["theta_r"], P["thickness"], pr, pe, check=False,
                                status_out=statuses, **ekw)
        lateral = catchment_route(catchment_sum(runoff, cmap, statuses[0]), routing)
        if grad:
            lateral.retain_grad()
        q = network_route_pool(lateral, net, pools, (kref, beta, X, qref), pool, dt, state=state)
        if grad:
            q.retain_grad()
        return P, lateral, q

    with torch.no_grad():
        lat0 = discharge_of(Pobs, False, 1.0, (1.0, 1.5, 0.0, 1.0, float("inf")), None)[1]
        unit = float(torch.clamp(lat0.mean(), min=1e-6))  # the mean lateral inflow; unit * dt is the volume of a mean row
        qref = torch.clamp(lat0.mean(dim=0) * torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64, device="cuda"), min=1e-6)
    # a pool that starts above smax (it spills in row 0) and whose release at smax is below the mean inflow from above
    cq, m, s0, smax = leaf([0.25 * unit]), leaf([1.5]), leaf([0.5 * unit * dt]), leaf([9.5 * unit * dt])
    sref = 4.0 * unit * dt
    state0 = torch.tensor([[0.5, 0.5, 0.5], [0.5, 12.0 * dt, 0.5]], dtype=torch.float64, device="cuda") * unit
    with torch.no_grad():
        obs = discharge_of(Pobs, False, qref, (cq * 1.3, m, s0, sref, smax * 1.2), state0)[2].clone()
    assert tuple(obs.shape) == (Tn, B) and float(obs.abs().max()) > 0
    score = lg.CatchmentScore(obs)
    P, lateral, q = discharge_of(Pn, True, qref, (cq, m, s0, sref, smax), state0)
    loss = score.loss(catchment_moments(q, score), "nse")
    loss.backward()
    assert np.isfinite(float(loss.detach())) and float(loss.detach()) > 0
    pm_np = np.stack([_np(kref.detach()), _np(beta.detach()), _np(X.detach()), _np(qref)])
    pp_np = np.array([[float(cq.detach())], [float(m.detach())], [float(s0.detach())], [sref], [float(smax.detach())]])
    x_np, st_np = _np(lateral.detach()), _np(state0)
    rr, prr = (1.0 / 64.0, 64.0), PH.PNARROW
    y_ref, _, sg_ref = PH.route_pool_ref(pt, x_np, pm_np, pp_np, dt, rr, prr, st_np)
    assert PH.same_bits(_np(q.detach()), y_ref)
    reg = PH.pool_regimes(pt, x_np, pm_np, pp_np, dt, rr, prr, st_np)
    print(reg)
    assert reg["inside"] > 0 and reg["free"] > 0 and reg["spill"] > 0, reg
    gx_ref, gpar_ref, gpool_ref, _ = PH.route_pool_grad_ref(pt, _np(q.grad), x_np, y_ref, sg_ref, pm_np, pp_np, dt, rr, prr, st_np)
    assert PH.same_bits(_np(lateral.grad), gx_ref) and float(np.abs(gx_ref).max()) > 0
    assert PH.same_bits(np.stack([_np(kref.grad), _np(beta.grad), _np(X.grad)]), gpar_ref) and not gpar_ref[:, 1].any()
    assert PH.same_bits(np.stack([_np(t.grad) for t in (cq, m, s0, smax)]), gpool_ref)
    for name, t in (("cq", cq), ("m", m), ("s0", s0), ("smax", smax)):
        assert bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().min()) > 0, name
    for name, t in (("kref", kref), ("beta", beta), ("X", X)):
        assert bool(torch.isfinite(t.grad).all()) and float(t.grad[[0, 2]].abs().min()) > 0, name
    for kind in ("alpha", "n", "ksat"):
        assert bool(torch.isfinite(P[kind].grad).all()) and float(P[kind].grad.abs().max()) > 0, kind
