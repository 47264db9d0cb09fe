"""GPU (-m gpu): the catchment network -- lgar_network_route / lgar_network_route_grad through network.CatchmentNetwork and
network.network_route (autograd).

y[.][b] is a pure function of the columns of x and coef in the upstream closure of b, gx[.][b] of gy and coef downstream of it
(include/lgar.h), so the kernels are held BIT FOR BIT to the numpy statement of the definition
(tests/network_host: route_ref, adjoint_ref and coef_grad_ref), the one tests/test_network_host.py holds the host build of the
same header to -- and that file holds the definition itself to exact rational arithmetic."""
import os

import numpy as np
import pytest

from _golden import engine_keywords
from conftest import GOLDEN

import network_host as NH

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GRID_CAP = 4096  # LGAR_NET_GRID_CAP (csrc/lgar_network.hip): workgroups of a level's launch; the rest by stride
GPU_T = (0, 1, 9, 17)


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _network(down):
    from lgar_py_amd.network import CatchmentNetwork
    return CatchmentNetwork(down)


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("name", sorted(NH.topologies()))
def test_kernels_equal_the_numpy_definition_bit_for_bit(name):
    """Every topology of the grid (a single reach, two, the chain of 65 levels, the star of in-degree 256, full binary trees,
    forests with isolated reaches, random forests with shuffled numbering, levels exactly 64 and 65 wide) x T in {0, 1, 9, 17} x
    the four coefficient sets (Muskingum, accumulation, lag, mixed signs) x state_in present or NULL: the forward with its
    state, the adjoint alone and the adjoint with the coefficient gradient.  x has mixed signs over several decades and -0.0."""
    topo = NH.Topology(NH.topologies()[name])
    net = _network(topo.down)
    rng = np.random.default_rng(1400 + topo.B)
    for T in GPU_T:
        for kind in NH.COEFS:
            x, gy, coef, state = NH.case_data(rng, T, topo.B, kind)
            dx, dgy, dcoef = _cuda(x), _cuda(gy), _cuda(coef)
            for st in (None, state):
                what = (name, T, kind, st is not None)
                y_ref, s_ref = NH.route_ref(topo, x, coef, st)
                y = net.route(dx, dcoef, carry=True, key=what, state=_cuda(st))
                assert NH.same_bits(_np(y), y_ref) and NH.same_bits(_np(net.state_of(what)), s_ref), what
                assert NH.same_bits(_np(net.route(dx, dcoef, carry=False, state=_cuda(st))), y_ref), what
                gx_ref = NH.adjoint_ref(topo, gy, coef)
                assert NH.same_bits(_np(net.adjoint(dgy, dcoef)), gx_ref), what
                gx, gc = net._backward(dgy, dcoef, dx, y, _cuda(st))
                assert NH.same_bits(_np(gx), gx_ref) and NH.same_bits(_np(gc), NH.coef_grad_ref(topo, x, y_ref, gy, coef, st)), what
                assert NH.same_bits(_np(net.coef_grad(dx, y, dgy, dcoef, state=_cuda(st))), _np(gc)), what
    net.reset()


def test_the_capped_grid_strides():
    """A level's launch has at most 4096 workgroups of 256 lanes.  A level of 256 x 4096 + 65 headwaters (into 1024 reaches of
    in-degree 1024 or 1025, into one outlet), T = 2: the lanes stride over the level.  Forward, adjoint and coefficient gradient
    against the numpy definition, bit for bit."""
    width = 256 * GRID_CAP + 65
    net = _network(np.asarray(NH.wide(width, mids=1024), dtype=np.int32))
    topo = NH.Topology.of_network(net)
    assert net.n_levels == 3 and int(np.diff(net.level_ptr).max()) == width > 256 * GRID_CAP
    rng = np.random.default_rng(8)
    T, B = 2, net.B
    x, gy, coef = rng.standard_normal((T, B)), rng.standard_normal((T, B)), NH.coefficients(rng, "muskingum", B)
    y_ref, _ = NH.route_ref(topo, x, coef)
    dx, dgy, dcoef = _cuda(x), _cuda(gy), _cuda(coef)
    y = net.route(dx, dcoef, carry=False)
    assert NH.same_bits(_np(y), y_ref)
    gx, gc = net._backward(dgy, dcoef, dx, y)
    assert NH.same_bits(_np(gx), NH.adjoint_ref(topo, gy, coef)) and NH.same_bits(_np(gc), NH.coef_grad_ref(topo, x, y_ref, gy, coef))


def test_chunked_calls_equal_one_call():
    """route(carry=True) cut at 1 row, at T - 1 rows and in the middle against one call, and a repeated call: the same bits."""
    rng = np.random.default_rng(23)
    topo = NH.Topology(NH.random_forest(257, 9))
    T, B = 17, topo.B
    x, _, coef, state = NH.case_data(rng, T, B, "muskingum")
    net = _network(topo.down)
    dx, dcoef = _cuda(x), _cuda(coef)
    for st in (None, state):
        want, want_state = NH.route_ref(topo, x, coef, st)
        one = net.route(dx, dcoef, carry=False, state=_cuda(st))
        assert NH.same_bits(_np(one), want) and torch.equal(net.route(dx, dcoef, carry=False, state=_cuda(st)), one)
        for cut in (1, T - 1, T // 2):
            key = (cut, st is None)
            a = net.route(dx[:cut], dcoef, key=key, state=_cuda(st))
            b = net.route(dx[cut:], dcoef, key=key)
            assert torch.equal(torch.cat([a, b]), one) and NH.same_bits(_np(net.state_of(key)), want_state), cut
    # accumulate: coef = (1, 0, 0), small integers -- the exact closure sums
    xi = rng.integers(-9, 10, (T, B)).astype(np.float64)
    assert NH.same_bits(_np(net.accumulate(_cuda(xi))) + 0.0, xi @ topo.closure().T.astype(np.float64) + 0.0)


def test_network_route_autograd():
    """General data at B = 7, T = 9: gx and gc of network_route equal adjoint_ref and coef_grad_ref bit for bit; the gradient
    to K and X through muskingum_coefficients equals torch autograd fed the kernel's gc; an explicit state is a constant."""
    from lgar_py_amd.network import muskingum_coefficients, network_route
    rng = np.random.default_rng(8)
    topo = NH.Topology(NH.random_forest(7, 104, roots=0.1))
    T, B = 9, topo.B
    x_np, gy_np, _, st_np = NH.case_data(rng, T, B, "muskingum")
    net = _network(topo.down)
    K = _cuda(0.5 + 5.0 * rng.random(B)).requires_grad_(True)
    X = _cuda(0.5 * rng.random(B)).requires_grad_(True)
    coef = muskingum_coefficients(K, X, 1.0)
    coef.retain_grad()
    x, state = _cuda(x_np).requires_grad_(True), _cuda(st_np).requires_grad_(True)
    y = network_route(x, net, coef, state)
    c_np = _np(coef.detach())
    y_ref, _ = NH.route_ref(topo, x_np, c_np, st_np)
    assert NH.same_bits(_np(y.detach()), y_ref) and net.state_of() is None
    (y * _cuda(gy_np)).sum().backward()
    gc_ref = NH.coef_grad_ref(topo, x_np, y_ref, gy_np, c_np, st_np)
    assert NH.same_bits(_np(x.grad), NH.adjoint_ref(topo, gy_np, c_np)) and NH.same_bits(_np(coef.grad), gc_ref) and state.grad is None
    assert float(np.abs(gc_ref).min()) > 0
    K2, X2 = K.detach().clone().requires_grad_(True), X.detach().clone().requires_grad_(True)
    muskingum_coefficients(K2, X2, 1.0).backward(coef.grad)
    assert torch.equal(K.grad, K2.grad) and torch.equal(X.grad, X2.grad) and float(K.grad.abs().min()) > 0
    x2 = _cuda(x_np).requires_grad_(True)
    (network_route(x2, net, coef.detach(), state.detach()) * _cuda(gy_np)).sum().backward()
    assert torch.equal(x2.grad, x.grad)


def test_entry_points_refuse_bad_arguments():
    """LGAR_E_ARG from the library itself: negative sizes, n_levels < 0, a level_ptr (host memory) that does not start at 0, end at
    B and never decrease, a null pointer the sizes say will be read or written, gc wanted without x.  Nothing is launched by a
    refused call."""
    from lgar_py_amd import _capi
    lib = _capi.load()
    net = _network([1, 2, -1, 2])
    buf = torch.zeros(1024, dtype=torch.float64, device="cuda")
    p, lp = buf.data_ptr(), net.level_ptr.ctypes.data
    fwd = (("x", p), ("T", 2), ("B", 4), ("coef", p + 1024), ("up_ptr", net.up_ptr.data_ptr()), ("up_idx", net.up_idx.data_ptr()), ("E", 3),
           ("order", net.order.data_ptr()), ("level_ptr", lp), ("L", 3), ("state_in", None), ("state_out", p + 2048), ("y", p + 4096))
    route = lambda **kw: lib.lgar_network_route(*[kw.get(k, d) for k, d in fwd], None)
    bad_ptrs = [np.array(v, dtype=np.int32) for v in ([1, 2, 3, 4], [0, 2, 3, 5], [0, 3, 2, 4])]
    for bad in [dict(T=-1), dict(B=-1), dict(E=-1), dict(L=-1), dict(x=None), dict(y=None), dict(coef=None), dict(up_ptr=None), dict(up_idx=None),
                dict(order=None), dict(level_ptr=None), dict(L=2)] + [dict(level_ptr=v.ctypes.data) for v in bad_ptrs]:
        assert route(**bad) == -1, bad
    assert route(B=0, x=None, y=None, level_ptr=None) == 0 and route(T=0, state_out=None, order=None) == 0 and route() == 0
    grd = (("gy", p), ("T", 2), ("B", 4), ("coef", p + 1024), ("down", net.down.data_ptr()), ("order", net.order.data_ptr()), ("level_ptr", lp),
           ("L", 3), ("gx", p + 4096), ("x", p), ("y", p + 6144), ("up_ptr", net.up_ptr.data_ptr()), ("up_idx", net.up_idx.data_ptr()), ("E", 3),
           ("state_in", None), ("gc", p + 2048))
    grad = lambda **kw: lib.lgar_network_route_grad(*[kw.get(k, d) for k, d in grd], None)
    for bad in [dict(T=-1), dict(B=-1), dict(L=-1), dict(gy=None), dict(gx=None), dict(coef=None), dict(down=None), dict(order=None),
                dict(level_ptr=None), dict(x=None), dict(y=None), dict(up_ptr=None), dict(up_idx=None)] + [dict(level_ptr=v.ctypes.data) for v in bad_ptrs]:
        assert grad(**bad) == -1, bad
    assert grad(gc=None, x=None, y=None, up_ptr=None, up_idx=None) == 0 and grad() == 0 and grad(B=0, gy=None, gx=None) == 0
    torch.cuda.synchronize()
    assert not buf.any()


def test_gradients_end_to_end():
    """lgar_series -> catchment_sum -> catchment_route -> network_route -> catchment_moments -> loss("nse"): 24 columns of
    grad_synth0_12h's soil in 3 catchments that form a chain (0 -> 1 -> 2), per-catchment hydrographs, Muskingum reaches;
    observations = the same chain on a perturbed parameter set.  The loss is finite, the parameter gradients finite and
    non-zero, K and X receive gradients.  network_route hands catchment_route the kernel's gx (adjoint_ref's bits); ahead of it the
    chain is the same deterministic linear tail as without a network (CatchmentRouting.adjoint, CatchmentMap.spread, the
    tangent kernels): fed the kernel's own gx it reproduces the parameter gradients bit for bit."""
    import lgar_py_amd as lg
    from lgar_py_amd import workloads as W
    from lgar_py_amd.autograd import lgar_series, parameter_vjp
    from lgar_py_amd.catchments import CatchmentMap, CatchmentRouting, catchment_route, catchment_sum
    from lgar_py_amd.network import muskingum_coefficients, network_route
    from lgar_py_amd.scores import catchment_moments
    g = np.load(os.path.join(GOLDEN, "grad_synth0_12h.npz"))
    n, B, K = 24, 3, 5
    base = {k: g[k] for k in W.PARAM_KEYS + ("thickness",)}
    Pn = W.perturbed_columns(n, frac=0.05, seed=21, base=base)
    Pobs = W.perturbed_columns(n, frac=0.05, seed=22, base=base)
    f = torch.tensor(g["forcing"], device="cuda")
    Tn = f.shape[0]
    pr, pe = f[:, 0:1].expand(Tn, n).contiguous(), f[:, 1:2].expand(Tn, n).contiguous()
    ekw = dict(engine_keywords(g), dtype=torch.float64)
    ids = np.array([0] * 9 + [2] * 5 + [-1] + [1] * 9)[np.random.default_rng(1).permutation(n)]
    cmap = CatchmentMap(ids, weights=np.random.default_rng(2).random(n) + 0.5)
    rng = np.random.default_rng(3)
    routing = CatchmentRouting(g["giuh_ordinates"][None, :] * (1.0 + 0.2 * rng.random((B, K))))
    net = lg.CatchmentNetwork([1, 2, -1])
    assert net.n_levels == 3
    Kh = torch.tensor([2.0, 3.0, 1.5], dtype=torch.float64, device="cuda", requires_grad=True)
    Xw = torch.tensor([0.2, 0.1, 0.3], dtype=torch.float64, device="cuda", requires_grad=True)

    def discharge_of(Pdict, grad):
        P = {k: torch.tensor(val, device="cuda") for k, val in Pdict.items()}
        for k in ("alpha", "n", "ksat"):
            P[k].requires_grad_(grad)
        statuses = []
        runoff, _ = lgar_series(P["alpha"], P["n"], P["ksat"], P["theta_e"], P["theta_r"], P["thickness"], pr, pe, check=False,
                                status_out=statuses, **ekw)
        routed = catchment_route(catchment_sum(runoff, cmap, statuses[0]), routing)
        if grad:
            routed.retain_grad()
        coef = muskingum_coefficients(Kh, Xw, float(ekw.get("dt_h", 1.0)))
        return P, statuses[0], routed, coef, network_route(routed, net, coef)

    with torch.no_grad():
        obs = discharge_of(Pobs, False)[4].clone()
    assert tuple(obs.shape) == (Tn, B) and float(obs.abs().max()) > 0
    score = lg.CatchmentScore(obs)
    P, status, routed, coef, q = discharge_of(Pn, True)
    q.retain_grad()
    coef.retain_grad()
    loss = score.loss(catchment_moments(q, score), "nse")
    loss.backward()
    assert np.isfinite(float(loss.detach())) and float(loss.detach()) > 0
    # the outlet carries what arrives from upstream: more than its own routed runoff
    assert float(q.detach()[:, 2].sum()) > float(routed.detach()[:, 2].sum()) > 0
    topo = NH.Topology([1, 2, -1])
    c_np = _np(coef.detach())
    y_ref, _ = NH.route_ref(topo, _np(routed.detach()), c_np)
    assert NH.same_bits(_np(q.detach()), y_ref)
    assert NH.same_bits(_np(routed.grad), NH.adjoint_ref(topo, _np(q.grad), c_np)) and float(routed.grad.abs().max()) > 0
    assert NH.same_bits(_np(coef.grad), NH.coef_grad_ref(topo, _np(routed.detach()), y_ref, _np(q.grad), c_np))
    assert bool(torch.isfinite(Kh.grad).all()) and float(Kh.grad.abs().min()) > 0 and bool(torch.isfinite(Xw.grad).all()) and float(Xw.grad.abs().min()) > 0
    # the linear tail: the parameter gradients are the tangent kernels on spread(adjoint(the kernel's gx)), bit for bit
    faulted = (status & 0x7F) != 0
    eng = lg.LgarEngine(P["alpha"].detach(), P["n"].detach(), P["ksat"].detach(), P["theta_e"], P["theta_r"], P["thickness"], **ekw)
    wr = cmap.spread(routing.adjoint(routed.grad), torch.float64, status=status)
    wanted = [(kind, l) for kind in ("alpha", "n", "ksat") for l in range(eng.L)]
    vj, _ = parameter_vjp(eng, pr, pe, wr, torch.zeros_like(wr), wanted, check=False)
    for kind in ("alpha", "n", "ksat"):
        want = torch.stack([vj[(kind, l)] for l in range(eng.L)])
        want = torch.where(faulted[None, :], torch.zeros_like(want), want)
        assert torch.equal(P[kind].grad, want) and float(want.abs().max()) > 0 and bool(torch.isfinite(want).all()), kind
