"""GPU (-m gpu): catchment routing -- lgar_catchment_route / lgar_catchment_route_grad through catchments.CatchmentRouting,
catchments.catchment_route (autograd) and LgarEngine.forward(routing=...).

y[t][b] is a pure function of column b of the inputs (include/lgar.h), so the kernels are held BIT FOR BIT
to the numpy statement of the definition (tests/route_host: route_ref, the queue recurrence row after row), the one
tests/test_route_host.py holds the host build of the same header -- and the reference's recorded queue -- to.  Where two
different evaluation orders are compared the bound is m 2^-52 sum|terms|, m = the rounded operations of one chain: each order
is within m 2^-53 sum|terms| of the exact value, to first order (Higham 3.1, 4.4), as in
test_gpu_catchments.test_one_catchment_agrees_with_the_basin_pass."""
import os

import numpy as np
import pytest

from _golden import engine_keywords
from conftest import GOLDEN

from post_host import route as RH

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

U2 = 2.0 ** -52
GRID_CAP = 4096  # LGAR_ROUTE_GRID_CAP (csrc/lgar_route.hip): workgroups of a launch; the rest by stride


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _routing(g, B):
    """g in the device layout ([K] or [K, B]) -> CatchmentRouting (which takes [K] or [B, K])"""
    from lgar_py_amd.catchments import CatchmentRouting
    return CatchmentRouting(g if g.ndim == 1 else g.T, n_catchments=B)


def _dense(x, g):
    """The plain torch statement of the convolution: y[t] = sum_k g[k] x[t - k], K shifted products added in increasing k.
    g: [K] or [B, K]."""
    T = x.shape[0]
    y = torch.zeros_like(x)
    for k in range(min(g.shape[-1], T)):
        y = y + torch.nn.functional.pad(g[..., k] * x[:T - k], (0, 0, k, 0))
    return y


@pytest.mark.parametrize("B", RH.SHAPE_B)
def test_kernel_equals_the_numpy_definition_bit_for_bit(B):
    """K in {1, 2, 5, 8, 64} x T in {0, 1, K - 1, K, K + 1, 11}, shared and per-catchment ordinates, with and without a queue,
    mixed signs, a NaN and -0.0 in the inputs: forward (y and the queue left), reverse and the ordinate gradient."""
    rng = np.random.default_rng(100 + B)
    for K in RH.SHAPE_K:
        for T in RH.shape_T(K):
            for per in (False, True):
                x, gy, g, q_in = RH.mixed_data(rng, T, B, K, per)
                r = _routing(g, B)
                assert (r.K, r.B, r.per_catchment) == (K, B, per)
                what = (B, K, T, per)
                for q in (None, q_in):
                    ref_y, ref_q = RH.route_ref(x, g, q)
                    r.reset()
                    y = r.route(_cuda(x), carry=True, queue=_cuda(q))
                    assert RH.same_bits(y.cpu().numpy(), ref_y) and RH.same_bits(r.queue.cpu().numpy(), ref_q), what
                    assert RH.same_bits(r.route(_cuda(x), carry=False, queue=_cuda(q)).cpu().numpy(), ref_y), what
                assert RH.same_bits(r.adjoint(_cuda(gy)).cpu().numpy(), RH.adjoint_ref(gy, g)), what
                if per:
                    gg = r.ordinate_grad(_cuda(x), _cuda(gy))
                    assert tuple(gg.shape) == (B, K) and RH.same_bits(gg.cpu().numpy(), RH.ordinate_grad_ref(x, gy, K).T.copy()), what


@pytest.mark.parametrize("K", [5, 8])
def test_chunked_calls_equal_one_call(K):
    """T = 11 in chunks of (3, 1, 7) through the queue the routing keeps on the device; K = 8 makes a chunk shorter than the
    queue.  The same bits as one call, for y and for the queue left; reset() starts anew."""
    rng = np.random.default_rng(K)
    for per in (False, True):
        x, _, g, _ = RH.mixed_data(rng, 11, 65, K, per)
        dev = _cuda(x)
        one, chunked = _routing(g, 65), _routing(g, 65)
        whole = one.route(dev)
        parts = [chunked.route(dev[a:b]) for a, b in ((0, 3), (3, 4), (4, 11))]
        ref_y, ref_q = RH.route_ref(x, g)
        same = lambda a, b: RH.same_bits(a.cpu().numpy(), b.cpu().numpy())  # (the data holds a NaN: torch.equal would refuse it)
        assert same(torch.cat(parts), whole) and same(chunked.queue, one.queue)
        assert RH.same_bits(whole.cpu().numpy(), ref_y) and RH.same_bits(one.queue.cpu().numpy(), ref_q)
        chunked.reset()
        assert chunked.queue is None and same(chunked.route(dev), whole)


def test_the_capped_grid_strides():
    """Route: a launch has at most 4096 workgroups of (four rows, 64 catchments); T = 8200 rows (+ 5 of the queue) of B = 65
    catchments are 2 x 2052 = 4104 of them, just past the cap.  Ordinate gradient: workgroups of (16 ordinates, 64 catchments),
    so B = 4097 x 64 - 63 catchments of K = 5 are 4097.  Both against the numpy definition, bit for bit."""
    rng = np.random.default_rng(8)
    T, B, K = 8200, 65, 5
    assert 2 * ((T + K + 3) // 4) > GRID_CAP
    x = rng.standard_normal((T, B))
    g, q_in = rng.random((K, B)), rng.standard_normal((K, B))
    r = _routing(g, B)
    y = r.route(_cuda(x), queue=_cuda(q_in))
    ref_y, ref_q = RH.route_ref(x, g, q_in)
    assert RH.same_bits(y.cpu().numpy(), ref_y) and RH.same_bits(r.queue.cpu().numpy(), ref_q)
    assert RH.same_bits(r.adjoint(_cuda(x)).cpu().numpy(), RH.adjoint_ref(x, g))
    T, B = 7, (GRID_CAP + 1) * 64 - 63
    assert (B + 63) // 64 > GRID_CAP
    x, gy = rng.standard_normal((T, B)), rng.standard_normal((T, B))
    wide = _routing(rng.random((K, B)), B)
    assert RH.same_bits(wide.ordinate_grad(_cuda(x), _cuda(gy)).cpu().numpy(), RH.ordinate_grad_ref(x, gy, K).T.copy())


def test_a_catchment_does_not_depend_on_the_others():
    """B = 257 catchments with their own hydrographs, then a permuted subset of 100 of their columns alone: the same bits for
    y, the queue, the adjoint and the ordinate gradient, and again on a repeated call."""
    rng = np.random.default_rng(21)
    T, B, K = 23, 257, 8
    x, gy, g, q_in = RH.mixed_data(rng, T, B, K, True)
    full = _routing(g, B)
    y = full.route(_cuda(x), queue=_cuda(q_in))
    pick = rng.permutation(B)[:100]
    part = _routing(g[:, pick], 100)
    y2 = part.route(_cuda(x[:, pick]), queue=_cuda(q_in[:, pick]))
    idx = torch.tensor(pick, device="cuda")
    same = lambda a, b: RH.same_bits(a.cpu().numpy(), b.cpu().numpy())
    assert same(y[:, idx].contiguous(), y2) and same(full.queue[:, idx].contiguous(), part.queue)
    assert same(full.adjoint(_cuda(gy))[:, idx].contiguous(), part.adjoint(_cuda(gy[:, pick])))
    assert same(full.ordinate_grad(_cuda(x), _cuda(gy))[idx].contiguous(), part.ordinate_grad(_cuda(x[:, pick]), _cuda(gy[:, pick])))
    assert same(full.route(_cuda(x), carry=False, queue=_cuda(q_in)), y)


def test_adjoint_and_ordinate_gradient_are_the_derivatives():
    """<route(x), v> against <x, adjoint(v)>: both are sums of the same T B K products g x v in two orders; one chain is K
    products and K - 1 adds of the fold, the product with v and at most T B - 1 adds of the final sum: m = 2 K + T B.
    ordinate_grad against the torch-autograd gradient of the dense torch statement: per (b, k) both sum the same <= T products
    gy x, T adds and one product a chain: m = T + 1; for shared ordinates the sum over b adds B - 1 adds: m = T + B."""
    from lgar_py_amd.catchments import catchment_route
    rng = np.random.default_rng(31)
    T, B, K = 40, 65, 8
    for per in (True, False):
        g = rng.random((K, B)) if per else rng.random(K)
        x, v = rng.standard_normal((T, B)), rng.standard_normal((T, B))
        r = _routing(g, B)
        dx, dv = _cuda(x), _cuda(v)
        y, gx = r.route(dx, carry=False), r.adjoint(dv)
        G = r.ordinates if per else r.ordinates[:, None].expand(K, B)
        terms = float((_dense(dx.abs(), G.t().contiguous()) * dv.abs()).sum())
        m = 2 * K + T * B
        err = abs(float((y * dv).sum()) - float((dx * gx).sum()))
        print("adjoint inner products (per=%s): error / bound = %.3g" % (per, err / (m * U2 * terms)))
        assert err <= m * U2 * terms and terms > 0
        # the ordinates as a leaf of torch's own graph over the dense statement
        leaf = (_cuda(g).t().contiguous() if per else _cuda(g)).requires_grad_(True)
        (_dense(dx, leaf) * dv).sum().backward()
        gg = r.ordinate_grad(dx, dv)
        assert gg.shape == leaf.grad.shape
        absterms = torch.stack([(dv[k:].abs() * dx[:T - k].abs()).sum(dim=0) for k in range(K)], dim=1)  # [B, K]
        bound = (T + 1) * U2 * absterms if per else (T + B) * U2 * absterms.sum(dim=0)
        print("ordinate gradient vs autograd of the dense statement (per=%s): worst error / bound = %.3g"
              % (per, float(((gg - leaf.grad).abs() / bound).max())))
        assert bool(((gg - leaf.grad).abs() <= bound).all()) and float(gg.abs().min()) > 0
        # and through catchment_route's own backward pass: the same kernels, the same bits
        leaf2 = leaf.detach().clone().requires_grad_(True)
        x2 = dx.clone().requires_grad_(True)
        out = catchment_route(x2, leaf2)
        assert torch.equal(out, y)
        (out * dv).sum().backward()
        assert torch.equal(x2.grad, gx)
        # (the sum over b of shared ordinates is torch's and not order-pinned)
        assert torch.equal(leaf2.grad, gg) if per else bool(((leaf2.grad - gg).abs() <= bound).all())


SIZES = (1, 63, 65, 130)


@pytest.fixture(scope="module")
def engine_job():
    """259 perturbed Phillipsburg columns (synth1_phil's soil +-10 %, its rain scaled per column; some of them fault) in
    catchments of 1, 63, 65 and 130 columns with area weights; fp64, num_subcycles = 1; the fixture's five ordinates in
    LgarDims.giuh and in a shared CatchmentRouting."""
    from lgar_py_amd.catchments import CatchmentMap, CatchmentRouting
    from test_gpu_moisture import _engine, perturbed_job
    N = sum(SIZES)
    g, P, pr, pe = perturbed_job("synth1_phil", N=N, seed=8)
    assert int(g["num_subcycles"]) == 1 and len(g["giuh_ordinates"]) == 5
    ids = np.repeat(np.arange(len(SIZES)), SIZES)[np.random.default_rng(2).permutation(N)]
    w = np.random.default_rng(6).random(N) + 0.1
    make = lambda: _engine(g, P, torch.float64)
    eng = make()
    cmap = CatchmentMap(ids, weights=w, device=eng.device)
    routing = CatchmentRouting(g["giuh_ordinates"], n_catchments=len(SIZES), device=eng.device)
    pr, pe = torch.tensor(pr), torch.tensor(pe)
    res = eng.forward(pr, pe, series=("runoff",), catchments=cmap, catchment=("runoff", "giuh_runoff"), routing=routing, check=False)
    return dict(g=g, make=make, cmap=cmap, ids=ids, w=w, pr=pr, pe=pe, res=res, eng=eng, routing=routing)


def test_through_the_engine(engine_job):
    """out["catchment:routed:runoff"] (summed, then routed) against out["catchment:giuh_runoff"] (routed inside the forward
    kernels column by column, then summed): per entry both are sums of the same n_b K products w g runoff; one chain is at most
    n_b adds of the catchment sum and its weight product, K products and K adds of the fold: the bound of the issue,
    (n_b + K + 4) 2^-52 sum_k g_k sum_i |w_i runoff_i[t - k]|.  It is tight enough to refuse a shifted or a reversed
    hydrograph.  Faulted columns drop out of both sides alike (the status skips them in every row of both sums)."""
    from lgar_py_amd.catchments import CatchmentRouting
    j = engine_job
    res, cmap, g = j["res"], j["cmap"], j["g"]
    routed, inside = res["catchment:routed:runoff"], res["catchment:giuh_runoff"]
    T = j["pr"].shape[0]
    assert routed.dtype == torch.float64 and tuple(routed.shape) == (T, len(SIZES)) and "catchment:routed:giuh_runoff" in res
    status = j["eng"].status
    live = (status & 0x7F) == 0
    assert 0.5 <= float(live.double().mean()) and float(routed.abs().max()) > 0.01
    K = 5
    absw = (res["runoff"].abs() * cmap.weights(torch.float64)[None, :]) * live[None, :]
    A = torch.zeros(T, len(SIZES), dtype=torch.float64, device=routed.device).index_add_(1, torch.tensor(j["ids"], device=routed.device), absw)
    gdev = torch.tensor(g["giuh_ordinates"], device=routed.device)
    n_b = torch.tensor(SIZES, device=routed.device, dtype=torch.float64)
    bound = (n_b[None, :] + K + 4) * U2 * _dense(A, gdev)
    err = (routed - inside).abs()
    print("routed catchment sums vs in-kernel routing: worst error / bound = %.3g, faulted columns %d"
          % (float((err / bound.clamp_min(1e-300)).max()), int((~live).sum())))
    assert bool((err <= bound).all())
    # routing equals the definition on the sums it was given, bit for bit
    ref_y, ref_q = RH.route_ref(res["catchment:runoff"].cpu().numpy(), g["giuh_ordinates"])
    assert RH.same_bits(routed.cpu().numpy(), ref_y) and RH.same_bits(j["routing"].queue_of("runoff").cpu().numpy(), ref_q)
    # the bound refuses a hydrograph shifted by one row and the reversed one
    for wrong in (np.roll(g["giuh_ordinates"], 1), g["giuh_ordinates"][::-1].copy()):
        other = CatchmentRouting(wrong, device=routed.device).route(res["catchment:runoff"], carry=False)
        assert not bool(((other - inside).abs() <= bound).all())


def test_two_forward_calls_over_the_halves_equal_one(engine_job):
    """The engine carries its state and the routing its queue: two calls over the halves of T give the rows of one call bit for
    bit; routing without catchments raises; without routing nothing changes."""
    import lgar_py_amd as lg
    from lgar_py_amd.catchments import CatchmentRouting
    j = engine_job
    eng, cmap, pr, pe = j["make"](), j["cmap"], j["pr"], j["pe"]
    routing = CatchmentRouting(j["g"]["giuh_ordinates"], device=eng.device)
    h = pr.shape[0] // 2
    kw = dict(series=("runoff",), catchments=cmap, catchment=("runoff", "giuh_runoff"), routing=routing, check=False)
    a = eng.forward(pr[:h].contiguous(), pe[:h].contiguous(), **kw)
    b = eng.forward(pr[h:].contiguous(), pe[h:].contiguous(), **kw)
    for nm in ("catchment:routed:runoff", "catchment:routed:giuh_runoff", "catchment:runoff"):
        assert torch.equal(torch.cat([a[nm], b[nm]]), j["res"][nm]), nm
    assert torch.equal(routing.queue_of("runoff"), j["routing"].queue_of("runoff"))
    with pytest.raises(lg.LgarError, match="routing needs catchments"):
        j["make"]().forward(pr, pe, routing=routing, check=False)
    with pytest.raises(lg.LgarError):
        j["make"]().forward(pr, pe, catchments=cmap, catchment=("runoff",), routing=CatchmentRouting(np.ones((3, 5)), device=eng.device), check=False)
    plain = j["make"]().forward(pr, pe, series=("runoff",), catchments=cmap, catchment=("runoff",), check=False)
    assert set(plain) == {"runoff", "catchment:runoff", "catchment:weight"} and torch.equal(plain["catchment:runoff"], j["res"]["catchment:runoff"])


def test_gradients_end_to_end():
    """lgar_series -> catchment_sum -> catchment_route -> loss = sum(v * routed) (24 columns of grad_synth0_12h's soil in 3
    catchments, per-catchment ordinates that require grad, v fixed) against the same chain with the dense torch statement in
    place of the kernel.  The loss is linear in the routed matrix, so both chains hand the SAME v to the routing's backward pass
    and differ only in it: the gradient with respect to the catchment sums is adjoint(v) against torch's own, two orders of
    the same <= K products and K - 1 adds (m = 2 K: the bound m 2^-52 sum_k |g_k v[t + k]|), the ordinate gradient as in the
    test above (m = T + 1).  Behind the routing both chains run the same deterministic linear tail (CatchmentMap.spread, the
    tangent kernels): fed with the kernel chain's own gradient of the sums it reproduces the parameter gradients bit for bit,
    which is how the bound reaches the parameters."""
    import lgar_py_amd as lg
    from lgar_py_amd import workloads as W
    from lgar_py_amd.autograd import lgar_series, parameter_vjp
    from lgar_py_amd.catchments import CatchmentMap, catchment_route, catchment_sum
    g = np.load(os.path.join(GOLDEN, "grad_synth0_12h.npz"))
    n, B, K = 24, 3, 5
    Pn = W.perturbed_columns(n, frac=0.05, seed=21, base={k: g[k] for k in W.PARAM_KEYS + ("thickness",)})
    f = torch.tensor(g["forcing"], device="cuda")
    Tn = f.shape[0]
    pr, pe = f[:, 0:1].expand(Tn, n).contiguous(), f[:, 1:2].expand(Tn, n).contiguous()
    ekw = dict(engine_keywords(g), dtype=torch.float64)
    ids = np.array([0] * 9 + [2] * 5 + [-1] + [1] * 9)[np.random.default_rng(1).permutation(n)]
    cmap = CatchmentMap(ids, weights=np.random.default_rng(2).random(n) + 0.5)
    rng = np.random.default_rng(3)
    g0 = torch.tensor(g["giuh_ordinates"][None, :] * (1.0 + 0.2 * rng.random((B, K))), device="cuda")
    v = torch.tensor(rng.standard_normal((Tn, B)), device="cuda")
    grads = {}
    for chain in ("kernel", "dense"):
        P = {k: torch.tensor(val, device="cuda") for k, val in Pn.items()}
        for k in ("alpha", "n", "ksat"):
            P[k].requires_grad_(True)
        ordinates = g0.clone().requires_grad_(True)
        statuses = []
        runoff, _ = lgar_series(P["alpha"], P["n"], P["ksat"], P["theta_e"], P["theta_r"], P["thickness"], pr, pe, check=False,
                                status_out=statuses, **ekw)
        catch = catchment_sum(runoff, cmap, statuses[0])
        catch.retain_grad()
        routed = catchment_route(catch, ordinates) if chain == "kernel" else _dense(catch, ordinates)
        assert routed.requires_grad and tuple(routed.shape) == (Tn, B)
        (routed * v).sum().backward()
        grads[chain] = dict(P=P, ordinates=ordinates.grad, catch=catch.grad, sums=catch.detach(), routed=routed.detach(), status=statuses[0])
    k_, d_ = grads["kernel"], grads["dense"]
    assert torch.equal(k_["sums"], d_["sums"]) and float(k_["sums"].abs().max()) > 0
    assert RH.same_bits(k_["routed"].cpu().numpy(), RH.route_ref(k_["sums"].cpu().numpy(), g0.t().cpu().numpy())[0])
    # the gradient of the catchment sums: m = 2 K
    bound = 2 * K * U2 * torch.flip(_dense(torch.flip(v.abs(), [0]), g0), [0])
    err = (k_["catch"] - d_["catch"]).abs()
    print("d loss / d sums, kernel chain vs dense chain: worst error / bound = %.3g" % float((err / bound).max()))
    assert bool((err <= bound).all()) and float(k_["catch"].abs().min()) > 0
    # the ordinates got their gradient: m = T + 1
    sums = k_["sums"]
    absterms = torch.stack([(v[k:].abs() * sums[:Tn - k].abs()).sum(dim=0) for k in range(K)], dim=1)
    assert k_["ordinates"] is not None and tuple(k_["ordinates"].shape) == (B, K)
    assert bool(((k_["ordinates"] - d_["ordinates"]).abs() <= (Tn + 1) * U2 * absterms).all()) and float(k_["ordinates"].abs().max()) > 0
    # the linear tail: the kernel chain's parameter gradients are the tangent kernels on spread(d loss / d sums), bit for bit
    status = k_["status"]
    faulted = (status & 0x7F) != 0
    P = k_["P"]
    eng = lg.LgarEngine(P["alpha"].detach(), P["n"].detach(), P["ksat"].detach(), P["theta_e"], P["theta_r"], P["thickness"], **ekw)
    wr = cmap.spread(k_["catch"], torch.float64, status=status)
    wanted = [(kind, l) for kind in ("alpha", "n", "ksat") for l in range(eng.L)]
    vj, _ = parameter_vjp(eng, pr, pe, wr, torch.zeros_like(wr), wanted, check=False)
    for kind in ("alpha", "n", "ksat"):
        want = torch.stack([vj[(kind, l)] for l in range(eng.L)])
        want = torch.where(faulted[None, :], torch.zeros_like(want), want)
        assert torch.equal(P[kind].grad, want) and float(want.abs().max()) > 0, kind
        assert d_["P"][kind].grad is not None and bool(torch.isfinite(d_["P"][kind].grad).all())
        # (where the two chains hand the tail the same bits -- an error of 0 against the bound above -- it returns the same bits)
        if torch.equal(k_["catch"], d_["catch"]):
            assert torch.equal(P[kind].grad, d_["P"][kind].grad), kind
