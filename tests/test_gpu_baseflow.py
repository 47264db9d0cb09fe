"""GPU (-m gpu): the catchment baseflow -- lgar_catchment_baseflow / lgar_catchment_baseflow_grad through
baseflow.CatchmentBaseflow and baseflow.catchment_baseflow (autograd).

q[.][b] and s[.][b] are pure functions of column b of r and par and of state_in[b] (include/lgar.h), so the
kernels are held BIT FOR BIT to the numpy statement of the definition (tests/baseflow_host: baseflow_ref, baseflow_grad_ref),
the one tests/test_baseflow_host.py holds the host build of the same header to -- and that file holds the definition itself to
mpmath: gw_exp to mpmath.exp, the adjoint to derivatives of the real-arithmetic statement."""
import os

import numpy as np
import pytest

from _golden import engine_keywords
from conftest import GOLDEN

import baseflow_host as BH

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GRID_CAP = 2048  # LGAR_GW_GRID_CAP (csrc/lgar_baseflow.hip): workgroups of a launch; the rest by stride
GPU_T = (0, 1, 9, 17)


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return None if t is None else t.cpu().numpy()


def _raw(B, dt):
    """The kernels behind the package's own launch helpers, with parameters the Python layer would refuse (a negative expon)."""
    from lgar_py_amd import _capi, baseflow
    lib, dev = _capi.load(), torch.device("cuda:0")
    fwd = lambda r, par, st, want_state, want_s: baseflow._forward(lib, dev, r, par, dt, st, want_state, want_s)
    bwd = lambda gq, gs, r, s, par, st, want_par, want_state: baseflow._backward(lib, dev, gq, gs, r, s, par, dt, st, want_par, want_state)
    return fwd, bwd


@pytest.mark.parametrize("B", BH.SHAPE_B)
def test_kernels_equal_the_numpy_definition_bit_for_bit(B):
    """B in {1, 2, 63, 64, 65, 257} x T in {0, 1, 9, 17} x state_in present or NULL: the forward with s and state_out and with
    neither, the adjoint with gs, gpar and gstate / without gs, gpar only / with gs, neither / without gs, gstate only -- the host
    test's case data (every branch of the walk: flux, z clamped at either end, emptied, zero; -0.0 in r)."""
    rng = np.random.default_rng(1500 + B)
    for T in GPU_T:
        r, gq, gs, par, state, dt = BH.case_data(rng, T, B)
        fwd, bwd = _raw(B, dt)
        dr, dgq, dgs, dpar = _cuda(r), _cuda(gq), _cuda(gs), _cuda(par)
        for st in (None, state):
            what = (B, T, st is not None)
            dst = _cuda(st)
            q_ref, s_ref, so_ref = BH.baseflow_ref(r, par, dt, st)
            q, s, so = fwd(dr, dpar, dst, True, True)
            assert BH.same_bits(_np(q), q_ref) and BH.same_bits(_np(s), s_ref) and BH.same_bits(_np(so), so_ref), what
            q2, s2, so2 = fwd(dr, dpar, dst, False, False)
            assert BH.same_bits(_np(q2), q_ref) and s2 is None and so2 is None, what
            full = BH.baseflow_grad_ref(gq, gs, r, s_ref, par, dt, st)
            bare = BH.baseflow_grad_ref(gq, None, r, s_ref, par, dt, st)
            for (g_s, want_par, want_state), ref in (((dgs, True, True), full), ((None, True, False), bare), ((dgs, False, False), full),
                                                     ((None, False, True), bare)):
                gr, gpar, gstate = bwd(dgq, g_s, dr, s, dpar, dst, want_par, want_state)
                assert BH.same_bits(_np(gr), ref[0]), what
                assert (gpar is None) == (not want_par) and (gpar is None or BH.same_bits(_np(gpar), ref[1])), what
                assert (gstate is None) == (not want_state) and (gstate is None or BH.same_bits(_np(gstate), ref[2])), what


def test_the_capped_grid_strides():
    """A launch has at most 2048 workgroups of 256 lanes.  B = 256 x 2048 + 65, T = 9: the lanes stride over the catchments.
    Forward and adjoint with every output against the numpy definition, bit for bit."""
    B, T = 256 * GRID_CAP + 65, 9
    rng = np.random.default_rng(8)
    r, gq, gs, par, state, dt = BH.case_data(rng, T, B)
    fwd, bwd = _raw(B, dt)
    q_ref, s_ref, so_ref = BH.baseflow_ref(r, par, dt, state)
    dr, dpar, dst = _cuda(r), _cuda(par), _cuda(state)
    q, s, so = fwd(dr, dpar, dst, True, True)
    assert BH.same_bits(_np(q), q_ref) and BH.same_bits(_np(s), s_ref) and BH.same_bits(_np(so), so_ref)
    ref = BH.baseflow_grad_ref(gq, gs, r, s_ref, par, dt, state)
    got = bwd(_cuda(gq), _cuda(gs), dr, s, dpar, dst, True, True)
    assert all(BH.same_bits(_np(a), b) for a, b in zip(got, ref))


def test_chunked_calls_equal_one_call():
    """run(carry=True) cut at 1 row, at T - 1 rows and in the middle against one call, and a repeated call: the same bits."""
    from lgar_py_amd.baseflow import CatchmentBaseflow
    rng = np.random.default_rng(23)
    T, B = 17, 257
    r, _, _, par, state, dt = BH.case_data(rng, T, B)
    par[1] = np.abs(par[1])
    store = CatchmentBaseflow(par[0], par[1], par[2], dt)
    dr = _cuda(r)
    for st in (None, state):
        want_q, want_s, want_state = BH.baseflow_ref(r, par, dt, st)
        q, s = store.run(dr, carry=False, state=_cuda(st), storage=True)
        assert BH.same_bits(_np(q), want_q) and BH.same_bits(_np(s), want_s)
        assert torch.equal(store.run(dr, carry=False, state=_cuda(st)), q) and store.state_of() is None
        for cut in (1, T - 1, T // 2):
            key = (cut, st is None)
            a, sa = store.run(dr[:cut], key=key, state=_cuda(st), storage=True)
            b, sb = store.run(dr[cut:], key=key, storage=True)
            assert torch.equal(torch.cat([a, b]), q) and torch.equal(torch.cat([sa, sb]), s), cut
            assert BH.same_bits(_np(store.state_of(key)), want_state), cut
    store.reset()
    assert store.state_of((1, True)) is None


def test_entry_points_refuse_bad_arguments():
    """LGAR_E_ARG from the library itself: negative sizes, a dt_h that is not finite or <= 0, a null pointer the sizes say will be
    read or written, gpar or gstate wanted without s.  Nothing is launched by a refused call."""
    from lgar_py_amd import _capi
    lib = _capi.load()
    buf = torch.zeros(1024, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    fwd = (("r", p), ("T", 2), ("B", 4), ("par", p), ("dt", 1.0), ("state_in", None), ("state_out", p + 2048), ("q", p + 4096), ("s", p + 6144))
    run = lambda **kw: lib.lgar_catchment_baseflow(*[kw.get(k, d) for k, d in fwd], None)
    for bad in (dict(T=-1), dict(B=-1), dict(r=None), dict(par=None), dict(q=None), dict(dt=0.0), dict(dt=-1.0), dict(dt=float("nan")),
                dict(dt=float("inf"))):
        assert run(**bad) == -1, bad
    grd = (("gq", p), ("gs", p), ("r", p), ("s", p), ("T", 2), ("B", 4), ("par", p), ("dt", 1.0), ("state_in", None), ("gr", p + 2048),
           ("gpar", p + 4096), ("gstate", p + 6144))
    grad = lambda **kw: lib.lgar_catchment_baseflow_grad(*[kw.get(k, d) for k, d in grd], None)
    for bad in (dict(T=-1), dict(B=-1), dict(gq=None), dict(r=None), dict(s=None), dict(par=None), dict(gr=None), dict(dt=0.0),
                dict(dt=float("nan")), dict(s=None, gpar=None), dict(s=None, gstate=None)):
        assert grad(**bad) == -1, bad
    torch.cuda.synchronize()
    assert not buf.any()
    # accepted: B = 0 and T = 0 with nothing to write launch nothing; the rest write zeros here (smax = 0: 0 / 0 is a NaN, which the
    # selects carry -- parameter values are not policed), so only the return codes are looked at
    assert run(B=0, r=None, par=None, q=None) == 0 and run(T=0, state_out=None, r=None, q=None) == 0 and grad(B=0, gq=None, gr=None) == 0
    assert grad(T=0, gpar=None, gstate=None, gq=None, s=None) == 0
    assert run() == 0 and run(s=None, state_out=None) == 0 and grad() == 0 and grad(gs=None, gpar=None, gstate=None) == 0
    torch.cuda.synchronize()


def test_gradients_end_to_end():
    """lgar_series (runoff, percolation) -> catchment_sum of both -> catchment_route(runoff) + catchment_baseflow(percolation sums)
    -> network_route -> catchment_moments -> loss("nse"): 24 columns of synth1_phil's soil in three 4 cm layers with
    bottom_mode=1 (fronts that reach the bottom leave as percolation) in 3 catchments that form a chain (0 -> 1 -> 2);
    observations = the same chain on a perturbed parameter set.  The percolation sums are non-zero in some row; the loss is
    finite; the gradients to the soil parameters and to cgw, expon, smax are finite and non-zero; the baseflow node hands back
    the definition's bits (gr, gpar of baseflow_grad_ref for the gq it received)."""
    import lgar_py_amd as lg
    from lgar_py_amd import workloads as W
    from lgar_py_amd.autograd import lgar_series
    from lgar_py_amd.baseflow import catchment_baseflow
    from lgar_py_amd.catchments import CatchmentMap, CatchmentRouting, catchment_route, catchment_sum
    from lgar_py_amd.network import muskingum_coefficients, network_route
    from lgar_py_amd.scores import catchment_moments
    g = np.load(os.path.join(GOLDEN, "synth1_phil.npz"))
    n, B, K = 24, 3, 5
    base = {k: g[k] for k in W.PARAM_KEYS}
    base["thickness"] = np.array([4.0, 4.0, 4.0])
    Pn = W.perturbed_columns(n, frac=0.05, seed=21, base=base)
    Pobs = W.perturbed_columns(n, frac=0.05, seed=22, base=base)
    f = torch.tensor(g["forcing"], device="cuda")
    Tn = f.shape[0]
    pr, pe = f[:, 0:1].expand(Tn, n).contiguous(), f[:, 1:2].expand(Tn, n).contiguous()
    ekw = dict(engine_keywords(g), dtype=torch.float64, bottom_mode=1, ponded_depth_max=0.0)
    dt = float(ekw["dt_h"])
    ids = np.array([0] * 9 + [2] * 5 + [-1] + [1] * 9)[np.random.default_rng(1).permutation(n)]
    cmap = CatchmentMap(ids, weights=np.random.default_rng(2).random(n) + 0.5)
    rng = np.random.default_rng(3)
    routing = CatchmentRouting(g["giuh_ordinates"][None, :] * (1.0 + 0.2 * rng.random((B, K))))
    net = lg.CatchmentNetwork([1, 2, -1])
    coef = muskingum_coefficients(torch.tensor([2.0, 3.0, 1.5], dtype=torch.float64, device="cuda"),
                                  torch.tensor([0.2, 0.1, 0.3], dtype=torch.float64, device="cuda"), dt)
    leaf = lambda v: torch.tensor(v, dtype=torch.float64, device="cuda", requires_grad=True)
    cgw, expon, smax = leaf([0.02, 0.05, 0.03]), leaf([3.0, 2.0, 4.0]), leaf([2.0, 1.5, 3.0])
    state0 = torch.tensor([0.5, 0.2, 0.8], dtype=torch.float64, device="cuda")

    def discharge_of(Pdict, grad):
        P = {k: torch.tensor(val, device="cuda") for k, val in Pdict.items()}
        for k in ("alpha", "n", "ksat"):
            P[k].requires_grad_(grad)
        statuses = []
        runoff, perc = lgar_series(P["alpha"], P["n"], P["ksat"], P["theta_e"], P["theta_r"], P["thickness"], pr, pe, check=False,
                                   status_out=statuses, **ekw)
        recharge = catchment_sum(perc, cmap, statuses[0])
        if grad:
            recharge.retain_grad()
        base_q = catchment_baseflow(recharge, cgw, expon, smax, dt, state=state0)
        if grad:
            base_q.retain_grad()
        lateral = catchment_route(catchment_sum(runoff, cmap, statuses[0]), routing) + base_q
        return P, statuses[0], recharge, base_q, network_route(lateral, net, coef)

    with torch.no_grad():
        obs = discharge_of(Pobs, False)[4].clone()
    assert tuple(obs.shape) == (Tn, B) and float(obs.abs().max()) > 0
    score = lg.CatchmentScore(obs)
    P, status, recharge, base_q, q = discharge_of(Pn, True)
    faulted = (status & 0x7F) != 0  # (a few of these thin perturbed columns leave the reference's domain: the sums leave them out)
    assert int(faulted.sum()) < n // 4
    rsum = recharge.detach()
    assert float(rsum.max()) > 0 and int((rsum > 0).any(dim=1).sum()) >= 1  # percolation reaches the stores in some row
    loss = score.loss(catchment_moments(q, score), "nse")
    loss.backward()
    assert np.isfinite(float(loss.detach())) and float(loss.detach()) > 0
    par_np = np.stack([_np(cgw.detach()), _np(expon.detach()), _np(smax.detach())])
    q_ref, s_ref, _ = BH.baseflow_ref(_np(rsum), par_np, dt, _np(state0))
    assert BH.same_bits(_np(base_q.detach()), q_ref) and float(q_ref.sum()) > 0
    gr_ref, gpar_ref, _ = BH.baseflow_grad_ref(_np(base_q.grad), None, _np(rsum), s_ref, par_np, dt, _np(state0))
    assert BH.same_bits(_np(recharge.grad), gr_ref) and float(np.abs(gr_ref).max()) > 0
    assert BH.same_bits(np.stack([_np(cgw.grad), _np(expon.grad), _np(smax.grad)]), gpar_ref)
    for name, t in (("cgw", cgw), ("expon", expon), ("smax", smax)):
        assert bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().min()) > 0, name
    for kind in ("alpha", "n", "ksat"):
        assert bool(torch.isfinite(P[kind].grad).all()) and float(P[kind].grad.abs().max()) > 0, kind
