"""GPU (-m gpu): the resumable tangent kernels (lgar_forward_tangent_window) against the oracles in the tree -- the existing
tangent kernels bit for bit (a fresh window; a run cut into windows), the forward kernels' own central differences (a window
that starts from a spun-up state held fixed), the reference's loss.backward() (the carried gradient) -- and the catchment chain
from a spun-up state end to end.  N = 3 columns, or 64 / 24 perturbed ones: every test takes seconds."""
import numpy as np
import pytest

import _golden as G
from _golden import engine_keywords

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PARAMS = ("alpha", "n", "ksat", "theta_e", "theta_r", "thickness")
KINDS = ("alpha", "n", "ksat")
VALUES = ("depth", "theta", "psi", "k", "dzdt", "scalars")
CAP_SMALL = 8


def _engine(g, N, **kw):
    import lgar_py_amd as lg
    return lg.LgarEngine(*[g[k] for k in PARAMS], n_columns=N, **dict(engine_keywords(g), **kw))


def _job(g, N, rows=None):
    f = torch.tensor(g["forcing"][:rows], device="cuda")
    T = f.shape[0]
    w = torch.linspace(0.5, 1.5, T, device="cuda", dtype=torch.float64)[:, None].expand(T, N).contiguous()
    return f[:, 0:1].expand(T, N).contiguous(), f[:, 1:2].expand(T, N).contiguous(), w


def _layouts(eng, shared):
    """The two ways a backward pass lays its directions out (autograd.parameter_vjp): one launch per one-hot direction, every
    lane on its own; or the 3 x L directions of a column side by side in adjacent lanes that share the trapezoid (groups of
    9 for three layers).  Yields (engine, direction, forcing_group, share, number of directions)."""
    L, N = eng.L, eng.N
    if not shared:
        for kind in KINDS:
            for l in range(L):
                d = torch.zeros(L, N, dtype=eng.dtype, device="cuda")
                d[l] = 1.0
                yield eng, {kind: d}, 1, 0, 1
        return
    D = 3 * L
    rep = lambda t: t.repeat_interleave(D, dim=1)
    big = eng.like(*[rep(getattr(eng, k)) for k in PARAMS], with_state=False)
    dirs = {k: torch.zeros(L, D * N, dtype=eng.dtype, device="cuda") for k in KINDS}
    for b, (kind, l) in enumerate((kind, l) for kind in KINDS for l in range(L)):
        dirs[kind][l, b::D] = 1.0
    yield big, dirs, D, D, D


def _cuts(T, middle=None):
    """(0, 1), (1, 8), (8, T / 2), (T / 2, T - 1), (T - 1, T) scaled to T (tests/test_tangent_window_host.py)."""
    second = 8 if T // 2 > 8 else max(2, T // 4)
    p = [0, 1, second, T // 2 if middle is None else middle, T - 1, T]
    assert p == sorted(set(p))
    return list(zip(p[:-1], p[1:]))


def _same_state(a, b):
    return (all(torch.equal(getattr(a.value, nm), getattr(b.value, nm)) for nm in a.value.FIELDS)
            and all(torch.equal(a.tangent[nm], b.tangent[nm]) for nm in VALUES) and torch.equal(a.grad, b.grad))


def _chunked(eng, d, pr, pe, w, cuts, drop_tangent_at=None, **kw):
    from lgar_py_amd import TangentState
    end, series = None, []
    for lo, hi in cuts:
        if lo == drop_tangent_at:
            end = TangentState(end.value, {nm: torch.zeros_like(t) for nm, t in end.tangent.items()}, end.grad)
        grad, ser, st, end = eng.tangent_window(d, pr[lo:hi], pe[lo:hi], w_runoff=w[lo:hi], w_perc=w[lo:hi], start=end, want_series=True, **kw)
        series.append(ser)
    return grad, torch.cat(series), st, end


CONFIGS = [(torch.float64, 1, False), (torch.float64, 2, False), (torch.float64, 0, False), (torch.float32, 1, False),
           (torch.float64, 1, True), (torch.float64, 2, True)]
IDS = ["f64_fast", "f64_chain", "f64_literal", "f32", "f64_fast_shared", "f64_chain_shared"]


@pytest.mark.parametrize("dtype, mode, shared", CONFIGS, ids=IDS)
def test_fresh_window_is_the_existing_tangent_bit_for_bit(dtype, mode, shared):
    g = G.load("grad_synth0_12h")
    eng = _engine(g, 3, dtype=dtype, search_mode=mode)
    pr, pe, w = _job(g, 3)
    moved = 0.0
    for e, d, fg, share, D in _layouts(eng, shared):
        want = e.tangent(d, pr, pe, w_runoff=w, w_perc=w, want_series=True, forcing_group=fg, share=share)
        got = e.tangent_window(d, pr, pe, w_runoff=w, w_perc=w, want_series=True, forcing_group=fg, share=share)
        assert tuple(want[0].shape) == (3 * D,) and all(torch.equal(a, b) for a, b in zip(want, got[:3]))
        moved += float(want[0].abs().sum())
    assert moved > 0.0


@pytest.mark.parametrize("name, middle", [("grad_synth0_12h", None), ("grad_manyfronts_60", 45)], ids=["synth0", "manyfronts"])
@pytest.mark.parametrize("dtype, mode, shared", [c for c in CONFIGS if c[1] != 0], ids=[i for i in IDS if i != "f64_literal"])
def test_chunked_windows_are_one_call_bit_for_bit(name, middle, dtype, mode, shared):
    """grad_manyfronts_60 with the chain (mode 2): more than 8 fronts at the cuts at rows 45 and 59 (handed over at load), and the
    column passes 8 inside the chunk (8, 45) (handed over inside a chunk); both resume from the chunk's own state_in."""
    g = G.load(name)
    eng = _engine(g, 3, dtype=dtype, search_mode=mode)
    pr, pe, w = _job(g, 3)
    T = pr.shape[0]
    cuts = _cuts(T, middle)
    if middle is not None:
        nf = g["nfronts"]
        assert nf[middle - 1] > CAP_SMALL and nf[T - 2] > CAP_SMALL and nf[cuts[2][0] - 1] <= CAP_SMALL
    differs = False
    for e, d, fg, share, D in _layouts(eng, shared):
        kw = dict(forcing_group=fg, share=share)
        one = e.tangent_window(d, pr, pe, w_runoff=w, w_perc=w, want_series=True, **kw)
        got = _chunked(e, d, pr, pe, w, cuts, **kw)
        assert all(torch.equal(a, b) for a, b in zip(one[:3], got[:3])) and _same_state(one[3], got[3])
        assert int(one[2].abs().max()) == 0
        if dtype == torch.float64:
            assert int(one[3].value.n_fronts[0]) == g["nfronts"][-1]
        dropped = _chunked(e, d, pr, pe, w, cuts, drop_tangent_at=cuts[3][0], **kw)
        differs |= not torch.equal(dropped[0], one[0])
    assert differs  # the tangent state matters


@pytest.mark.parametrize("shared", [False, True], ids=["own_lanes", "shared_trapezoid"])
def test_carried_gradient_matches_reference_autograd(shared):
    """grad_synth0_12h, loss = mean(runoff^2) of column 0: the gradient folded over five windows is the reference's own
    loss.backward() at the project's gradient bar."""
    g = G.load("grad_synth0_12h")
    eng = _engine(g, 3)
    pr, pe, _ = _job(g, 3)
    T = pr.shape[0]
    r = eng.forward(pr, pe, series=("runoff",))["runoff"]
    loss = float(torch.mean(r[:, 0] ** 2))
    w = (2.0 * r / T).contiguous()
    got = {kind: np.zeros(3) for kind in KINDS}
    for e, d, fg, share, D in _layouts(eng, shared):
        grad, _, st, _ = _chunked(e, d, pr, pe, w, _cuts(T), forcing_group=fg, share=share)
        assert int(st.abs().max()) == 0
        if D == 1:
            (kind, mat), = d.items()
            got[kind][int(mat[:, 0].argmax())] = float(grad[0])
        else:
            for b, (kind, l) in enumerate((kind, l) for kind in KINDS for l in range(3)):
                got[kind][l] = float(grad[b])  # column 0's directions are lanes 0 .. 8
    G.check_gradients(g, loss, got)


SPIN = 60


def _storm(N, frac, seed):
    """N perturbed columns under the scaled synth_1 storm (tests/test_gpu_autograd.py::test_tangent_matches_finite_differences)"""
    from lgar_py_amd import workloads as W
    Pn = W.perturbed_columns(N, frac=frac, seed=seed)
    sc = W.forcing_scale(N, 0.5, 1.0, seed=12)
    pr = torch.tensor(W.synth1_forcing()[:, 0:1] * sc[None, :], device="cuda")
    kw = dict(dt_h=300.0 / 3600.0, ponded_depth_max=0.0, dtype=torch.float64)
    return Pn, pr, torch.zeros_like(pr), kw


def test_stop_gradient_window_is_the_derivative_of_the_forward_from_that_state():
    """test_tangent_matches_finite_differences over the last 84 rows from a snapshot taken after 60: its workload, directions,
    step sizes and (bulk) bars."""
    import lgar_py_amd as lg
    N = 64
    Pn, pr, pe, kw = _storm(N, 0.10, 11)
    T = pr.shape[0]
    w = torch.linspace(0.5, 1.5, T, device="cuda", dtype=torch.float64)[:, None].expand(T, N).contiguous()
    base = lg.LgarEngine(*[Pn[k] for k in PARAMS], **kw)
    base.forward(pr[:SPIN], pe[:SPIN], series=(), check=False)
    snap = base.snapshot()
    prw, pew, ww = pr[SPIN:].contiguous(), pe[SPIN:].contiguous(), w[SPIN:].contiguous()

    def J(P):
        e = lg.LgarEngine(*[P[k] for k in PARAMS], **kw)
        e.restore(snap)
        r = e.forward(prw, pew, series=("runoff",), check=False)["runoff"]
        return (ww * r).sum(0).cpu().numpy(), e.status.cpu().numpy()

    _, st0 = J(Pn)
    checked = 0
    for kind, l, h in (("alpha", 0, 1e-7), ("n", 0, 1e-6), ("ksat", 0, 1e-6), ("ksat", 1, 1e-6), ("n", 1, 1e-6)):
        d = torch.zeros(3, N, dtype=torch.float64)
        d[l] = 1.0
        g, _, st, _ = base.tangent_window({kind: d}, prw, pew, w_runoff=ww, start=snap, keep_state=False)
        fresh, _, _ = base.tangent({kind: d}, prw, pew, w_runoff=ww)
        assert not torch.equal(fresh, g)
        Pp = {k: v.copy() for k, v in Pn.items()}
        Pm = {k: v.copy() for k, v in Pn.items()}
        Pp[kind][l] += h * Pn[kind][l]
        Pm[kind][l] -= h * Pn[kind][l]
        jp, sp = J(Pp)
        jm, sm = J(Pm)
        fd = (jp - jm) / (2 * h * Pn[kind][l])
        got = g.cpu().numpy()
        ok = (st0 == 0) & (sp == 0) & (sm == 0) & (st.cpu().numpy() == 0)
        rel = np.abs(got - fd)[ok] / np.maximum(np.abs(fd[ok]), 1e-3 * np.abs(fd[ok]).max() + 1e-12)
        print(kind, l, "median", np.median(rel), "within 1e-2", (rel <= 1e-2).mean(), "columns", int(ok.sum()))
        assert np.median(rel) <= 1e-4, (kind, l, np.median(rel))
        assert (rel <= 1e-2).mean() >= 0.5, (kind, l, (rel <= 1e-2).mean())
        checked += int(ok.sum())
    assert checked > 100


@pytest.mark.parametrize("shared", [False, True], ids=["own_lanes", "shared_trapezoid"])
def test_catchment_chain_from_a_spun_up_state_end_to_end(shared, monkeypatch):
    """24 columns in 3 catchments, 60 rows of spin-up, then lgar_series(initial_state=) -> catchment_sum -> catchment_route ->
    catchment_moments -> loss("nse") over the other 84 rows: the loss and the parameter gradients are finite and non-zero and
    equal the direct contraction parameter_vjp(start=) of the same incoming gradient, bit for bit."""
    import lgar_py_amd as lg
    import lgar_py_amd.autograd as A
    from lgar_py_amd import workloads as W
    from lgar_py_amd.catchments import CatchmentMap, CatchmentRouting, catchment_route, catchment_sum
    from lgar_py_amd.scores import catchment_moments
    monkeypatch.setattr(A, "SHARE_MIN_LANES", 1 if shared else 1 << 30)
    n, B, K = 24, 3, 5
    Pn, pr, pe, kw = _storm(n, 0.05, 21)
    Pobs = _storm(n, 0.05, 22)[0]
    ids = np.array([0] * 9 + [2] * 5 + [-1] + [1] * 9)[np.random.default_rng(1).permutation(n)]
    cmap = CatchmentMap(ids, weights=np.random.default_rng(2).random(n) + 0.5)
    rng = np.random.default_rng(3)
    routing = CatchmentRouting(np.asarray(W.GIUH)[None, :] * (1.0 + 0.2 * rng.random((B, K))))
    prw, pew = pr[SPIN:].contiguous(), pe[SPIN:].contiguous()

    def spun_up(Pdict):
        e = lg.LgarEngine(*[Pdict[k] for k in PARAMS], **kw)
        e.forward(pr[:SPIN], pe[:SPIN], series=(), check=False)
        return e.snapshot()

    def routed_of(Pdict, snap, grad):
        P = {k: torch.tensor(val, device="cuda") for k, val in Pdict.items()}
        for k in KINDS:
            P[k].requires_grad_(grad)
        statuses = []
        runoff, _ = A.lgar_series(*[P[k] for k in PARAMS], prw, pew, check=False, status_out=statuses, initial_state=snap, **kw)
        return P, statuses[0], catchment_route(catchment_sum(runoff, cmap, statuses[0]), routing)

    with torch.no_grad():
        obs = routed_of(Pobs, spun_up(Pobs), False)[2].clone()
    assert float(obs.abs().max()) > 0
    score = lg.CatchmentScore(obs)
    snap = spun_up(Pn)
    P, status, routed = routed_of(Pn, snap, True)
    routed.retain_grad()
    loss = score.loss(catchment_moments(routed, score), "nse")
    loss.backward()
    assert np.isfinite(float(loss)) and float(loss) != 0.0
    faulted = (status & 0x7F) != 0
    eng = lg.LgarEngine(*[P[k].detach() for k in PARAMS], **kw)
    wr = cmap.spread(routing.adjoint(routed.grad), torch.float64, status=status)
    wanted = [(kind, l) for kind in KINDS for l in range(eng.L)]
    vj, _ = A.parameter_vjp(eng, prw, pew, wr, torch.zeros_like(wr), wanted, check=False, start=snap)
    for kind in KINDS:
        want = torch.stack([vj[(kind, l)] for l in range(eng.L)])
        want = torch.where(faulted[None, :], torch.zeros_like(want), want)
        assert torch.equal(P[kind].grad, want) and float(want.abs().max()) > 0 and bool(torch.isfinite(want).all()), kind
