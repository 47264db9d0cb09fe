"""CPU: the tangent of the soil-moisture output (lgar_soil_moisture_tangent, LgarEngine.soil_moisture_tangent,
autograd.lgar_moisture_series) on the host build of the kernel's own header (tests/moisture_tangent_host): bit for bit against the
numpy statement of the definition, against the reference's own autograd of the same bins (tests/golden/moisture_grad), and the
autograd node through the device-code simulator."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import _golden as G
from lgar_py_amd import _capi
from lgar_py_amd._capi import LgarDims, LgarParams, LgarState

PARAMS = ("alpha", "n", "ksat", "theta_e", "theta_r", "thickness")
KINDS = ("alpha", "n", "ksat")
FIXTURES = ("grad_synth0_12h", "grad_synth1_phil", "grad_manyfronts_60", "grad_two_layer_phil_150", "grad_six_layer_synth1")


def _engine(name, N, **kw):
    import moisture_tangent_host as H
    g = G.load(name)
    return H.MoistureTangentSimEngine(*[g[k] for k in PARAMS], n_columns=N, **dict(G.engine_keywords(g), **kw))


@functools.lru_cache(maxsize=None)
def _bases():
    import moisture_tangent_host as H
    bases = {name: H.base_state(_engine(name, 1, search_mode=2), G.load(name)) for name in H.BASES}
    assert int(bases["grad_manyfronts_60"]["n_fronts"][0]) == 19 and bases["grad_manyfronts_60"]["depth"].shape[0] == 32
    return bases


def mgrad(name):
    import moisture_tangent_host as H
    return H.mgrad(name)


# 1 ---- bit for bit against the numpy statement ------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, 63, 64, 65, 257])
def test_grid_is_the_numpy_statement_bit_for_bit(M):
    import moisture_tangent_host as H
    n = 0
    for label, c in H.grid(_bases(), shapes=(M,)):
        rc, out, grad = H.host_call(c)
        assert rc == 0, label
        H.check(c, (out, grad), label)
        n += 1
    assert n == 2 * 2 * 2 * len(H.BIN_SETS) * 3


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_planted_ties_take_the_stated_side(dtype):
    import moisture_tangent_host as H
    for label, c, want in H.ties(dtype):
        rc, out, grad = H.host_call(c)
        assert rc == 0, label
        H.check(c, (out, grad), label)
        assert np.isfinite(grad).all() and np.isfinite(out).all(), label
        for (_, i), v in want.items():
            assert out[i, 0] == dtype(v) and (v != 0.0 or not np.signbit(out[i, 0])), (label, i, out[:, 0], v)
    # the half-open rule keeps closure with a front on an edge: the covering bins sum to the tangent of the stored volume
    label, c, _ = H.ties(np.float64)[0]
    _, out, _ = H.host_call(c)
    d, th, dd, dth = (c[k][:4, 0].astype(np.float64) for k in ("depth", "theta", "ddepth", "dtheta"))
    t, dt = np.array([0.0, d[0], 44.0, 175.0]), np.array([0.0, dd[0], 0.0, 0.0])
    assert abs(out[:, 0].sum() - (dth * (d - t) + th * (dd - dt)).sum()) <= 1e-15


def test_corrupt_table_stays_in_bounds_and_is_the_statement():
    import moisture_tangent_host as H
    cases = H.corrupt(_bases()["grad_manyfronts_60"]) + H.corrupt(_bases()["grad_synth0_12h"], np.float32)
    for c, got in zip(cases, H.run(cases)):
        H.check(c, got, "corrupt")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_program_runs_the_grid_plain_and_sanitized(sanitize):
    """The stand-alone program (its arrays allocated at their exact sizes) over every 8th case of the grid, every tie and the
    corrupt tables; the second build is AddressSanitizer + UBSan, any finding aborts.  Nothing is loaded into python."""
    import moisture_tangent_host as H
    cases = [c for _, c in H.grid(_bases(), keep_every=8)] + [c for dt in (np.float64, np.float32) for _, c, _ in H.ties(dt)]
    cases += H.corrupt(_bases()["grad_manyfronts_60"]) + H.corrupt(_bases()["grad_synth0_12h"], np.float32)
    assert len(cases) > 100
    for c, got in zip(cases, H.run(cases, sanitize)):
        H.check(c, got, "program")


# 2 ---- reference parity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("name", FIXTURES)
def test_reference_parity(name, mode):
    import moisture_tangent_host as H
    H.reference_parity(_engine, name, mode)


# 3 ---- the autograd node ---------------------------------------------------------------------------------------------------
@pytest.fixture()
def sim():
    import lgar_py_amd.autograd as A
    import moisture_tangent_host as H
    before = H.install()
    yield A
    A.LgarEngine = before


def _leaves(g, N, dev="cpu"):
    P = {k: torch.tensor(np.repeat(g[k][:, None], N, 1), device=dev) for k in PARAMS}
    if N > 1:  # columns that differ
        for k in KINDS:
            P[k] = P[k] * torch.linspace(0.97, 1.03, N, dtype=torch.float64, device=dev)[None, :]
    for k in KINDS:
        P[k] = P[k].detach().requires_grad_(True)
    return P


def _grads(P):
    return {k: P[k].grad.clone() for k in KINDS}


def test_forward_has_the_bits_of_the_existing_runs(sim):
    import moisture_tangent_host as H
    name, N = "grad_synth0_12h", 3
    g = G.load(name)
    kw = dict(G.engine_keywords(g), dtype=torch.float64)
    pr, pe = G.replicated_forcing(g, N)
    P = _leaves(g, N)
    edges = mgrad(name)["edges_fixed"]
    for every, e, what in ((3, edges, "theta"), (5, None, "storage")):
        ro, pc, mo = sim.lgar_moisture_series(*[P[k] for k in PARAMS], pr, pe, every, edges=e, what=what, **kw)
        ro0, pc0 = sim.lgar_series(*[P[k] for k in PARAMS], pr, pe, **kw)
        eng = H.MoistureTangentSimEngine(*[P[k].detach() for k in PARAMS], **kw)
        want = eng.run_with_soil_moisture(pr, pe, every, e, what)
        assert torch.equal(ro, ro0) and torch.equal(pc, pc0) and mo.shape[0] == 12 // every
        assert H.same_bits(mo.detach().numpy(), want["soil_moisture"].numpy())
        assert mo.requires_grad and ro.requires_grad


@pytest.mark.parametrize("every", [3, 5, 12, 20], ids=["every3", "every5_trailing", "one_window", "no_snapshot"])
def test_zero_moisture_cotangent_gives_lgar_series_gradients_bit_for_bit(sim, every):
    """The windows carry the bits of one call, and a zero cotangent adds +0.0: also with a trailing partial window (every = 5 over
    12 rows) and with no full window at all."""
    name, N = "grad_synth0_12h", 3
    g = G.load(name)
    kw = dict(G.engine_keywords(g), dtype=torch.float64)
    pr, pe = G.replicated_forcing(g, N)
    w = torch.linspace(0.5, 1.5, 12, dtype=torch.float64)[:, None]
    P = _leaves(g, N)
    ro, pc = sim.lgar_series(*[P[k] for k in PARAMS], pr, pe, **kw)
    (w * ro + 0.5 * w * pc).sum().backward()
    want = _grads(P)
    P = _leaves(g, N)
    ro, pc, mo = sim.lgar_moisture_series(*[P[k] for k in PARAMS], pr, pe, every, what="storage", **kw)
    ((w * ro + 0.5 * w * pc).sum() + (mo * 0.0).sum()).backward()
    for k in KINDS:
        assert torch.equal(P[k].grad, want[k]) and float(want[k].abs().max()) > 0.0, k


def test_moisture_only_loss_is_the_fixtures_contraction(sim):
    """loss = sum weights * moisture on grad_synth0_12h, every = 3 (the fixture's rows are its four snapshots): the gradient is
    sum_s,i weights * J.  Each J entry is held to GRADIENT * max |J| of its kind, so the contraction is held to that times
    sum |weights|."""
    name = "grad_synth0_12h"
    g, m = G.load(name), mgrad(name)
    assert list(m["rows"]) == [2, 5, 8, 11]
    kw = dict(G.engine_keywords(g), dtype=torch.float64)
    pr, pe = G.replicated_forcing(g, 1)
    rng = np.random.default_rng(3)
    for key, edges in (("fixed", m["edges_fixed"]), ("layers", None)):
        J = m["J_" + key] * np.array([1.0, 1.0, float(g["frozen_factor"])])[None, None, :, None]
        w = rng.uniform(-1.0, 2.0, J.shape[:2])
        P = _leaves(g, 1)
        _, _, mo = sim.lgar_moisture_series(*[P[k] for k in PARAMS], pr, pe, 3, edges=edges, what="storage", **kw)
        assert np.abs(mo.detach().numpy()[:, :, 0] - m["S_" + key]).max() <= G.NATIVE * np.abs(m["S_" + key]).max()
        (torch.tensor(w)[:, :, None] * mo).sum().backward()
        for ki, k in enumerate(KINDS):
            want = np.einsum("sd,sdl->l", w, J[:, :, ki, :])
            bar = G.GRADIENT * np.abs(J[:, :, ki, :]).max() * np.abs(w).sum()
            err = np.abs(P[k].grad[:, 0].numpy() - want).max()
            print("%s %s: |got - sum w J| = %.3g, bar %.3g" % (key, k, err, bar))
            assert err <= bar and np.abs(want).max() > 0.0, (key, k, err, bar)


def _by_hand(eng_of, P, pr, pe, every, edges, what, w, start=None):
    """The moisture-only gradient by one-hot directions, one at a time, each snapshot's tangent taken as an array (out mode) and
    contracted with the weights on the host: the same launches as the node's backward pass in another association."""
    L, N = P["alpha"].shape
    eng = eng_of(N)
    out = {k: np.zeros((L, N)) for k in KINDS}
    for k in KINDS:
        for l in range(L):
            d = torch.zeros(L, N, dtype=torch.float64)
            d[l] = 1.0
            state = start
            for s in range(pr.shape[0] // every):
                _, _, _, state = eng.tangent_window({k: d}, pr[s * every:(s + 1) * every], pe[s * every:(s + 1) * every], start=state)
                t = eng.soil_moisture_tangent(state, edges, what).numpy()
                out[k][l] += (w[s] * t).sum(0)
    return out


def test_carried_windows_equal_the_contractions_done_by_hand(sim):
    """Also with a trailing partial window (every = 5 over 12 rows), from a given initial state, and for what = 'theta' with a dead
    bin whose snapshot is NaN.  The two associations use the same launches in another order: 1e-12 of the largest entry."""
    import moisture_tangent_host as H
    name, N = "grad_synth0_12h", 2
    g = G.load(name)
    kw = dict(G.engine_keywords(g), dtype=torch.float64)
    pr, pe = G.replicated_forcing(g, N)
    rng = np.random.default_rng(5)
    worst = 0.0
    for every, edges, what, spun in ((3, np.array(H.SEVEN), "theta", False), (5, None, "storage", False), (4, np.array(H.SEVEN), "storage", True)):
        P = _leaves(g, N)
        vals = [P[k].detach() for k in PARAMS]
        eng_of = lambda n: H.MoistureTangentSimEngine(*vals, **kw)
        start, rows = None, slice(None)
        if spun:
            e0 = eng_of(N)
            e0.forward(pr[:4], pe[:4])
            start, rows = e0.snapshot(), slice(4, None)
        extra = dict(initial_state=start) if spun else {}
        _, _, mo = sim.lgar_moisture_series(*[P[k] for k in PARAMS], pr[rows], pe[rows], every, edges=edges, what=what, **kw, **extra)
        w = rng.uniform(-1.0, 2.0, tuple(mo.shape))
        dead = torch.isnan(mo.detach())
        assert bool(dead.any()) == (what == "theta")
        torch.where(dead, torch.zeros_like(mo), torch.tensor(w) * mo).sum().backward()
        hand = _by_hand(eng_of, P, pr[rows], pe[rows], every, edges, what, w, start)
        for k in KINDS:
            got = P[k].grad.numpy()
            assert np.isfinite(got).all() and np.abs(hand[k]).max() > 0.0
            worst = max(worst, np.abs(got - hand[k]).max() / np.abs(hand[k]).max())
    print("carried windows against contractions by hand: %.3g of the largest entry" % worst)
    assert worst <= 1e-12


def test_a_nan_cotangent_under_a_dead_bin_is_discarded(sim):
    import moisture_tangent_host as H
    g = G.load("grad_synth0_12h")
    kw = dict(G.engine_keywords(g), dtype=torch.float64)
    pr, pe = G.replicated_forcing(g, 1)
    P = _leaves(g, 1)
    _, _, mo = sim.lgar_moisture_series(*[P[k] for k in PARAMS], pr, pe, 3, edges=np.array(H.SEVEN), what="theta", **kw)
    cot = torch.ones_like(mo)
    cot[:, 6] = float("nan")
    assert bool(torch.isnan(mo[:, 6]).all())
    mo.backward(cot)
    assert all(bool(torch.isfinite(P[k].grad).all()) and float(P[k].grad.abs().max()) > 0.0 for k in KINDS)


def test_a_forcing_direction_reaches_scale_p_from_a_moisture_only_loss(sim):
    import lgar_py_amd as lg
    g = G.load("grad_synth0_12h")
    kw = dict(G.engine_keywords(g), dtype=torch.float64)
    pr, pe = G.replicated_forcing(g, 2)
    sp = torch.ones(2, dtype=torch.float64, requires_grad=True)
    se = torch.tensor(1.0, dtype=torch.float64, requires_grad=True)
    prs, pes, fd = lg.scaled_forcing(pr, pe, sp, se)
    P = _leaves(g, 2)
    _, _, mo = sim.lgar_moisture_series(*[P[k] for k in PARAMS], prs, pes, 3, what="storage", forcing_directions=fd, **kw)
    mo.sum().backward()
    assert bool(torch.isfinite(sp.grad).all()) and float(sp.grad.abs().min()) > 0.0


# 4 ---- refusals and messages -----------------------------------------------------------------------------------------------
def test_refusals_of_the_entry_point():
    import moisture_tangent_host as H
    entry = H.library().mthost_soil_moisture_tangent
    L, F, M, D = 3, 8, 6, 7
    buf = np.ones(4096)
    a = buf.ctypes.data
    nf = np.full(M, 3, np.int32)
    fl = np.zeros((F, M), np.uint8)

    def run(dims=True, params=True, thickness=True, state=True, dstate=True, null=(), edges=a, n_bins=D, what=0, out=a + 8 * 1024,
            cot=a, group=1, grad=a + 8 * 2048, dtype=_capi.F64, M=M, L=L, F=F):
        d = LgarDims()
        d.n_columns, d.n_layers, d.front_slots = M, L, F
        p = LgarParams()
        p.thickness = a if thickness else None
        s, ds = LgarState(), LgarState()
        s.depth, s.theta, s.flags, s.n_fronts = a, a, fl.ctypes.data, nf.ctypes.data
        ds.depth, ds.theta = a, a
        for which, field in null:
            setattr(s if which == "state" else ds, field, None)
        ref = lambda x, on: C.byref(x) if on else None
        return entry(ref(d, dims), ref(p, params), ref(s, state), ref(ds, dstate), edges, n_bins, what, out, cot, group, grad, dtype)

    assert run() == 0 and run(out=None) == 0 and run(cot=None, grad=None) == 0 and run(edges=None, n_bins=L) == 0 and run(group=3) == 0
    bad = [dict(dims=False), dict(params=False), dict(thickness=False), dict(state=False), dict(dstate=False), dict(null=[("state", "depth")]),
           dict(null=[("state", "theta")]), dict(null=[("state", "flags")]), dict(null=[("state", "n_fronts")]), dict(null=[("dstate", "depth")]),
           dict(null=[("dstate", "theta")]), dict(out=None, cot=None, grad=None), dict(cot=None), dict(grad=None), dict(out=None, cot=None),
           dict(group=0), dict(group=-1), dict(group=4), dict(n_bins=0), dict(n_bins=33), dict(edges=None, n_bins=D), dict(what=2), dict(what=-1),
           dict(dtype=2), dict(L=1), dict(L=7), dict(F=33), dict(F=3), dict(M=-1)]
    for kw in bad:
        assert run(**kw) == -1, kw
    buf[:] = 7.0
    assert run(M=0) == 0 and run(M=0, out=None) == 0 and (buf == 7.0).all()  # no lanes: nothing is touched
    assert run(M=0, out=None, cot=None, grad=None) == -1 and run(M=0, group=0) == -1  # ... but a bad call is still refused


def test_messages_of_the_engine():
    import lgar_py_amd as lg
    import moisture_tangent_host as H
    g = G.load("grad_synth0_12h")
    eng = _engine("grad_synth0_12h", 6)
    pr, pe = G.replicated_forcing(g, 6)
    d = {"ksat": torch.ones(3, 6, dtype=torch.float64)}
    _, _, _, end = eng.tangent_window(d, pr[:3], pe[:3])
    out = eng.soil_moisture_tangent(end, H.SEVEN)
    assert tuple(out.shape) == (7, 6) and out.dtype == torch.float64
    before = end.grad.clone()
    assert eng.soil_moisture_tangent(end, H.SEVEN, cot=torch.zeros(7, 2, dtype=torch.float64), group=3) is end and torch.equal(end.grad, before)
    for kw, msg in ((dict(what="volume"), "what must be 'theta' or 'storage'"), (dict(edges=[0.0]), "at least two entries"),
                    (dict(edges=[0.0, 5.0, 5.0]), "strictly increasing"), (dict(edges=np.arange(34.0)), "at most 32 bins"),
                    (dict(group=4), "group must be >= 1 and divide"), (dict(group=0), "group must be >= 1 and divide"),
                    (dict(cot=torch.zeros(3, 5, dtype=torch.float64)), r"cot must be a contiguous fp64 \[3, 6\]"),
                    (dict(cot=torch.zeros(3, 6, dtype=torch.float32)), "cot must be a contiguous fp64"),
                    (dict(cot=torch.zeros(3, 2, dtype=torch.float64), group=2), r"fp64 \[3, 3\]")):
        with pytest.raises(lg.LgarError, match=msg):
            eng.soil_moisture_tangent(end, **kw)
    with pytest.raises(lg.LgarError, match="tstate must be a TangentState"):
        eng.soil_moisture_tangent(end.value)
    with pytest.raises(lg.LgarError, match="tstate holds 6 columns, this engine has 3"):
        _engine("grad_synth0_12h", 3).soil_moisture_tangent(end)
    with pytest.raises(lg.LgarError, match="tstate is torch.float64"):
        _engine("grad_synth0_12h", 6, dtype=torch.float32).soil_moisture_tangent(end)
    with pytest.raises(lg.LgarError, match="every must be >= 1"):
        lg.autograd.parameter_vjp(eng, pr, pe, None, None, [("ksat", 0)], moisture=(0, None, "theta", torch.zeros(0)))
    with pytest.raises(lg.LgarError, match=r"cotangent must be a fp64 \[4, 3, 6\]"):
        lg.autograd.parameter_vjp(eng, pr, pe, None, None, [("ksat", 0)], moisture=(3, None, "theta", torch.zeros(4, 3, 5, dtype=torch.float64)))
    assert "lgar_soil_moisture_tangent" in _capi.EXPORTS and _capi.ABI_VERSION == 4
