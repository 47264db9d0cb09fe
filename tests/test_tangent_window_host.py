"""CPU: the resumable tangent (lgar_forward_tangent_window, LgarEngine.tangent_window / snapshot / restore,
autograd.parameter_vjp(start=) and lgar_series(initial_state=)) on the host build of the kernels' own headers
(tests/window_host).  The oracle is in the tree: the tangent path that existed before (devsim_tangent), bit for bit, and the
forward engine's own central differences for the stop-gradient window."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _golden as G
import _hostbuild
from lgar_py_amd import _capi
from lgar_py_amd import workloads as W

PARAMS = ("alpha", "n", "ksat", "theta_e", "theta_r", "thickness")
KINDS = ("alpha", "n", "ksat")
VALUES = ("depth", "theta", "psi", "k", "dzdt", "scalars")


def _engine(name, N, **kw):
    import window_host
    g = G.load(name)
    return window_host.WindowSimEngine(*[g[k] for k in PARAMS], n_columns=N, **dict(G.engine_keywords(g), **kw))


def _job(name, N=3, rows=None):
    """precip, pet [T, N] (the fixture's one series for every column) and the ramp weights [T, N]."""
    f = G.load(name)["forcing"][:rows]
    T = f.shape[0]
    w = np.repeat(np.linspace(0.5, 1.5, T)[:, None], N, 1)
    return np.repeat(f[:, 0:1], N, 1), np.repeat(f[:, 1:2], N, 1), w


def _directions(L, N):
    for kind in KINDS:
        for l in range(L):
            d = np.zeros((L, N))
            d[l] = 1.0
            yield {kind: d}


def _cuts(T, middle=None):
    """The cuts of test_gpu_parity.py::test_chunked_run_equals_single_run -- (0, 1), (1, 8), (8, T / 2), (T / 2, T - 1), (T - 1, T)
    -- scaled to T: a run too short for a cut at row 8 before its middle takes T / 4."""
    second = 8 if T // 2 > 8 else max(2, T // 4)
    p = [0, 1, second, T // 2 if middle is None else middle, T - 1, T]
    assert p == sorted(set(p))
    return list(zip(p[:-1], p[1:]))


def _same_state(a, b):
    """value state, tangent state and gradient of two TangentStates, bit for bit"""
    return (all(torch.equal(getattr(a.value, nm), getattr(b.value, nm)) for nm in a.value.FIELDS)
            and all(torch.equal(a.tangent[nm], b.tangent[nm]) for nm in VALUES) and torch.equal(a.grad, b.grad))


def _chunked(eng, direction, pr, pe, w, cuts, drop_tangent_at=None):
    """The rows in chunks, end -> start carried; returns (grad, tangent series, status, end)."""
    from lgar_py_amd.engine import TangentState
    end, series = None, []
    for lo, hi in cuts:
        if lo == drop_tangent_at:
            end = TangentState(end.value, {nm: torch.zeros_like(t) for nm, t in end.tangent.items()}, end.grad)
        grad, ser, st, end = eng.tangent_window(direction, pr[lo:hi], pe[lo:hi], w_runoff=w[lo:hi], w_perc=w[lo:hi], start=end,
                                                want_series=True)
        series.append(ser)
    return grad, torch.cat(series), st, end


# 1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype, mode, rows", [(torch.float64, 1, None), (torch.float64, 0, 60), (torch.float64, 2, None),
                                               (torch.float32, 1, None)], ids=["f64_fast", "f64_literal", "f64_chain", "f32"])
def test_fresh_window_is_the_existing_tangent_bit_for_bit(dtype, mode, rows):
    eng = _engine("grad_synth0_12h", 3, dtype=dtype, search_mode=mode)
    pr, pe, w = _job("grad_synth0_12h", rows=rows)
    moved = 0.0
    for d in _directions(3, 3):
        want = eng.tangent(d, pr, pe, w_runoff=w, w_perc=w, want_series=True)
        got = eng.tangent_window(d, pr, pe, w_runoff=w, w_perc=w, want_series=True, keep_state=False)
        assert got[3] is None and all(torch.equal(a, b) for a, b in zip(want, got[:3])), d
        kept = eng.tangent_window(d, pr, pe, w_runoff=w, w_perc=w, want_series=True)  # storing the end state changes nothing
        assert all(torch.equal(a, b) for a, b in zip(want, kept[:3])), d
        moved += float(want[0].abs().sum())
    assert moved > 0.0


# 2 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, dtype, mode, middle", [("grad_synth0_12h", torch.float64, 1, None), ("grad_synth0_12h", torch.float32, 1, None),
                                                       ("grad_synth0_12h", torch.float64, 0, None), ("grad_manyfronts_60", torch.float64, 2, 45)],
                         ids=["synth0_f64", "synth0_f32", "synth0_literal", "manyfronts_chain"])
def test_chunked_windows_are_one_call_bit_for_bit(name, dtype, mode, middle):
    """grad_manyfronts_60 with the capacity chain forced: the fixture holds more than 8 fronts at the cuts at rows 45 and 59 (the
    chunks that start there are handed over at load) and passes 8 inside the chunk (8, 45) (handed over inside a chunk): both
    resume from the chunk's own state_in."""
    g = G.load(name)
    eng = _engine(name, 3, dtype=dtype, search_mode=mode)
    pr, pe, w = _job(name)
    T = pr.shape[0]
    cuts = _cuts(T, middle)
    if middle is not None:
        nf = g["nfronts"]  # (fronts after each row)
        assert nf[middle - 1] > _capi.CAP_SMALL and nf[T - 2] > _capi.CAP_SMALL and nf[cuts[2][0] - 1] <= _capi.CAP_SMALL
    differs = False
    for d in _directions(3, 3):
        one = eng.tangent_window(d, pr, pe, w_runoff=w, w_perc=w, want_series=True)
        got = _chunked(eng, d, pr, pe, w, cuts)
        assert all(torch.equal(a, b) for a, b in zip(one[:3], got[:3])), d
        assert int(one[2].abs().max()) == 0 and _same_state(one[3], got[3]), d
        assert int(one[3].value.n_fronts[0]) == g["nfronts"][-1]
        # sensitivity: with the tangent state dropped at the middle cut the gradient is another one (else dstate_in is ignored)
        dropped = _chunked(eng, d, pr, pe, w, cuts, drop_tangent_at=cuts[3][0])
        assert torch.equal(dropped[3].value.depth, one[3].value.depth)  # (the values do not depend on the tangents)
        differs |= not torch.equal(dropped[0], one[0])
        if "ksat" in d and d["ksat"][0, 0] == 1.0:
            assert not torch.equal(dropped[0], one[0])
    assert differs


# 3 ---------------------------------------------------------------------------------------------------------------------
def test_null_pointers_are_zeros_and_an_empty_window_copies_through():
    from lgar_py_amd.engine import TangentState
    eng = _engine("grad_synth0_12h", 3)
    pr, pe, w = _job("grad_synth0_12h")
    d = {"ksat": np.eye(3)[:, :1].repeat(3, 1)}
    _, _, _, mid = eng.tangent_window(d, pr[:8], pe[:8], w_runoff=w[:8])  # (the runoff's tangent first moves in row 6)
    zeros = TangentState(mid.value, {nm: torch.zeros_like(t) for nm, t in mid.tangent.items()}, torch.zeros_like(mid.grad))
    a = eng.tangent_window(d, pr[8:], pe[8:], w_runoff=w[8:], start=mid.value, want_series=True)  # dstate_in = grad_in = NULL
    b = eng.tangent_window(d, pr[8:], pe[8:], w_runoff=w[8:], start=zeros, want_series=True)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and _same_state(a[3], b[3]) and float(a[0].abs().sum()) > 0.0
    # n_steps = 0: state, tangent state and grad come out as they went in
    g0, ser, st, end = eng.tangent_window(d, pr[:0], pe[:0], start=mid, want_series=True)
    assert tuple(ser.shape) == (0, 3) and int(st.abs().max()) == 0 and _same_state(end, mid) and torch.equal(g0, mid.grad)
    assert float(mid.grad.abs().sum()) > 0.0 and float(mid.tangent["theta"].abs().sum()) > 0.0


# 4 ---------------------------------------------------------------------------------------------------------------------
SPIN, N4 = 60, 64
KW4 = dict(dt_h=300.0 / 3600.0, ponded_depth_max=0.0, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def _spun_up():
    """64 perturbed columns under the scaled synth_1 storm, spun up 60 rows: (soil, precip, pet, weights, engine, snapshot)."""
    import window_host
    Pn = W.perturbed_columns(N4, seed=11)
    sc = W.forcing_scale(N4, 0.5, 1.0, seed=12)
    pr = W.synth1_forcing()[:, 0:1] * sc[None, :]
    pe = np.zeros_like(pr)
    w = np.repeat(np.linspace(0.5, 1.5, pr.shape[0])[:, None], N4, 1)
    eng = window_host.WindowSimEngine(*[Pn[k] for k in PARAMS], **KW4)
    eng.forward(pr[:SPIN], pe[:SPIN], series=())
    return Pn, pr, pe, w, eng, eng.snapshot()


def test_stop_gradient_window_is_the_derivative_of_the_forward_from_that_state():
    """test_gpu_autograd.py::test_tangent_matches_finite_differences over a window that starts from a snapshot: its workload,
    directions, step sizes and bars (bulk bars, for the reason stated there: line-search offsets are constants).  26 of the 64
    columns produce runoff in the window; on the 23 with a non-zero difference quotient the median relative error is 1.3e-2 --
    the figure the existing fresh tangent over all 144 rows gives on the same columns."""
    import window_host
    Pn, pr, pe, w, base, snap = _spun_up()
    prw, pew, ww = pr[SPIN:], pe[SPIN:], torch.tensor(w[SPIN:])
    assert prw.shape[0] == 84

    def J(P):
        e = window_host.WindowSimEngine(*[P[k] for k in PARAMS], **KW4)
        e.restore(snap)
        r = e.forward(prw, pew, series=("runoff",))["runoff"]
        return (ww * r).sum(0).numpy(), e.status.numpy()

    _, st0 = J(Pn)
    checked = 0
    for kind, l, h in (("alpha", 0, 1e-7), ("n", 0, 1e-6), ("ksat", 0, 1e-6), ("ksat", 1, 1e-6), ("n", 1, 1e-6)):
        d = torch.zeros(3, N4, dtype=torch.float64)
        d[l] = 1.0
        g, _, st, end = base.tangent_window({kind: d}, prw, pew, w_runoff=ww, start=snap, keep_state=False)
        assert end is None
        fresh, _, _ = base.tangent({kind: d}, prw, pew, w_runoff=ww)
        assert not torch.equal(fresh, g)  # another run altogether: the same rows from set_internal_states
        Pp = {k: v.copy() for k, v in Pn.items()}
        Pm = {k: v.copy() for k, v in Pn.items()}
        Pp[kind][l] += h * Pn[kind][l]
        Pm[kind][l] -= h * Pn[kind][l]
        jp, sp = J(Pp)
        jm, sm = J(Pm)
        fd = (jp - jm) / (2 * h * Pn[kind][l])
        got = g.numpy()
        ok = (st0 == 0) & (sp == 0) & (sm == 0) & (st.numpy() == 0)
        rel = np.abs(got - fd)[ok] / np.maximum(np.abs(fd[ok]), 1e-3 * np.abs(fd[ok]).max() + 1e-12)
        print(kind, l, "median", np.median(rel), "within 1e-2", (rel <= 1e-2).mean(), "columns", int(ok.sum()))
        assert np.median(rel) <= 1e-4, (kind, l, np.median(rel))
        assert (rel <= 1e-2).mean() >= 0.5, (kind, l, (rel <= 1e-2).mean())
        checked += int(ok.sum())
    assert checked > 100


# 5 ---------------------------------------------------------------------------------------------------------------------
def test_lgar_series_from_an_initial_state(monkeypatch):
    import lgar_py_amd.autograd as A
    import window_host
    monkeypatch.setattr(A, "LgarEngine", window_host.WindowSimEngine)
    Pn, pr, pe, w, _, snap = _spun_up()
    prw, pew = torch.tensor(pr[SPIN:]), torch.tensor(pe[SPIN:])
    ww = torch.tensor(w[SPIN:]).clone()
    ww[:, 5:] = 0.0  # the loss sees five columns
    P = {k: torch.tensor(Pn[k]) for k in PARAMS}
    for k in KINDS:
        P[k].requires_grad_(True)
    args = [P[k] for k in PARAMS]
    ends = []
    # (a few of the perturbed columns leave the reference's domain of validity in the storm: check=False, they get no gradient)
    runoff, perc = A.lgar_series(*args, prw, pew, initial_state=snap, state_out=ends, check=False, **KW4)
    eng = window_host.WindowSimEngine(*[Pn[k] for k in PARAMS], **KW4)
    eng.restore(snap)
    want = eng.forward(prw, pew)
    ok = eng.status == 0
    assert bool(ok[:5].all()) and 0 < int((~ok).sum()) < 8
    assert torch.equal(runoff.detach(), want["runoff"]) and torch.equal(perc.detach(), want["percolation"])
    assert len(ends) == 1 and all(torch.equal(getattr(ends[0], nm), getattr(eng, nm)) for nm in ends[0].FIELDS)
    (ww * runoff).sum().backward()
    wanted = [(kind, l) for kind in KINDS for l in range(3)]
    vj, st = A.parameter_vjp(eng, prw, pew, ww, torch.zeros_like(ww), wanted, check=False, start=snap)
    assert int(st[ok].abs().max()) == 0
    for kind in KINDS:
        got = P[kind].grad
        assert torch.equal(got[:, ok], torch.stack([vj[(kind, l)] for l in range(3)])[:, ok]), kind
        assert float(got[:, 5:].abs().max()) == 0.0 and float(got[:, :5].abs().max()) > 0.0
    # state_out chains a second window: two windows are the uncut run
    with torch.no_grad():
        ends = []
        first, _ = A.lgar_series(*args, prw[:40], pew[:40], initial_state=snap, state_out=ends, check=False, **KW4)
        second, _ = A.lgar_series(*args, prw[40:], pew[40:], initial_state=ends[0], check=False, **KW4)
    assert torch.equal(torch.cat([first, second])[:, ok], want["runoff"][:, ok])
    # initial_state=None is the function as it was: a run from a fresh state, the gradient of the fresh tangent
    Q = {k: torch.tensor(Pn[k]) for k in PARAMS}
    for k in KINDS:
        Q[k].requires_grad_(True)
    r0, _ = A.lgar_series(*[Q[k] for k in PARAMS], prw, pew, initial_state=None, check=False, **KW4)
    fresh = window_host.WindowSimEngine(*[Pn[k] for k in PARAMS], **KW4)
    r0_want = fresh.forward(prw, pew)["runoff"]
    ok0 = fresh.status == 0
    assert bool(ok0[:5].all()) and torch.equal(r0.detach()[:, ok0], r0_want[:, ok0]) and not torch.equal(r0.detach()[:, :5], want["runoff"][:, :5])
    (ww * r0).sum().backward()
    vj0, _ = A.parameter_vjp(fresh, prw, pew, ww, torch.zeros_like(ww), wanted, check=False)
    for kind in KINDS:
        assert torch.equal(Q[kind].grad[:, ok0], torch.stack([vj0[(kind, l)] for l in range(3)])[:, ok0]), kind


# 6 ---------------------------------------------------------------------------------------------------------------------
def test_raw_entry_point_refuses_what_the_header_says():
    import window_host
    lib = window_host.library(3)
    N, L, T, F = 2, 3, 2, 8
    g = G.load("grad_synth0_12h")
    keep = []

    def arr(shape, dtype=np.float64, fill=0.0):
        a = np.full(shape, fill, dtype=dtype)
        keep.append(a)
        return a.ctypes.data

    def state(values_only=False):
        return _capi.LgarState(*[arr((F, N)) for _ in range(5)], None if values_only else arr((F, N), np.uint8),
                               None if values_only else arr(N, np.int32), arr((_capi.NSCAL, N)), None, None)

    dims = _capi.make_dims(n_columns=N, n_layers=L, front_slots=F, **{k: v for k, v in G.engine_keywords(g).items()})
    dims.n_steps = T
    soil = [np.ascontiguousarray(np.repeat(g[k][:, None], N, 1)) for k in PARAMS]
    par = _capi.LgarParams(*[a.ctypes.data for a in soil])
    direction = _capi.LgarParams(None, None, arr((L, N), fill=1.0), None, None, None)
    forcing = _capi.LgarForcing(arr((T, N)), arr((T, N)), None)
    grad, status = arr(N), arr(N, np.int32)
    status_words = keep[-1]
    si, di, so, do = state(), state(True), state(), state(True)

    def call(window, dims=dims, par=par, direction=direction, forcing=forcing, grad=grad, status=status, dtype=_capi.F64):
        ref = lambda x: None if x is None else C.byref(x)
        return lib.winhost_forward_tangent_window(ref(dims), ref(par), ref(direction), ref(forcing), None, None, ref(window), grad,
                                                  None, status, dtype)

    win = lambda a=None, b=None, c=None, d=None, gin=None: _capi.LgarTangentWindow(*[None if s is None else C.addressof(s) for s in (a, b, c, d)], gin)
    assert call(win()) == 0 and call(win(None, None, so, do)) == 0  # fresh, with and without an end state
    # (si is all zeros: no fronts, LGAR_ST_STRUCT for every column, and still a well-formed call)
    assert call(win(si, di, so, do, grad)) == 0 and status_words.tolist() == [_capi.ST_STRUCT] * N
    E = -1
    assert call(None) == E                                   # a null window
    assert call(win(None, di)) == E                          # dstate_in without state_in
    assert call(win(si, di, so, None)) == E and call(win(si, di, None, do)) == E  # exactly one of state_out / dstate_out
    for field in ("depth", "theta", "psi", "k", "dzdt", "scalars", "flags", "n_fronts"):
        for which in ("si", "di", "so", "do"):
            if field in ("flags", "n_fronts") and which in ("di", "do"):
                continue  # (ignored there)
            s = {"si": state(), "di": state(True), "so": state(), "do": state(True)}
            setattr(s[which], field, None)
            assert call(win(s["si"], s["di"], s["so"], s["do"])) == E, (which, field)
    assert call(win(si, di, si, do)) == E and call(win(si, di, so, di)) == E  # an output state over the input's arrays
    shared = state()
    shared.theta = si.theta
    assert call(win(si, di, shared, do)) == E
    # ... and everything lgar_forward_tangent refuses
    assert call(win(), dims=None) == E and call(win(), par=None) == E and call(win(), direction=None) == E
    assert call(win(), forcing=None) == E and call(win(), grad=None) == E and call(win(), status=None) == E
    assert call(win(), forcing=_capi.LgarForcing(None, forcing.pet, None)) == E and call(win(), dtype=7) == E
    bad = _capi.make_dims(n_columns=N, n_layers=L, front_slots=F)
    bad.n_steps, bad.tangent_share = T, 3
    assert call(win(), dims=bad) == E


def test_restore_and_tangent_window_refuse_a_state_that_is_not_this_engines():
    from lgar_py_amd import EngineState, LgarError
    eng = _engine("grad_synth0_12h", 3)
    pr, pe, w = _job("grad_synth0_12h")
    snap = eng.snapshot()
    assert isinstance(snap, EngineState) and snap.depth is not eng.depth and torch.equal(snap.depth, eng.depth)
    eng.forward(pr, pe)
    assert not torch.equal(snap.theta, eng.theta)  # a clone: the run did not move it
    eng.restore(snap)
    assert all(torch.equal(getattr(snap, nm), getattr(eng, nm)) for nm in snap.FIELDS)
    other = {"N": _engine("grad_synth0_12h", 4).snapshot(), "front_slots": _engine("grad_synth0_12h", 3, front_slots=12).snapshot(),
             "dtype": _engine("grad_synth0_12h", 3, dtype=torch.float32).snapshot(),
             "device": EngineState(**{nm: torch.empty_like(getattr(snap, nm), device="meta") for nm in snap.FIELDS})}
    message = {"N": "holds 4 columns, this engine has 3", "front_slots": "has front_slots = 12, this engine 32",
               "dtype": "is torch.float32, this engine torch.float64", "device": "is on meta, this engine on cpu"}
    d = {"n": np.ones((3, 3))}
    for what, bad in other.items():
        with pytest.raises(LgarError, match="the snapshot " + message[what]):
            eng.restore(bad)
        with pytest.raises(LgarError, match="start " + message[what]):
            eng.tangent_window(d, pr, pe, w_runoff=w, start=bad)
    with pytest.raises(LgarError, match="must be an EngineState"):
        eng.restore({"depth": snap.depth})
    with pytest.raises(LgarError, match="with_state=False"):
        eng.like(*[getattr(eng, k) for k in PARAMS], with_state=False).snapshot()


# 7 ---------------------------------------------------------------------------------------------------------------------
def test_stand_alone_program_runs_clean_under_the_sanitizers():
    """window_host_main.cpp: case 2's shape in double and single precision, with and without the capacity chain, under
    AddressSanitizer + UBSan (host code in a program of its own)."""
    import window_host
    assert _hostbuild.run_clean([window_host.program(sanitize=True)]).strip() == "ok"
