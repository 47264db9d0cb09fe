"""TEST INFRASTRUCTURE ONLY: what the tangent with a forcing direction (lgar_forward_tangent_forced, LgarEngine.tangent /
tangent_window with d_precip / d_pet) owes its oracles, as functions of an engine factory `make(g, N, **kw)` and a device -- the
simulator's suite (test_forcing_tangent_host.py, tests/forced_host) and the GPU's (test_gpu_forcing_tangent.py) run the same
bodies.  The oracles: the reference's own x.grad (tests/golden/forcing_grad, make_forcing_grad_golden.py), the window family bit
for bit, and a lane's own single-direction launch."""
import ctypes as C
import os

import numpy as np
import torch

import _golden as G
from conftest import GOLDEN
from lgar_py_amd import _capi

PARAMS = ("alpha", "n", "ksat", "theta_e", "theta_r", "thickness")
KINDS = ("alpha", "n", "ksat")
VALUES = ("depth", "theta", "psi", "k", "dzdt", "scalars")
CASES = ("grad_synth0_12h", "grad_synth1_phil", "grad_manyfronts_60", "grad_two_layer_phil_150", "grad_six_layer_synth1")
GROUPS = (1, 2, 9, 11)


def load_gradx(name):
    """(the gradient fixture of make_golden.py, the reference's x.grad [T, 2] for its loss) -- the same run, by its forcing"""
    g, x = G.load(name), np.load(os.path.join(GOLDEN, "forcing_grad", "gradx_" + name + ".npz"))
    assert np.array_equal(g["forcing"], x["forcing"]) and float(g["loss"]) == float(x["loss"])
    return g, x["grad_x"]


def same_state(a, b):
    """value state, tangent state and gradient of two TangentStates, bit for bit"""
    return (all(torch.equal(getattr(a.value, nm), getattr(b.value, nm)) for nm in a.value.FIELDS)
            and all(torch.equal(a.tangent[nm], b.tangent[nm]) for nm in VALUES) and torch.equal(a.grad, b.grad))


def same_call(a, b):
    """(grad, series, status[, end]) of two tangent calls, bit for bit"""
    return all(torch.equal(x, y) for x, y in zip(a[:3], b[:3])) and (len(a) < 4 or a[3] is None or same_state(a[3], b[3]))


def cuts(T, middle=None):
    """The cuts of test_tangent_window_host._cuts: (0, 1), (1, 8), (8, T / 2), (T / 2, T - 1), (T - 1, T) scaled to T."""
    second = 8 if T // 2 > 8 else max(2, T // 4)
    p = [0, 1, second, T // 2 if middle is None else middle, T - 1, T]
    assert p == sorted(set(p))
    return list(zip(p[:-1], p[1:]))


# ---- reference parity -------------------------------------------------------------------------------------------------
def reference_parity(make, dev, name, mode, mixed=False):
    """One column of the fixture in 2 T lanes of ONE launch: lane t carries the direction "precipitation of row t" (one-hot in
    time), lane T + t "PET of row t".  Weights 2 runoff / T, the gradient of loss = mean(runoff^2) as
    test_gradients_match_reference_autograd forms it, so grad[t] is d loss / d precip[t] and grad[T + t] d loss / d pet[t]:
    the reference's x.grad[t, 0] and x.grad[t, 1], each within 1e-6 of max |x.grad| (the bar of the gradient fixtures,
    _golden.GRADIENT).  Returns the two worst errors as fractions of that bar."""
    g, gx = load_gradx(name)
    T = gx.shape[0]
    N = 2 * T
    eng = make(g, N, search_mode=mode, **(dict(geff_mode=1) if mixed else {}))
    pr, pe = G.replicated_forcing(g, N, device=dev)
    r = eng.forward(pr, pe, series=("runoff",))["runoff"]
    assert mixed or abs(float(torch.mean(r[:, 0] ** 2)) - float(g["loss"])) <= G.GRADIENT_LOSS * float(g["loss"])
    w = (2.0 * r / T).contiguous()
    dp = torch.zeros(T, N, dtype=torch.float64, device=dev)
    de = torch.zeros(T, N, dtype=torch.float64, device=dev)
    dp[torch.arange(T), torch.arange(T)] = 1.0
    de[torch.arange(T), T + torch.arange(T)] = 1.0
    grad, _, st = eng.tangent({}, pr, pe, w_runoff=w, d_precip=dp, d_pet=de)
    assert int(st.abs().max()) == 0  # (no fault, and no lane left with LGAR_ST_RESUME)
    if mode == 2 and name == "grad_manyfronts_60":
        # the capacity chain was asked for and the column outgrows the first kernel: every lane was handed over
        assert int(g["nfronts"].max()) > _capi.CAP_SMALL and int(g["nfronts"][0]) <= _capi.CAP_SMALL
        if dev != "cpu":  # the first kernel's count of the columns it handed over (the host build walks the chain without counters)
            assert int(eng._last_tickets[4]) == N, eng._last_tickets
    got = grad.cpu().numpy().reshape(2, T).T
    bar = G.GRADIENT * np.abs(gx).max()
    err = np.abs(got - gx).max(0) / bar
    print("%s mode %d%s: |got - x.grad| / bar  precip %.3e  pet %.3e   (max |x.grad| %.4g / %.4g)"
          % (name, mode, " mixed" if mixed else "", err[0], err[1], np.abs(gx[:, 0]).max(), np.abs(gx[:, 1]).max()))
    G._within("d loss / d precip[t] against the reference's x.grad[t, 0]", np.abs(got[:, 0] - gx[:, 0]), bar)
    G._within("d loss / d pet[t] against the reference's x.grad[t, 1]", np.abs(got[:, 1] - gx[:, 1]), bar)
    return err


# ---- a small job of its own: three columns, two storms ----------------------------------------------------------------------
def storm_job(dev, N=3, T=24, dtype=torch.float64):
    """tests/window_host/window_host_main.cpp's job: the Phillipsburg soil under two storms with PET between them, the rain of
    column c scaled by (1, 0.5, 1.3)[c % 3]; ramp weights.  Returns (fixture for the engine keywords, precip, pet, w)."""
    t = np.arange(T)
    rain = ((t >= 2) & (t < 7)) | ((t >= 13) & (t < 16))
    scale = np.array([1.0, 0.5, 1.3])[np.arange(N) % 3]
    pr = np.where(rain[:, None], 2.0 * scale[None, :], 0.0)
    pe = np.where(rain[:, None], 0.0, 0.02) * np.ones((1, N))
    w = np.repeat((0.5 + t / (T - 1.0))[:, None], N, 1)
    to = lambda a: torch.tensor(a, dtype=dtype, device=dev).contiguous()
    return G.load("grad_synth0_12h"), to(pr), to(pe), to(w)


def forcing_directions_of(pr, pe, seed=5):
    """Two forcing tangents [T, N] that move every row: a multiplier on the rain plus a little noise, and one on the PET."""
    rng = np.random.default_rng(seed)
    noise = torch.tensor(rng.random(tuple(pr.shape)) - 0.5, dtype=pr.dtype, device=pr.device)
    return (pr * (1.0 + 0.25 * noise)).contiguous(), (pe * (1.0 - 0.25 * noise)).contiguous()


def null_call(eng, direction, pr, pe, w):
    """lgar_forward_tangent_forced with BOTH tangents NULL and a window of NULLs: (grad, series, status), by the engine's own
    argument blocks (LgarEngine.tangent_window sends such a call to lgar_forward_tangent_window instead)."""
    inputs = eng._tangent_inputs(direction, pr, pe, w, w, 1, 0, None)
    win = _capi.LgarTangentWindow(None, None, None, None, None)
    return eng._tangent_call("forward_tangent_window", inputs, None, True, (C.byref(win),), d_forcing=(None, None))


def null_tangents(make, dev, dtype, mode):
    """With both tangents NULL, one NULL and the other all zero, or both all zero: grad, series, status and both end states have
    the bits of tangent_window (and a non-zero tangent moves the gradient: the arrays are read)."""
    g, pr, pe, w = storm_job(dev, dtype=dtype)
    eng = make(g, 3, dtype=dtype, search_mode=mode)
    zero = torch.zeros_like(pr)
    moved = False
    for kind in KINDS:
        d = {kind: torch.ones(3, 3, dtype=dtype, device=dev)}
        want = eng.tangent_window(d, pr, pe, w_runoff=w, w_perc=w, want_series=True)
        assert int(want[2].abs().max()) == 0 and float(want[0].abs().sum()) > 0.0
        for dp, de in ((zero, None), (None, zero), (zero, zero)):
            got = eng.tangent_window(d, pr, pe, w_runoff=w, w_perc=w, want_series=True, d_precip=dp, d_pet=de)
            assert same_call(want, got), (kind, dp is None, de is None)
            assert all(torch.equal(a, b) for a, b in zip(want[:3], eng.tangent(d, pr, pe, w_runoff=w, w_perc=w, want_series=True,
                                                                               d_precip=dp, d_pet=de)))
        assert all(torch.equal(a, b) for a, b in zip(want[:3], null_call(eng, d, pr, pe, w)))
        other = eng.tangent_window(d, pr, pe, w_runoff=w, w_perc=w, want_series=True, d_precip=pr, d_pet=zero)
        assert torch.equal(other[3].value.depth, want[3].value.depth)  # (a forcing direction changes no value)
        moved |= not torch.equal(other[0], want[0])
    assert moved


def chunked_windows(make, dev, name, dtype, mode, middle=None):
    """Parameter and forcing direction together over the fixture's rows: the cuts leave the bits of one call."""
    g = G.load(name)
    eng = make(g, 3, dtype=dtype, search_mode=mode)
    pr, pe = (t.to(dtype) for t in G.replicated_forcing(g, 3, device=dev))
    T = pr.shape[0]
    w = torch.linspace(0.5, 1.5, T, dtype=dtype, device=dev)[:, None].expand(T, 3).contiguous()
    dp, de = forcing_directions_of(pr, pe + 0.01)
    d = {"ksat": torch.ones(eng.L, 3, dtype=dtype, device=dev)}
    one = eng.tangent_window(d, pr, pe, w_runoff=w, w_perc=w, want_series=True, d_precip=dp, d_pet=de)
    plain = eng.tangent_window(d, pr, pe, w_runoff=w, w_perc=w, want_series=True)
    assert int(one[2].abs().max()) == 0 and not torch.equal(one[0], plain[0])
    end, series = None, []
    for lo, hi in cuts(T, middle):
        grad, ser, st, end = eng.tangent_window(d, pr[lo:hi], pe[lo:hi], w_runoff=w[lo:hi], w_perc=w[lo:hi], start=end,
                                                want_series=True, d_precip=dp[lo:hi], d_pet=de[lo:hi])
        series.append(ser)
    assert same_call(one, (grad, torch.cat(series), st, end))


# ---- layouts ----------------------------------------------------------------------------------------------------------
N_CELLS, N_SOIL = 3, 24
CELL_OF = np.array([0] * 11 + [1] * 4 + [2] * 9)  # unequal cells


def _lane_directions(group, L):
    """What the lanes of a direction group carry: parameter directions (kind, layer) first, then "precip" and "pet" -- 1: precip;
    2: ksat of layer 0 and precip; 9: seven parameter directions and both; 11: all nine and both."""
    par = [(kind, l) for kind in KINDS for l in range(L)]
    return {1: ["precip"], 2: [par[6], "precip"], 9: par[:7] + ["precip", "pet"], 11: par + ["precip", "pet"]}[group]


def layouts(make, dev, group, share):
    """24 soil columns in 3 cells of 11, 4 and 9 columns that read [T, 3] forcing through a ForcingMap, each column in `group`
    adjacent lanes, parameter and forcing directions mixed in one group.  share = 0: every lane equals its own single-direction
    launch over the 24 columns bit for bit.  share = group (the lanes of a group share the trapezoid): every lane within 1e-6 of
    the column's largest gradient, the bar of test_gpu_autograd.py for the shared launch."""
    from lgar_py_amd import workloads as W
    from lgar_py_amd.forcing import ForcingMap
    g, prc, pec, _ = storm_job(dev, N=N_CELLS)
    T, L = prc.shape[0], 3
    Pn = W.perturbed_columns(N_SOIL, frac=0.05, seed=31)
    kw = dict(G.engine_keywords(g), dtype=torch.float64)
    soil = {k: torch.tensor(Pn[k], device=dev) for k in PARAMS}
    fmap = ForcingMap(CELL_OF, N_CELLS, device=dev)
    rng = np.random.default_rng(7)
    w = torch.tensor(0.5 + rng.random((T, N_SOIL)), device=dev)  # one weight column per entry of the map
    dpc, dec = forcing_directions_of(prc, pec)                   # [T, B]: the forcing tangent of a cell
    lanes = _lane_directions(group, L)
    big = make(g, None, soil=[soil[k].repeat_interleave(group, dim=1) for k in PARAMS], with_state=False, **kw)
    dirs = {k: torch.zeros(L, N_SOIL * group, dtype=torch.float64, device=dev) for k in KINDS}
    dp = torch.zeros(T, N_CELLS, group, dtype=torch.float64, device=dev)
    de = torch.zeros(T, N_CELLS, group, dtype=torch.float64, device=dev)
    for j, what in enumerate(lanes):
        if what == "precip":
            dp[:, :, j] = dpc
        elif what == "pet":
            de[:, :, j] = dec
        else:
            dirs[what[0]][what[1], j::group] = 1.0
    got, _, st = big.tangent(dirs, prc, pec, w_runoff=w, w_perc=w, forcing_group=group, share=share, forcing_map=fmap,
                             d_precip=dp, d_pet=de)
    assert int(st.abs().max()) == 0
    got = got.reshape(N_SOIL, group)
    one = make(g, None, soil=[soil[k] for k in PARAMS], with_state=False, **kw)
    want = torch.zeros_like(got)
    for j, what in enumerate(lanes):
        d, f = {}, {}
        if what == "precip":
            f = dict(d_precip=dpc)
        elif what == "pet":
            f = dict(d_pet=dec)
        else:
            d = {what[0]: torch.zeros(L, N_SOIL, dtype=torch.float64, device=dev)}
            d[what[0]][what[1]] = 1.0
        want[:, j], _, st = one.tangent(d, prc, pec, w_runoff=w, w_perc=w, forcing_map=fmap, **f)
        assert int(st.abs().max()) == 0
    moves = want.abs().max(0).values > 0  # (a deep layer's parameters may move nothing in 24 rows; the forcing must)
    assert all(bool(moves[j]) for j, what in enumerate(lanes) if isinstance(what, str)) and int(moves.sum()) >= min(group, 8)
    if share == 0:
        assert torch.equal(got, want)
    else:
        scale = want.abs().max(1, keepdim=True).values  # (0 for a column that yields nothing: its lanes must be 0 too)
        live = scale[:, 0] > 0
        err = float(((got - want).abs()[live] / scale[live]).max())
        print("group %d shared: worst |shared - own launch| / column's largest gradient %.3e (%d of %d columns move)"
              % (group, err, int(live.sum()), N_SOIL))
        assert int(live.sum()) >= N_SOIL // 2 and bool(torch.isfinite(got).all())
        assert bool(((got - want).abs() <= 1e-6 * scale).all())
    return got


# ---- autograd: forcing_directions ------------------------------------------------------------------------------------------
def series_baseline(make, dev):
    """lgar_series WITHOUT forcing_directions on a gradient fixture: the parameter gradients are, bit for bit, the one-hot
    launches of LgarEngine.tangent -- kernels whose objects are the parent's (profiles/r18/objects_identical.txt) on the path the
    parent took -- and meet the reference's loss.backward() as before."""
    import lgar_py_amd.autograd as A
    g = G.load("grad_synth0_12h")
    N = 3
    pr, pe = G.replicated_forcing(g, N, device=dev)
    P = {k: torch.tensor(np.repeat(g[k][:, None], N, 1), device=dev) for k in PARAMS}
    for k in KINDS:
        P[k].requires_grad_(True)
    kw = dict(G.engine_keywords(g), dtype=torch.float64)
    runoff, _ = A.lgar_series(*[P[k] for k in PARAMS], pr, pe, **kw)
    runoff.retain_grad()
    loss = torch.mean(runoff[:, 0] ** 2)
    loss.backward()
    G.check_gradients(g, float(loss.detach()), {k: P[k].grad[:, 0].cpu().numpy() for k in KINDS})
    eng = make(g, N)
    w = runoff.grad.contiguous()  # the incoming gradient as autograd formed it
    for kind in KINDS:
        for l in range(3):
            d = torch.zeros(3, N, dtype=torch.float64, device=dev)
            d[l] = 1.0
            want, _, _ = eng.tangent({kind: d}, pr, pe, w_runoff=w)
            assert torch.equal(P[kind].grad[l], want), (kind, l)


def series_gradients(dev):
    """{kind: d mean(runoff[:, 0]^2) / d kind [L, 3]} of grad_synth0_12h through lgar_series without forcing_directions"""
    import lgar_py_amd.autograd as A
    g = G.load("grad_synth0_12h")
    pr, pe = G.replicated_forcing(g, 3, device=dev)
    P = {k: torch.tensor(np.repeat(g[k][:, None], 3, 1), device=dev) for k in PARAMS}
    for k in KINDS:
        P[k].requires_grad_(True)
    runoff, _ = A.lgar_series(*[P[k] for k in PARAMS], pr, pe, **dict(G.engine_keywords(g), dtype=torch.float64))
    torch.mean(runoff[:, 0] ** 2).backward()
    return {k: P[k].grad.cpu().numpy() for k in KINDS}


def series_parent_bits(dev):
    want = np.load(os.path.join(GOLDEN, "forcing_grad", "series_baseline_parent.npz"))
    got = series_gradients(dev)
    for k in KINDS:
        assert got[k].shape == want[k].shape and (got[k].view(np.uint64) == want[k].view(np.uint64)).all() and np.abs(want[k]).max() > 0, k


def series_scale_matches_reference(dev, name="grad_two_layer_phil_150"):
    """lg.scaled_forcing at scale 1 on the fixture that has PET and ponding, scalar multipliers: d loss / d scale_p is
    sum_t x.grad[t, 0] precip[t] and d loss / d scale_e is sum_t x.grad[t, 1] pet[t] of the reference.  Every term is held to the
    fixtures' bar, 1e-6 max |x.grad|, times its |forcing[t]|: the sums to 1e-6 max |x.grad| sum_t |forcing[t]|.  The soil
    gradients ride in the same launches and stay at their own bar."""
    import lgar_py_amd as lg
    import lgar_py_amd.autograd as A
    g, gx = load_gradx(name)
    N, L = 3, g["alpha"].shape[0]
    pr, pe = G.replicated_forcing(g, N, device=dev)
    sp = torch.tensor(1.0, dtype=torch.float64, device=dev, requires_grad=True)
    se = torch.tensor(1.0, dtype=torch.float64, device=dev, requires_grad=True)
    prs, pes, fd = lg.scaled_forcing(pr, pe, sp, se)
    assert torch.equal(prs, pr) and torch.equal(pes, pe) and not prs.requires_grad
    P = {k: torch.tensor(np.repeat(g[k][:, None], N, 1), device=dev) for k in PARAMS}
    for k in KINDS:
        P[k].requires_grad_(True)
    runoff, _ = A.lgar_series(*[P[k] for k in PARAMS], prs, pes, forcing_directions=fd, **dict(G.engine_keywords(g), dtype=torch.float64))
    loss = torch.mean(runoff[:, 0] ** 2)
    loss.backward()
    G.check_gradients(g, float(loss.detach()), {k: P[k].grad[:, 0].cpu().numpy() for k in KINDS})
    x = g["forcing"]
    for nm, got, j in (("scale_p", sp.grad, 0), ("scale_e", se.grad, 1)):
        want, bar = float((gx[:, j] * x[:, j]).sum()), G.GRADIENT * np.abs(gx).max() * float(np.abs(x[:, j]).sum())
        print("%s: d loss / d %s %.9g, the reference's %.9g, |difference| / bar %.3e" % (name, nm, float(got), want, abs(float(got) - want) / bar))
        assert got.shape == () and abs(float(got) - want) <= bar and want != 0.0, nm


def series_cells_two_ways(make, dev, shared_lanes=None, monkeypatch=None):
    """24 perturbed columns in 3 unequal cells read [T, 3] forcing through a ForcingMap; the loss is a weighted sum of the
    runoff.  d loss / d scale_p[b] and d loss / d scale_e[b] by lgar_series(forcing_directions=scaled_forcing's) against the other
    association: one lane per (cell's column, row t) with the one-hot forcing directions gives d loss / d precip[t, b] and
    d loss / d pet[t, b], contracted with precip and pet afterwards.  The same sums in another order: within 1e-6 of the largest
    entry (the project's bar for that).  A [B] parameter gets [B], a scalar the sum over the cells; with initial_state the same
    holds from a spun-up state; the soil gradients beside them equal the run without forcing_directions (bit for bit with every lane
    on its own)."""
    import lgar_py_amd as lg
    import lgar_py_amd.autograd as A
    from lgar_py_amd import workloads as W
    from lgar_py_amd.forcing import ForcingMap
    if shared_lanes is not None:
        monkeypatch.setattr(A, "SHARE_MIN_LANES", shared_lanes)
    g, prc, pec, _ = storm_job(dev, N=N_CELLS, T=17)
    prc = (prc * torch.tensor([1.0, 2.4, 1.0], dtype=torch.float64, device=dev)).contiguous()  # (every cell yields runoff)
    T = prc.shape[0]
    Pn = W.perturbed_columns(N_SOIL, frac=0.05, seed=31)
    kw = dict(G.engine_keywords(g), dtype=torch.float64)
    fmap = ForcingMap(CELL_OF, N_CELLS, device=dev)
    rng = np.random.default_rng(11)
    wl = torch.tensor(0.5 + rng.random((T, N_SOIL)), device=dev)
    worst = 0.0
    for spin in (0, 5):
        start = None
        if spin:
            e0 = make(g, None, soil=[torch.tensor(Pn[k], device=dev) for k in PARAMS], **kw)
            e0.forward(prc[:spin], pec[:spin], series=(), forcing_map=fmap)
            start = e0.snapshot()
        rows = slice(spin, T)
        res = {}
        for with_fd in (True, False):
            P = {k: torch.tensor(Pn[k], device=dev) for k in PARAMS}
            for k in KINDS:
                P[k].requires_grad_(True)
            sp = torch.ones(N_CELLS, dtype=torch.float64, device=dev, requires_grad=True)
            se = torch.tensor(1.0, dtype=torch.float64, device=dev, requires_grad=True)
            prs, pes, fd = lg.scaled_forcing(prc[rows], pec[rows], sp, se)
            runoff, _ = A.lgar_series(*[P[k] for k in PARAMS], prs, pes, forcing_map=fmap, initial_state=start,
                                      **dict(kw, **(dict(forcing_directions=fd) if with_fd else {})))
            (wl[rows] * runoff).sum().backward()
            res[with_fd] = (P, sp.grad, se.grad)
        P, gsp, gse = res[True]
        assert res[False][1] is None
        for k in KINDS:
            # own lanes: the same bits.  Lanes that share the trapezoid split its nodes among 11 lanes here and 9 there: the same
            # sums in another order, the shared launch's bar (1e-6 of the column's largest gradient, test_gpu_autograd.py)
            a, b = P[k].grad, res[False][0][k].grad
            if shared_lanes == 1:
                assert bool(((a - b).abs() <= 1e-6 * b.abs().max(0, keepdim=True).values).all()), k
            else:
                assert torch.equal(a, b), k
        assert tuple(gsp.shape) == (N_CELLS,) and gse.shape == () and bool(torch.isfinite(gsp).all())
        # the other association: d loss / d forcing[t, b], one launch of one-hot lanes per cell's columns
        Tw = T - spin
        eng = make(g, None, soil=[torch.tensor(Pn[k], device=dev).repeat_interleave(2 * Tw, dim=1) for k in PARAMS], with_state=False, **kw)
        dp = torch.zeros(Tw, N_CELLS, 2 * Tw, dtype=torch.float64, device=dev)
        de = torch.zeros(Tw, N_CELLS, 2 * Tw, dtype=torch.float64, device=dev)
        dp[torch.arange(Tw), :, torch.arange(Tw)] = 1.0
        de[torch.arange(Tw), :, Tw + torch.arange(Tw)] = 1.0
        st = None if start is None else start.expand(2 * Tw)
        gl, _, status, _ = eng.tangent_window({}, prc[rows], pec[rows], w_runoff=wl[rows].contiguous(), start=st, keep_state=False,
                                              forcing_group=2 * Tw, forcing_map=fmap, d_precip=dp, d_pet=de)
        assert int(status.abs().max()) == 0
        gl = gl.reshape(N_SOIL, 2, Tw)  # [column, precip | pet, row]
        cell = torch.tensor(CELL_OF, device=dev)
        gcell = torch.zeros(N_CELLS, 2, Tw, dtype=torch.float64, device=dev).index_add_(0, cell, gl)  # d loss / d forcing[t, b]
        want_p = (gcell[:, 0] * prc[rows].T).sum(1)
        want_e = (gcell[:, 1] * pec[rows].T).sum()
        scale = float(torch.cat([want_p.abs(), want_e.abs()[None]]).max())
        gap = max(float((gsp - want_p).abs().max()), abs(float(gse - want_e))) / scale
        print("spin %d: d loss / d scale_p %s, d loss / d scale_e %.6g; two associations differ by %.3e of the largest entry"
              % (spin, gsp.cpu().numpy(), float(gse), gap))
        assert scale > 0.0 and float(gsp.abs().min()) > 0.0 and float(gse) != 0.0 and gap <= 1e-6
        worst = max(worst, gap)
    return worst


def snow_chain_two_ways(make, dev, snow_class, snow_function):
    """Section 19's shape: 24 columns in 3 cells (11, 4, 9 columns), T = 17 rows of dt_h = 1/8 h, cell 1 cold (a pack of 3 cm, the
    air around the melt threshold), cells 0 and 2 warm (no pack: water = precip).  water = snow(scale_p precip, temp), the columns
    run on (water, scale_e pet) through a ForcingMap, the loss is a weighted sum of catchment_sum(runoff).  The gradients to cfmax,
    tm, sfcf ([B] each), scale_p ([B]) and scale_e (a scalar), two ways:
      directly: ONE lgar_catchment_snow_tangent launch gives d water along the three parameters and along dp = precip, they go
      into a ForcingDirections beside scale_e's d_pet, and lgar_series(forcing_directions=) returns the five gradients;
      by the other association: 2 x 17 one-hot time lanes per column give d loss / d water[t, b] and d loss / d pet[t, b];
      d loss / d water goes as gw into the existing adjoint (catchment_snow's backward), which returns the parameters' gradients
      and gp, contracted with precip.
    The same sums in another order: each gradient within 1e-6 of its largest entry.  Every gradient of the cold cell is finite and
    non-zero; the warm cells' scale_p gradient equals the run with scaled_forcing alone in bits (there the tangent of the snowpack
    along dp = precip IS precip: dt_h is a power of two).  Returns the measured gaps."""
    import lgar_py_amd as lg
    import lgar_py_amd.autograd as A
    from lgar_py_amd import workloads as W
    from lgar_py_amd.catchments import catchment_sum
    from lgar_py_amd.forcing import ForcingDirections, ForcingMap
    T, dt = 17, 0.125
    t = np.arange(T)
    rain = ((t >= 2) & (t < 5)) | ((t >= 8) & (t < 14))
    precip = torch.tensor(np.where(rain[:, None], np.array([9.0, 6.0, 11.0])[None, :], 0.0), device=dev)
    pet = torch.tensor(np.where((t >= 5) & (t < 8), 0.0, 0.3)[:, None] * np.ones((1, N_CELLS)), device=dev)  # a rain pause with PET
    temp = torch.tensor(np.stack([np.full(T, 10.0), 1.2 + 1.5 * np.sin(0.7 * t), np.full(T, 12.0)], axis=1), device=dev)
    state = torch.tensor([[0.0, 3.0, 0.0], [0.0, 0.05, 0.0]], dtype=torch.float64, device=dev)
    names = ("tlo", "thi", "tm", "sfcf", "cfmax", "cfr", "cwh")
    values = dict(tlo=-1.0, thi=2.0, tm=0.4, sfcf=1.1, cfmax=0.9, cfr=0.05, cwh=0.1)
    Pn = W.perturbed_columns(N_SOIL, frac=0.05, seed=31)
    kw = dict(G.engine_keywords(G.load("grad_synth0_12h")), dtype=torch.float64, dt_h=dt)
    cmap = A.CatchmentMap(CELL_OF, n_catchments=N_CELLS, device=dev)
    fmap = ForcingMap(CELL_OF, N_CELLS, device=dev)
    wl = torch.tensor(0.5 + np.random.default_rng(13).random((T, N_CELLS)), device=dev)
    soil = [torch.tensor(Pn[k], device=dev) for k in PARAMS]
    leaf = lambda v: torch.full((N_CELLS,), v, dtype=torch.float64, device=dev, requires_grad=True)

    def loss_of(water, pes, fd):
        runoff, _ = A.lgar_series(*soil, water, pes, forcing_map=fmap, forcing_directions=fd, **kw)
        return (wl * catchment_sum(runoff, cmap)).sum()

    # directly
    par = {k: leaf(v) for k, v in values.items()}
    sp, se = leaf(1.0), torch.tensor(1.0, dtype=torch.float64, device=dev, requires_grad=True)
    snow = snow_class(*[par[k].detach() for k in names], dt, device=dev)
    ps = (precip * sp.detach()).contiguous()
    water = snow.run(ps, temp, carry=False, state=state)
    dpar = torch.zeros(4, 7, N_CELLS, dtype=torch.float64, device=dev)
    dp = torch.zeros(4, T, N_CELLS, dtype=torch.float64, device=dev)
    for k, nm in enumerate(("cfmax", "tm", "sfcf")):
        dpar[k, names.index(nm)] = 1.0
    dp[3] = precip
    dw = snow.tangent(ps, temp, 4, dp=dp, dpar=dpar, state=state)[0].permute(2, 0, 1)  # [4, T, B]
    zero = torch.zeros_like(precip)
    fd = ForcingDirections((par["cfmax"], par["tm"], par["sfcf"], sp, se), d_precip=torch.cat([dw, zero[None]]).contiguous(),
                           d_pet=torch.stack([zero, zero, zero, zero, pet]))
    loss_of(water, (pet * se.detach()).contiguous(), fd).backward()
    direct = dict(cfmax=par["cfmax"].grad, tm=par["tm"].grad, sfcf=par["sfcf"].grad, scale_p=sp.grad, scale_e=se.grad)
    # the other association
    eng = make(None, None, soil=[x.repeat_interleave(2 * T, dim=1) for x in soil], with_state=False, **kw)
    d1 = torch.zeros(T, N_CELLS, 2 * T, dtype=torch.float64, device=dev)
    d2 = torch.zeros(T, N_CELLS, 2 * T, dtype=torch.float64, device=dev)
    d1[torch.arange(T), :, torch.arange(T)] = 1.0
    d2[torch.arange(T), :, T + torch.arange(T)] = 1.0
    wcol = cmap.spread(wl, torch.float64)  # the loss's gradient at the runoff, [T, N]
    gl, _, status = eng.tangent({}, water, pet, w_runoff=wcol, forcing_group=2 * T, forcing_map=fmap, d_precip=d1, d_pet=d2)
    assert int(status.abs().max()) == 0
    gl = gl.reshape(N_SOIL, 2, T)
    gcell = torch.zeros(N_CELLS, 2, T, dtype=torch.float64, device=dev).index_add_(0, torch.tensor(CELL_OF, device=dev), gl)
    par2 = {k: leaf(v) for k, v in values.items()}
    ps2 = ps.clone().requires_grad_(True)
    w2 = snow_function(ps2, temp, *[par2[k] for k in names], dt, state=state)
    assert torch.equal(w2.detach(), water)
    w2.backward(gcell[:, 0].T.contiguous())
    other = dict(cfmax=par2["cfmax"].grad, tm=par2["tm"].grad, sfcf=par2["sfcf"].grad, scale_p=(ps2.grad * precip).sum(0),
                 scale_e=(gcell[:, 1] * pet.T).sum())
    gaps = {}
    for k in direct:
        a, b = direct[k], other[k]
        gaps[k] = float((a - b).abs().max() / b.abs().max())
        print("%-8s direct %s  other association %s  gap %.3e of the largest entry" % (k, a.detach().cpu().numpy(), b.detach().cpu().numpy(), gaps[k]))
        assert bool(torch.isfinite(a).all()) and gaps[k] <= 1e-6, k
        assert float(a.reshape(-1)[1 if a.dim() else 0].abs()) > 0.0, k  # the cold cell (scale_e: the scalar)
    # the warm cells: the snowpack is the identity there, and so is its tangent along dp = precip
    sp3, se3 = leaf(1.0), torch.tensor(1.0, dtype=torch.float64, device=dev, requires_grad=True)
    prs, pes, fd3 = lg.scaled_forcing(precip, pet, sp3, se3)
    assert torch.equal(water[:, [0, 2]], prs[:, [0, 2]]) and torch.equal(dw[3][:, [0, 2]], precip[:, [0, 2]])
    loss_of(torch.where(torch.tensor([True, False, True], device=dev)[None, :], prs, water).contiguous(), pes, fd3).backward()
    assert torch.equal(sp3.grad[[0, 2]], direct["scale_p"][[0, 2]])
    return gaps


def series_refuses(dev):
    """The broadcast [T, Nf] layout, directions of another shape, and something that is no ForcingDirections raise LgarError."""
    import lgar_py_amd as lg
    import lgar_py_amd.autograd as A
    g, pr, pe, _ = storm_job(dev, N=3)
    P = [torch.tensor(np.repeat(g[k][:, None], 6, 1), device=dev) for k in PARAMS]
    kw = dict(G.engine_keywords(g), dtype=torch.float64)
    one = torch.ones(3, dtype=torch.float64, device=dev, requires_grad=True)
    _, _, fd = lg.scaled_forcing(pr, pe, one, one)
    with pytest_raises(lg.LgarError, "broadcast"):
        A.lgar_series(*P, pr, pe, forcing_directions=fd, **kw)  # six columns read three forcing columns by the layout
    with pytest_raises(lg.LgarError, r"must be \[K, T, B\]"):
        A.lgar_series(*[p[:, :3].contiguous() for p in P], pr[:-1], pe[:-1], forcing_directions=fd, **kw)
    with pytest_raises(lg.LgarError, "must be a forcing.ForcingDirections"):
        A.lgar_series(*P, pr, pe, forcing_directions=(one,), **kw)
    with pytest_raises(lg.LgarError, "d_precip and d_pet alike"):
        lg.ForcingDirections((one,), d_precip=pr[None], d_pet=pe[None, :-1])
    with pytest_raises(lg.LgarError, "need d_precip or d_pet"):
        lg.ForcingDirections((one,))


def pytest_raises(kind, match):
    import pytest
    return pytest.raises(kind, match=match)


# ---- the raw entry point ---------------------------------------------------------------------------------------------
def refusals(raw, alloc):
    """raw(dims, params, direction, forcing, dforcing, w_runoff, w_perc, window, grad, series, status, dtype): the entry point
    with the arguments of include/lgar.h up to the dtype (ctypes references and addresses).  alloc(shape, numpy dtype, fill): the
    address of a new array where the entry point reads it, kept alive by the caller.  A well-formed call of two columns and two
    rows returns 0; every refusal the header lists for lgar_forward_tangent_forced returns LGAR_E_ARG."""
    N, L, T, F, E = 2, 3, 2, 8, -1
    g = G.load("grad_synth0_12h")
    dims = _capi.make_dims(n_columns=N, n_layers=L, front_slots=F, **G.engine_keywords(g))
    dims.n_steps = T
    par = _capi.LgarParams(*[alloc((L, N), np.float64, np.repeat(g[k][:, None], N, 1)) for k in PARAMS])
    direction = _capi.LgarParams(None, None, alloc((L, N), np.float64, 1.0), None, None, None)
    forcing = _capi.LgarForcing(alloc((T, N), np.float64, 1.0), alloc((T, N), np.float64, 0.0), None)
    dprecip, dpet, cmap = alloc((T, N), np.float64, 1.0), alloc((T, N), np.float64, 0.5), alloc((N,), np.int32, 0)
    dforcing = _capi.LgarForcing(dprecip, dpet, None)
    grad, status = alloc((N,), np.float64, 0.0), alloc((N,), np.int32, 0)
    state = lambda: _capi.LgarState(*[alloc((F, N), np.float64, 0.0) for _ in range(5)], alloc((F, N), np.uint8, 0),
                                    alloc((N,), np.int32, 0), alloc((_capi.NSCAL, N), np.float64, 0.0), None, None)
    si, di, so, do = state(), state(), state(), state()
    win = lambda a=None, b=None, c=None, d=None, gin=None: _capi.LgarTangentWindow(*[None if x is None else C.addressof(x) for x in (a, b, c, d)], gin)
    ref = lambda x: None if x is None else C.byref(x)

    def call(window=win(), dims=dims, par=par, direction=direction, forcing=forcing, dforcing=dforcing, grad=grad, status=status,
             dtype=_capi.F64):
        return raw(ref(dims), ref(par), ref(direction), ref(forcing), ref(dforcing), None, None, ref(window), grad, None, status, dtype)

    assert call() == 0 and call(win(None, None, so, do)) == 0 and call(win(si, di, so, do, grad)) == 0
    assert call(dforcing=_capi.LgarForcing(None, None, None)) == 0  # both tangents NULL: zeros
    assert call(dforcing=_capi.LgarForcing(dprecip, None, None)) == 0 and call(dforcing=_capi.LgarForcing(None, dpet, None)) == 0
    # the new refusals
    assert call(dforcing=None) == E                                      # a null dforcing
    assert call(dforcing=_capi.LgarForcing(dprecip, dpet, cmap)) == E    # a column_map in dforcing
    assert call(dforcing=_capi.LgarForcing(None, None, cmap)) == E
    # ... what lgar_forward_tangent_window refuses
    assert call(None) == E and call(win(None, di)) == E
    assert call(win(si, di, so, None)) == E and call(win(si, di, None, do)) == E
    assert call(win(si, di, si, do)) == E and call(win(si, di, so, di)) == E
    broken = state()
    broken.theta = None
    assert call(win(broken, di, so, do)) == E and call(win(si, di, broken, do)) == E
    # ... and what lgar_forward_tangent refuses
    assert call(dims=None) == E and call(par=None) == E and call(direction=None) == E and call(forcing=None) == E
    assert call(grad=None) == E and call(status=None) == E and call(dtype=7) == E
    assert call(forcing=_capi.LgarForcing(None, forcing.pet, None)) == E
    bad = _capi.make_dims(n_columns=N, n_layers=L, front_slots=F)
    bad.n_steps, bad.tangent_share = T, 3
    assert call(dims=bad) == E
