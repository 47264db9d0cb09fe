"""GPU (-m gpu): the catchment snowpack -- lgar_catchment_snow / lgar_catchment_snow_grad through snow.CatchmentSnow and
snow.catchment_snow (autograd).

w, ice and liq of cell b are pure functions of column b of p, ta and par and of state_in[.][b] (include/lgar.h; DESIGN.md section
19), so the kernels are held BIT FOR BIT to the numpy statement of the definition (tests/snow_host: snow_ref, snow_grad_ref), the
one tests/test_snow_host.py holds the host build of the same header to -- and that file holds the definition itself to statements
that do not come from it: the warm identity, the degree-day recurrence, the mass balance, the adjoint to derivatives of the
real-arithmetic statement in mpmath."""
import itertools
from fractions import Fraction

import numpy as np
import pytest

import _forcing_map_job as J
import snow_host as SH

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GRID_CAP = 2048  # LGAR_SN_GRID_CAP (csrc/lgar_snow.hip): workgroups of a launch; the rest by stride
GPU_T = (0, 1, 9, 17)
U = 2.0 ** -53


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return None if t is None else t.cpu().numpy()


def _raw(dt):
    """The kernels behind the package's own launch helpers, with values the Python layer would refuse or never sees."""
    from lgar_py_amd import _capi, snow
    lib, dev = _capi.load(), torch.device("cuda:0")
    fwd = lambda p, ta, par, st, want_state, want_pack: snow._forward(lib, dev, p, ta, par, dt, st, want_state, want_pack)
    bwd = lambda gw, gi, gl, p, ta, ice, liq, par, st, want_ta, want_par, want_state: snow._backward(
        lib, dev, gw, gi, gl, p, ta, ice, liq, par, dt, st, want_ta, want_par, want_state)
    return fwd, bwd


@pytest.mark.parametrize("B", SH.SHAPE_B)
def test_kernels_equal_the_numpy_definition_bit_for_bit(B):
    """B in {1, 2, 63, 64, 65, 257} x T in {0, 1, 9, 17} x state_in present or NULL: the forward with every combination of pack and
    state_out wanted, the adjoint with every combination of gta, gpar and gstate wanted, with gice / gliq given and NULL -- the
    host test's case data (every regime of the walk, the planted ties, negative p and liq, -0.0 in p)."""
    rng = np.random.default_rng(1900 + B)
    for T in GPU_T:
        p, ta, gw, gi, gl, par, state, dt = SH.case_data(rng, T, B)
        fwd, bwd = _raw(dt)
        dp, dta, dgw, dgi, dgl, dpar = (_cuda(a) for a in (p, ta, gw, gi, gl, par))
        for st in (None, state):
            what = (B, T, st is not None)
            dst = _cuda(st)
            w_ref, ice_ref, liq_ref, so_ref = SH.snow_ref(p, ta, par, dt, st)
            for want_pack, want_state in itertools.product((True, False), repeat=2):
                w, ice, liq, so = fwd(dp, dta, dpar, dst, want_state, want_pack)
                assert SH.same_bits(_np(w), w_ref), what
                assert (ice is None) == (liq is None) == (not want_pack) and (so is None) == (not want_state), what
                assert not want_pack or (SH.same_bits(_np(ice), ice_ref) and SH.same_bits(_np(liq), liq_ref)), what
                assert not want_state or SH.same_bits(_np(so), so_ref), what
            dice, dliq = _cuda(ice_ref), _cuda(liq_ref)
            full = SH.snow_grad_ref(gw, gi, gl, p, ta, ice_ref, liq_ref, par, dt, st)
            bare = SH.snow_grad_ref(gw, None, None, p, ta, ice_ref, liq_ref, par, dt, st)
            for gpack, want_ta, want_par, want_state in itertools.product((True, False), repeat=4):
                ref = full if gpack else bare
                got = bwd(dgw, dgi if gpack else None, dgl if gpack else None, dp, dta, dice, dliq, dpar, dst, want_ta, want_par, want_state)
                assert SH.same_bits(_np(got[0]), ref[0]), what
                for have, want, wanted in zip(got[1:], ref[1:], (want_ta, want_par, want_state)):
                    assert (have is None) == (not wanted) and (have is None or SH.same_bits(_np(have), want)), what


def test_the_capped_grid_strides():
    """A launch has at most 2048 workgroups of 256 lanes.  B = 256 x 2048 + 65, T = 2: the lanes stride over the cells.  Forward
    and adjoint with every output against the numpy definition, bit for bit."""
    B, T = 256 * GRID_CAP + 65, 2
    rng = np.random.default_rng(8)
    p, ta, gw, gi, gl, par, state, dt = SH.case_data(rng, T, B)
    fwd, bwd = _raw(dt)
    ref = SH.snow_ref(p, ta, par, dt, state)
    dp, dta, dpar, dst = _cuda(p), _cuda(ta), _cuda(par), _cuda(state)
    w, ice, liq, so = fwd(dp, dta, dpar, dst, True, True)
    assert all(SH.same_bits(_np(a), b) for a, b in zip((w, ice, liq, so), ref))
    g_ref = SH.snow_grad_ref(gw, gi, gl, p, ta, ref[1], ref[2], par, dt, state)
    got = bwd(_cuda(gw), _cuda(gi), _cuda(gl), dp, dta, ice, liq, dpar, dst, True, True, True)
    assert all(SH.same_bits(_np(a), b) for a, b in zip(got, g_ref))


def test_chunked_calls_equal_one_call():
    """run(carry=True) cut at 1 row, at T - 1 rows and in the middle against one call, and a repeated call: the same bits."""
    from lgar_py_amd.snow import CatchmentSnow
    rng = np.random.default_rng(23)
    T, B = 17, 257
    p, ta, _, _, _, par, state, dt = SH.case_data(rng, T, B)
    store = CatchmentSnow(*par, dt)
    dp, dta = _cuda(p), _cuda(ta)
    for st in (None, state):
        want = SH.snow_ref(p, ta, par, dt, st)
        one = store.run(dp, dta, carry=False, state=_cuda(st), pack=True)
        assert all(SH.same_bits(_np(a), b) for a, b in zip(one, want))
        assert torch.equal(store.run(dp, dta, carry=False, state=_cuda(st)), one[0]) and store.state_of() is None
        for cut in (1, T - 1, T // 2):
            key = (cut, st is None)
            a = store.run(dp[:cut], dta[:cut], key=key, state=_cuda(st), pack=True)
            b = store.run(dp[cut:], dta[cut:], key=key, pack=True)
            assert all(torch.equal(torch.cat([x, y]), z) for x, y, z in zip(a, b, one)), cut
            assert SH.same_bits(_np(store.state_of(key)), want[3]), cut
    store.reset()
    assert store.state_of((1, True)) is None


def test_entry_points_refuse_bad_arguments():
    """LGAR_E_ARG from the library itself: negative sizes, a dt_h that is not finite or <= 0, a null pointer the sizes say will be
    read or written, exactly one of ice / liq, the adjoint without its pack.  Nothing is launched by a refused call."""
    from lgar_py_amd import _capi
    lib = _capi.load()
    buf = torch.zeros(2048, dtype=torch.float64, device="cuda")
    a = buf.data_ptr()
    fwd = (("p", a), ("ta", a), ("T", 2), ("B", 4), ("par", a), ("dt", 1.0), ("state_in", None), ("state_out", a + 2048), ("w", a + 4096),
           ("ice", a + 6144), ("liq", a + 8192))
    run = lambda **kw: lib.lgar_catchment_snow(*[kw.get(k, d) for k, d in fwd], None)
    for bad in (dict(T=-1), dict(B=-1), dict(p=None), dict(ta=None), dict(par=None), dict(w=None), dict(ice=None), dict(liq=None), dict(dt=0.0),
                dict(dt=-1.0), dict(dt=float("nan")), dict(dt=float("inf")), dict(B=0, ice=None)):
        assert run(**bad) == -1, bad
    grd = (("gw", a), ("gice", a), ("gliq", a), ("p", a), ("ta", a), ("ice", a), ("liq", a), ("T", 2), ("B", 4), ("par", a), ("dt", 1.0),
           ("state_in", None), ("gp", a + 2048), ("gta", a + 4096), ("gpar", a + 6144), ("gstate", a + 8192))
    grad = lambda **kw: lib.lgar_catchment_snow_grad(*[kw.get(k, d) for k, d in grd], None)
    for bad in (dict(T=-1), dict(B=-1), dict(gw=None), dict(p=None), dict(ta=None), dict(ice=None), dict(liq=None), dict(ice=None, liq=None),
                dict(par=None), dict(gp=None), dict(dt=0.0), dict(dt=float("nan")), dict(T=0, liq=None)):
        assert grad(**bad) == -1, bad
    torch.cuda.synchronize()
    assert not buf.any()
    # accepted: B = 0 and T = 0 with nothing to write launch nothing; the rest write zeros here (all parameters 0: tlo == thi, no
    # quotient is selected, and parameter values are not policed), so only the return codes are looked at
    assert run(B=0, p=None, ta=None, par=None, w=None) == 0 and run(T=0, state_out=None, p=None, w=None) == 0 and grad(B=0, gw=None, gp=None) == 0
    assert grad(T=0, gpar=None, gstate=None, gw=None, ice=None, liq=None) == 0
    assert run() == 0 and run(ice=None, liq=None, state_out=None) == 0 and grad() == 0 and grad(gice=None, gliq=None, gta=None, gpar=None, gstate=None) == 0
    torch.cuda.synchronize()


# ---- end to end -----------------------------------------------------------------------------------------------------------------
E2E = dict(n=24, B=3, T=17, dt_h=0.125)  # dt_h a power of two: the warm identity hands the forcing on bit for bit


def _forward_end_to_end(engine, snow_of, dev):
    """24 perturbed three-layer columns read 3 forcing cells through a ForcingMap; 17 rows of synth_1's long storm scaled per cell.
    engine(): a fresh engine; snow_of(...): the store's class; dev: where the tensors live."""
    from lgar_py_amd import ForcingMap
    from lgar_py_amd import workloads as W
    n, B, T, dt = E2E["n"], E2E["B"], E2E["T"], E2E["dt_h"]
    f = W.synth1_forcing()[59:59 + T]
    p = np.ascontiguousarray(f[:, 0:1] * np.array([0.8, 1.0, 1.5])[None, :])
    pet = np.ascontiguousarray(f[:, 1:2] * np.ones(B)[None, :])
    idx = np.random.default_rng(0).permutation(np.arange(n) % B)
    fm = ForcingMap(idx, n_forcing=B, device=dev)
    names = ("runoff", "percolation", "precip", "infiltration")
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def run(water):
        eng = engine()
        out = eng.forward(water, on(pet), series=names, check=False, forcing_map=fm)
        return {k: v.cpu().numpy() for k, v in out.items()}, eng.status.cpu().numpy()

    # sfcf = 1: what falls as snow enters the pack as it is, so the cold run differs from the warm one by the pack alone
    snow = snow_of(-1.0, 2.0, 0.5, 1.0, 0.2, 0.05, 0.1, dt, n_catchments=B)
    rng = np.random.default_rng(1)
    ta = 6.0 + 4.0 * rng.random((T, B))
    water = snow.run(on(p), on(ta), carry=False)
    plain, status = run(on(p))
    through, status2 = run(water)
    assert not (status & 0x7F).any() and float(plain["runoff"].sum()) > 0.1
    assert plain["runoff"].tobytes() == through["runoff"].tobytes() and plain["percolation"].tobytes() == through["percolation"].tobytes()
    assert all(plain[k].tobytes() == through[k].tobytes() for k in names) and status.tobytes() == status2.tobytes()
    # cell 1 is cold for ten rows
    cold_rows, cold = 10, idx == 1
    ta2 = ta.copy()
    ta2[:cold_rows, 1] = -5.0 - rng.random(cold_rows)
    w2, ice, liq = (v.cpu().numpy() for v in snow.run(on(p), on(ta2), carry=False, pack=True))
    held, _ = run(on(w2))
    assert cold.sum() == n // B and not w2[:cold_rows, 1].any()
    for k in ("precip", "infiltration", "runoff"):
        assert not held[k][:cold_rows][:, cold].any(), k           # no water while it is cold
        assert held[k][:, ~cold].tobytes() == plain[k][:, ~cold].tobytes(), k  # the other cells' columns as before
    assert float(held["precip"][cold_rows:][:, cold].sum()) > 0     # melt and rain arrive after the thaw
    assert np.array_equal(held["precip"], (w2 * dt)[:, idx])         # the columns were given exactly the store's water
    # the water totals: warm - cold = the pack left at the end, within the closure bound of the host test (gamma_22T M,
    # M = sum (1 + sfcf) p dt, taken exactly)
    F = lambda v: Fraction(float(v))
    pack = ice[-1] + liq[-1]
    assert pack[1] > 0.5 and not pack[[0, 2]].any()
    worst = 0.0
    for b in range(B):
        warm_total = F(dt) * sum(F(v) for v in _np(water)[:, b])
        cold_total = F(dt) * sum(F(v) for v in w2[:, b])
        miss = abs(warm_total - cold_total - F(ice[-1, b]) - F(liq[-1, b]))
        M = 2 * F(dt) * sum(F(v) for v in p[:, b])
        bar = Fraction(22 * T * U / (1.0 - 22 * T * U)) * M
        assert miss <= bar, b
        worst = max(worst, float(miss / bar))
    print("end to end: water totals, warm - cold - pack: worst miss / bound %.3g" % worst)
    # the engine's own totals of the water it was given, per cell (a sum of T fp64 terms per column: gamma_T on top)
    for b in range(B):
        cols = np.nonzero(idx == b)[0]
        diff = plain["precip"][:, cols].sum(0) - held["precip"][:, cols].sum(0)
        M = 2.0 * dt * float(p[:, b].sum())
        assert np.all(np.abs(diff - pack[b]) <= (22 * T + 2 * T + 2) * U * M), b


def test_forward_end_to_end():
    """With warm temperatures eng.forward(snow.run(p, ta), pet, forcing_map=...) equals eng.forward(p, pet, forcing_map=...) bit for
    bit on runoff and percolation (and on every other series asked for, and the status).  With one cold cell that cell's columns
    receive no water while it is cold and the other cells' columns are untouched; the run's water totals differ from the warm
    run's by the pack left at the end, within the closure bound."""
    import lgar_py_amd as lg
    n, dt = E2E["n"], E2E["dt_h"]
    _forward_end_to_end(lambda: lg.LgarEngine(*J.soil(n, 3), dt_h=dt, ponded_depth_max=0.0), lg.CatchmentSnow, torch.device("cuda:0"))


def _gradients_end_to_end(function, score_of, dev):
    """A pack over 17 rows in 3 cells under an oscillating temperature; snow-water-equivalent observations with gaps from a
    perturbed parameter set; CatchmentScore(obs).loss(ice + liq) through catchment_snow."""
    T, B, dt = 17, 3, 1.0
    rng = np.random.default_rng(11)
    ta = 3.5 * np.sin(0.9 * np.arange(T)[:, None] + np.array([0.0, 1.0, 2.0])[None, :]) + rng.normal(0.0, 0.8, (T, B))
    p = 0.05 + 0.4 * rng.random((T, B))
    par = np.array([[-1.0, -1.5, -0.5], [2.0, 1.5, 2.5], [0.3, 0.5, 0.1], [1.1, 0.9, 1.0], [0.15, 0.2, 0.1], [0.5, 0.8, 0.3], [0.1, 0.05, 0.08]])
    state = np.array([[3.0, 2.0, 1.5], [0.1, 0.05, 0.1]])
    truth = par * (1.0 + 0.2 * (rng.random(par.shape) - 0.5))
    _, ice_o, liq_o, _ = SH.snow_ref(p, ta, truth, dt, state * 1.1)
    obs = ice_o + liq_o
    obs[3, 0] = obs[7:9, 1] = obs[12, 2] = np.nan  # gaps
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    leaf = lambda a: on(a).clone().requires_grad_(True)
    tp, tt, ts = leaf(p), leaf(ta), leaf(state)
    tpar = [leaf(par[k]) for k in range(7)]
    w, ice, liq = function(tp, tt, *tpar, dt, state=ts, return_pack=True)
    swe = ice + liq
    swe.retain_grad()
    score = score_of(obs)
    loss = score.loss(swe)
    loss.backward()
    assert np.isfinite(float(loss.detach())) and float(loss.detach()) > 0
    for name, t in zip(("tlo", "thi", "tm", "sfcf", "cfmax", "cfr", "cwh", "state"), tpar + [ts]):
        assert bool(torch.isfinite(t.grad).all()) and float(t.grad.abs().max()) > 0, name
    ref = SH.snow_ref(p, ta, par, dt, state)
    assert all(SH.same_bits(a.detach().cpu().numpy(), b) for a, b in zip((w, ice, liq), ref))
    g = swe.grad.cpu().numpy()
    assert not g[3, 0] and not g[7:9, 1].any() and not g[12, 2] and float(np.abs(g).max()) > 0  # nothing comes back under a gap
    gp, gta, gpar, gstate = SH.snow_grad_ref(np.zeros((T, B)), g, g, p, ta, ref[1], ref[2], par, dt, state)
    assert SH.same_bits(np.stack([v.grad.cpu().numpy() for v in tpar]), gpar) and SH.same_bits(tp.grad.cpu().numpy(), gp)
    assert SH.same_bits(tt.grad.cpu().numpy(), gta) and SH.same_bits(ts.grad.cpu().numpy(), gstate)


def test_gradients_end_to_end():
    """CatchmentScore(swe observations with gaps).loss(ice + liq) through catchment_snow: the loss is finite, the gradients to tm,
    cfmax, sfcf, cfr, cwh, tlo, thi and state are finite and non-zero, and gpar, gp (and gta, gstate) have the numpy adjoint's bits
    for the gradient the score handed back."""
    import lgar_py_amd as lg
    _gradients_end_to_end(lg.catchment_snow, lambda obs: lg.CatchmentScore(obs), torch.device("cuda:0"))
