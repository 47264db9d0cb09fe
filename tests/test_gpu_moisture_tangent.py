"""GPU (-m gpu): the tangent of the soil-moisture output on the hardware -- lgar_soil_moisture_tangent bit for bit against the numpy
statement of the definition (tests/moisture_tangent_host: the grid of the host suite), against the reference's own autograd of the
same bins (tests/golden/moisture_grad), and autograd.lgar_moisture_series through catchment sums into a CatchmentScore loss."""
import ctypes as C
import functools

import numpy as np
import pytest

import _golden as G

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
PARAMS = ("alpha", "n", "ksat", "theta_e", "theta_r", "thickness")
KINDS = ("alpha", "n", "ksat")


def _engine(name, N, **kw):
    import lgar_py_amd as lg
    g = G.load(name)
    return lg.LgarEngine(*[g[k] for k in PARAMS], n_columns=N, **dict(G.engine_keywords(g), device=DEV, **kw))


@functools.lru_cache(maxsize=None)
def _bases():
    """The end states the lanes are made from, integrated by the tangent kernels themselves (capacity chain forced)."""
    import moisture_tangent_host as H
    bases = {name: H.base_state(_engine(name, 1, search_mode=2), G.load(name)) for name in H.BASES}
    assert int(bases["grad_manyfronts_60"]["n_fronts"][0]) == 19 and bases["grad_manyfronts_60"]["depth"].shape[0] == 32
    return bases


def gpu_call(c):
    """One case of tests/moisture_tangent_host through the library's raw entry point: (out, grad) as numpy arrays or None."""
    from lgar_py_amd import _capi
    from lgar_py_amd._capi import F32, F64, MOIST_WHAT, LgarDims, LgarParams, LgarState
    import moisture_tangent_host as H
    dev = torch.device(DEV)
    dt = c["depth"].dtype
    F, lanes = c["depth"].shape
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    thick, depth, theta, flags, nf, dd, dth = keep = [up(a) for a in H._arrays(c)]
    dims = LgarDims()
    dims.n_columns, dims.n_layers, dims.front_slots = lanes, thick.shape[0], F
    dims.nint, dims.num_subcycles, dims.dt_h = 120, 1, 1.0  # (the fields lgar_soil_moisture's refusals read as well)
    p = LgarParams()
    p.thickness = thick.data_ptr()
    s, ds = LgarState(), LgarState()
    s.depth, s.theta, s.flags, s.n_fronts = depth.data_ptr(), theta.data_ptr(), flags.data_ptr(), nf.data_ptr()
    ds.depth, ds.theta = dd.data_ptr(), dth.data_ptr()
    D = H.n_bins(c)
    edges = None if c["edges"] is None else up(np.asarray(c["edges"], dtype=np.float64))
    out = torch.full((D, lanes), float("nan"), dtype=depth.dtype, device=dev) if c["mode"] != "cot" else None
    cot = up(np.asarray(c["cot"], dtype=np.float64)) if c["mode"] != "out" else None
    grad = up(np.array(c["grad"], dtype=dt)) if c["mode"] != "out" else None
    _capi.launch(_capi.load(), "soil_moisture_tangent", dev, C.byref(dims), C.byref(p), C.byref(s), C.byref(ds), _capi.ptr(edges), D,
                 MOIST_WHAT[c["what"]], _capi.ptr(out), _capi.ptr(cot), c["group"], _capi.ptr(grad), F64 if dt == np.float64 else F32)
    res = (None if out is None else out.cpu().numpy(), None if grad is None else grad.cpu().numpy())
    del keep
    return res


# 1 ---- bit for bit against the numpy statement ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("M", [1, 65, 257])
def test_grid_is_the_numpy_statement_bit_for_bit(M, dtype):
    import moisture_tangent_host as H
    n = 0
    for label, c in H.grid(_bases(), shapes=(M,), dtypes=(dtype,)):
        H.check(c, gpu_call(c), label)
        n += 1
    assert n == 2 * 2 * len(H.BIN_SETS) * 3


def test_ties_and_the_corrupt_table_on_the_hardware():
    """The planted ties with the side they take, and tables with n_fronts and layer tags out of range: the kernel clamps both (read
    in lgar_moisture_tangent.hpp: nf into [0, front_slots], the tag to n_layers - 1, before any index is formed)."""
    import moisture_tangent_host as H
    for dtype in (np.float64, np.float32):
        for label, c, want in H.ties(dtype):
            out, grad = gpu_call(c)
            H.check(c, (out, grad), label)
            assert np.isfinite(grad).all() and np.isfinite(out).all(), label
            for (_, i), v in want.items():
                assert out[i, 0] == dtype(v) and (v != 0.0 or not np.signbit(out[i, 0])), (label, i, out[:, 0], v)
    for c in H.corrupt(_bases()["grad_manyfronts_60"]) + H.corrupt(_bases()["grad_synth0_12h"], np.float32):
        H.check(c, gpu_call(c), "corrupt")


def test_one_large_launch():
    """256 * 2048 + 65 lanes with 3 bins: 2049 workgroups, the last one ragged; fp32 in 8 front slots."""
    import moisture_tangent_host as H
    base = {k: (v[:8] if v.ndim == 2 and v.shape[0] == 32 else v) for k, v in _bases()["grad_synth0_12h"].items()}
    assert int(base["n_fronts"][0]) <= 8
    lanes = 256 * 2048 + 65
    c = H.with_call(H.lanes_of(base, lanes, np.float32, seed=4), np.array([0.0, 20.0, 60.0, 250.0]), "theta", "both", 1, seed=6)
    H.check(c, gpu_call(c), "large")


# 2 ---- reference parity ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("share_group", [False, True], ids=["own_forcing", "shared_group"])
@pytest.mark.parametrize("name, mode", [("grad_synth0_12h", 0), ("grad_synth0_12h", 1), ("grad_synth0_12h", 2), ("grad_manyfronts_60", 2)])
def test_reference_parity(name, mode, share_group):
    import moisture_tangent_host as H
    H.reference_parity(_engine, name, mode, share_group)


# 3 ---- the autograd node ---------------------------------------------------------------------------------------------------
N_SOIL, N_CELLS, T, EVERY = 24, 3, 24, 6
CELL_OF = np.array([0] * 11 + [1] * 4 + [2] * 9, dtype=np.int32)


def _storm(dev):
    """tests/_forcing_tangent.py's storm job: 24 hourly rows, two storms with PET between them, the rain scaled per column"""
    import _forcing_tangent as FT
    _, pr, pe, _ = FT.storm_job(dev, N=N_SOIL, T=T)
    return pr, pe


def _soil(dev):
    """grad_synth0_12h's soil, alpha, n and ksat moved by up to 3 % from column to column"""
    g = G.load("grad_synth0_12h")
    P = {k: torch.tensor(np.repeat(g[k][:, None], N_SOIL, 1), device=dev) for k in PARAMS}
    for k in KINDS:
        P[k] = (P[k] * torch.linspace(0.97, 1.03, N_SOIL, dtype=torch.float64, device=dev)[None, :]).detach().requires_grad_(True)
    return P


def _score_loss(mo, cmap, score):
    """catchment means of the top bin's water content, snapshot by snapshot, against the observations"""
    import lgar_py_amd as lg
    sim = torch.stack([lg.catchment_sum(mo[s], cmap)[0] for s in range(mo.shape[0])])  # [S, B]
    return score.loss(sim, metric="mse")


@pytest.mark.parametrize("forcing", [False, True], ids=["parameters", "scaled_forcing"])
def test_moisture_series_into_a_catchment_score(forcing):
    """lgar_moisture_series -> catchment_sum(moisture[s]) -> CatchmentScore.loss on 24 columns in 3 catchments, T = 24, every = 6:
    finite, non-zero gradients to alpha, n and ksat, and through scaled_forcing's directions to scale_p."""
    import lgar_py_amd as lg
    import lgar_py_amd.autograd as A
    dev = torch.device(DEV)
    g = G.load("grad_synth0_12h")
    kw = dict(G.engine_keywords(g), dtype=torch.float64, device=DEV)
    pr, pe = _storm(dev)
    P = _soil(dev)
    sizes = np.bincount(CELL_OF, minlength=N_CELLS)
    cmap = lg.CatchmentMap(CELL_OF, n_catchments=N_CELLS, weights=1.0 / sizes[CELL_OF], device=dev)
    obs = 0.25 + 0.1 * np.random.default_rng(2).random((T // EVERY, N_CELLS))
    score = lg.CatchmentScore(obs, device=dev)
    more = {}
    if forcing:
        sp = torch.ones(N_SOIL, dtype=torch.float64, device=dev, requires_grad=True)
        se = torch.tensor(1.0, dtype=torch.float64, device=dev, requires_grad=True)
        pr, pe, fd = lg.scaled_forcing(pr, pe, sp, se)
        more = dict(forcing_directions=fd)
    edges = [0.0, 10.0, 40.0, 250.0]
    ro, pc, mo = A.lgar_moisture_series(*[P[k] for k in PARAMS], pr, pe, EVERY, edges=edges, what="theta", **kw, **more)
    assert tuple(mo.shape) == (T // EVERY, 3, N_SOIL) and bool(torch.isfinite(mo).all())
    loss = _score_loss(mo, cmap, score)
    loss.backward()
    assert np.isfinite(float(loss.detach())) and float(loss.detach()) > 0.0
    for k in KINDS:
        gk = P[k].grad
        assert bool(torch.isfinite(gk).all()) and float(gk.abs().max()) > 0.0, k
        assert bool((gk.abs().amax(dim=0) > 0).all()), k  # every column
    if forcing:
        assert bool(torch.isfinite(sp.grad).all()) and bool((sp.grad.abs() > 0).all())


def test_lgar_series_is_unchanged_in_bits():
    """lgar_series beside the new node: the two series and, under a zero cotangent on the moisture, the gradients have the same
    bits.  (That lgar_series itself still gives what it gave before the new code existed is held by
    tests/test_gpu_forcing_tangent.py against tests/golden/forcing_grad/series_baseline_parent.npz; that file runs unchanged.)"""
    import lgar_py_amd.autograd as A
    dev = torch.device(DEV)
    g = G.load("grad_synth0_12h")
    kw = dict(G.engine_keywords(g), dtype=torch.float64, device=DEV)
    pr, pe = _storm(dev)
    w = torch.linspace(0.5, 1.5, T, dtype=torch.float64, device=dev)[:, None]
    P = _soil(dev)
    ro0, pc0 = A.lgar_series(*[P[k] for k in PARAMS], pr, pe, **kw)
    (w * ro0 + 0.5 * w * pc0).sum().backward()
    want = {k: P[k].grad.clone() for k in KINDS}
    P = _soil(dev)
    ro, pc, mo = A.lgar_moisture_series(*[P[k] for k in PARAMS], pr, pe, EVERY, what="storage", **kw)
    assert torch.equal(ro, ro0) and torch.equal(pc, pc0)
    ((w * ro + 0.5 * w * pc).sum() + (mo * 0.0).sum()).backward()
    for k in KINDS:
        assert torch.equal(P[k].grad, want[k]) and float(want[k].abs().max()) > 0.0, k
