"""GPU (-m gpu): the catchment-canopy kernels (lgar_catchment_canopy / _grad / _tangent, csrc/lgar_canopy.hip) on the hardware against
the numpy statement of the definition bit for bit (tests/canopy_host has the statement; the host suite holds it to statements
that do not come from it), the capped grid, the refusals of the raw entry points, and the chain canopy -> snow -> columns ->
catchment sums with its gradients taken two ways.  Shapes of a few hundred cells: every case takes seconds."""
import ctypes as C

import numpy as np
import pytest

import _forcing_tangent as FT
import _golden as G
import canopy_host as CH
from _hostbuild import same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

_uploaded = {}  # id(numpy array) -> (the array, its copy on the device): the grid calls with the same inputs many times


def _up(a):
    if id(a) not in _uploaded:
        if len(_uploaded) > 64:
            _uploaded.clear()
        _uploaded[id(a)] = (a, torch.tensor(a, device="cuda"))
    return _uploaded[id(a)][1]


def _gpu_launch(name, *args):
    """`launch` of canopy_host.call on the library: the inputs uploaded (once per array), the outputs uploaded as they are and
    copied back after the launch"""
    from lgar_py_amd import _capi
    outs = {i: torch.tensor(args[i], device="cuda") for i in CH.OUTPUT_ARGS[name] if isinstance(args[i], np.ndarray)}
    dev = [outs[i] if i in outs else (_up(a) if isinstance(a, np.ndarray) else a) for i, a in enumerate(args)]
    q = lambda x: (None if x.numel() == 0 else x.data_ptr()) if isinstance(x, torch.Tensor) else x
    _capi.launch(_capi.load(), name, torch.device("cuda"), *[q(x) for x in dev])
    for i, t in outs.items():
        args[i][...] = t.cpu().numpy()
    return 0


def _gpu_call(case):
    rc, o = CH.call(case, _gpu_launch)
    assert rc == 0
    return o


@pytest.mark.parametrize("B", CH.SHAPE_B)
def test_kernels_equal_the_numpy_statement_bit_for_bit(B):
    """canopy_host.grid(B) in full on the hardware: T in {0, 1, 9, 17} x state present / NULL x lai present / NULL, and at each point
    every combination of optional inputs and wanted outputs of the forward (4), the adjoint (32) and the tangent (256; D in {1, 3}
    and two (ld, k0) rotating): 4672 launches of microseconds each, each bit for bit against the numpy statement."""
    n = 0
    for case, want in CH.grid(B):
        CH.check(case, want, _gpu_call(case))
        n += 1
    assert n == 16 * (4 + 32 + 256)
    rows, ties = CH.grid_counts(B)
    if B >= 63:
        assert all(v > 0 for v in rows.values()) and all(v > 0 for v in ties.values()), (rows, ties)


def test_capped_grid_strides_over_the_cells():
    """B = 256 x 2048 + 65 cells, T = 2: the grid is capped at 2048 workgroups, so every lane takes a second cell and 65 a third --
    forward, adjoint and tangent (D = 1) bit for bit against the statement."""
    rng = np.random.default_rng(3)
    T, B = 2, 256 * 2048 + 65
    p, e, lai, par, state, dt = CH.case_data(rng, T, B)
    g = tuple(CH.mixed(rng, T, B) for _ in range(4))
    dirs = (CH.mixed(rng, 1, T, B), CH.mixed(rng, 1, T, B), CH.mixed(rng, 1, T, B), CH.mixed(rng, 1, 3, B), CH.mixed(rng, 1, B))
    fwd = ("fwd", p, e, lai, par, dt, state, True, True)
    want = CH.reference(fwd)
    CH.check(fwd, want, _gpu_call(fwd))
    for case in (("grad", *g, p, e, lai, want[2], par, dt, state, True, True, True), ("tan", p, e, lai, par, dt, state, 1, *dirs, 1, 0, True, True, True)):
        CH.check(case, CH.reference(case), _gpu_call(case))
    rows = CH.regimes(p, e, lai, par, dt, state)[0]
    assert all(v > 0 for v in rows.values()), rows


@pytest.mark.parametrize("which", ["p", "e", "lai", "state"])
def test_a_nan_stays_in_its_cell(which):
    CH.nan_confinement(_gpu_call, which)


def test_raw_entry_points_refuse_what_the_header_says():
    from lgar_py_amd import _capi
    lib = _capi.load()
    dev = torch.ones(1024, dtype=torch.float64, device="cuda")

    def entry(name):
        fn = getattr(lib, "lgar_" + name)

        def call(*args):
            rc = fn(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream))
            torch.cuda.synchronize()
            return rc
        return call

    class Buffer:
        address = dev.data_ptr()
        get = staticmethod(lambda lo, hi: dev[lo:hi].cpu().tolist())

        @staticmethod
        def set(lo, hi, values):
            dev[lo:hi] = torch.as_tensor(values, dtype=torch.float64)
    CH.refusals(entry, Buffer)


def test_python_surface_on_the_library():
    """CatchmentCanopy.run (carried chunks), catchment_canopy (autograd) and catchment_canopy_directions on the library: the bits of
    the statement."""
    import lgar_py_amd as lg
    rng = np.random.default_rng(12)
    T, B = 17, 65
    p, e, lai, par, state, dt = CH.case_data(rng, T, B)
    p, state = np.abs(p), np.abs(state)
    t = lambda x: torch.tensor(x, device="cuda")
    canopy = lg.CatchmentCanopy(*[par[k] for k in range(3)], dt)
    want = CH.canopy_ref(p, e, lai, par, dt, state)
    a = canopy.run(t(p[:9]), t(e[:9]), t(lai[:9]), state=t(state), store=True)
    b = canopy.run(t(p[9:]), t(e[9:]), t(lai[9:]), store=True)
    assert all(same_bits(torch.cat([x, y]).cpu().numpy(), z) for x, y, z in zip(a, b, want))
    assert same_bits(canopy.state_of().cpu().numpy(), want[4])
    g = tuple(CH.mixed(rng, T, B) for _ in range(4))
    leaf = lambda x: t(x).requires_grad_(True)
    tp, te, tl, ts, tpar = leaf(p), leaf(e), leaf(lai), leaf(state), [leaf(par[k]) for k in range(3)]
    outs = lg.catchment_canopy(tp, te, *tpar, dt, lai=tl, state=ts, return_store=True)
    sum((o * t(gk)).sum() for o, gk in zip(outs, g)).backward()
    ref = CH.canopy_grad_ref(*g, p, e, lai, want[2], par, dt, state)
    mine = (tp.grad, te.grad, tl.grad, torch.stack([v.grad for v in tpar]), ts.grad)
    assert all(same_bits(x.cpu().numpy(), y) for x, y in zip(mine, ref))
    water, pet_out, fd = lg.catchment_canopy_directions(t(p), t(e), *tpar, dt, lai=t(lai), state=t(state))
    dpar = np.zeros((3, 3, B))
    dpar[[0, 1, 2], [0, 1, 2]] = 1.0
    tan = CH.canopy_tangent_ref(p, e, lai, par, dt, state, 3, dpar=dpar)
    assert fd.K == 3 and same_bits(fd.d_precip.permute(1, 2, 0).cpu().numpy(), tan[0]) and same_bits(fd.d_pet.permute(1, 2, 0).cpu().numpy(), tan[1])
    assert same_bits(water.cpu().numpy(), want[0]) and same_bits(pet_out.cpu().numpy(), want[1])


def _make(g, N, soil=None, **kw):
    import lgar_py_amd as lg
    return lg.LgarEngine(*soil, **kw)


def test_canopy_snow_columns_gradients_two_ways(monkeypatch):
    """Section 20's shape with the canopy ahead of it: 24 columns in 3 cells (11, 4, 9 columns) through a ForcingMap, T = 17 rows of
    dt_h = 1/8 h, cell 1 cold (a pack of 3 cm, the air around the melt threshold), cells 0 and 2 warm.  (water_c, pet_out) =
    canopy(precip, pet, lai), water = snow(water_c, temp), the columns run on (water, pet_out), the loss is a weighted sum of
    catchment_sum(runoff).  The gradients to cmax, fe, cover, cfmax and sfcf ([B] each), two ways:
      directly: catchment_canopy_directions (ONE canopy-tangent launch) gives d water_c and d pet_out along the three canopy
      parameters, catchment_snow_directions(upstream=) (ONE snow-tangent launch over 3 + 2 directions) carries them through the
      pack beside its own two, and lgar_series(forcing_directions=) returns the five gradients;
      by the other association: 2 x 17 one-hot time lanes per column give d loss / d water[t, b] and d loss / d pet_out[t, b];
      d loss / d water goes as gw into lgar_catchment_snow_grad, and its gp with d loss / d pet_out as gpet into
      lgar_catchment_canopy_grad (the backward passes of catchment_snow and catchment_canopy).
    The same sums in another order: each gradient within 1e-6 of its largest entry, the bar section 20 uses for the same
    comparison.  Every canopy gradient is finite and non-zero.  With cover = 0 the water is the no-canopy run's in bits.
    Measured on the hardware: profiles/r19/two_associations.txt."""
    import lgar_py_amd as lg
    import lgar_py_amd.autograd as A
    from lgar_py_amd import _capi
    from lgar_py_amd import workloads as W
    from lgar_py_amd.catchments import catchment_sum
    from lgar_py_amd.forcing import ForcingMap
    dev = "cuda:0"
    N_CELLS, N_SOIL, CELL_OF = FT.N_CELLS, FT.N_SOIL, FT.CELL_OF
    T, dt = 17, 0.125
    r = np.arange(T)
    rain = ((r >= 2) & (r < 5)) | ((r >= 8) & (r < 14))
    precip = torch.tensor(np.where(rain[:, None], np.array([9.0, 6.0, 11.0])[None, :], 0.0), device=dev)
    pet = torch.tensor(np.where((r >= 5) & (r < 8), 0.2, 1.2)[:, None] * np.array([1.0, 0.8, 1.1])[None, :], device=dev)
    lai = torch.tensor(1.0 + 0.4 * np.sin(0.5 * r)[:, None] * np.array([1.0, 0.5, -0.7])[None, :], device=dev)
    temp = torch.tensor(np.stack([np.full(T, 10.0), 1.2 + 1.5 * np.sin(0.7 * r), np.full(T, 12.0)], axis=1), device=dev)
    state = torch.tensor([[0.0, 3.0, 0.0], [0.0, 0.05, 0.0]], dtype=torch.float64, device=dev)
    snow_names = ("tlo", "thi", "tm", "sfcf", "cfmax", "cfr", "cwh")
    snow_values = dict(tlo=-1.0, thi=2.0, tm=0.4, sfcf=1.1, cfmax=0.9, cfr=0.05, cwh=0.1)
    canopy_values = dict(cmax=0.35, fe=0.9, cover=0.7)
    Pn = W.perturbed_columns(N_SOIL, frac=0.05, seed=31)
    kw = dict(G.engine_keywords(G.load("grad_synth0_12h")), dtype=torch.float64, dt_h=dt)
    cmap = A.CatchmentMap(CELL_OF, n_catchments=N_CELLS, device=dev)
    fmap = ForcingMap(CELL_OF, N_CELLS, device=dev)
    wl = torch.tensor(0.5 + np.random.default_rng(13).random((T, N_CELLS)), device=dev)
    soil = [torch.tensor(Pn[k], device=dev) for k in FT.PARAMS]
    leaf = lambda v: torch.full((N_CELLS,), v, dtype=torch.float64, device=dev, requires_grad=True)
    const = lambda v: torch.full((N_CELLS,), v, dtype=torch.float64, device=dev)

    def snow_pars(grad):
        return [(leaf if k in ("cfmax", "sfcf") and grad else const)(snow_values[k]) for k in snow_names]

    launches = []
    real = _capi.launch
    monkeypatch.setattr(_capi, "launch", lambda lib, name, *a, **k: (launches.append(name), real(lib, name, *a, **k))[1])
    # directly
    cpar = {k: leaf(v) for k, v in canopy_values.items()}
    spar = snow_pars(True)
    water_c, pet_out, fd_c = lg.catchment_canopy_directions(precip, pet, cpar["cmax"], cpar["fe"], cpar["cover"], dt, lai=lai)
    water, fd = lg.catchment_snow_directions(water_c, temp, *spar, dt, state=state, upstream=fd_c)
    assert launches == ["catchment_canopy", "catchment_canopy_tangent", "catchment_snow", "catchment_snow_tangent"]
    assert fd.K == 5 and tuple(fd.d_precip.shape) == (5, T, N_CELLS) and tuple(fd.d_pet.shape) == (5, T, N_CELLS)
    runoff, _ = A.lgar_series(*soil, water, pet_out, forcing_map=fmap, forcing_directions=fd, **kw)
    (wl * catchment_sum(runoff, cmap)).sum().backward()
    direct = dict(cmax=cpar["cmax"].grad, fe=cpar["fe"].grad, cover=cpar["cover"].grad, cfmax=spar[4].grad, sfcf=spar[3].grad)
    # the other association
    eng = _make(None, None, soil=[x.repeat_interleave(2 * T, dim=1) for x in soil], with_state=False, **kw)
    d1 = torch.zeros(T, N_CELLS, 2 * T, dtype=torch.float64, device=dev)
    d2 = torch.zeros(T, N_CELLS, 2 * T, dtype=torch.float64, device=dev)
    d1[torch.arange(T), :, torch.arange(T)] = 1.0
    d2[torch.arange(T), :, T + torch.arange(T)] = 1.0
    wcol = cmap.spread(wl, torch.float64)  # the loss's gradient at the runoff, [T, N]
    gl, _, status = eng.tangent({}, water, pet_out, w_runoff=wcol, forcing_group=2 * T, forcing_map=fmap, d_precip=d1, d_pet=d2)
    assert int(status.abs().max()) == 0
    gl = gl.reshape(N_SOIL, 2, T)
    gcell = torch.zeros(N_CELLS, 2, T, dtype=torch.float64, device=dev).index_add_(0, torch.tensor(CELL_OF, device=dev), gl)
    cpar2 = {k: leaf(v) for k, v in canopy_values.items()}
    spar2 = snow_pars(True)
    del launches[:]
    wc2, pet2 = lg.catchment_canopy(precip, pet, cpar2["cmax"], cpar2["fe"], cpar2["cover"], dt, lai=lai)
    w2 = lg.catchment_snow(wc2, temp, *spar2, dt, state=state)
    assert torch.equal(wc2.detach(), water_c) and torch.equal(pet2.detach(), pet_out) and torch.equal(w2.detach(), water)
    torch.autograd.backward([w2, pet2], [gcell[:, 0].T.contiguous(), gcell[:, 1].T.contiguous()])
    assert launches == ["catchment_canopy", "catchment_snow", "catchment_snow_grad", "catchment_canopy_grad"]
    other = dict(cmax=cpar2["cmax"].grad, fe=cpar2["fe"].grad, cover=cpar2["cover"].grad, cfmax=spar2[4].grad, sfcf=spar2[3].grad)
    for k in direct:
        a, b = direct[k], other[k]
        gap = float((a - b).abs().max() / b.abs().max())
        print("%-6s direct %s  other association %s  gap %.3e of the largest entry" % (k, a.cpu().numpy(), b.cpu().numpy(), gap))
        assert bool(torch.isfinite(a).all()) and gap <= 1e-6, k
        if k in canopy_values:
            assert float(a.abs().min()) > 0.0, k  # every cell's canopy moves the loss
        else:
            assert float(a[1].abs()) > 0.0, k     # the cold cell
    # bare ground: the canopy is the identity on the water (dt_h is a power of two), and the chain behind it is the no-canopy run
    wc0, pet0 = lg.CatchmentCanopy(canopy_values["cmax"], canopy_values["fe"], 0.0, dt, n_catchments=N_CELLS).run(precip, pet, lai, carry=False)
    snow = lg.CatchmentSnow(*[snow_values[k] for k in snow_names], dt, n_catchments=N_CELLS)
    assert torch.equal(wc0, precip) and torch.equal(pet0, pet)
    assert torch.equal(snow.run(wc0, temp, carry=False, state=state), snow.run(precip, temp, carry=False, state=state))
