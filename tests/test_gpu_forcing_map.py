"""GPU (-m gpu): the forcing map (LgarForcing.column_map, forcing.ForcingMap) in every kernel family -- N soil columns read
[T, B] forcing through a per-column index.  Every equality is bitwise against the same engine settings run with the gathered
forcing precip[:, index] (tests/_forcing_map_job.py; tests/test_forcing_map_host.py runs the same device code on the host).
Only in-range maps are given to the GPU: the clamp is tested on the host."""
import ctypes as C

import numpy as np
import pytest

import _forcing_map_job as J

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _engine(n, seed=3, cols=None, **kw):
    import lgar_py_amd as lg
    return lg.LgarEngine(*(J.soil(n, seed) if cols is None else cols), **dict(J.KW, **kw))


def _fmap(idx):
    from lgar_py_amd import ForcingMap
    return ForcingMap(idx, n_forcing=J.B)


def _cuda(a):
    return torch.tensor(a, device="cuda")


# 1 ------------------------------------------------------------------------------------------------------------------------
FAMILIES = {
    "fp32-ragged": (130, dict(dtype=torch.float32)),
    "fp32-chain": (130, dict(dtype=torch.float32, search_mode=2)),
    "fp32-tickets-1025-blocks": (65600, dict(dtype=torch.float32)),
    "fp64-one-lane": (130, dict(dtype=torch.float64, forward_lanes=1)),
    "fp64-64-lanes": (100, dict(dtype=torch.float64, forward_lanes=0)),
    "fp64-8-lanes": (130, dict(dtype=torch.float64, forward_lanes=8)),
    "mixed": (130, dict(dtype=torch.float64, geff_precision="f32")),
    "literal": (130, dict(dtype=torch.float64, search_mode=0)),
}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_mapped_forward_equals_the_gathered_run_bit_for_bit(family):
    """All ten series, the final front table, scalars, totals and status."""
    n, kw = FAMILIES[family]
    idx = J.index(n)
    pr, pe = J.forcing()
    ref = _engine(n, **kw)
    if family == "fp64-64-lanes":
        assert ref.cooperating_lanes() == 64
    if family == "fp32-tickets-1025-blocks":
        assert (n + 63) // 64 == 1025  # past 1024 blocks: the natural capacity chain, persistent waves
    want = J.run(ref, *J.gathered(pr, pe, idx))
    J.forcing_matters(want, idx)
    eng = _engine(n, **kw)
    J.same(J.run(eng, pr, pe, forcing_map=_fmap(idx)), want)
    assert (eng.dims.forcing_columns, eng.dims.forcing_group) == (J.B, 1)


def test_forcing_group_and_pet_go_through_the_map():
    """forcing_group = 2 (a map of N / 2 entries) under a forcing whose PET differs per forcing column, fp32 and fp64."""
    n = 130
    idx = J.index(n // 2, seed=1)
    pr, pe = J.forcing(pet=0.004)
    for dtype in (torch.float32, torch.float64):
        want = J.run(_engine(n, dtype=dtype), *J.gathered(pr, pe, idx, group=2))
        J.forcing_matters(want, idx, group=2)
        assert float(want["AET"].sum()) > 0.0
        J.same(J.run(_engine(n, dtype=dtype), pr, pe, forcing_map=_fmap(idx), forcing_group=2), want)


# 2 ------------------------------------------------------------------------------------------------------------------------
def _same_tangent(got, want):
    for a, b in zip(got, want):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_tangent_mapped_equals_gathered(dtype):
    n = 130
    idx = J.index(n, seed=4)
    pr, pe = J.forcing()
    rng = np.random.default_rng(1)
    d = {"ksat": np.ones((3, n))}
    wr, wp = rng.random((J.T, n)), rng.random((J.T, n))
    want = _engine(n, dtype=dtype).tangent(d, *J.gathered(pr, pe, idx), w_runoff=wr, w_perc=wp, want_series=True)
    got = _engine(n, dtype=dtype).tangent(d, pr, pe, w_runoff=wr, w_perc=wp, want_series=True, forcing_map=_fmap(idx))
    ok = (want[2] & 0x7F) == 0
    wet = _cuda(idx == J.B - 1) & ok
    moved = want[1].double().abs().sum(0)[wet]  # d runoff / d ksat of the columns that shed runoff
    assert int(wet.sum()) > 0 and bool((moved[torch.isfinite(moved)] > 0.0).any())
    if dtype == torch.float64:  # (an fp32 tangent may overflow to NaN in a column whose status stays 0: compared all the same)
        assert float(moved.min()) > 0.0 and float(want[0].abs().max()) > 0.0
    _same_tangent(got, want)


@pytest.mark.parametrize("share", [0, 9])
def test_tangent_nine_directions_per_column_in_adjacent_lanes(share):
    """The direction-batched launch of autograd.parameter_vjp: every column nine times over (eng.like), forcing_group = 9, the
    SAME map of N entries and weights [T, N]; the lanes of a column stand alone (share = 0) or share the Geff trapezoid
    (share = 9).  Each against the same launch with the gathered [T, N] forcing."""
    n = 130
    idx = J.index(n, seed=5)
    pr, pe = J.forcing()
    eng = _engine(n, dtype=torch.float64)
    rep = lambda t: t.repeat_interleave(9, dim=1)
    dirs = {k: torch.zeros(3, 9 * n, dtype=torch.float64, device="cuda") for k in ("alpha", "n", "ksat")}
    for b, (kind, l) in enumerate([(k, l) for k in ("alpha", "n", "ksat") for l in range(3)]):
        dirs[kind][l, b::9] = 1.0
    w = np.random.default_rng(2).random((J.T, n))
    res = []
    for kw in (dict(), dict(forcing_map=_fmap(idx))):
        big = eng.like(*[rep(getattr(eng, k)) for k in J.PARAMS], with_state=False)
        f = (pr, pe) if kw else J.gathered(pr, pe, idx)
        res.append(big.tangent(dirs, *f, w_runoff=w, want_series=True, forcing_group=9, share=share, **kw))
        assert big.dims.tangent_share == share
    want, got = res
    # (48 rows: the wetting has not reached every layer, so not every direction moves the runoff -- the top layer's three do)
    assert sum(float(want[0][b::9].abs().max()) > 0.0 for b in range(9)) >= 3 and float(want[1].abs().max()) > 0.0
    _same_tangent(got, want)


# 3 ------------------------------------------------------------------------------------------------------------------------
def test_catchment_forcing_in_catchment_sums_out_and_back():
    """[T, B] forcing in through cmap.forcing_map(), [T, B] catchment runoff out through catchment_sum, sum of squares, backward:
    loss and all parameter gradients are bitwise those of the graph fed with the gathered [T, N] forcing.  And the engine's own
    catchment sums under a mapped forward."""
    from lgar_py_amd import CatchmentMap, catchment_sum
    from lgar_py_amd.autograd import lgar_series
    n = 130
    idx = J.index(n, seed=7)
    cmap = CatchmentMap(idx, n_catchments=J.B, weights=np.random.default_rng(4).random(n) + 0.5)
    fm = cmap.forcing_map()
    assert (fm.M, fm.B) == (n, J.B) and fm.index.device.type == "cuda"
    pr, pe = J.forcing()
    cols = J.soil(n, 11)

    def graph(forcing, **kw):
        P = [_cuda(c).requires_grad_(i < 3) for i, c in enumerate(cols)]
        statuses = []
        ro, _ = lgar_series(*P, _cuda(forcing[0]), _cuda(forcing[1]), check=False, status_out=statuses,
                            **dict(J.KW, dtype=torch.float64, **kw))
        catch = catchment_sum(ro, cmap, statuses[0])
        loss = (catch ** 2).sum()
        loss.backward()
        return loss.detach(), catch.detach(), [p.grad for p in P[:3]], statuses

    want = graph(J.gathered(pr, pe, idx))
    got = graph((pr, pe), forcing_map=fm)
    assert float(want[0]) > 0.0 and all(float(g.abs().max()) > 0.0 for g in want[2])
    assert float(want[1][:, J.B - 1].max()) > float(want[1][:, 0].max()) >= 0.0
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    for a, b in zip(got[2], want[2]):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert all(torch.equal(a, b) for a, b in zip(got[3], want[3])) and len(got[3]) == 2
    # forward(catchments=..., catchment=..., forcing_map=...)
    for dtype in (torch.float32, torch.float64):
        a = _engine(n, cols=cols, dtype=dtype).forward(*map(_cuda, J.gathered(pr, pe, idx)), catchments=cmap, catchment=("runoff",),
                                                       check=False)
        b = _engine(n, cols=cols, dtype=dtype).forward(_cuda(pr), _cuda(pe), catchments=cmap, catchment=("runoff",), check=False,
                                                       forcing_map=fm)
        assert tuple(a["catchment:runoff"].shape) == (J.T, J.B) and float(a["catchment:runoff"][:, J.B - 1].max()) > 0.0
        assert torch.equal(a["catchment:runoff"], b["catchment:runoff"]) and torch.equal(a["catchment:weight"], b["catchment:weight"])
        assert torch.equal(a["runoff"], b["runoff"])


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_raw_c_abi_and_the_engine_after_a_mapped_call():
    """The entry points' own checks: a map needs forcing_columns >= 1 and no divisibility; without a map the rule stays.  After a
    mapped forward whose B does not divide N, reset(), soil_moisture(), run_with_soil_moisture() and a plain [T, N] forward work
    and equal a fresh engine's bit for bit."""
    from lgar_py_amd import _capi
    n = 130
    lib = _capi.load()
    idx = J.index(n)
    pr, pe = J.forcing()
    fm = _fmap(idx)
    eng = _engine(n, dtype=torch.float32)
    d = _capi.LgarDims()
    C.memmove(C.byref(d), C.byref(eng.dims), C.sizeof(d))
    prd, ped = _cuda(pr).float().contiguous(), _cuda(pe).float().contiguous()
    d.n_steps, d.forcing_group = J.T, 1

    def call(dims, with_map):
        fo = _capi.LgarForcing(prd.data_ptr(), ped.data_ptr(), fm.index.data_ptr() if with_map else None)
        rc = lib.lgar_forward(C.byref(dims), C.byref(eng._params), C.byref(eng._state), C.byref(fo), None, eng.status.data_ptr(),
                              _capi.F32, None)
        torch.cuda.synchronize()
        return rc
    d.forcing_columns = 0
    assert call(d, True) == -1      # LGAR_E_ARG: a map needs the number of forcing columns
    d.forcing_columns = 7
    assert call(d, False) == -1     # without a map 7 must divide 130, as ever
    d.forcing_columns = J.B
    assert n % J.B == 0 and call(d, True) == 0
    want = J.run(_engine(n, dtype=torch.float32), *J.gathered(pr, pe, idx))
    J.same(J.state(eng), want, J.STATE)
    # B = 5 does not divide N = 128
    n = 128
    idx = J.index(n)
    eng, fresh = _engine(n), _engine(n)
    eng.forward(_cuda(pr), _cuda(pe), forcing_map=_fmap(idx), check=False)
    assert n % eng.dims.forcing_columns != 0
    eng.reset()
    J.same(J.state(eng), J.state(fresh))
    assert torch.equal(eng.soil_moisture(), fresh.soil_moisture())
    g = J.gathered(pr, pe, idx)
    J.same(J.run(eng, *g), J.run(fresh, *g))
    assert torch.equal(eng.soil_moisture(what="storage"), fresh.soil_moisture(what="storage"))
    # run_with_soil_moisture(forcing_map=...) against the gathered forcing
    a = _engine(n).run_with_soil_moisture(_cuda(pr), _cuda(pe), every=16, forcing_map=_fmap(idx), check=False)
    b = _engine(n).run_with_soil_moisture(*map(_cuda, g), every=16, check=False)
    assert all(torch.equal(a[k], b[k]) for k in b) and tuple(a["soil_moisture"].shape) == (3, 3, n)
