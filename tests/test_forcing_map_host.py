"""CPU: the forcing map (LgarForcing.column_map, forcing.ForcingMap) -- N soil columns read [T, B] forcing through a
per-column index.  The device code runs through devsim.SimEngine (the kernels' own source compiled for the host, argument
blocks by the library's make_args / make_targs), the host logic is the product's.  Every equality is bitwise against the same
engine settings run with the gathered forcing precip[:, index] (tests/_forcing_map_job.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _forcing_map_job as J

N = 70


def _engine(n=N, seed=3, cols=None, **kw):
    import devsim
    return devsim.SimEngine(*(J.soil(n, seed) if cols is None else cols), **dict(J.KW, **kw))


def _fmap(idx, **kw):
    from lgar_py_amd import ForcingMap
    return ForcingMap(idx, device="cpu", **dict(dict(n_forcing=J.B), **kw))


# 1 ------------------------------------------------------------------------------------------------------------------------
def test_forcing_map_validation():
    from lgar_py_amd import CatchmentMap, ForcingMap, LgarError
    idx = J.index(N)
    fm = _fmap(idx)
    assert (fm.M, fm.B) == (N, J.B) and fm.index.dtype == torch.int32 and fm.index.tolist() == idx.tolist()
    assert ForcingMap(torch.tensor([0, 2, 1]), device="cpu").B == 3 and ForcingMap(np.array([1, 0], np.uint8), device="cpu").M == 2
    with pytest.raises(LgarError, match=r"\[M\]"):
        ForcingMap(idx.reshape(2, -1), device="cpu")                 # 2-D
    with pytest.raises(LgarError, match="integers"):
        ForcingMap(idx.astype(np.float64), device="cpu")              # float
    with pytest.raises(LgarError, match="0 .. 4"):
        ForcingMap(np.where(idx == 2, -1, idx), n_forcing=J.B, device="cpu")  # negative entry
    with pytest.raises(LgarError, match="0 .. 3"):
        ForcingMap(idx, n_forcing=J.B - 1, device="cpu")              # entry >= n_forcing
    with pytest.raises(LgarError):
        ForcingMap(np.array([], dtype=np.int64), device="cpu")
    pr, pe = J.forcing()
    eng = _engine()
    before = J.state(eng)
    with pytest.raises(LgarError, match="forcing_map has 69 entries"):
        eng.forward(pr, pe, forcing_map=_fmap(idx[:-1]))                # wrong M for the engine
    with pytest.raises(LgarError, match="forcing_map has 70 entries"):
        eng.forward(pr, pe, forcing_map=fm, forcing_group=2)
    with pytest.raises(LgarError, match=r"forcing must be \[T, 5\]"):
        eng.forward(pr[:, :4], pe[:, :4], forcing_map=fm)               # wrong B for the forcing
    with pytest.raises(LgarError, match=r"forcing must be \[T, 5\]"):
        eng.forward(*J.gathered(pr, pe, idx), forcing_map=fm)           # (the gathered forcing AND a map)
    with pytest.raises(LgarError, match="same device as the engine"):
        eng.forward(pr, pe, forcing_map=ForcingMap(idx, n_forcing=J.B, device="meta"))  # map on another device
    with pytest.raises(LgarError, match="same device as the engine"):
        eng.forward(pr, pe, forcing_map=idx)                            # not a map at all
    with pytest.raises(LgarError, match=r"w_runoff must be \[T, 70\]"):
        eng.tangent({}, pr, pe, w_runoff=np.ones((J.T, J.B)), forcing_map=fm)  # the weights do not go through the map
    J.same(J.state(eng), before)                                        # a refused call launches nothing
    # CatchmentMap.forcing_map(): the map of its ids; a column of no catchment has no forcing
    cm = CatchmentMap(idx, n_catchments=J.B + 2, device="cpu")
    assert cm.forcing_map() is cm.forcing_map() and (cm.forcing_map().M, cm.forcing_map().B) == (N, J.B + 2)
    assert cm.forcing_map().index.tolist() == idx.tolist()
    with pytest.raises(LgarError, match="belong to no catchment"):
        CatchmentMap(np.where(idx == J.LONE, -1, idx), n_catchments=J.B, device="cpu").forcing_map()


# 2 ------------------------------------------------------------------------------------------------------------------------
FAMILIES = [dict(dtype=torch.float64, search_mode=1), dict(dtype=torch.float64, search_mode=2), dict(dtype=torch.float64, search_mode=0),
            dict(dtype=torch.float32, search_mode=1), dict(dtype=torch.float32, search_mode=2), dict(dtype=torch.float32, search_mode=0),
            dict(dtype=torch.float64, search_mode=1, geff_mode=1)]


@pytest.mark.parametrize("kw", FAMILIES, ids=lambda kw: "-".join("%s" % str(v).replace("torch.", "") for v in kw.values()))
def test_mapped_forward_equals_the_gathered_run_bit_for_bit(kw):
    """All ten series, the final front table, scalars, totals and status."""
    idx = J.index(N)
    pr, pe = J.forcing()
    want = J.run(_engine(**kw), *J.gathered(pr, pe, idx))
    J.forcing_matters(want, idx)
    eng = _engine(**kw)
    got = J.run(eng, pr, pe, forcing_map=_fmap(idx))
    J.same(got, want)
    assert (eng.dims.forcing_columns, eng.dims.forcing_group, eng.dims.n_steps) == (J.B, 1, J.T)


def test_precip_and_pet_both_go_through_the_map():
    """(The job above has synth_1's PET, zero: here the two arrays differ in every forcing column.)"""
    idx = J.index(N, seed=5)
    pr, pe = J.forcing(pet=0.004)
    want = J.run(_engine(), *J.gathered(pr, pe, idx))
    J.forcing_matters(want, idx)
    aet = want["AET"].double().sum(0).numpy()
    assert aet[idx == 0].min() > 0.0 and not np.array_equal(aet[idx == 0][:1], aet[idx == J.B - 1][:1])
    J.same(J.run(_engine(), pr, pe, forcing_map=_fmap(idx)), want)


# 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_forcing_group_two_reads_one_map_entry_per_pair(dtype):
    idx = J.index(N // 2, seed=1)
    pr, pe = J.forcing()
    want = J.run(_engine(dtype=dtype), *J.gathered(pr, pe, idx, group=2))
    J.forcing_matters(want, idx, group=2)
    J.same(J.run(_engine(dtype=dtype), pr, pe, forcing_map=_fmap(idx), forcing_group=2), want)


# 4 ------------------------------------------------------------------------------------------------------------------------
def test_a_corrupt_map_is_clamped():
    """Memory safety before meaning (CPU only: an out-of-range map is never given to a GPU).  A valid map whose device index is
    then overwritten with entries from -3 to B + 2: the run equals the one with the clamped index.  The forcing is rows 1 .. 48 of
    contiguous 50-row tensors, so that even an UNCLAMPED read (column -3 of the first row, column B + 2 of the last) would stay
    inside the allocation."""
    idx = J.index(N, seed=2)
    bad = idx.copy()
    bad[[0, 7, 20, 33, 69]] = [-3, J.B + 2, J.B, -1, 2 ** 31 - 1]
    pr50, pe50 = J.forcing(rows=50)
    pr50, pe50 = torch.tensor(pr50), torch.tensor(pe50)
    pr, pe = pr50[1:49], pe50[1:49]
    assert pr.is_contiguous() and pr.data_ptr() == pr50.data_ptr() + 8 * J.B
    fm = _fmap(idx)
    fm.index = torch.tensor(bad, dtype=torch.int32)
    clamped = np.clip(bad, 0, J.B - 1)
    assert (clamped != bad).sum() == 5
    want = J.run(_engine(), *J.gathered(pr.numpy(), pe.numpy(), clamped))
    J.forcing_matters(want, clamped)
    J.same(J.run(_engine(), pr, pe, forcing_map=fm), want)
    # the tangent reads the map the same way
    d = {"ksat": np.ones((3, N))}
    w = np.random.default_rng(0).random((J.T, N))
    a = _engine().tangent(d, pr, pe, w_runoff=w, forcing_map=fm)
    b = _engine().tangent(d, *J.gathered(pr.numpy(), pe.numpy(), clamped), w_runoff=w)
    assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and float(a[0].abs().max()) > 0.0


# 5 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(dtype=torch.float64), dict(dtype=torch.float32), dict(dtype=torch.float64, search_mode=2)],
                         ids=["fp64", "fp32", "fp64-chain"])
def test_tangent_mapped_equals_gathered(kw):
    """grad, tangent_runoff and status for a ksat direction with w_runoff [T, N] (and w_perc): the forcing goes through the map,
    the weights do not."""
    idx = J.index(N, seed=4)
    pr, pe = J.forcing()
    rng = np.random.default_rng(1)
    d = {"ksat": np.ones((3, N))}
    wr, wp = rng.random((J.T, N)), rng.random((J.T, N))
    want = _engine(**kw).tangent(d, *J.gathered(pr, pe, idx), w_runoff=wr, w_perc=wp, want_series=True)
    got = _engine(**kw).tangent(d, pr, pe, w_runoff=wr, w_perc=wp, want_series=True, forcing_map=_fmap(idx))
    ok = (want[2] & 0x7F) == 0
    by_col = want[1].double().abs().sum(0)
    assert float(by_col[torch.tensor(idx == J.B - 1) & ok].min()) > 0.0 and float(want[0].abs().max()) > 0.0
    assert not torch.equal(want[1][:, idx == 0][:, :1], want[1][:, idx == J.B - 1][:, :1])  # the forcing columns differ
    for a, b in zip(got, want):
        assert a.numpy().tobytes() == b.numpy().tobytes()


def test_tangent_with_forcing_group_three_reads_weight_column_c_over_three():
    """Each column three times over (adjacent lanes), forcing_group = 3: map entry and weight column c // 3, weights [T, N / 3]."""
    n0 = 24
    idx = J.index(n0, seed=6)
    pr, pe = J.forcing()
    cols = tuple(np.repeat(p, 3, axis=1) for p in J.soil(n0, 9))
    d = {"ksat": np.tile(np.array([1.0, 0.5, 2.0]), (3, n0))}  # three directions per column
    w = np.random.default_rng(2).random((J.T, n0))
    prg, peg = J.gathered(pr, pe, idx)
    want = _engine(cols=cols).tangent(d, prg, peg, w_runoff=w, want_series=True, forcing_group=3)
    got = _engine(cols=cols).tangent(d, pr, pe, w_runoff=w, want_series=True, forcing_group=3, forcing_map=_fmap(idx))
    assert float(want[0].abs().max()) > 0.0 and not torch.equal(want[0][0::3], want[0][1::3])
    for a, b in zip(got, want):
        assert a.numpy().tobytes() == b.numpy().tobytes()
    from lgar_py_amd import LgarError
    with pytest.raises(LgarError, match=r"w_runoff must be \[T, 24\]"):
        _engine(cols=cols).tangent(d, pr, pe, w_runoff=np.ones((J.T, 72)), forcing_group=3, forcing_map=_fmap(idx))


# 6 ------------------------------------------------------------------------------------------------------------------------
def test_lgar_series_with_a_map_gives_the_gradients_of_the_gathered_forcing(monkeypatch):
    import lgar_py_amd.autograd as A
    import lgar_py_amd.model as M
    import _sim_lgar_engine
    monkeypatch.setattr(A, "LgarEngine", A.LgarEngine)  # (restored after the test: install() is for a whole process)
    monkeypatch.setattr(M, "LgarEngine", M.LgarEngine)
    _sim_lgar_engine.install()
    n = 20
    idx = J.index(n, seed=7)
    pr, pe = J.forcing()
    cols = J.soil(n, 11)
    seen = []
    real = A.LgarEngine.forward

    def spy(self, precip, pet, *a, **kw):
        seen.append(tuple(torch.as_tensor(precip).shape))
        return real(self, precip, pet, *a, **kw)
    monkeypatch.setattr(A.LgarEngine, "forward", spy)

    def grads(forcing, **kw):
        P = [torch.tensor(c, requires_grad=i < 3) for i, c in enumerate(cols)]
        ro, pc = A.lgar_series(*P, torch.tensor(forcing[0]), torch.tensor(forcing[1]), check=False, **dict(J.KW, **kw))
        loss = (ro ** 2).sum() + (pc ** 2).sum()
        loss.backward()
        return loss.detach(), ro.detach(), [p.grad for p in P[:3]]

    want = grads(J.gathered(pr, pe, idx))
    got = grads((pr, pe), forcing_map=_fmap(idx))
    assert seen == [(J.T, n), (J.T, J.B)]  # with a map the forcing is not expanded
    assert float(want[0]) > 0.0 and all(float(g.abs().max()) > 0.0 for g in want[2])
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    for a, b in zip(got[2], want[2]):
        assert a.numpy().tobytes() == b.numpy().tobytes()
    # the direction-batched launch reuses the map as it is: parameter_vjp directly, all nine directions side by side
    eng = _engine(cols=cols)
    wanted = [(k, l) for k in A.KINDS for l in range(3)]
    w = torch.tensor(np.random.default_rng(3).random((J.T, n)))
    prg, peg = J.gathered(pr, pe, idx)
    a, sa = A.parameter_vjp(eng, torch.tensor(pr), torch.tensor(pe), w, None, wanted, check=False, forcing_map=_fmap(idx))
    b, sb = A.parameter_vjp(eng, torch.tensor(prg), torch.tensor(peg), w, None, wanted, check=False)
    assert torch.equal(sa, sb) and all(torch.equal(a[k], b[k]) for k in wanted)


# 7 ------------------------------------------------------------------------------------------------------------------------
def test_the_engine_goes_on_after_a_mapped_call_whose_forcing_columns_do_not_divide_n():
    """B = 5 forcing columns over N = 70 columns, and over N = 72, which 5 does not divide: after that mapped forward the
    engine's LgarDims carry a layout no unmapped call accepts.  reset() and a plain [T, N] forward equal a fresh engine's bit for bit, and the library's own
    check of the dims an entry point that reads no forcing performs (lgar_cooperating_lanes: host logic) accepts them."""
    from lgar_py_amd import _capi
    idx = J.index(N)
    pr, pe = J.forcing()
    prg, peg = J.gathered(pr, pe, idx)
    eng = _engine()
    eng.forward(pr, pe, forcing_map=_fmap(idx))
    assert eng.dims.forcing_columns == 5
    eng2 = _engine(n=72, seed=3)
    eng2.forward(pr, pe, forcing_map=_fmap(J.index(72)))
    assert 72 % eng2.dims.forcing_columns != 0
    lib = _capi.load()
    assert lib.lgar_cooperating_lanes(C.byref(eng2.dims), _capi.F64) == 64  # check_dims passes: 72 columns, 64 lanes each
    for e, n, i in ((eng, N, idx), (eng2, 72, J.index(72))):
        e.reset()
        fresh = _engine(n=n, seed=3)
        J.same(J.state(e), J.state(fresh))
        g = J.gathered(pr, pe, i)
        J.same(J.run(e, *g), J.run(fresh, *g))


# 8 ------------------------------------------------------------------------------------------------------------------------
def test_the_struct_and_the_entry_points_checks():
    """sizeof(LgarForcing) is three pointers and the two-argument construction engine.py uses leaves the map NULL.  The forcing
    layout rule by column_map, through the real library on the host: a call of zero steps returns before anything is launched or
    read, after the argument checks."""
    from lgar_py_amd import _capi
    assert C.sizeof(_capi.LgarForcing) == 24 and _capi.ABI_VERSION == 4
    fo = _capi.LgarForcing(1, 2)
    assert fo.column_map is None and (fo.precip, fo.pet) == (1, 2)
    lib = _capi.load()
    assert lib.lgar_abi_version() == 4
    d = _capi.make_dims(n_columns=130, n_layers=3)
    fake = 4096  # never read: n_steps = 0
    params = _capi.LgarParams(*[fake] * 6)
    state = _capi.LgarState(*([fake] * 9 + [None]))
    call = lambda f: lib.lgar_forward(C.byref(d), C.byref(params), C.byref(state), C.byref(f), None, fake, _capi.F64, None)
    mapped, plain = _capi.LgarForcing(fake, fake, fake), _capi.LgarForcing(fake, fake)
    d.forcing_columns = 0
    assert call(mapped) == -1 and call(plain) == 0     # a map needs the number of forcing columns
    d.forcing_columns = 5
    assert call(mapped) == 0 and call(plain) == 0      # 5 divides 130
    d.forcing_columns = 7
    assert call(mapped) == 0 and call(plain) == -1     # no divisibility with a map; the rule stays without one
    d.forcing_group = 4
    assert call(mapped) == -1                          # n_columns % forcing_group, as ever
    d.forcing_group, d.forcing_columns = 2, 9
    assert call(mapped) == 0 and call(plain) == -1
