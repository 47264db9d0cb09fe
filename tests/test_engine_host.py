"""CPU: lgar_py_amd.engine.LgarEngine's own host code -- argument checks, forcing layouts, output buffers, the basin-scratch
budget, the tangent's checks, the sibling constructor, the status message -- run through devsim.SimEngine, the same class with
the device-code simulator (tests/devsim) in the HIP library's place.  Three layers, 2..4 columns, 12 rows of synth1_phil around
its first storm."""
import hashlib
import os

import numpy as np
import pytest
import torch

from _golden import engine_keywords
from conftest import GOLDEN

PARAMS = ("alpha", "n", "ksat", "theta_e", "theta_r", "thickness")
SCALE = np.array([1.0, 0.5, 0.8, 1.3])  # rainfall per column: the columns differ
T = 12


def _golden(name="synth1_phil"):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


def _engine(ncol=4, name="synth1_phil", **kw):
    import devsim
    g = _golden(name)
    return devsim.SimEngine(*[g[k] for k in PARAMS], n_columns=ncol, **dict(engine_keywords(g), **kw))


def _forcing(ncol=4, rows=T):
    f = _golden()["forcing"][4:4 + rows]  # two dry rows, five of rain, five dry
    return f[:, 0:1] * SCALE[None, :ncol], np.repeat(f[:, 1:2], ncol, 1)


def _state(eng):
    return [t.clone() for t in (eng.depth, eng.theta, eng.psi, eng.k, eng.dzdt, eng.flags, eng.n_fronts, eng.scalars,
                                eng.totals, eng.status)]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# forcing layout ---------------------------------------------------------------------------------------------------------
def test_forcing_layouts_are_accepted_and_broadcast_gives_the_bits_of_replicated_forcing():
    pr, pe = _forcing()
    full = _engine()
    want = full.forward(np.repeat(pr[:, :1], 4, 1), pe, series=("infiltration", "AET"))
    assert float(want["infiltration"].sum()) > 0.0
    one = _engine()
    got = one.forward(pr[:, :1], pe[:, :1], series=("infiltration", "AET"))  # [T, 1]: one series for every column
    assert all(torch.equal(got[nm], want[nm]) for nm in want) and _same(_state(one), _state(full))
    assert (one.dims.forcing_columns, one.dims.forcing_group, one.dims.n_steps) == (1, 1, T)
    # [T, Nf] with forcing_group: columns (0, 1) read forcing column 0, (2, 3) column 1
    rep = _engine().forward(pr[:, [0, 0, 1, 1]], pe, series=("infiltration",))
    grp = _engine()
    out = grp.forward(pr[:, :2], pe[:, :2], series=("infiltration",), forcing_group=2)
    assert torch.equal(out["infiltration"], rep["infiltration"]) and (grp.dims.forcing_columns, grp.dims.forcing_group) == (2, 2)
    # [T, Nf] alone: column c reads forcing column c % Nf
    mod = _engine().forward(pr[:, :2], pe[:, :2], series=("infiltration",))
    assert torch.equal(mod["infiltration"], _engine().forward(pr[:, [0, 1, 0, 1]], pe, series=("infiltration",))["infiltration"])
    # a 1-D pair is one row
    row = _engine()
    out = row.forward(pr[2], pe[2], series=("precip",))
    assert tuple(out["precip"].shape) == (1, 4) and row.dims.n_steps == 1
    assert torch.equal(out["precip"], _engine().forward(pr[2:3], pe[2:3], series=("precip",))["precip"])


def test_bad_forcing_layouts_raise():
    from lgar_py_amd import LgarError
    pr, pe = _forcing()
    eng = _engine()
    before = _state(eng)
    with pytest.raises(LgarError, match="forcing must be"):
        eng.forward(pr, pe[:, :2])  # precip and pet shaped differently
    with pytest.raises(LgarError, match="forcing must be"):
        eng.forward(pr[:-1], pe)
    with pytest.raises(LgarError, match="forcing must be"):
        eng.forward(pr[:, :3], pe[:, :3])  # Nf = 3 does not divide N // forcing_group = 4
    with pytest.raises(LgarError, match="forcing must be"):
        eng.forward(pr[:, :2], pe[:, :2], forcing_group=4)  # ... nor 2 the one group of four
    with pytest.raises(LgarError, match="forcing must be"):
        eng.forward(pr[:, :1], pe[:, :1], forcing_group=3)  # forcing_group does not divide N
    with pytest.raises(LgarError, match="forcing must be"):
        eng.forward(np.zeros((3, 5)), np.zeros((3, 5)))  # wrong column count
    assert _same(_state(eng), before)  # a refused call launches nothing


# out= ---------------------------------------------------------------------------------------------------------------
def test_out_buffers_are_written_in_place_and_checked():
    from lgar_py_amd import LgarError
    pr, pe = _forcing()
    want = _engine().forward(pr, pe, series=("infiltration", "precip"))
    eng = _engine()
    buf = torch.full((T, 4), -1.0, dtype=torch.float64)
    got = eng.forward(pr, pe, series=("infiltration", "precip"), out={"infiltration": buf})
    assert got["infiltration"] is buf and torch.equal(buf, want["infiltration"]) and torch.equal(got["precip"], want["precip"])
    for bad in (torch.zeros(T, 3, dtype=torch.float64), torch.zeros(T + 1, 4, dtype=torch.float64),
                torch.zeros(T, 4, dtype=torch.float32), torch.zeros(4, T, dtype=torch.float64).T):
        fresh = _engine()
        before = _state(fresh)
        with pytest.raises(LgarError, match="bad output buffer for series 'infiltration'"):
            fresh.forward(pr, pe, series=("infiltration",), out={"infiltration": bad})
        assert _same(_state(fresh), before)


# basin= -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [None, [0.5, 2.0, 1.0, 0.25]], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("scratch", [0, 1 << 20], ids=["no_scratch", "scratch"])
def test_basin_sums_equal_the_column_sums_of_the_stored_series(weights, scratch):
    pr, pe = _forcing()
    stored = _engine().forward(pr, pe, series=("infiltration", "precip"))
    eng = _engine(basin_scratch_bytes=scratch)
    out = eng.forward(pr, pe, series=("infiltration",), basin=("infiltration", "precip"), weights=weights)  # precip: basin only
    assert sorted(out) == ["basin:infiltration", "basin:precip", "infiltration"]
    assert sorted(eng._basin_scratch[1]) == (["precip"] if scratch else [])
    w = torch.ones(4, dtype=torch.float64) if weights is None else torch.tensor(weights, dtype=torch.float64)
    for nm in ("infiltration", "precip"):
        want = (stored[nm] * w[None, :]).sum(1)
        got = out["basin:" + nm]
        assert got.dtype == torch.float64 and tuple(got.shape) == (T,)
        assert float(want.abs().max()) > 0.0
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max()), nm


def test_basin_weights_of_the_wrong_length_raise():
    from lgar_py_amd import LgarError
    pr, pe = _forcing()
    with pytest.raises(LgarError, match=r"weights must be \[N\]"):
        _engine().forward(pr, pe, basin=("runoff",), weights=[1.0, 2.0, 3.0])


def test_basin_scratch_budget_and_lifetime():
    """Room for one [T, N] series but not two: the first basin-only name gets a scratch series, the second none; another T
    replaces the buffers; release_scratch() empties them."""
    pr, pe = _forcing()
    one = T * 4 * 8
    eng = _engine(basin_scratch_bytes=2 * one - 1)
    assert _engine()._basin_scratch == (0, {}) and _engine().basin_scratch_bytes == 0  # (the simulator's default: never)
    eng.forward(pr, pe, series=(), basin=("precip", "infiltration"))
    rows, bufs = eng._basin_scratch
    assert rows == T and list(bufs) == ["precip"] and tuple(bufs["precip"].shape) == (T, 4)
    kept = bufs["precip"]
    eng.forward(pr, pe, series=(), basin=("infiltration", "precip"))  # same T: the buffer is kept, still no room for a second
    assert list(eng._basin_scratch[1]) == ["precip"] and eng._basin_scratch[1]["precip"] is kept
    eng.forward(pr[:5], pe[:5], series=(), basin=("infiltration", "precip"))  # another T: new buffers, room for both now
    rows, bufs = eng._basin_scratch
    assert rows == 5 and sorted(bufs) == ["infiltration", "precip"] and all(tuple(b.shape) == (5, 4) for b in bufs.values())
    eng.release_scratch()
    assert eng._basin_scratch == (0, {})


# tangent() ----------------------------------------------------------------------------------------------------------
def _grouped_engine(differ=False):
    """Four columns that are two soil columns twice over (share = 2)."""
    import devsim
    g = _golden()
    P = {k: np.repeat(np.asarray(g[k], dtype=np.float64)[:, None], 4, 1) for k in PARAMS}
    P["ksat"][:, 2:] *= 1.1
    if differ:
        P["n"][1, 1] *= 1.01
    return devsim.SimEngine(*[P[k] for k in PARAMS], **engine_keywords(g))


def test_tangent_refuses_what_the_kernels_would_misread():
    from lgar_py_amd import LgarError
    pr, pe = _forcing()
    d = {"ksat": np.ones((3, 4))}
    eng = _grouped_engine()
    for share in (1, 33, -2, 3):  # outside 2..32, or not dividing N = 4
        with pytest.raises(LgarError, match="share must be 0 or 2..32"):
            eng.tangent(d, pr[:, :1], pe[:, :1], share=share)
    with pytest.raises(LgarError, match="share=2 needs identical soil parameters within each group of 2 columns"):
        _grouped_engine(differ=True).tangent(d, pr[:, :1], pe[:, :1], share=2)
    with pytest.raises(LgarError, match="share=2 needs the columns of a group to read the same forcing column"):
        eng.tangent(d, pr, pe, share=2)  # forcing_group 1, four forcing columns
    with pytest.raises(LgarError, match="share=2 needs the columns of a group to read the same forcing column"):
        _engine(6).tangent({}, np.zeros((T, 2)), np.zeros((T, 2)), forcing_group=3, share=2)
    with pytest.raises(LgarError, match=r"w_runoff must be \[T, N\] like the forcing"):
        eng.tangent(d, pr, pe, w_runoff=np.ones((T, 1)))
    with pytest.raises(LgarError, match=r"w_perc must be \[T, N\] like the forcing"):
        eng.tangent(d, pr[:, :1], pe[:, :1], w_perc=np.ones((T, 4)))
    with pytest.raises(LgarError, match=r"direction\['n'\] must be \[L, N\]"):
        eng.tangent({"n": np.ones((3, 1))}, pr, pe)
    with pytest.raises(LgarError, match="forcing must be"):
        eng.tangent(d, pr, pe[:, :2])


def test_tangent_without_sharing_gives_the_bits_it_gave_before_the_engines_were_one():
    """share = 0 on grad_synth0_12h, every one-hot direction, unit weights on the runoff: sha256 over gradient, tangent series
    and status as the simulator's own numpy front-end computed them before it became a subclass of LgarEngine."""
    g = _golden("grad_synth0_12h")
    eng = _engine(1, "grad_synth0_12h")
    f = g["forcing"]
    h = hashlib.sha256()
    for key in ("alpha", "n", "ksat"):
        for k in range(3):
            gr, ser, st = eng.tangent({key: np.eye(3)[:, k:k + 1]}, f[:, 0:1], f[:, 1:2], w_runoff=np.ones((f.shape[0], 1)),
                                      want_series=True)
            assert gr.dtype == torch.float64 and st.dtype == torch.int32 and tuple(ser.shape) == (f.shape[0], 1)
            h.update(gr.numpy().tobytes() + ser.numpy().tobytes() + st.numpy().tobytes())
    assert eng.dims.tangent_share == 0
    assert h.hexdigest() == "bb8b53c281e21eedef4f598c3ef5ba87ffb8eb2fd94234dc7155dff44ae5cd2e"


# constructor --------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_rejected():
    """(tests/test_gpu_parity.py::test_bad_arguments_are_rejected, the part that is the wrapper's)"""
    import devsim
    from lgar_py_amd import LgarError
    with pytest.raises(LgarError, match="soil layers"):
        devsim.SimEngine([1e-2] * 7, [1.5] * 7, [1.0] * 7, [0.4] * 7, [0.1] * 7, [10.0] * 7, n_columns=4)  # 7 layers: not compiled in
    with pytest.raises(LgarError, match="n > 1"):
        devsim.SimEngine([1e-2] * 3, [1.0, 1.5, 1.5], [1.0] * 3, [0.4] * 3, [0.1] * 3, [10.0] * 3, n_columns=4)
    with pytest.raises(LgarError, match="theta_e > theta_r"):
        devsim.SimEngine([1e-2] * 3, [1.5] * 3, [1.0] * 3, [0.4, 0.05, 0.4], [0.1] * 3, [10.0] * 3, n_columns=4)
    with pytest.raises(LgarError, match="n_columns is required"):
        devsim.SimEngine([1e-2] * 3, [1.5] * 3, [1.0] * 3, [0.4] * 3, [0.1] * 3, [10.0] * 3)
    with pytest.raises(LgarError, match="front_slots must be in 4..32"):
        _engine(front_slots=3)
    with pytest.raises(LgarError, match="forward_lanes must be"):
        _engine(forward_lanes=3)
    with pytest.raises(LgarError, match="forward_lanes=8 cannot be honoured"):
        _engine(forward_lanes=8, dtype=torch.float32)
    with pytest.raises(TypeError, match="unexpected keyword"):
        _engine(geff="f32")
    with pytest.raises(LgarError):
        _engine().forward(torch.zeros(3, 5), torch.zeros(3, 5))  # wrong column count


def test_mixed_precision_is_an_fp64_fast_mode_option():
    """(tests/test_gpu_mixed.py's test of the same name)"""
    import devsim
    from lgar_py_amd import LgarError
    from lgar_py_amd import workloads as W
    args = [W.PHILLIPSBURG[k] for k in PARAMS]
    with pytest.raises(LgarError, match="mixed mode of the fp64 fast searches"):
        devsim.SimEngine(*args, n_columns=4, dtype=torch.float32, geff_precision="f32")
    with pytest.raises(LgarError, match="mixed mode of the fp64 fast searches"):
        devsim.SimEngine(*args, n_columns=4, dtype=torch.float64, search_mode=0, geff_precision="f32")
    with pytest.raises(LgarError, match="geff_precision must be 'native' or 'f32'"):
        devsim.SimEngine(*args, n_columns=4, geff_precision="half")
    assert devsim.SimEngine(*args, n_columns=4, geff_precision="f32").dims.geff_mode == 1


def test_tangent_sibling_takes_the_engines_settings_and_what_the_tangent_kernels_have():
    import devsim
    eng = _engine(2, geff_precision="f32", forward_lanes=8, search_mode=2, front_slots=12, bottom_mode=1, iter_cap=77)
    assert (eng.dims.geff_mode, eng.dims.forward_lanes) == (1, 8)
    eng.dims.ponded_depth_max = 1.25  # (what model.update_soil_parameters does)
    rep = lambda t: t.repeat_interleave(3, dim=1)
    sib = eng.like(*[rep(getattr(eng, k)) for k in PARAMS], with_state=False)
    assert type(sib) is devsim.SimEngine and sib._state is None and (sib.L, sib.N) == (3, 6)
    assert sib.dtype == eng.dtype and sib.device == eng.device
    a, b = sib.dims, eng.dims
    assert (a.geff_mode, a.forward_lanes) == (0, 0)
    for field in ("front_slots", "search_mode", "bottom_mode", "iter_cap", "use_closed_form_G", "dt_h", "num_subcycles", "nint",
                  "initial_psi", "wilting_point_psi", "frozen_factor", "ponded_depth_max", "n_giuh"):
        assert getattr(a, field) == getattr(b, field), field
    assert (a.front_slots, a.search_mode, a.bottom_mode, a.iter_cap, a.ponded_depth_max) == (12, 2, 1, 77, 1.25)
    assert list(a.giuh) == list(b.giuh)
    twin = eng.like(*[getattr(eng, k) for k in PARAMS])  # with state: the settings as they are
    assert (twin.dims.geff_mode, twin.dims.forward_lanes, twin.front_slots) == (1, 8, 12) and twin._state is not None
    f32 = _engine(2, dtype=np.float32).like(*[rep(getattr(eng, k)) for k in PARAMS], with_state=False)
    assert f32.dtype == torch.float32 and f32.alpha.dtype == torch.float32


# status -------------------------------------------------------------------------------------------------------------
def test_check_status_names_the_faults_like_the_product():
    from lgar_py_amd import LgarStatusError, _capi
    g = _golden("crash_insert_water_bench_col2")
    crash = int(g["crash_step"])
    f = g["forcing"][:crash + 1]
    pr = f[:, 0:1] * np.array([[1.0, 0.0, 1.0]])  # column 1 never sees rain
    eng = _engine(3, "crash_insert_water_bench_col2")
    eng.forward(pr, np.repeat(f[:, 1:2], 3, 1), series=())  # (the simulator's forward() leaves the raising to the caller)
    st = eng.status.tolist()
    assert st[0] != 0 and st[1] == 0 and st[2] == st[0]
    names = ", ".join(nm for bit, nm in _capi.STATUS_NAMES.items() if st[0] & bit)
    assert names
    with pytest.raises(LgarStatusError) as e:
        eng.check_status()
    assert str(e.value) == "2 of 3 columns faulted (%s); first column 0, max status %d" % (names, st[0])
    with pytest.raises(LgarStatusError):
        eng.raise_for_status(eng.status.clone())
    with pytest.raises(LgarStatusError):
        eng.forward(pr[:1], pr[:1] * 0, check=True)
    ok = _engine()
    ok.forward(*_forcing(), check=True)
    ok.check_status()


# what the simulator does not have -------------------------------------------------------------------------------------
def test_entry_points_the_simulator_lacks_raise():
    from lgar_py_amd import LgarError
    pr, pe = _forcing()
    eng = _engine()
    with pytest.raises(LgarError, match="simulator has no basin sums of the soil moisture"):
        eng.soil_moisture(basin=True)
    with pytest.raises(LgarError, match="simulator has no basin sums of the soil moisture"):
        eng.soil_moisture(weights=[1.0, 2.0, 3.0, 4.0], basin=torch.zeros(3, dtype=torch.float64))
    with pytest.raises(LgarError, match="simulator has no lgar_cooperating_lanes"):
        eng.cooperating_lanes()
    with pytest.raises(LgarError, match="with_state=False"):
        eng.like(*[getattr(eng, k) for k in PARAMS], with_state=False).forward(pr, pe)


# ... and what it has: the post-processing entry points, from the host build of their headers (tests/post_host) -----------
EDGES = [0.0, 10.0, 50.0, 1000.0]  # the last bin reaches below the column: it is divided by its in-column width
F64_F32 = pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])


def _profile(eng, edges, what):
    """The numpy definition on the engine's own front table, rounded once to the engine's dtype."""
    from post_host import moisture as MH
    fr = eng.fronts()
    ref = MH.profile_ref(fr["depth"], fr["theta"], fr["layer"], fr["n_fronts"], eng.thickness.numpy(), edges, what)
    return ref.astype(fr["depth"].dtype)


@F64_F32
def test_soil_moisture_equals_the_numpy_definition_bit_for_bit(dtype):
    from post_host import same_bits
    pr, pe = _forcing()
    eng = _engine(dtype=dtype)
    eng.forward(pr, pe)
    assert int(eng.n_fronts.max()) > eng.L and not bool(eng.status.any())
    for edges in (None, EDGES):
        for what in ("theta", "storage"):
            got = eng.soil_moisture(edges, what)
            assert got.dtype == dtype and tuple(got.shape) == (3, 4)
            assert same_bits(got.numpy(), _profile(eng, edges, what)), (edges, what)
    out = torch.empty(3, 4, dtype=dtype)
    assert eng.soil_moisture(EDGES, "storage", out=out) is out and torch.equal(out, got)


@F64_F32
@pytest.mark.parametrize("rows", [12, 10], ids=["whole_windows", "ragged_tail"])
def test_windows_with_snapshots_equal_one_forward(rows, dtype):
    """(tests/test_gpu_moisture.py's window test at the smallest shape.)  every=4: every series, the state, the status and the
    run totals are those of ONE forward() over the same rows; snapshot r is soil_moisture() of an engine stepped 4 (r + 1) rows."""
    names = ("runoff", "infiltration", "AET", "ending_volume")
    pr, pe = _forcing(rows=rows)
    one, eng, step = _engine(dtype=dtype), _engine(dtype=dtype), _engine(dtype=dtype)
    want = one.forward(pr, pe, series=names)
    got = eng.run_with_soil_moisture(pr, pe, every=4, edges=EDGES, what="storage", series=names)
    assert sorted(got) == sorted(names + ("soil_moisture",)) and all(torch.equal(got[nm], want[nm]) for nm in names)
    assert float(want["infiltration"].sum()) > 0.0
    a, b = _state(eng), _state(one)
    assert _same(a[:8] + a[9:], b[:8] + b[9:]) and torch.equal(eng.totals[:8], one.totals[:8])
    assert float(one.totals[:8].abs().sum()) > 0.0
    assert tuple(got["soil_moisture"].shape) == (rows // 4, 3, 4)
    for r in range(rows // 4):
        step.forward(pr[4 * r:4 * r + 4], pe[4 * r:4 * r + 4])
        assert torch.equal(got["soil_moisture"][r], step.soil_moisture(EDGES, "storage")), r


def _catchment_job():
    """Six columns of crash_insert_water_bench_col2 under rain scaled per column (the unscaled ones fault where the reference
    crashes), spun up to three rows before that step; ids in a non-contiguous order with an empty catchment (1) and a column of
    none; 12 rows."""
    import devsim
    g = _golden("crash_insert_water_bench_col2")
    crash = int(g["crash_step"])
    scale = np.array([[1.0, 0.95, 1.0, 0.9, 0.3, 0.95]])
    f = g["forcing"]
    pr, pe = f[:, 0:1] * scale, np.repeat(f[:, 1:2], 6, 1)
    eng = _engine(6, "crash_insert_water_bench_col2")
    eng.forward(pr[:crash - 3], pe[:crash - 3], series=())
    assert not bool(eng.status.any())
    cmap = devsim.SimCatchmentMap([2, 0, -1, 2, 0, 2], n_catchments=4, weights=[0.5, 2.0, 1.0, 0.25, 1.5, 0.125], device="cpu")
    routing = devsim.SimCatchmentRouting(list(g["giuh_ordinates"]), device="cpu")
    return eng, cmap, routing, pr[crash - 3:crash + 9], pe[crash - 3:crash + 9]


def _check_catchment_block(res, eng, cmap, routing, queues):
    """One forward()'s catchment sums, weight sums and routed sums against the numpy definitions; queues: {name: the queue the
    call started from}, replaced by the queue it must have left."""
    from post_host import catchment as CH, route as RH, same_bits
    st = eng.status.numpy()
    for nm in ("runoff", "giuh_runoff"):
        sums, wsum = CH.sums_ref(res[nm].numpy(), cmap.offsets_host, cmap.order_host, cmap.weights_host.numpy(), st)
        assert same_bits(res["catchment:" + nm].numpy(), sums) and same_bits(res["catchment:weight"].numpy(), wsum), nm
        y, queues[nm] = RH.route_ref(sums, routing.ordinates_host.numpy(), queues.get(nm))
        assert same_bits(res["catchment:routed:" + nm].numpy(), y) and same_bits(routing.queue_of(nm).numpy(), queues[nm]), nm
    return wsum


def test_catchment_sums_and_routing_through_forward_in_one_call_and_in_two():
    """forward(catchments=, catchment=, routing=) on the simulator: the [T, B] sums equal sums_ref of the returned series with
    the engine's status (the faulted column drops out of every row), the weight sums are those of the columns left, the routed
    sums equal route_ref; 12 rows as 5 + 7 give the bits of one call, the queue carried across the cut included."""
    names = ("runoff", "giuh_runoff")
    eng, cmap, routing, pr, pe = _catchment_job()
    assert cmap.order is not None and cmap.sizes.tolist() == [2, 0, 3, 0]
    one = eng.forward(pr, pe, series=names, catchments=cmap, catchment=names, routing=routing)
    st = eng.status.tolist()
    assert st[0] != 0 and st[2] == st[0] and st[1] == st[3] == st[4] == st[5] == 0  # a member of catchment 2, and the column of none
    queues = {}
    wsum = _check_catchment_block(one, eng, cmap, routing, queues)
    assert wsum.tolist() == [3.5, 0.0, 0.375, 0.0]
    assert bool((one["catchment:runoff"][:5, [0, 2]] > 0).all()) and bool((one["catchment:runoff"][:, [1, 3]] == 0).all())
    assert bool((one["catchment:routed:giuh_runoff"][:, [0, 2]] > 0).all())  # (the queues are still draining at the end)
    # ... and cut after five rows: the fault (row 3) lies before the cut, so every row is summed over the same columns
    eng2, cmap2, routing2, _, _ = _catchment_job()
    queues2, parts = {}, []
    for lo, hi in ((0, 5), (5, 12)):
        parts.append(eng2.forward(pr[lo:hi], pe[lo:hi], series=names, catchments=cmap2, catchment=names, routing=routing2))
        _check_catchment_block(parts[-1], eng2, cmap2, routing2, queues2)
    for key in ("catchment:runoff", "catchment:giuh_runoff", "catchment:routed:runoff", "catchment:routed:giuh_runoff"):
        assert torch.equal(torch.cat([p[key] for p in parts]), one[key]), key
    assert all(torch.equal(routing2.queue_of(nm), routing.queue_of(nm)) for nm in names)
    assert torch.equal(parts[-1]["catchment:weight"], one["catchment:weight"])


@F64_F32
@pytest.mark.parametrize("T", [0, 1, 6])
def test_catchment_sum_under_autograd(T, dtype):
    import devsim
    from lgar_py_amd import catchment_sum
    from post_host import catchment as CH, same_bits
    rng = np.random.default_rng(T)
    ids, w = [2, 0, -1, 2, 0, 2], rng.random(6)
    status = torch.tensor([0, 0, 0, 4, 128, 0], dtype=torch.int32)
    cmap = devsim.SimCatchmentMap(ids, n_catchments=3, weights=w, device="cpu")
    series = torch.tensor(rng.standard_normal((T, 6)), dtype=dtype, requires_grad=True)
    grad = torch.tensor(rng.standard_normal((T, 3)))
    out = catchment_sum(series, cmap, status)
    wd = cmap.weights(dtype).numpy()
    assert same_bits(out.detach().numpy(), CH.sums_ref(series.detach().numpy(), cmap.offsets_host, cmap.order_host, wd, status.numpy())[0])
    out.backward(grad)
    assert series.grad.dtype == dtype
    assert same_bits(series.grad.numpy(), CH.spread_ref(grad.numpy(), ids, wd, status.numpy(), series.detach().numpy().dtype))


@pytest.mark.parametrize("per", [False, True], ids=["shared", "per_catchment"])
@pytest.mark.parametrize("K", [1, 5])
@pytest.mark.parametrize("T", [0, 1, 6])
def test_catchment_route_under_autograd(T, K, per, monkeypatch):
    """Through a routing object (its ordinates are constants) and through an ordinates tensor that takes a gradient."""
    import devsim
    from lgar_py_amd import catchment_route, catchments
    from post_host import route as RH, same_bits
    monkeypatch.setattr(catchments, "CatchmentRouting", devsim.SimCatchmentRouting)  # (what catchment_route builds for a tensor)
    rng = np.random.default_rng(10 * T + K)
    g = torch.tensor(rng.random((3, K) if per else K), requires_grad=True)
    gk = g.detach().numpy().T if per else g.detach().numpy()  # the device layout: [K, B] or [K]
    x = torch.tensor(rng.standard_normal((T, 3)), requires_grad=True)
    gy, q_in = torch.tensor(rng.standard_normal((T, 3))), torch.tensor(rng.standard_normal((K, 3)))
    y = catchment_route(x, g, queue=q_in)
    assert same_bits(y.detach().numpy(), RH.route_ref(x.detach().numpy(), gk, q_in.numpy())[0])
    y.backward(gy)
    assert same_bits(x.grad.numpy(), RH.adjoint_ref(gy.numpy(), gk))
    gg = torch.from_numpy(RH.ordinate_grad_ref(x.detach().numpy(), gy.numpy(), K))  # [K, B]
    assert torch.equal(g.grad, gg.t().contiguous() if per else gg.sum(dim=1))
    x2 = x.detach().clone().requires_grad_(True)
    y2 = catchment_route(x2, devsim.SimCatchmentRouting(g.detach(), n_catchments=3, device="cpu"))
    assert same_bits(y2.detach().numpy(), RH.route_ref(x.detach().numpy(), gk)[0])
    y2.backward(gy)
    assert torch.equal(x2.grad, x.grad)
