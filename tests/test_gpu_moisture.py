"""GPU (-m gpu): the soil-moisture output -- lgar_soil_moisture through LgarEngine.soil_moisture / run_with_soil_moisture and
model.dpLGAR.soil_moisture.  The output is a pure function of the stored front table (include/lgar.h), so the kernel is held
BIT FOR BIT to the numpy statement of the definition (tests/moisture_host: profile_ref) evaluated on the same engine's
fronts(); against the reference it is held to the bound that the project's front-table bar (1e-6 relative on every depth and
theta, test_gpu_parity.py) implies for a bin."""
import ctypes as C
import os

import numpy as np
import pytest

from _golden import engine_keywords
from conftest import GOLDEN

from post_host import moisture as MH

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

NCOL = 67  # one full wave + a ragged tail
COLUMN_SEED = 8  # (the oracle keeps 65 and 67 of the 67 columns of the two fixtures valid: test_the_chosen_columns_...)


def perturbed_job(name, N=NCOL, seed=COLUMN_SEED):
    """The fixture's soil perturbed per column -- parameters +-10 % (workloads.perturbed_columns, which keeps the thickness) and
    thickness +-10 % here, so the layer bins differ from column to column -- under the fixture's rain scaled per column by
    U(0.5, 1): heavier rain than the fixture's drives a sixth of such columns out of the reference's domain of validity (the Se > 1
    fault of insert_water), more in fp32."""
    from lgar_py_amd import workloads as W
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    base = {k: g[k] for k in W.PARAM_KEYS + ("thickness",)}
    P = W.perturbed_columns(N, seed=seed, base=base)
    P["thickness"] = P["thickness"] * (1.0 + 0.10 * (2.0 * np.random.default_rng(seed + 1000).random(P["thickness"].shape) - 1.0))
    sc = W.forcing_scale(N, 0.5, 1.0, seed=seed + 1)
    pr = g["forcing"][:, 0:1] * sc[None, :]
    pe = g["forcing"][:, 1:2] * np.ones((1, N))
    return g, P, pr, pe


def _engine(g, P, dtype, **kw):
    import lgar_py_amd as lg
    return lg.LgarEngine(P["alpha"], P["n"], P["ksat"], P["theta_e"], P["theta_r"], P["thickness"], dtype=dtype,
                         **dict(engine_keywords(g), **kw))


def _replicated(name, ncol, dtype, **kw):
    import lgar_py_amd as lg
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    eng = lg.LgarEngine(g["alpha"], g["n"], g["ksat"], g["theta_e"], g["theta_r"], g["thickness"], n_columns=ncol, dtype=dtype,
                        **dict(engine_keywords(g), **kw))
    f = torch.tensor(g["forcing"])
    return g, eng, f[:, 0:1].expand(-1, ncol).contiguous(), f[:, 1:2].expand(-1, ncol).contiguous()


def _ref_of(eng, edges, what):
    """The numpy definition on the engine's own front table, rounded once to the engine's dtype."""
    fr = eng.fronts()
    ref = MH.profile_ref(fr["depth"], fr["theta"], fr["layer"], fr["n_fronts"], eng.thickness.cpu().numpy(), edges, what)
    return ref.astype(fr["depth"].dtype)


def _edges_for(P):
    return [0.0, 5.0, 10.0, 30.0, 60.0, 100.0, float(P["thickness"].sum(axis=0).max()) + 50.0]


@pytest.mark.parametrize("name", ["synth1_phil", "six_layer_synth1"])
def test_the_chosen_columns_stay_inside_the_reference(name):
    """The CPU oracle on the perturbed columns of the next test: at least 90 % of them stay inside the reference's domain of
    validity, so the bit-for-bit comparison below covers the bulk of a wave and its ragged tail."""
    from oracle import lgar_oracle as O
    g, P, pr, pe = perturbed_job(name)
    *_, st = O.run_columns(P["alpha"], P["n"], P["ksat"], P["theta_e"], P["theta_r"], P["thickness"], pr, pe,
                           initial_psi=float(g["initial_psi"]), pdm=float(g["pdm"]), wp_psi=float(g["wilting_point_psi"]),
                           frozen_factor=float(g["frozen_factor"]), dt_h=float(g["dt_h"]), nint=int(g["nint"]),
                           num_subcycles=int(g["num_subcycles"]), giuh=tuple(g["giuh_ordinates"]), want_series=False)
    assert (st == 0).mean() >= 0.9, float((st == 0).mean())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", ["synth1_phil", "six_layer_synth1"])
def test_kernel_equals_the_numpy_definition_bit_for_bit(name, dtype):
    """67 different columns (soil and thickness perturbed, forcing scaled), all 144 steps, fp64 and fp32: after EVERY step
    soil_moisture() -- mean theta and storage, explicit edges and each column's own layers -- equals the numpy loop over
    fronts() of the same engine bit for bit on the columns that have not faulted (>= 90 % of them)."""
    g, P, pr, pe = perturbed_job(name)
    eng = _engine(g, P, dtype)
    pr, pe = torch.tensor(pr), torch.tensor(pe)
    edges = _edges_for(P)
    out = torch.empty(len(edges) - 1, NCOL, dtype=dtype, device=eng.device)
    layer_theta_differs = False
    for t in range(pr.shape[0]):
        eng.forward(pr[t:t + 1], pe[t:t + 1], series=(), check=False)
        ok = eng.status.cpu().numpy() == 0
        for e in (edges, None):
            for what in ("theta", "storage"):
                got = eng.soil_moisture(e, what, out=out if e is not None else None)
                assert got.dtype == dtype and tuple(got.shape) == ((len(edges) - 1) if e is not None else eng.L, NCOL)
                got, ref = got.cpu().numpy(), _ref_of(eng, e, what)
                assert MH.same_bits(got[:, ok], ref[:, ok]), (t, e is None, what)
        layer_theta_differs |= bool((got[:, ok].std(axis=1) > 0).all())
    assert ok.mean() >= 0.9, float(ok.mean())
    assert layer_theta_differs  # the columns really differ: the layer bins of every layer hold different water
    assert int(eng.n_fronts.max()) > eng.L  # fronts were created: more than the initial one per layer


def test_many_fronts_every_step_vs_the_reference_table():
    """manyfronts_pulse_84 through the front-capacity chain (search_mode 2, 32 slots: 31 fronts, steps with transiently
    non-monotone depths), one snapshot per step from run_with_soil_moisture(every=1): every row against the profile computed
    from the REFERENCE's table of that step.  The project holds every depth and theta of the table to 1e-6 relative
    (test_gpu_parity.py); to first order that moves a bin's storage by at most 1e-6 * sum_j theta_j (|w_j| + |d_j| + |t_j|)
    (clip is 1-Lipschitz; 1.01 covers the second order), and its mean theta by that over the bin's in-column width."""
    g, eng, pr, pe = _replicated("manyfronts_pulse_84", 3, torch.float64, search_mode=2, front_slots=32)
    t = MH.tables("manyfronts_pulse_84")
    args = (t["depth"], t["theta"], t["layer"], t["n_fronts"], t["thickness"])
    T = pr.shape[0]
    assert int(t["n_fronts"].max()) == 31
    for edges in ([0.0, 5.0, 10.0, 30.0, 60.0, 100.0, t["Z"] + 50.0], None):
        for what in ("theta", "storage"):
            eng.reset()
            res = eng.run_with_soil_moisture(pr, pe, 1, edges=edges, what=what, series=())
            got = res["soil_moisture"].cpu().numpy()  # [T, D, N]
            assert got.shape[0] == T and (got == got[:, :, :1]).all()
            ref = MH.profile_ref(*args, edges, what)  # [D, T]
            bound = 1.01e-6 * MH.profile_ref(*args, edges, what, sensitivity=True)
            if what == "theta":
                E = np.asarray(edges) if edges is not None else np.concatenate([[0.0], np.cumsum(g["thickness"])])
                width = np.minimum(np.maximum(t["Z"], E[:-1]), E[1:]) - E[:-1]
                bound = bound / width[:, None]
            err = np.abs(got[:, :, 0].T - ref)
            print("manyfronts %s %s: worst error / bound = %.3g" % ("layers" if edges is None else "edges", what,
                                                                   float((err / bound).max())))
            assert (err <= bound).all(), (what, edges is None, float((err / bound).max()))
    assert int(eng.n_fronts.max()) == 31


def _windowed_and_single(dtype=torch.float64):
    g, P, pr, pe = perturbed_job("synth1_phil")
    pr, pe = torch.tensor(pr), torch.tensor(pe)
    w = torch.tensor(np.random.default_rng(3).random(NCOL))
    series, basin = ("runoff", "percolation", "infiltration", "ending_volume"), ("runoff", "AET")
    a = _engine(g, P, dtype)
    win = a.run_with_soil_moisture(pr, pe, 12, what="storage", series=series, basin=basin, weights=w, check=False)
    b = _engine(g, P, dtype)
    one = b.forward(pr, pe, series=series, basin=basin, weights=w, check=False)
    return g, P, pr, pe, a, win, b, one


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_windowed_run_totals_equal_a_single_forward(dtype):
    """The run totals after run_with_soil_moisture(every=12) against ONE forward() over the same 144 rows, bit for bit.

    forward() sums a call's accumulators and adds that sum to the run totals (rows 0..7 of `totals`), so twelve bare windows
    add twelve partial sums where one call adds one: equal to the last bits only (1.95e-14 cm in fp64 on this job;
    test_gpu_parity.py::test_chunked_run_equals_single_run says so for any chunked run).  run_with_soil_moisture therefore
    replays the one-call summation order over the accumulators its windows store (lgar_totals_replay): bitwise equal, faulted
    columns included, and a second run on top of the first keeps adding to the totals like a second forward() does."""
    *_, pr, pe, a, win, b, one = _windowed_and_single(dtype)
    diff = (a.totals - b.totals).abs()
    print("windowed totals (%s): worst absolute difference %.3g" % (dtype, float(diff.max())))
    assert torch.equal(a.totals, b.totals)
    assert float(b.totals[:8].abs().max()) > 1.0  # (something was summed)
    a.run_with_soil_moisture(pr[:30], pe[:30], 12, series=(), check=False)
    b.forward(pr[:30], pe[:30], series=(), check=False)
    assert torch.equal(a.totals, b.totals)


def test_windowed_run_equals_a_single_forward():
    """run_with_soil_moisture(every=12) against ONE forward() of a fresh engine over the same 144 rows: requested series, basin
    sums, the final front table, the scalars and the status bit for bit (the run totals have a test of their own above);
    snapshot r is soil_moisture() of a third engine stepped 12 (r + 1) rows."""
    g, P, pr, pe, a, win, b, one = _windowed_and_single()
    assert set(win) == set(one) | {"soil_moisture"}
    for k in one:
        assert torch.equal(win[k], one[k]), k
    for nm in ("depth", "theta", "psi", "k", "dzdt", "flags", "n_fronts", "scalars", "status"):
        assert torch.equal(getattr(a, nm), getattr(b, nm)), nm
    assert torch.equal(a.totals[8:], b.totals[8:])
    snaps = win["soil_moisture"]
    assert tuple(snaps.shape) == (12, 3, NCOL)
    c = _engine(g, P, torch.float64)
    for r in range(12):
        c.forward(pr[12 * r:12 * (r + 1)], pe[12 * r:12 * (r + 1)], series=(), check=False)
        assert torch.equal(snaps[r], c.soil_moisture(what="storage")), r
    # a ragged tail is integrated but gives no snapshot
    d = _engine(g, P, torch.float64)
    tail = d.run_with_soil_moisture(pr[:30], pe[:30], 12, series=("runoff",), check=False)
    assert tuple(tail["soil_moisture"].shape) == (2, 3, NCOL) and torch.equal(tail["runoff"], one["runoff"][:30])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_layer_storage_closes_on_ending_volume(dtype):
    """The layer bins cover the column: their storage sums to the engine's own ending_volume (the reference's mass_balance,
    layers/Layer.py:795-824) within 1e-6 relative, the project's parity bar, after every 12 rows of the perturbed job.  The fp32
    engine keeps ending_volume in fp32 (relative spacing 6e-8), so the same bar is the comparison's floor there, not slack."""
    g, P, pr, pe = perturbed_job("synth1_phil")
    eng = _engine(g, P, dtype)
    res = eng.run_with_soil_moisture(torch.tensor(pr), torch.tensor(pe), 12, what="storage", series=("ending_volume",), check=False)
    ok = (eng.status == 0).cpu().numpy()
    vol = res["ending_volume"][11::12].double().cpu().numpy()
    tot = res["soil_moisture"].double().sum(dim=1).cpu().numpy()
    rel = (np.abs(tot - vol) / np.abs(vol))[:, ok]
    print("closure of layer storage on ending_volume (%s): worst relative %.3g" % (dtype, float(rel.max())))
    assert ok.mean() >= 0.9 and rel.max() <= 1e-6, float(rel.max())


def test_basin_sums():
    """basin=True: sum_c weights[c] * result[:, c] by the stored-series reduction -- within 1e-12 relative of numpy's fp64 sum,
    the same bits on every run, and ACCUMULATED into a caller's block (a second call doubles it)."""
    g, P, pr, pe = perturbed_job("synth1_phil", N=1000)  # (1000 different columns as initialised: no column has faulted)
    for dtype in (torch.float64, torch.float32):
        eng = _engine(g, P, dtype)
        w = np.random.default_rng(5).random(1000)
        edges = [0.0, 10.0, 44.0, 100.0, 150.0]
        for weights in (w, None):
            x, s1 = eng.soil_moisture(edges, "storage", weights=weights, basin=True)
            x2, s2 = eng.soil_moisture(edges, "storage", weights=weights, basin=True)
            assert torch.equal(s1, s2) and torch.equal(x, x2) and s1.dtype == torch.float64 and tuple(s1.shape) == (4,)
            wd = np.ones(1000) if weights is None else torch.tensor(w).to(dtype).double().numpy()
            want = (x.double().cpu().numpy() * wd[None, :]).sum(axis=1)
            assert (np.abs(s1.cpu().numpy() - want) <= 1e-12 * np.abs(want)).all()
            _, s3 = eng.soil_moisture(edges, "storage", weights=weights, basin=s2)
            assert s3 is s2 and torch.equal(s3, 2.0 * s1)
        # 1001 columns: rows that are not 16-byte aligned take the reduction's scalar path
    g, P, pr, pe = perturbed_job("synth1_phil", N=1001)
    eng = _engine(g, P, torch.float32)
    x, s = eng.soil_moisture(None, "theta", basin=True)
    assert (np.abs(s.cpu().numpy() - x.double().cpu().numpy().sum(axis=1)) <= 1e-12 * np.abs(s.cpu().numpy())).all()


def test_bins_below_the_column_on_gpu():
    g, eng, pr, pe = _replicated("synth1_phil", 5, torch.float32)
    edges = [0.0, 190.0, 210.0, 220.0]
    th, st = eng.soil_moisture(edges, "theta"), eng.soil_moisture(edges, "storage")
    assert bool(torch.isnan(th[2]).all()) and bool((st[2] == 0).all()) and bool(torch.isfinite(th[:2]).all())
    # the straddling bin [190, 210] is divided by the 10 cm of it that lie inside the 200 cm column
    assert MH.same_bits(th.cpu().numpy(), _ref_of(eng, edges, "theta")) and float((th[1] - st[1] / 10.0).abs().max()) <= 1e-7


def test_argument_checks():
    import lgar_py_amd as lg
    from lgar_py_amd import _capi
    g, eng, pr, pe = _replicated("synth1_phil", 4, torch.float64)
    for bad in ([0.0, 10.0, 10.0], [0.0, 20.0, 10.0], [-1.0, 5.0], [0.0, float("nan")], [0.0, float("inf")], [5.0],
                [[0.0, 1.0], [2.0, 3.0]], list(range(_capi.MOIST_BINS + 2))):
        with pytest.raises(lg.LgarError):
            eng.soil_moisture(bad)
    assert tuple(eng.soil_moisture(list(range(_capi.MOIST_BINS + 1))).shape) == (_capi.MOIST_BINS, 4)
    with pytest.raises(lg.LgarError):
        eng.soil_moisture(what="psi")
    dev = eng.device
    for out in (torch.empty(3, 5, dtype=torch.float64, device=dev), torch.empty(3, 4, dtype=torch.float32, device=dev),
                torch.empty(4, 3, dtype=torch.float64, device=dev).t(), torch.empty(3, 4, dtype=torch.float64), "x"):
        with pytest.raises(lg.LgarError):
            eng.soil_moisture(out=out)
    with pytest.raises(lg.LgarError):
        eng.soil_moisture(basin=torch.zeros(2, dtype=torch.float64, device=dev))
    with pytest.raises(lg.LgarError):
        eng.soil_moisture(weights=[1.0] * 5, basin=True)
    with pytest.raises(lg.LgarError):
        eng.run_with_soil_moisture(pr, pe, 0)
    # the raw C-ABI
    lib = _capi.load()
    out = torch.empty(3, 4, dtype=torch.float64, device=dev)
    e = torch.tensor([0.0, 1.0, 2.0, 3.0, 4.0], dtype=torch.float64, device=dev)
    call = lambda edges, nb, what, o: lib.lgar_soil_moisture(C.byref(eng.dims), C.byref(eng._params), C.byref(eng._state), edges, nb,
                                                             what, o, None, None, _capi.F64, None)
    assert call(None, 3, 0, None) == -1                       # NULL out
    assert call(None, 2, 0, out.data_ptr()) == -1             # layer bins need n_bins == n_layers
    assert call(e.data_ptr(), 0, 0, out.data_ptr()) == -1
    assert call(e.data_ptr(), _capi.MOIST_BINS + 1, 0, out.data_ptr()) == -1
    assert call(e.data_ptr(), 3, 2, out.data_ptr()) == -1     # unknown `what`
    assert lib.lgar_soil_moisture(None, None, None, None, 3, 0, None, None, None, 1, None) == -1
    run, so = torch.zeros(8, 4, dtype=torch.float64, device=dev), _capi.LgarStepOut()
    assert lib.lgar_totals_replay(C.byref(eng.dims), C.byref(so), 3, None, _capi.F64, None) == -1
    assert lib.lgar_totals_replay(C.byref(eng.dims), None, 3, run.data_ptr(), _capi.F64, None) == -1
    assert lib.lgar_totals_replay(C.byref(eng.dims), C.byref(so), -1, run.data_ptr(), _capi.F64, None) == -1
    assert lib.lgar_totals_replay(C.byref(eng.dims), C.byref(so), 3, run.data_ptr(), _capi.F64, None) == 0  # no series: no-op
    assert call(None, 3, 1, out.data_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, eng.soil_moisture(what="storage"))


def test_model_surface(tmp_path):
    """model.dpLGAR.soil_moisture(): [L] for one column, [L, N] otherwise (the _shape convention of ending_volume), on the
    Phillipsburg configuration; the layers' storage sums to the model's ending_volume."""
    from lgar_py_amd.data import Data
    from lgar_py_amd.model import dpLGAR
    from _model_files import model_cfg as _cfg
    g = np.load(os.path.join(GOLDEN, "phil_hourly_3000.npz"))
    cfg = _cfg(tmp_path, g, n=40)
    data = Data(cfg)
    one = dpLGAR(cfg)
    for i in range(40):
        one(data[i][0])
    sm = one.soil_moisture()
    assert tuple(sm.shape) == (3,) and sm.dtype == torch.float64
    st = one.soil_moisture(what="storage")
    assert abs(float(st.sum()) - float(one.ending_volume)) <= 1e-6 * float(one.ending_volume)
    assert abs(float(one.ending_volume) - g["acc"][39, 9]) <= 1e-6 * g["acc"][39, 9]
    assert tuple(one.soil_moisture([0.0, 10.0, 50.0]).shape) == (2,)
    many = dpLGAR(cfg, n_columns=5)
    assert tuple(many.soil_moisture().shape) == (3, 5) and tuple(many.soil_moisture([0.0, 10.0, 50.0], "storage").shape) == (2, 5)
    assert torch.equal(many.soil_moisture()[:, 0].cpu(), dpLGAR(cfg).soil_moisture().cpu())
