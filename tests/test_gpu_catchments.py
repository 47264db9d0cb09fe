"""GPU (-m gpu): catchment sums -- lgar_catchment_sums / lgar_catchment_spread through catchments.CatchmentMap,
LgarEngine.forward(catchments=...), catchments.catchment_sum (autograd) and model.dpLGAR.soil_moisture(catchments=...).

out[t][b] is a pure function of catchment b's own members (include/lgar.h), so the kernel is held BIT FOR
BIT to the numpy statement of the definition (tests/catchment_host: sums_ref), the one tests/test_catchment_host.py holds the
host build of the same header to."""
import os

import numpy as np
import pytest

from _golden import engine_keywords
from conftest import GOLDEN

from post_host import catchment as CH

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = sum(CH.SIZES)  # 2121
T = 5
NP = {torch.float64: np.float64, torch.float32: np.float32}


def _data(dtype, flagged, seed=0):
    """Random [T, N] rows over seven decades and both signs; flagged: 40 columns with a fault bit over NaN / inf rows, 3 with a
    status word that has no fault bit."""
    rng = np.random.default_rng(seed)
    series = ((rng.random((T, N)) - 0.3) * 10.0 ** rng.integers(-3, 4, (T, N))).astype(NP[dtype])
    status = None
    if flagged:
        status = np.zeros(N, dtype=np.int32)
        bad = rng.choice(N, 43, replace=False)
        status[bad[:40]] = 2 ** rng.integers(0, 7, 40)
        status[bad[40:]] = 128
        series[:, bad[:20]] = np.nan
        series[0, bad[20:30]] = np.inf
        series[1:, bad[20:30]] = -np.inf
    return series, status, rng.random(N)


def _cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_kernel_equals_the_numpy_definition_bit_for_bit(dtype):
    """Catchments of 0, 1, 63, 64, 65, 255, 256, 257 and 1000 members in one map (N = 2121), five rows: with and without
    weights, contiguous (order = None: lane-contiguous reads) and permuted (gather), with and without flagged columns over NaN
    rows -- sums and weight sums against the plain loop over the partials and the tree."""
    from lgar_py_amd.catchments import CatchmentMap
    for permuted in (False, True):
        ids = CH.sized_ids(permute=7 if permuted else None)
        for weighted in (False, True):
            for flagged in (False, True):
                series, status, w = _data(dtype, flagged)
                cmap = CatchmentMap(ids, weights=w if weighted else None)
                assert (cmap.order is None) == (not permuted) and cmap.B == len(CH.SIZES) and cmap.sizes.tolist() == list(CH.SIZES)
                got, wsum = cmap.sums(_cuda(series), status=_cuda(status), weight_sums=True)
                assert got.dtype == torch.float64 and tuple(got.shape) == (T, cmap.B) and tuple(wsum.shape) == (cmap.B,)
                ref, rw = CH.sums_ref(series, cmap.offsets_host, cmap.order_host, w.astype(NP[dtype]) if weighted else None, status)
                what = (permuted, weighted, flagged)
                assert CH.same_bits(got.cpu().numpy(), ref), what
                assert CH.same_bits(wsum.cpu().numpy(), rw), what
                assert np.isfinite(ref).all() and (ref[:, 0] == 0).all()  # the NaN rows stay out; the empty catchment is +0.0
                # a caller's buffer is written, not added to
                buf = torch.full((T, cmap.B), 7.0, dtype=torch.float64, device="cuda")
                assert cmap.sums(_cuda(series), status=_cuda(status), out=buf) is buf and torch.equal(buf, got)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_large_catchments_run_the_main_loop_of_the_one_row_kernel(dtype):
    """From 1024 members on a lane of the one-row kernel takes whole blocks of 16 loads: catchments of 2500, 1024, 1025 and 1023
    members (4 catchments x 5 rows = 20 waves: the one-row kernel), weighted, with flagged columns over NaN rows, contiguous and
    gathered, against the numpy loop; and the 2500-member catchment keeps its bits alone in a map 77 columns further on."""
    from lgar_py_amd.catchments import CatchmentMap
    n = sum(CH.BIG_SIZES)
    rng = np.random.default_rng(13)
    series = ((rng.random((T, n)) - 0.3) * 10.0 ** rng.integers(-3, 4, (T, n))).astype(NP[dtype])
    status = np.where(rng.random(n) < 0.03, 2, 0).astype(np.int32)
    series[:, status != 0] = np.nan
    w = rng.random(n)
    for permuted in (False, True):
        ids = CH.sized_ids(CH.BIG_SIZES, permute=3 if permuted else None)
        cmap = CatchmentMap(ids, weights=w)
        assert (cmap.order is None) == (not permuted) and cmap.sizes.tolist() == list(CH.BIG_SIZES)
        got, wsum = cmap.sums(_cuda(series), status=_cuda(status), weight_sums=True)
        ref, rw = CH.sums_ref(series, cmap.offsets_host, cmap.order_host, w.astype(NP[dtype]), status)
        assert CH.same_bits(got.cpu().numpy(), ref) and CH.same_bits(wsum.cpu().numpy(), rw) and np.isfinite(ref).all()
        alone = CatchmentMap(np.concatenate([np.full(77, -1), np.where(ids == 0, 0, -1)]), weights=np.concatenate([np.ones(77), w]))
        s2 = np.concatenate([np.full((T, 77), np.nan, NP[dtype]), series], axis=1)
        st2 = np.concatenate([np.zeros(77, np.int32), status])
        assert torch.equal(alone.sums(_cuda(s2), status=_cuda(st2))[:, 0], got[:, 0])


def test_a_map_over_no_columns_sums_to_zero():
    """N = 0 (a rank that holds no column of any catchment): rows of +0.0, not an argument error."""
    from lgar_py_amd.catchments import CatchmentMap
    cmap = CatchmentMap(np.array([], dtype=np.int64), n_catchments=3)
    got, wsum = cmap.sums(torch.empty(2, 0, dtype=torch.float32, device="cuda"), weight_sums=True)
    assert tuple(got.shape) == (2, 3) and bool((got == 0).all()) and not bool(torch.signbit(got).any()) and bool((wsum == 0).all())
    assert tuple(cmap.spread(torch.ones(2, 3, device="cuda"), torch.float64).shape) == (2, 0)


def test_many_catchments_take_four_rows_per_wave():
    """Jobs of many catchments run one wave per (four rows, catchment): 40 000 small catchments and a large one over 101 003
    columns, six rows (a full group of four and a ragged one), gathered and contiguous.  The four-row kernel starts at four
    waves per wave slot of the chip after the division by four (32 768 on the MI355X's 256 CUs; 2 x 40 001 here).  The
    reference that takes the ONE-row kernel: the same catchments in two maps of 20 000 and 20 001 (the other columns in no
    catchment), one row per call -- 20 001 waves, below the threshold.  A catchment's bits depend on neither: the same bits;
    and the numpy loop on the first 300 catchments and the large one."""
    from lgar_py_amd.catchments import CatchmentMap
    rng = np.random.default_rng(4)
    sizes = np.concatenate([rng.integers(0, 6, 40000), [0]])
    sizes[-1] = 101003 - sizes.sum()
    n, B, rows, half = 101003, 40001, 6, 20000
    assert sizes[-1] > 256
    series = ((rng.random((rows, n)) - 0.3) * 10.0 ** rng.integers(-3, 4, (rows, n))).astype(np.float32)
    status = np.where(rng.random(n) < 0.02, 4, 0).astype(np.int32)
    series[:, status != 0] = np.nan
    w = rng.random(n)
    dev, st = _cuda(series), _cuda(status)
    for permuted in (False, True):
        ids = CH.sized_ids(sizes, permute=12 if permuted else None)
        cmap = CatchmentMap(ids, n_catchments=B, weights=w)
        assert (cmap.order is None) == (not permuted)
        got = cmap.sums(dev, status=st)
        assert bool(torch.isfinite(got).all())
        lower = CatchmentMap(np.where(ids < half, ids, -1), n_catchments=half, weights=w)
        upper = CatchmentMap(np.where(ids >= half, ids - half, -1), n_catchments=B - half, weights=w)
        by_row = torch.cat([torch.cat([lower.sums(dev[t:t + 1], status=st), upper.sums(dev[t:t + 1], status=st)], dim=1)
                            for t in range(rows)])
        assert torch.equal(got, by_row)
        some = np.concatenate([np.arange(300), [B - 1]])
        # (the definition on those catchments alone: a sub-map of their members in map order)
        sub = np.concatenate([[0], np.cumsum(cmap.sizes[some])]).astype(np.int32)
        members = [CH.members_of(cmap.offsets_host, cmap.order_host, b, n) for b in some]
        ref, _ = CH.sums_ref(series, sub, np.concatenate(members), w.astype(np.float32), status)
        assert CH.same_bits(got[:, some].cpu().numpy(), ref)


def test_a_catchment_does_not_depend_on_the_others():
    """Catchment b's rows keep their bits when the other catchments are regrouped (B = 9 -> 40), when the job is embedded at
    another column offset, and when the call is repeated -- with the order array and on the contiguous path."""
    from lgar_py_amd.catchments import CatchmentMap
    series, _, w = _data(torch.float32, False, seed=3)
    dev = _cuda(series)
    for permuted in (True, False):
        ids = CH.sized_ids(permute=11 if permuted else None)
        base = CatchmentMap(ids, weights=w)
        got = base.sums(dev)
        assert torch.equal(got, base.sums(dev))  # repeated
        # regrouped: the 1000- and the 257-member catchments keep their members (as catchments 39 and 0), every other column
        # moves to one of 38 new catchments
        re = np.where(ids == 8, 39, np.where(ids == 7, 0, 1 + np.arange(N) % 38))
        many = CatchmentMap(re, weights=w)
        assert many.B == 40
        g40 = many.sums(dev)
        assert torch.equal(g40[:, 39], got[:, 8]) and torch.equal(g40[:, 0], got[:, 7])
        # embedded 131 columns further on (the contiguous path: behind one more catchment, so that order stays None)
        pad = np.full(131, 0 if not permuted else -1)
        ids2 = np.concatenate([pad, ids + (0 if permuted else 1)])
        moved = CatchmentMap(ids2, weights=np.concatenate([np.ones(131), w]))
        assert (moved.order is None) == (not permuted)
        s2 = torch.cat([torch.full((T, 131), float("nan"), dtype=dev.dtype, device="cuda"), dev], dim=1).contiguous()
        g2 = moved.sums(s2)
        assert torch.equal(g2[:, (0 if permuted else 1):], got)


def _replicated_job(dtype, ncol):
    """synth1_phil's soil for every column under its rain scaled per column by U(0.5, 1)."""
    import lgar_py_amd as lg
    from lgar_py_amd import workloads as W
    g = np.load(os.path.join(GOLDEN, "synth1_phil.npz"))
    eng = lg.LgarEngine(g["alpha"], g["n"], g["ksat"], g["theta_e"], g["theta_r"], g["thickness"], n_columns=ncol, dtype=dtype,
                        **engine_keywords(g))
    sc = W.forcing_scale(ncol, 0.5, 1.0, seed=4)
    return eng, torch.tensor(g["forcing"][:, 0:1] * sc[None, :]), torch.tensor(g["forcing"][:, 1:2] * np.ones((1, ncol)))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_one_catchment_agrees_with_the_basin_pass(dtype):
    """B = 1 against forward(basin=("runoff",), weights=w) over the same stored series: both are fp64 sums of the same n exact
    (fp32) or once-rounded (fp64) products in two different orders, and two fp64 summation orders of n terms cannot differ by
    more than 2 n 2^-53 sum|w x| (each is within n 2^-53 sum|w x| of the exact sum, to first order, Higham 4.4)."""
    from lgar_py_amd.catchments import CatchmentMap
    n = 1000
    eng, pr, pe = _replicated_job(dtype, n)
    w = np.random.default_rng(5).random(n)
    stored = {"runoff": torch.zeros(pr.shape[0], n, dtype=dtype, device=eng.device)}  # (zeros: a row no kernel writes reads 0 in both)
    res = eng.forward(pr, pe, series=("runoff",), out=stored, basin=("runoff",), weights=w, check=False)
    cmap = CatchmentMap(np.zeros(n, dtype=np.int64), weights=w)
    got = cmap.sums(res["runoff"])
    assert cmap.order is None and tuple(got.shape) == (pr.shape[0], 1)
    x = res["runoff"].double() * cmap.weights(dtype).double()[None, :]
    bound = 2 * n * 2.0 ** -53 * x.abs().sum(dim=1)
    err = (got[:, 0] - res["basin:runoff"]).abs()
    print("B = 1 vs the basin pass (%s): worst error / bound = %.3g" % (dtype, float((err / bound.clamp_min(1e-300)).max())))
    assert bool((err <= bound).all()) and float(got.abs().max()) > 0.0


IDS67 = np.array([4] * 30 + [0] * 5 + [2] * 20 + [-1] + [3] + [5] * 3 + [6] * 6 + [-1])  # 7 catchments, catchment 1 empty


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("name", ["synth1_phil", "six_layer_synth1"])
def test_through_the_engine(name, dtype):
    """The 67 perturbed columns of test_gpu_moisture.py (some of them fault) in 7 uneven catchments, one empty, two columns in
    none: forward(catchment=("runoff", "infiltration"), catchments=cmap) equals the numpy definition over the returned series
    and the engine's status bit for bit; a name without a series goes through a scratch series (the same bits) and raises when
    the engine may not allocate one."""
    import lgar_py_amd as lg
    from lgar_py_amd.catchments import CatchmentMap
    from test_gpu_moisture import _engine, perturbed_job
    g, P, pr, pe = perturbed_job(name, N=67, seed=8)
    pr, pe = torch.tensor(pr), torch.tensor(pe)
    ids = IDS67[np.random.default_rng(2).permutation(67)]
    w = np.random.default_rng(6).random(67)
    eng = _engine(g, P, dtype)
    cmap = CatchmentMap(ids, n_catchments=7, weights=w, device=eng.device)
    assert cmap.sizes.tolist() == [5, 0, 20, 1, 30, 3, 6] and cmap.order is not None
    names = ("runoff", "infiltration")
    res = eng.forward(pr, pe, series=names, catchments=cmap, catchment=names, check=False)
    status = eng.status.cpu().numpy()
    if dtype == torch.float64:
        assert ((status & 0x7F) == 0).mean() >= 0.9, float(((status & 0x7F) == 0).mean())
    wd = w.astype(NP[dtype])
    for nm in names:
        got = res["catchment:" + nm]
        assert got.dtype == torch.float64 and tuple(got.shape) == (pr.shape[0], 7)
        ref, rw = CH.sums_ref(res[nm].cpu().numpy(), cmap.offsets_host, cmap.order_host, wd, status)
        assert CH.same_bits(got.cpu().numpy(), ref), nm
        assert np.isfinite(ref).all() and (ref[:, 1] == 0).all()
    assert CH.same_bits(res["catchment:weight"].cpu().numpy(), rw) and float(res["catchment:runoff"].abs().max()) > 0.01
    # a name without a series of its own: a scratch series behind it, the same bits
    eng2 = _engine(g, P, dtype)
    res2 = eng2.forward(pr, pe, series=("runoff",), catchments=cmap, catchment=names, check=False)
    assert "infiltration" not in res2 and torch.equal(res2["catchment:infiltration"], res["catchment:infiltration"])
    assert torch.equal(res2["catchment:runoff"], res["catchment:runoff"])
    # ... and no scratch allowed: an error, not another way to sum
    eng3 = _engine(g, P, dtype, basin_scratch_bytes=0)
    with pytest.raises(lg.LgarError, match="basin_scratch_bytes"):
        eng3.forward(pr, pe, series=("runoff",), catchments=cmap, catchment=names, check=False)
    with pytest.raises(lg.LgarError):
        eng3.forward(pr, pe, catchment=("runoff",), check=False)  # names without a map
    with pytest.raises(lg.LgarError):
        eng3.forward(pr, pe, catchments=CatchmentMap(ids[:66], device=eng.device), catchment=("runoff",), check=False)
    # without catchments nothing changes
    assert set(_engine(g, P, dtype).forward(pr, pe, check=False)) == {"runoff", "percolation"}


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_spread_equals_torch_indexing(dtype):
    """The adjoint: out[t, c] = grad[t, ids[c]] * w[c] in fp64, rounded once -- (g[:, ids].double() * w.double()).to(dtype) by
    torch, bit for bit; zero for flagged columns and for columns of no catchment."""
    from lgar_py_amd.catchments import CatchmentMap
    rng = np.random.default_rng(9)
    ids = CH.sized_ids(permute=5)
    ids[rng.choice(N, 50, replace=False)] = -1
    _, status, w = _data(dtype, True, seed=1)
    g = torch.tensor(rng.standard_normal((T, len(CH.SIZES))), device="cuda")
    for weights in (w, None):
        cmap = CatchmentMap(ids, n_catchments=len(CH.SIZES), weights=weights)
        for st in (None, _cuda(status)):
            got = cmap.spread(g, dtype, status=st)
            assert got.dtype == dtype and tuple(got.shape) == (T, N)
            wt = cmap.weights(dtype) if weights is not None else torch.ones(N, dtype=dtype, device="cuda")
            idx = torch.tensor(np.maximum(ids, 0), device="cuda")
            want = (g[:, idx].double() * wt.double()).to(dtype)
            dead = torch.tensor(ids < 0, device="cuda")
            if st is not None:
                dead = dead | ((st & 0x7F) != 0)
            want = torch.where(dead[None, :], torch.zeros_like(want), want)
            assert torch.equal(got, want)
            assert bool((got[:, dead] == 0).all()) and bool((got[:, ~dead] != 0).all())


def test_gradients_through_catchment_sums():
    """24 columns of grad_synth0_12h's soil perturbed +-5 % in 3 catchments (one column in none), loss = sum (catchment runoff -
    target)^2: the parameter gradients through catchment_sum(lgar_series(...)) are torch.equal to parameter_vjp fed with the
    torch-made tangent weights of the test above -- the tangent kernels are deterministic and the weights are the same bits.
    Two of these 24 columns leave the reference's domain of validity (the fault of DESIGN.md section 4), so the run goes on
    without them (check=False): the forward status drops them from the sums and from the spread, and their gradient is zero."""
    import lgar_py_amd as lg
    from lgar_py_amd import workloads as W
    from lgar_py_amd.autograd import lgar_series, parameter_vjp
    from lgar_py_amd.catchments import CatchmentMap, catchment_sum
    g = np.load(os.path.join(GOLDEN, "grad_synth0_12h.npz"))
    n = 24
    Pn = W.perturbed_columns(n, frac=0.05, seed=21, base={k: g[k] for k in W.PARAM_KEYS + ("thickness",)})
    P = {k: torch.tensor(v, device="cuda") for k, v in Pn.items()}
    for k in ("alpha", "n", "ksat"):
        P[k].requires_grad_(True)
    f = torch.tensor(g["forcing"], device="cuda")
    Tn = f.shape[0]
    pr, pe = f[:, 0:1].expand(Tn, n).contiguous(), f[:, 1:2].expand(Tn, n).contiguous()
    ekw = dict(engine_keywords(g), dtype=torch.float64)
    ids = np.array([0] * 9 + [2] * 5 + [-1] + [1] * 9)[np.random.default_rng(1).permutation(n)]
    w = np.random.default_rng(2).random(n) + 0.5
    cmap = CatchmentMap(ids, weights=w)
    statuses = []
    runoff, _ = lgar_series(P["alpha"], P["n"], P["ksat"], P["theta_e"], P["theta_r"], P["thickness"], pr, pe, check=False,
                            status_out=statuses, **ekw)
    status = statuses[0]
    faulted = (status & 0x7F) != 0
    assert int(faulted.sum()) <= 4, int(faulted.sum())  # (at least 20 of the 24 columns carry the comparison)
    catch = catchment_sum(runoff, cmap, status)
    assert tuple(catch.shape) == (Tn, 3) and catch.requires_grad
    ref, _ = CH.sums_ref(runoff.detach().cpu().numpy(), cmap.offsets_host, cmap.order_host, w, status.cpu().numpy())
    assert CH.same_bits(catch.detach().cpu().numpy(), ref) and np.isfinite(ref).all()
    target = torch.tensor(np.random.default_rng(3).random((Tn, 3)), device="cuda") * float(catch.detach().max())
    loss = ((catch - target) ** 2).sum()
    loss.backward()
    # the same weights by torch indexing, through the tangent kernels directly
    gl = 2.0 * (catch.detach() - target)
    idx = torch.tensor(np.maximum(ids, 0), device="cuda")
    wr = (gl[:, idx].double() * cmap.weights(torch.float64).double()).to(torch.float64)
    dead = torch.tensor(ids < 0, device="cuda") | faulted
    wr = torch.where(dead[None, :], torch.zeros_like(wr), wr)
    assert torch.equal(wr, cmap.spread(gl, torch.float64, status=status))
    eng = lg.LgarEngine(P["alpha"].detach(), P["n"].detach(), P["ksat"].detach(), P["theta_e"], P["theta_r"], P["thickness"], **ekw)
    wanted = [(kind, l) for kind in ("alpha", "n", "ksat") for l in range(eng.L)]
    vj, st = parameter_vjp(eng, pr, pe, wr, torch.zeros_like(wr), wanted, check=False)
    assert not bool(st[~faulted].any())
    for kind in ("alpha", "n", "ksat"):
        want = torch.stack([vj[(kind, l)] for l in range(eng.L)])
        want = torch.where(faulted[None, :], torch.zeros_like(want), want)  # (lgar_series gives a faulted column no gradient)
        assert torch.equal(P[kind].grad, want), kind
        assert float(want.abs().max()) > 0 and bool((want[:, dead] == 0).all())


def test_model_soil_moisture_per_catchment(tmp_path):
    """model.dpLGAR.soil_moisture(catchments=cmap): the [D, B] storage sums are cmap.sums of the [D, N] storage block."""
    from lgar_py_amd.catchments import CatchmentMap
    from lgar_py_amd.model import dpLGAR
    from _model_files import model_cfg as _cfg
    g = np.load(os.path.join(GOLDEN, "phil_hourly_3000.npz"))
    many = dpLGAR(_cfg(tmp_path, g, n=40), n_columns=5)
    cmap = CatchmentMap([0, 1, 1, -1, 0], n_catchments=3, weights=[0.5, 0.25, 0.75, 1.0, 0.5], device=many.engine.device)
    for edges, D in ((None, 3), ([0.0, 10.0, 50.0], 2)):
        got = many.soil_moisture(edges, catchments=cmap)
        block = many.engine.soil_moisture(edges, "storage")
        assert tuple(got.shape) == (D, 3) and got.dtype == torch.float64
        assert torch.equal(got, cmap.sums(block, status=many.engine.status)) and torch.equal(got, cmap.sums(block))
        assert bool((got[:, 2] == 0).all()) and bool((got[:, :2] > 0).all())
        ref, _ = CH.sums_ref(block.cpu().numpy(), cmap.offsets_host, cmap.order_host, cmap.weights(block.dtype).cpu().numpy(), None)
        assert CH.same_bits(got.cpu().numpy(), ref)
