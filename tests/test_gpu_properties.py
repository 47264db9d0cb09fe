"""GPU (-m gpu): size-independent properties of the HIP path at BASELINE.json's full single-GPU size (configs[2]: 1 048 576
synthetic columns x 144 steps, fp32, fast search) -- the oracle cannot run a million columns in seconds, these can be
checked exactly:

* replicas: the job is 16 384 distinct columns tiled 64 times in a scrambled order, so equal columns sit in different
  wavefronts next to different neighbours; every copy must give bit-identical series (a column's result may not depend on
  which columns share its wavefront);
* permutation: permuting the columns permutes the outputs, bit for bit;
* mass closure per column: precipitation = infiltration + runoff + ponded water on every column; start volume +
  infiltration = AET + percolation + end volume within fp32 rounding on the bulk of the columns (the reference computes the
  same residual per step, layers/Layer.py:795-824, and itself loses water in a few columns, see the test);
* basin sums are linear in the weights;
* the first 1024 columns equal the fp64 oracle within the fp32 tolerance of tests/test_gpu_parity.py (anchors the big job
  to the checker).

Plus the accuracy of the lean fp64 log2 / exp2 / pow on the real hardware (the CPU simulator divides exactly where the
device uses v_rcp_f64 + Newton, so only a GPU run measures the shipped arithmetic)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_FULL = 1 << 20
N_DISTINCT = 1 << 14


def _job(dtype, order=None):
    """(engine, precip[T,N], pet[T,N], order): N_FULL columns = N_DISTINCT distinct ones, column j is distinct column order[j]"""
    import lgar_py_amd as lg
    from lgar_py_amd import workloads as W
    P = W.perturbed_columns(N_DISTINCT, seed=0)
    sc = W.forcing_scale(N_DISTINCT, seed=1000)
    if order is None:
        order = np.random.default_rng(7).permutation(N_FULL) % N_DISTINCT
    f = W.synth1_forcing()
    Q = {k: np.ascontiguousarray(v[:, order]) for k, v in P.items()}
    eng = lg.LgarEngine(Q["alpha"], Q["n"], Q["ksat"], Q["theta_e"], Q["theta_r"], Q["thickness"], dt_h=300.0 / 3600.0,
                        ponded_depth_max=0.0, dtype=dtype)
    pr = (torch.tensor(f[:, 0], device="cuda")[:, None] * torch.tensor(sc[order], device="cuda")[None, :]).to(dtype).contiguous()
    pe = torch.zeros_like(pr)
    return eng, pr, pe, order


@pytest.fixture(scope="module")
def full_run():
    eng, pr, pe, order = _job(torch.float32)
    w = torch.rand(N_FULL, device="cuda", dtype=torch.float32)
    start = eng.ending_volume.double().clone()  # set_internal_states' volume (models/dpLGAR.py:131-137)
    out = eng.forward(pr, pe, series=("runoff", "percolation"), basin=("runoff",), weights=w, check=False)
    torch.cuda.synchronize()
    return dict(eng=eng, pr=pr, pe=pe, order=order, out=out, w=w, start=start)


def _first_copy(order):
    """for every distinct column, the position of its first copy; and for every column the position of that first copy"""
    first = np.full(N_DISTINCT, -1, dtype=np.int64)
    u, pos = np.unique(order, return_index=True)
    first[u] = pos
    return first, first[order]


def test_replicated_columns_are_bitwise_equal_across_wavefronts(full_run):
    order, out, eng = full_run["order"], full_run["out"], full_run["eng"]
    _, ref_pos = _first_copy(order)
    ref_pos = torch.tensor(ref_pos, device="cuda")
    for k in ("runoff", "percolation"):
        s = out[k]
        assert torch.equal(s, s[:, ref_pos]), k
    assert torch.equal(eng.status, eng.status[ref_pos])
    assert torch.equal(eng.totals, eng.totals[:, ref_pos])
    assert torch.equal(eng.n_fronts, eng.n_fronts[ref_pos])


def test_permuting_the_columns_permutes_the_outputs(full_run):
    order = full_run["order"]
    perm = np.random.default_rng(11).permutation(N_FULL)
    eng2, pr2, pe2, _ = _job(torch.float32, order=order[perm])
    out2 = eng2.forward(pr2, pe2, series=("runoff",), check=False)
    p = torch.tensor(perm, device="cuda")
    assert torch.equal(out2["runoff"], full_run["out"]["runoff"][:, p])
    assert torch.equal(eng2.status, full_run["eng"].status[p])
    assert torch.equal(eng2.totals, full_run["eng"].totals[:, p])


def test_mass_closes_on_every_valid_column(full_run):
    eng = full_run["eng"]
    ok = (eng.status == 0)
    assert float(ok.float().mean()) > 0.9
    tot = eng.totals.double()  # rows: precip, pet, aet, infiltration, runoff, percolation, giuh, discharge, ponded, end volume
    surface = tot[0] - tot[3] - tot[4] - tot[8]
    assert float(surface[ok].abs().max()) <= 1e-4
    end = eng.ending_volume.double()
    soil = full_run["start"] + tot[3] - tot[2] - tot[5] - end
    # the reference itself drops one sub-step's infiltration in a few columns (top layer saturated, front advancing in
    # layer 2: fixtures bench_col15731 / bench_col10707 are its own runs, 0.125 cm lost in one step), so the worst column
    # is not a property; the bulk is
    soil = (soil.abs() / torch.clamp(end.abs(), min=1.0))[ok]
    assert float(soil.median()) <= 1e-5 and float(torch.quantile(soil[:1 << 20].float(), 0.99)) <= 1e-4
    assert float((soil > 1e-3).double().mean()) <= 0.02
    # the series add up to the totals the kernel keeps
    ro = full_run["out"]["runoff"].double().sum(0)
    assert float(((ro - tot[4]).abs() / torch.clamp(tot[0], min=1.0))[ok].max()) <= 1e-5


def test_basin_sums_are_the_weighted_column_sums_and_linear(full_run):
    out, w, eng = full_run["out"], full_run["w"], full_run["eng"]
    ok = (eng.status == 0)
    b = out["basin:runoff"].double()
    direct = (out["runoff"].double() * w.double()[None, :]).sum(1)
    scale = float(direct.abs().max())
    assert float((b - direct).abs().max()) <= 2e-5 * scale  # fp32 partial sums per wavefront, fp64 atomics across them
    # linearity: weights a*w1 + w2 in one launch = a*basin(w1) + basin(w2) from two more
    eng2, pr, pe, _ = _job(torch.float32, order=full_run["order"])
    w1 = torch.rand(N_FULL, device="cuda", dtype=torch.float32)
    w2 = ok.float()
    res = []
    for ww in (w1, w2, 0.5 * w1 + w2):
        eng2.reset()
        res.append(eng2.forward(pr, pe, series=(), basin=("runoff",), weights=ww, check=False)["basin:runoff"].double())
    assert float((res[2] - (0.5 * res[0] + res[1])).abs().max()) <= 2e-5 * float(res[2].abs().max())


def test_head_of_the_full_job_matches_the_oracle(full_run):
    from lgar_py_amd import workloads as W
    from oracle import lgar_oracle as O
    order, eng = full_run["order"], full_run["eng"]
    n = 1024
    P = W.perturbed_columns(N_DISTINCT, seed=0)
    sc = W.forcing_scale(N_DISTINCT, seed=1000)
    f = W.synth1_forcing()
    sel = order[:n]
    pr = f[:, 0:1] * sc[sel][None, :]
    ro, pc, acc, st = O.run_columns(*(np.ascontiguousarray(P[k][:, sel]) for k in ("alpha", "n", "ksat", "theta_e", "theta_r", "thickness")),
                                    pr, np.zeros_like(pr), pdm=0.0, dt_h=300.0 / 3600.0)
    gst = eng.status[:n].cpu().numpy()
    ok = (st == 0) & (gst == 0)
    assert ok.mean() > 0.5
    tot = eng.totals[:, :n].double().cpu().numpy()
    for j in (0, 3, 9):
        r = np.abs(tot[j] - acc[j])[ok] / np.maximum(np.abs(acc[j][ok]), 1e-2)
        assert np.percentile(r, 99) <= 5e-3 and r.max() <= 5e-2, (j, r.max())
    dro = np.abs(tot[4] - acc[4])[ok] / np.maximum(acc[0][ok], 1.0)
    assert np.percentile(dro, 99) <= 5e-3 and dro.max() <= 5e-2


def test_fp32_kernel_against_the_fp64_kernel_on_131072_columns():
    """The throughput precision against the parity precision on the bench ensemble, at a size no CPU checker reaches: run
    totals of the columns both integrate agree to 2e-5 (median) / 5e-3 (99th percentile) relative; the basin runoff of the
    whole ensemble to 1e-3.  (fp32 cannot hold the reference's 1e-12 mass tolerance; a handful of columns take another
    branch at a psi tie, hence percentiles -- DESIGN.md section 4.)"""
    import lgar_py_amd as lg
    from lgar_py_amd import workloads as W
    N = 1 << 17
    P = W.perturbed_columns(N, seed=0)
    sc = W.forcing_scale(N, seed=1000)
    f = W.synth1_forcing()
    res = {}
    for dt in (torch.float64, torch.float32):
        eng = lg.LgarEngine(P["alpha"], P["n"], P["ksat"], P["theta_e"], P["theta_r"], P["thickness"], dt_h=300.0 / 3600.0,
                            ponded_depth_max=0.0, dtype=dt)
        pr = (torch.tensor(f[:, 0], device="cuda")[:, None] * torch.tensor(sc, device="cuda")[None, :]).to(dt).contiguous()
        out = eng.forward(pr, torch.zeros_like(pr), series=(), basin=("runoff",), weights=None, check=False)
        res[dt] = (eng.totals.double(), eng.status.clone(), out["basin:runoff"].clone())
    t64, s64, b64 = res[torch.float64]
    t32, s32, b32 = res[torch.float32]
    ok = (s64 == 0) & (s32 == 0)
    assert float(ok.double().mean()) > 0.8
    for j, scale_row in ((3, 3), (4, 0), (9, 9)):  # infiltration, runoff (against the precipitation scale), end volume
        r = ((t32[j] - t64[j]).abs() / torch.clamp(t64[scale_row].abs(), min=1.0))[ok].float()
        assert float(r.median()) <= 2e-5, (j, float(r.median()))
        assert float(torch.quantile(r, 0.99)) <= 5e-3, (j, float(torch.quantile(r, 0.99)))
    # the basin sums include the few columns only one precision integrates to the end: compare on the common ones
    w = ok.double()
    tot32 = float((t32[4] * w).sum())
    tot64 = float((t64[4] * w).sum())
    assert abs(tot32 - tot64) <= 1e-3 * abs(tot64)


def test_fp64_replicas_and_chunking_at_scale():
    """fp64 (the parity precision), 262 144 columns: replicas bitwise equal, and 3 launches of 48 steps = 1 launch of 144"""
    import lgar_py_amd as lg
    from lgar_py_amd import workloads as W
    n = 1 << 18
    order = np.random.default_rng(3).permutation(n) % 4096
    P = W.perturbed_columns(4096, seed=5)
    sc = W.forcing_scale(4096, seed=6)
    f = W.synth1_forcing()
    Q = {k: np.ascontiguousarray(v[:, order]) for k, v in P.items()}
    mk = lambda: lg.LgarEngine(Q["alpha"], Q["n"], Q["ksat"], Q["theta_e"], Q["theta_r"], Q["thickness"], dt_h=300.0 / 3600.0,
                               ponded_depth_max=0.0, dtype=torch.float64)
    pr = (torch.tensor(f[:, 0], device="cuda")[:, None] * torch.tensor(sc[order], device="cuda")[None, :]).contiguous()
    pe = torch.zeros_like(pr)
    a = mk()
    one = a.forward(pr, pe, series=("runoff",), check=False)["runoff"]
    first = np.full(4096, -1, dtype=np.int64)
    u, pos = np.unique(order, return_index=True)
    first[u] = pos
    ref_pos = torch.tensor(first[order], device="cuda")
    assert torch.equal(one, one[:, ref_pos])
    b = mk()
    parts = [b.forward(pr[s:s + 48].contiguous(), pe[s:s + 48].contiguous(), series=("runoff",), check=False)["runoff"].clone()
             for s in (0, 48, 96)]
    assert torch.equal(torch.cat(parts, 0), one)
    assert torch.equal(a.status, b.status) and torch.equal(a.n_fronts, b.n_fronts)


def test_device_log2_exp2_pow_accuracy_on_hardware():
    """lgar_math.hpp on the GPU against x87 long double: log2 <= 5e-16 (relative to max(1, |log2 x|)), <= 5e-15 relative to
    itself near x = 1; exp2 <= 3e-16; pow <= 5e-14 over |y log2 x| <= 160 (measured: 2.4e-16, 2.3e-15, 1.4e-16, 1.7e-14)."""
    import lgar_py_amd as lg
    rng = np.random.default_rng(0)
    n = 1 << 18
    one = np.ones(n)
    kw = dict(alpha=one, n=one * 2, ksat=one, theta_e=one, theta_r=one * 0)
    L = np.longdouble
    x = np.concatenate([np.exp(rng.uniform(np.log(1e-12), np.log(1e12), n // 2)), 1.0 + rng.uniform(-0.3, 0.4, n // 2)])
    got = lg.leaf_batch("log2", x, **kw).cpu().numpy().astype(L)
    ref = np.log2(x.astype(L))
    assert float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref)))) <= 5e-16
    near = (np.abs(x - 1.0) < 0.4) & (x != 1.0)
    assert float(np.max(np.abs(got[near] - ref[near]) / np.abs(ref[near]))) <= 5e-15
    y = rng.uniform(-1000.0, 1000.0, n)
    got = lg.leaf_batch("exp2", y, **kw).cpu().numpy().astype(L)
    ref = np.exp2(y.astype(L))
    assert float(np.max(np.abs(got - ref) / ref)) <= 3e-16
    xb = np.exp(rng.uniform(np.log(1e-8), np.log(1e8), n))
    yb = rng.uniform(-6.0, 6.0, n)
    got = lg.leaf_batch("pow", xb, yb, **kw).cpu().numpy().astype(L)
    ref = np.power(xb.astype(L), yb.astype(L))
    assert float(np.max(np.abs(got - ref) / ref)) <= 5e-14


def test_lean_division_and_pairwise_polynomials_on_hardware():
    """The fast modes' double-precision quotient (v_rcp_f64 + one Newton step + one correction, lgar_scalar.hpp lean_div) against
    the exact quotient: <= 1 ulp (2.3e-16 relative; measured 1.2e-16), over the magnitudes the column physics divides; and the
    mixed-precision kernels' log2 / exp2 / pow (high-order terms combined pairwise) to the bounds of the Horner forms."""
    import lgar_py_amd as lg
    rng = np.random.default_rng(1)
    n = 1 << 18
    one = np.ones(n)
    kw = dict(alpha=one, n=one * 2, ksat=one, theta_e=one, theta_r=one * 0)
    L = np.longdouble
    a = np.exp(rng.uniform(np.log(1e-12), np.log(1e12), n)) * rng.choice([-1.0, 1.0], n)
    b = np.exp(rng.uniform(np.log(1e-12), np.log(1e12), n)) * rng.choice([-1.0, 1.0], n)
    got = lg.leaf_batch("div", a, b, **kw).cpu().numpy().astype(L)
    ref = a.astype(L) / b.astype(L)
    assert float(np.max(np.abs(got - ref) / np.abs(ref))) <= 2.3e-16
    assert float(lg.leaf_batch("div", [0.0], [3.0], **{k: v[:1] for k, v in kw.items()})[0]) == 0.0
    # the edges: a zero, infinite or denormal divisor, an infinite dividend -- the IEEE quotient, not the NaN of a Newton step
    # through inf * 0 (an overflowed (alpha h)^n in theta_from_h must give theta_r)
    ea = np.array([1.0, 1.0, 1.0, 1.0, 0.0, np.inf, np.inf, 3.0, -2.0, 1e300, 0.0])
    eb = np.array([0.0, np.inf, 5e-324, 1e308, np.inf, 2.0, 1e308, -0.0, 1e-310, 1e-300, 0.0])
    ke = {k: v[:len(ea)] for k, v in kw.items()}
    got = lg.leaf_batch("div", ea, eb, **ke).cpu().numpy()
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ref = ea / eb
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(ref).sum() == 1  # only 0 / 0
    ok = ~np.isnan(ref)
    assert np.array_equal(np.isinf(got[ok]), np.isinf(ref[ok])) and np.array_equal(np.sign(got[ok]), np.sign(ref[ok]))
    fin = ok & np.isfinite(ref) & (ref != 0)
    assert np.allclose(got[fin], ref[fin], rtol=1e-15, atol=0)
    x = np.concatenate([np.exp(rng.uniform(np.log(1e-12), np.log(1e12), n // 2)), 1.0 + rng.uniform(-0.3, 0.4, n // 2)])
    got = lg.leaf_batch("log2_pairwise", x, **kw).cpu().numpy().astype(L)
    ref = np.log2(x.astype(L))
    assert float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref)))) <= 5e-16
    near = (np.abs(x - 1.0) < 0.4) & (x != 1.0)
    assert float(np.max(np.abs(got[near] - ref[near]) / np.abs(ref[near]))) <= 5e-15
    y = rng.uniform(-1000.0, 1000.0, n)
    got = lg.leaf_batch("exp2_pairwise", y, **kw).cpu().numpy().astype(L)
    ref = np.exp2(y.astype(L))
    assert float(np.max(np.abs(got - ref) / ref)) <= 3e-16
    xb = np.exp(rng.uniform(np.log(1e-8), np.log(1e8), n))
    yb = rng.uniform(-6.0, 6.0, n)
    got = lg.leaf_batch("pow_pairwise", xb, yb, **kw).cpu().numpy().astype(L)
    ref = np.power(xb.astype(L), yb.astype(L))
    assert float(np.max(np.abs(got - ref) / ref)) <= 5e-14


@pytest.mark.parametrize("which", ["f32", "f64", "mixed"])
def test_the_same_job_twice_is_bit_identical(which):
    """Run-to-run determinism of the forward kernels (persistent waves pull their 64-column blocks in whatever order the
    hardware grants the tickets): the same 262 144-column job twice gives the same status words, series and front tables bit
    for bit.  Round 4 met two builds of the fp32 kernel that did not (an address-taken local array; a variant with 54 spilled
    registers) -- the replica tests above catch that too, this one says it in so many words."""
    import lgar_py_amd as lg
    from lgar_py_amd import workloads as W
    N = 1 << 18
    dt = torch.float32 if which == "f32" else torch.float64
    kw = dict(geff_precision="f32") if which == "mixed" else {}
    P = W.perturbed_columns(N, seed=0)
    sc = torch.tensor(W.forcing_scale(N, seed=1000), device="cuda")
    f = W.synth1_forcing()
    eng = lg.LgarEngine(P["alpha"], P["n"], P["ksat"], P["theta_e"], P["theta_r"], P["thickness"], dt_h=300.0 / 3600.0,
                        ponded_depth_max=0.0, dtype=dt, **kw)
    pr = (torch.tensor(f[:, 0], device="cuda")[:, None] * sc[None, :]).to(dt).contiguous()
    pe = torch.zeros_like(pr)
    # between the runs another kernel with a large scratch footprint (the mixed-precision one: 300 B per lane) leaves its own
    # bytes in the scratch memory the next run will be given: a kernel that read spill slots it had not written would show it
    dirty = lg.LgarEngine(P["alpha"], P["n"], P["ksat"], P["theta_e"], P["theta_r"], P["thickness"], dt_h=300.0 / 3600.0,
                          ponded_depth_max=0.0, dtype=torch.float64, geff_precision="f32")
    pr64, pe64 = pr.double(), pe.double()
    runs = []
    for k in range(3):
        if k:
            dirty.reset()
            dirty.forward(pr64[: 24 * k], pe64[: 24 * k], series=(), check=False)
        eng.reset()
        o = eng.forward(pr, pe, series=("runoff", "infiltration"), check=False)
        runs.append((eng.status.clone(), o["runoff"].clone(), o["infiltration"].clone(), eng.theta.clone(), eng.depth.clone(),
                     eng.totals.clone()))
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(torch.nan_to_num(a.double(), nan=-1.0), torch.nan_to_num(b.double(), nan=-1.0))


@pytest.mark.parametrize("which", ["f32", "f64", "mixed"])
@pytest.mark.parametrize("case", ["two_layers", "six_layers", "capacity_chain_16_and_32_slots"])
def test_the_same_job_twice_is_bit_identical_other_kernels(case, which):
    """... and the kernels the storm ensemble above does not reach: the two- and six-layer translation units, and -- under a pulsed
    rain that grows up to ~30 wetting fronts per column -- the 16- and 32-slot members of the front-capacity chain, which pick up
    the columns the 8-slot kernel hands over (persistent waves again: which wave integrates which block, and with what left in
    its LDS and scratch from the block before, differs from run to run)."""
    import lgar_py_amd as lg
    name = {"two_layers": "two_layer_synth1", "six_layers": "six_layer_synth1", "capacity_chain_16_and_32_slots": "manyfronts_pulse_84"}[case]
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    N = 1 << 17  # 2 048 wavefronts: above the 1 024 of a small job, so the capacity chain runs (include/lgar.h)
    rng = np.random.default_rng(11)
    L = len(g["alpha"])
    pert = lambda v: np.asarray(v, dtype=np.float64)[:, None] * (1.0 + 0.1 * (2.0 * rng.random((L, N)) - 1.0))
    dt = torch.float32 if which == "f32" else torch.float64
    kw = dict(geff_precision="f32") if which == "mixed" else {}
    eng = lg.LgarEngine(pert(g["alpha"]), pert(g["n"]), pert(g["ksat"]), pert(g["theta_e"]), pert(g["theta_r"]),
                        np.repeat(np.asarray(g["thickness"], dtype=np.float64)[:, None], N, 1), dt_h=float(g["dt_h"]),
                        num_subcycles=int(g["num_subcycles"]), ponded_depth_max=float(g["pdm"]), initial_psi=float(g["initial_psi"]),
                        wilting_point_psi=float(g["wilting_point_psi"]), nint=int(g["nint"]), dtype=dt, **kw)
    sc = torch.tensor(0.7 + 0.6 * rng.random(N), device="cuda")
    f = torch.tensor(g["forcing"], device="cuda")
    pr = (f[:, 0:1] * sc[None, :]).to(dt).contiguous()
    pe = f[:, 1:2].expand(-1, N).to(dt).contiguous()
    runs = []
    for k in range(3):
        eng.reset()
        o = eng.forward(pr, pe, series=("runoff", "infiltration"), check=False)
        runs.append((eng.status.clone(), o["runoff"].clone(), o["infiltration"].clone(), eng.theta.clone(), eng.depth.clone(),
                     eng.n_fronts.clone()))
    if case.startswith("capacity_chain"):
        ok = runs[0][0] == 0
        assert int(runs[0][5][ok].max()) > 16 and int(((runs[0][5] > 8) & ok).sum()) > N // 10  # the 16- and 32-slot kernels ran
    assert int((runs[0][0] == 0).sum()) > N // 2
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(torch.nan_to_num(a.double(), nan=-1.0), torch.nan_to_num(b.double(), nan=-1.0))
