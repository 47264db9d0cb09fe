"""CPU: the DEVICE CODE (lgar_py_amd/csrc/*.hpp: column physics, per-lane kernel bodies, front-capacity chain, tangent
kernels) compiled for the host by the test-only simulator (tests/devsim) against the vectors captured from the reference.
The same source runs on the GPU (tests/test_gpu_*.py repeat these checks there through the C-ABI); here logic errors
surface without a GPU.  Bars and checks: tests/_golden.py, the same as on the GPU."""
import numpy as np
import pytest

import _golden as G
from _golden import GRADS, TRAJ, load, to_numpy as _np


def _engine(g, ncol, dtype=np.float64, **kw):
    import devsim
    return devsim.SimEngine(*G.soil(g), n_columns=ncol, dtype=dtype, **G.engine_keywords(g), **kw)


@pytest.mark.parametrize("mode", [1, 2], ids=["fast", "fast_capacity_chain"])
@pytest.mark.parametrize("name", TRAJ)
def test_device_code_fp64_trajectory_vs_reference_golden(name, mode):
    G.trajectory_vs_reference(_engine, name, 2, G.check_native_trajectory, search_mode=mode, call_sums=True)


# engine settings per mode: fast through the capacity chain, literal, mixed precision; (bar, usual) from _golden.py
STEPWISE_MODES = {"fast": (dict(search_mode=2), G.STEPWISE_NATIVE), "literal": (dict(search_mode=0), G.STEPWISE_LITERAL),
                  "mixed": (dict(search_mode=2, geff_mode=1), G.STEPWISE_MIXED_SIM)}


@pytest.mark.parametrize("mode", list(STEPWISE_MODES))
@pytest.mark.parametrize("name", TRAJ)
def test_device_code_front_table_at_every_step_vs_reference_golden(name, mode):
    """north_star: "per-front depth/theta".  The engine is stepped one forcing row at a time and its WHOLE front table --
    front count, layer tags, to_bottom flags, depth, theta (layers/WettingFront.py:38-49, models/dpLGAR.py:176-298) -- is compared
    with the reference's at EVERY step, not only at the last one."""
    kw, (bar, usual) = STEPWISE_MODES[mode]
    g = load(name)
    T = G.steps_before_crash(g, G.STEPWISE_LITERAL_STEPS if mode == "literal" else None)[1]
    G.check_front_table_at_every_step(g, G.run_row_by_row(_engine, g, 1, T, **kw), T, bar, usual)


@pytest.mark.parametrize("name", ["synth1_phil", "phil_hourly_3000", "four_layer_synth0_600", "two_layer_phil_600",
                                  "closedG_synth1_phil", "frozen07_phil_hourly_400", "manyfronts_pulse_84", "rand06"])
def test_device_code_literal_mode_vs_reference_golden(name):
    """search_mode 0: the reference's literal line searches, update_psi pass and (fp64) operation-by-operation trapezoid."""
    g = load(name)
    run = G.run_trajectory(_engine, g, 1, search_mode=0)
    G.check_accumulators(g, run["acc"][:, 0], run["T"], G.LITERAL)
    G.check_clean(run["status"])
    assert int(run["eng"].n_fronts[0]) == int(g["nfronts"][run["T"] - 1])


@pytest.mark.parametrize("name", TRAJ)
def test_device_code_mixed_precision_geff_vs_reference_golden(name):
    """The mixed-precision Geff (search_mode 2, geff_mode 1) within the mixed-mode bars of _golden.py."""
    G.trajectory_vs_reference(_engine, name, 2, G.check_mixed_trajectory, search_mode=2, geff_mode=1)


def test_mixed_precision_geff_leaf_accuracy():
    """The mixed trapezoid against the reference's literal one (library pow) over the ranges the three call sites see: no
    systematic error, <= 3e-7 relative for every input (observed on the CPU: median 8e-9, 99th percentile 7e-8, max 1.6e-7;
    the plain fp32 loop: median 1e-6, 99th percentile 6e-4)."""
    import ctypes as C
    import devsim
    L = devsim.lib(3)
    dp = np.ctypeslib.ndpointer(dtype=np.float64)
    L.devsim_geff.argtypes = [C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, dp, C.c_int, dp]
    rng = np.random.default_rng(0)
    n = 4000
    alpha, nn = rng.uniform(0.003, 0.009, n), rng.uniform(1.25, 1.75, n)
    ks, te, tr = np.full(n, 0.3), np.full(n, 0.46), np.full(n, 0.07)

    def run(v, t1, t2):
        o = np.zeros(n)
        L.devsim_geff(v, n, np.ascontiguousarray(t1), np.ascontiguousarray(t2), alpha, nn, ks, te, tr, 120, o)
        return o

    theta = lambda h: tr + (te - tr) * (1 + (alpha * h) ** nn) ** -(1 - 1 / nn)
    h1 = 10 ** rng.uniform(0.5, 3.3, n)
    for t1, t2 in ((theta(h1), te.copy()), (theta(h1), theta(h1 * 10 ** rng.uniform(-2, -0.05, n))),
                   (theta(h1), theta(h1 * rng.uniform(0.7, 0.98, n)))):
        ref, mix = run(2, t1, t2), run(1, t1, t2)
        e = (mix - ref) / ref
        assert np.abs(e).max() <= 3e-7 and np.median(np.abs(e)) <= 3e-8 and abs(e.mean()) <= 1e-8
        assert np.abs(run(0, t1, t2) - ref).max() <= 1e-11 * np.abs(ref).max()  # the fused fp64 trapezoid, for scale


def test_mixed_precision_flags_the_columns_the_oracle_flags():
    """Fault parity of the mixed mode on the +-10 % ensemble (the reference raises on ~13 % of it): same columns flagged,
    the others within the mixed-mode bars."""
    import devsim
    o = G.oracle_ensemble(192, seed=7, scale=(8,))
    eng = devsim.SimEngine(*o["cols"], **o["kw"], search_mode=1, geff_mode=1)
    out = _np(eng.forward(o["pr"], o["pe"], series=("runoff",)))
    G.check_oracle_agreement(o, _np(eng.status), out["runoff"], _np(eng.totals), flips=(), mixed=True)


def test_capacity_chain_hands_columns_over_and_resumes():
    """Columns with few fronts finish in the 8-slot kernel, the others move to 16 and 32 slots at different steps of the
    same call; results equal the single-kernel run bitwise, chunked calls included, and the per-call sums add up."""
    import devsim
    g = load("manyfronts_pulse_84")
    N, T = 6, 84
    scale = np.array([1.0, 0.0, 1.0, 0.3, 1.0, 0.6])  # column 1 never sees rain, the others grow at different rates
    pr = g["forcing"][:T, 0:1] * scale[None, :]
    pe = np.zeros_like(pr)
    a = _engine(g, N, search_mode=1)
    ref = _np(a.forward(pr, pe, series=devsim.ACC_NAMES, basin=("runoff", "infiltration"), call_sums=True))
    assert a.n_fronts.max() > 16 and a.n_fronts.min() == 3 and (a.status == 0).all()
    b = _engine(g, N, search_mode=2)
    got = _np(b.forward(pr, pe, series=devsim.ACC_NAMES, basin=("runoff", "infiltration"), call_sums=True))
    for nm in ref:
        if nm.startswith("basin") or nm == "call_sums":  # sums are split at the hand-over points: last-bit differences
            assert np.allclose(got[nm], ref[nm], rtol=1e-13, atol=1e-15), nm
        else:
            assert np.array_equal(got[nm], ref[nm]), nm
    for x, y in ((a.depth, b.depth), (a.theta, b.theta), (a.psi, b.psi), (a.dzdt, b.dzdt), (a.flags, b.flags),
                 (a.n_fronts, b.n_fronts), (a.scalars, b.scalars), (a.status, b.status)):
        assert np.array_equal(_np(x), _np(y))
    assert np.allclose(_np(a.totals), _np(b.totals), rtol=1e-14, atol=0)
    c = _engine(g, N, search_mode=2)  # ragged chunks: hand-overs happen in different calls
    parts = []
    for lo, hi in ((0, 7), (7, 30), (30, 31), (31, 70), (70, 84)):
        parts.append(_np(c.forward(pr[lo:hi], pe[lo:hi], series=("runoff", "ending_volume"), call_sums=True)))
        assert (c.status == 0).all()  # LGAR_ST_RESUME never survives a call
    assert np.array_equal(np.concatenate([p["runoff"] for p in parts]), ref["runoff"])
    assert np.array_equal(np.concatenate([p["ending_volume"] for p in parts]), ref["ending_volume"])
    assert np.allclose(sum(p["call_sums"][:8] for p in parts), ref["call_sums"][:8], rtol=1e-13, atol=1e-15)
    assert np.array_equal(_np(c.n_fronts), _np(a.n_fronts)) and np.array_equal(_np(c.depth), _np(a.depth))


def test_front_overflow_is_flagged_at_the_reference_state_limit():
    """The reference's lists are unbounded; here a column holds at most front_slots (<= 32) fronts: one more -> the
    column stops with LGAR_ST_OVERFLOW, in every mode, with the state arrays never written past their rows."""
    import devsim
    g = load("manyfronts_pulse_84")
    f = np.concatenate([g["forcing"], g["forcing"][:40] * 0 + np.array([[0.02, 0.0]])])  # keep pulsing past 32 fronts
    T = g["forcing"].shape[0]
    for mode in (0, 1, 2):
        for slots in (None, 10):
            eng = _engine(g, 1, search_mode=mode, front_slots=slots)
            pr = np.concatenate([g["forcing"][:, 0], np.tile([0.02, 0.0], 30)])[:, None]
            eng.forward(pr, np.zeros_like(pr), series=())
            lim = slots or 32
            assert int(eng.status[0]) & 8, (mode, slots)
            assert int(eng.n_fronts[0]) == lim
            assert eng.depth.shape[0] == lim


def test_device_code_fp32_close_to_reference():
    """The fp32 instantiation (bench.py's configuration; host libm stands in for v_log_f32 / v_exp_f32) on the golden
    cases of its workload family: run totals within 5e-3 of the reference."""
    import devsim
    for name in ("synth1_phil", "synth1_pert0", "synth1_pert3", "synth2_phil", "phil_pert1_500"):
        g = load(name)
        eng = _engine(g, 1, dtype=np.float32)
        f = g["forcing"]
        eng.forward(f[:, 0:1], f[:, 1:2], series=())
        assert int(eng.status[0]) == 0
        ref = g["acc"][:, :8].sum(0)
        got = _np(eng.totals)[:8, 0].astype(np.float64)
        scale = max(ref[0], 1.0)  # precipitation scale
        assert np.abs(got - ref).max() <= 5e-3 * scale, (name, got, ref)
        assert abs(float(eng.totals[9, 0]) - g["acc"][-1, 9]) <= 5e-3 * g["acc"][-1, 9]


@pytest.mark.parametrize("mode", [1, 2, 0], ids=["fast", "fast_capacity_chain", "literal"])
@pytest.mark.parametrize("name", GRADS)
def test_device_tangent_matches_reference_autograd(name, mode):
    """Forward-mode tangents of the device code (Dual numbers) contracted with d loss / d runoff_t reproduce the gradients
    torch autograd produced through the reference (loss = mean(runoff^2)): nominal, 4-layer, +-10 % ensemble members,
    wide-range ensemble members, and a column with up to 19 fronts."""
    g = load(name)
    f = g["forcing"]
    T = f.shape[0]
    L = len(g["alpha"])
    eng = _engine(g, 1, search_mode=mode)
    out = _np(eng.forward(f[:, 0:1], f[:, 1:2], series=("runoff",)))
    r = out["runoff"][:, 0]
    loss = float(np.mean(r * r))
    w = (2.0 * r / T)[:, None]
    got = {kind: np.zeros(L) for kind in ("alpha", "n", "ksat")}
    for kind in got:
        for l in range(L):
            d = np.zeros((L, 1))
            d[l] = 1.0
            gr, _, st = _np(eng.tangent({kind: d}, f[:, 0:1], f[:, 1:2], w_runoff=w))
            assert int(st[0]) == 0
            got[kind][l] = gr[0]
    G.check_gradients(g, loss, got)


def test_tangent_capacity_chain_and_status():
    """Tangent kernels: the 8-slot kernel hands the many-front column to the 32-slot kernel (same gradient as the
    single-kernel run), and a column that overflows even that reports it in the tangent status."""
    g = load("grad_manyfronts_60")
    f = g["forcing"]
    T = f.shape[0]
    N = 3
    scale = np.array([1.0, 0.0, 0.5])
    pr, pe = f[:, 0:1] * scale[None, :], np.zeros((T, N))
    w = np.ones((T, N))
    d = np.zeros((3, N))
    d[0] = 1.0
    g1, _, s1 = _np(_engine(g, N, search_mode=1).tangent({"ksat": d}, pr, pe, w_runoff=w))
    g2, _, s2 = _np(_engine(g, N, search_mode=2).tangent({"ksat": d}, pr, pe, w_runoff=w))
    assert (s1 == 0).all() and (s2 == 0).all()
    assert np.array_equal(g1, g2) and g1[0] != 0.0 and g1[1] == 0.0
    long = np.concatenate([load("manyfronts_pulse_84")["forcing"][:, 0], np.tile([0.02, 0.0], 30)])[:, None]
    gl, _, sl = _np(_engine(g, 1, search_mode=2).tangent({"ksat": d[:, :1]}, long, np.zeros_like(long), w_runoff=np.ones_like(long)))
    assert int(sl[0]) & 8


def test_columns_outside_the_reference_domain_are_flagged_like_the_oracle():
    """+-10 % perturbed columns under the synth_1 storm: ~13 % of them make the reference raise ValueError (negative pow
    base in insert_water's Geff, quirk q3).  Device code (every mode) and oracle must flag exactly the same columns and
    agree on all the others."""
    import devsim
    o = G.oracle_ensemble(192, seed=7, scale=(8,))
    assert 0 < (o["st"] != 0).mean() < 0.5
    for mode in (0, 1, 2):
        eng = devsim.SimEngine(*o["cols"], **o["kw"], search_mode=mode)
        out = _np(eng.forward(o["pr"], o["pe"], series=("runoff",)))
        G.check_oracle_agreement(o, _np(eng.status), out["runoff"], _np(eng.totals), flips=())


def test_forcing_broadcast_equals_replicated_forcing():
    """LgarDims.forcing_columns: soil column c reads forcing column c % Nf.  One basin series for every column (Nf = 1, what
    the reference's Data yields) and the direction-major layout of the differentiable path (Nf = N / D) give bitwise the
    results of explicitly replicated forcing, forward and tangent."""
    import devsim
    g = load("synth0_phil_1500")
    f = g["forcing"][:200]
    N = 6
    a = _engine(g, N)
    full = _np(a.forward(np.repeat(f[:, 0:1], N, 1), np.repeat(f[:, 1:2], N, 1), series=("runoff", "AET")))
    b = _engine(g, N)
    one = _np(b.forward(f[:, 0:1], f[:, 1:2], series=("runoff", "AET")))
    for nm in full:
        assert np.array_equal(full[nm], one[nm])
    assert np.array_equal(_np(a.theta), _np(b.theta)) and np.array_equal(_np(a.totals), _np(b.totals))
    sc = np.array([1.0, 0.5, 0.8])
    pr3, pe3 = f[:, 0:1] * sc[None, :], f[:, 1:2] * np.ones((1, 3))
    c = _engine(g, N)
    half = _np(c.forward(pr3, pe3, series=("runoff",)))  # columns 0..2 and 3..5 see forcing columns 0..2
    d = _engine(g, N)
    rep = _np(d.forward(np.tile(pr3, (1, 2)), np.tile(pe3, (1, 2)), series=("runoff",)))
    assert np.array_equal(half["runoff"], rep["runoff"])
    w = np.linspace(0.5, 1.5, 200)[:, None] * np.ones((1, 3))
    dirs = np.zeros((3, N))
    dirs[0, :3] = 1.0   # first direction: layer-0 Ksat on columns 0..2
    dirs[1, 3:] = 1.0   # second direction: layer-1 Ksat on columns 3..5 (same soils, same forcing)
    g1, _, s1 = _np(c.tangent({"ksat": dirs}, pr3, pe3, w_runoff=w))
    g2, _, s2 = _np(d.tangent({"ksat": dirs}, np.tile(pr3, (1, 2)), np.tile(pe3, (1, 2)), w_runoff=np.tile(w, (1, 2))))
    assert np.array_equal(g1, g2) and (s1 == 0).all() and np.abs(g1).max() > 0
    # forcing_group: G consecutive columns share a forcing column (the differentiable path's interleaved directions)
    e = _engine(g, N)
    grp = _np(e.forward(pr3, pe3, series=("runoff",), forcing_group=2))  # columns (0,1), (2,3), (4,5) see forcing columns 0, 1, 2
    assert np.array_equal(grp["runoff"], rep["runoff"][:, [0, 3, 1, 4, 2, 5]])
    dirs2 = np.zeros((3, N))
    dirs2[0, 0::2] = 1.0
    dirs2[1, 1::2] = 1.0
    g3, _, s3 = _np(e.tangent({"ksat": dirs2}, pr3, pe3, w_runoff=w, forcing_group=2))
    assert np.array_equal(g3, g2[[0, 3, 1, 4, 2, 5]]) and (s3 == 0).all()


def test_nan_in_the_forcing_is_flagged():
    """The reference lets a NaN forcing value through (comparisons with it are false, the step's runoff is NaN, nothing
    raises); the engine flags the column (LGAR_ST_NAN) so that the caller hears about the bad datum."""
    g = load("synth1_phil")
    f = g["forcing"].copy()
    f[100, 0] = np.nan
    for mode in (0, 1):
        e = _engine(g, 2, search_mode=mode)
        pr = np.stack([f[:, 0], g["forcing"][:, 0]], 1)
        pe = np.stack([f[:, 1], g["forcing"][:, 1]], 1)
        e.forward(pr, pe, series=("runoff",))
        assert e.status[0] & 1 and e.status[1] == 0


@pytest.mark.parametrize("name", ["rand03", "synth2_phil", "bench_col10707", "five_layer_synth1", "manyfronts_pulse_84"])
def test_giuh_queue_in_place_survives_cut_launches_and_matches_the_reference_queue(name):
    """The mixed-precision kernels update the GIUH queue in place in the `scalars` rows of the state (ModeTraits::giuh_mem) instead of
    carrying it in registers; the flag "something is queued" is rebuilt from those rows at every launch.  A run cut into four
    launches must equal the one-launch run bit for bit -- series, scalars, front table --, and at every cut the queue rows must
    hold the reference's own queue (lgar/giuh.py:8-20; fixtures: `giuh_queue[t]`): to 1e-9 in the native mode, to the
    mixed-mode flux bar otherwise."""
    import devsim
    g = load(name)
    T = g["forcing"].shape[0]
    f = g["forcing"]
    pr, pe = np.repeat(f[:, 0:1], 2, 1), np.repeat(f[:, 1:2], 2, 1)
    ng = len(g["giuh_ordinates"])
    cuts = (7, 31, 32, T)
    for geff_mode, bar in ((1, G.MIXED_FLUX), (0, 1e-9)):
        one = _engine(g, 2, search_mode=2, geff_mode=geff_mode)
        whole = _np(one.forward(pr, pe, series=devsim.ACC_NAMES))
        cut = _engine(g, 2, search_mode=2, geff_mode=geff_mode)
        parts, t0 = [], 0
        scale = max(float(np.abs(g["giuh_queue"]).max()), 1e-6)
        for t1 in cuts:
            if t1 <= t0:
                continue
            parts.append(_np(cut.forward(pr[t0:t1], pe[t0:t1], series=devsim.ACC_NAMES)))
            q = _np(cut.scalars)[3:3 + ng, 0]
            assert np.abs(q - g["giuh_queue"][t1 - 1]).max() <= bar * scale, (geff_mode, t1)
            assert (cut.scalars[3 + ng:, 0] == 0).all()
            t0 = t1
        for nm in devsim.ACC_NAMES:
            assert np.array_equal(np.concatenate([p[nm] for p in parts], 0), whole[nm]), (geff_mode, nm)
        assert np.array_equal(_np(cut.scalars), _np(one.scalars)) and np.array_equal(_np(cut.status), _np(one.status))
        a, b = cut.fronts(), one.fronts()
        assert all(np.array_equal(a[k], b[k]) for k in a)
        assert (whole["giuh_runoff"][:, 0] > 0).sum() > 3  # the fixture routes runoff
