"""GPU (-m gpu): the differentiable path (BASELINE configs[4]).  Gradients of loss = mean(runoff^2) w.r.t. the
van Genuchten parameters, computed by forward-mode tangents in the HIP kernel, against (1) the gradients the
reference's own torch autograd produced (golden fixtures grad_*.npz) and (2) central finite differences."""
import os

import numpy as np
import pytest

import _golden as G
from _golden import GRADS, engine_keywords
from _model_files import write_forcing, write_soil_dat
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _setup(g, N, dtype=torch.float64, **kw):
    T = g["forcing"].shape[0]
    f = torch.tensor(g["forcing"], device="cuda")
    pr = f[:, 0:1].expand(T, N).contiguous()
    pe = f[:, 1:2].expand(T, N).contiguous()
    P = {k: torch.tensor(np.repeat(g[k][:, None], N, 1), device="cuda", dtype=dtype) for k in
         ("alpha", "n", "ksat", "theta_e", "theta_r", "thickness")}
    ekw = dict(engine_keywords(g), dtype=dtype)
    ekw.update(kw)
    return P, pr, pe, ekw


@pytest.mark.parametrize("name", GRADS)
@pytest.mark.parametrize("mode", [1, 2, 0], ids=["fast_search", "fast_capacity_chain", "literal_search"])
@pytest.mark.parametrize("shared", [False, True], ids=["one_launch", "shared_trapezoid"])
def test_gradients_match_reference_autograd(name, mode, shared, monkeypatch):
    """Fixtures from the reference's own loss.backward(): nominal Phillipsburg, 4 layers, +-10 % ensemble members
    (grad_synth1_pert*), wide-range ensemble members (grad_wide*: BASELINE configs[4]'s parameter ranges) and a column
    with up to 19 fronts (grad_manyfronts_60: more than the 8-slot tangent kernel holds -> capacity chain).  Both ways the
    backward pass lays out its directions: every lane on its own (small jobs), and the 3 x L directions of a column sharing
    the Geff trapezoid in one group of lanes (jobs that fill the chip; forced here: groups of 6, 9, 12, 15 and 18 lanes)."""
    import lgar_py_amd.autograd as A
    from lgar_py_amd.autograd import lgar_series
    monkeypatch.setattr(A, "SHARE_MIN_LANES", 1 if shared else 1 << 30)
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    N = 3
    P, pr, pe, ekw = _setup(g, N, search_mode=mode)
    for k in ("alpha", "n", "ksat"):
        P[k].requires_grad_(True)
    runoff, perc = lgar_series(P["alpha"], P["n"], P["ksat"], P["theta_e"], P["theta_r"], P["thickness"], pr, pe, **ekw)
    assert runoff.requires_grad
    assert runoff.grad_fn is not None
    loss = torch.mean(runoff[:, 0] ** 2)
    # torch.autograd.grad works like for the reference's graph (models/dpLGAR.py:299), and so does backward()
    direct = dict(zip(("alpha", "n", "ksat"), torch.autograd.grad(loss, [P["alpha"], P["n"], P["ksat"]], retain_graph=True)))
    loss.backward()
    G.check_gradients(g, float(loss), {k: P[k].grad[:, 0].cpu().numpy() for k in direct})
    for k in direct:
        assert np.abs(P[k].grad[:, 1:].cpu().numpy()).max() == 0.0  # other columns do not enter the loss
        assert torch.equal(direct[k], P[k].grad)


def test_tangent_matches_finite_differences():
    """Independent check on perturbed columns: d(sum_t w_t runoff_t)/dp by tangents vs central differences (fp64)."""
    import lgar_py_amd as lg
    from lgar_py_amd import workloads as W
    N = 64
    Pn = W.perturbed_columns(N, seed=11)
    sc = W.forcing_scale(N, 0.5, 1.0, seed=12)
    f = W.synth1_forcing()
    pr = torch.tensor(f[:, 0:1] * sc[None, :], device="cuda")
    pe = torch.zeros_like(pr)
    T = pr.shape[0]
    w = torch.linspace(0.5, 1.5, T, device="cuda", dtype=torch.float64)[:, None].expand(T, N).contiguous()
    kw = dict(dt_h=300.0 / 3600.0, ponded_depth_max=0.0, dtype=torch.float64)

    def J(P):
        e = lg.LgarEngine(P["alpha"], P["n"], P["ksat"], P["theta_e"], P["theta_r"], P["thickness"], **kw)
        r = e.forward(pr, pe, series=("runoff",), check=False)["runoff"]
        return (w * r).sum(0).cpu().numpy(), e.status.cpu().numpy()

    base = lg.LgarEngine(Pn["alpha"], Pn["n"], Pn["ksat"], Pn["theta_e"], Pn["theta_r"], Pn["thickness"], **kw)
    _, st0 = J(Pn)
    checked = 0
    for kind, l, h in (("alpha", 0, 1e-7), ("n", 0, 1e-6), ("ksat", 0, 1e-6), ("ksat", 1, 1e-6), ("n", 1, 1e-6)):
        d = torch.zeros(3, N, dtype=torch.float64)
        d[l] = 1.0
        g, ser, st = base.tangent({kind: d}, pr, pe, w_runoff=w, want_series=True)
        assert ser.shape == (T, N)
        Pp = {k: v.copy() for k, v in Pn.items()}
        Pm = {k: v.copy() for k, v in Pn.items()}
        Pp[kind][l] += h * Pn[kind][l]
        Pm[kind][l] -= h * Pn[kind][l]
        jp, sp = J(Pp)
        jm, sm = J(Pm)
        fd = (jp - jm) / (2 * h * Pn[kind][l])
        got = g.cpu().numpy()
        ok = (st0 == 0) & (sp == 0) & (sm == 0) & (st.cpu().numpy() == 0)
        # Reference-faithful gradients are NOT the true derivative wherever a line search is active: the psi / depth
        # offsets found by the searches are constants to autograd (Layer.py:277-288, 683-696), and the
        # response is only piecewise smooth (discrete front events).  Finite differences therefore agree for the
        # columns/steps where no search contributes -- the bulk -- which is what is asserted here; exact agreement
        # with the reference's own autograd is asserted in test_gradients_match_reference_autograd.
        rel = np.abs(got - fd)[ok] / np.maximum(np.abs(fd[ok]), 1e-3 * np.abs(fd[ok]).max() + 1e-12)
        assert np.median(rel) <= 1e-4, (kind, l, np.median(rel))
        assert (rel <= 1e-2).mean() >= 0.5, (kind, l, (rel <= 1e-2).mean())
        checked += int(ok.sum())
    assert checked > 100


def test_stepwise_model_backward_equals_series_backward(tmp_path):
    """The reference's calling convention -- model(x[i]) per row, loss at the end, loss.backward(), optimizer.step() --
    produces the same parameter gradients as the one-shot series function (and as the reference's autograd)."""
    from lgar_py_amd import config
    from lgar_py_amd.model import MassBalance, dpLGAR
    g = np.load(os.path.join(GOLDEN, "grad_synth0_12h.npz"))
    os.makedirs(tmp_path / "data", exist_ok=True)
    soil = write_soil_dat(str(tmp_path / "data" / "soil.dat"))
    forcing = write_forcing(str(tmp_path / "data" / "f.csv"), g["forcing"])
    cfg = config.load_config(cwd=str(tmp_path), overrides={"data.forcing_file": forcing, "data.soil_params_file": soil,
                                                           "data.ponded_depth_max": 0.0, "models.endtime": 12.0})
    model = dpLGAR(cfg)
    mb = MassBalance(cfg, model)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    opt.zero_grad()
    ys = []
    x = torch.tensor(g["forcing"])
    for i in range(12):
        runoff, _ = model(x[i])
        ys.append(runoff)
        mb.change_mass(model)
    y = torch.stack(ys)
    assert y.requires_grad and y.grad_fn is not None  # graph-connected like the reference's outputs (models/dpLGAR.py:299)
    loss = torch.mean(y * y)
    assert abs(float(loss) - float(g["loss"])) <= 1e-9 * float(g["loss"])
    direct = torch.autograd.grad(loss, list(model.parameters()), retain_graph=True, allow_unused=True)
    loss.backward()
    for plist, ref in ((model.alpha, g["d_alpha"]), (model.n, g["d_n"]), (model.ksat, g["d_ksat"])):
        ref = np.nan_to_num(ref, nan=0.0)
        got = np.array([float(p.grad) for p in plist])
        assert np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max(), (got, ref)
    for p, d in zip(model.parameters(), direct):
        assert d is not None and float(d) == float(p.grad)
    # a loss on part of the series only (steps 6..11) still reaches the parameters through the chained nodes
    for p in model.parameters():
        p.grad = None
    torch.mean(y[6:] * y[6:]).backward()
    assert float(model.ksat[0].grad) != 0.0
    before = float(model.alpha[0])
    opt.step()
    assert float(model.alpha[0]) != before
    # the optimizer changed the parameters: continuing the recorded series is refused (its gradient would belong to
    # another run); the agent resets the state after every epoch (agents/DifferentiableLGAR.py:105)
    with pytest.raises(RuntimeError, match="parameters changed"):
        model(x[0])
    model.set_internal_states()
    model(x[0])


def test_model_gradients_with_frozen_factor_follow_the_reference_convention(tmp_path):
    """cfg.constants.frozen_factor = 0.7: the reference's Ksat Parameter IS Ksat x frozen_factor (models/dpLGAR.py:57), so
    d loss / d model.ksat is taken with respect to the scaled value; the drop-in model reproduces the reference's own
    gradients (fixture grad_frozen07_synth1), while the engine-level gradient is with respect to its unscaled input."""
    from lgar_py_amd import config
    from lgar_py_amd.model import MassBalance, dpLGAR
    g = np.load(os.path.join(GOLDEN, "grad_frozen07_synth1.npz"))
    os.makedirs(tmp_path / "data", exist_ok=True)
    soil = write_soil_dat(str(tmp_path / "data" / "soil.dat"))
    forcing = write_forcing(str(tmp_path / "data" / "f.csv"), g["forcing"], step_min=5)
    cfg = config.load_config(cwd=str(tmp_path), overrides={
        "data.forcing_file": forcing, "data.soil_params_file": soil, "data.ponded_depth_max": 0.0, "models.endtime": 12.0,
        "models.subcycle_length": 300, "models.forcing_resolution": 300, "constants.frozen_factor": 0.7})
    model = dpLGAR(cfg)
    mb = MassBalance(cfg, model)
    ys = []
    x = torch.tensor(g["forcing"])
    for i in range(x.shape[0]):
        runoff, _ = model(x[i])
        ys.append(runoff)
        mb.change_mass(model)
    loss = torch.mean(torch.stack(ys) ** 2)
    assert abs(float(loss) - float(g["loss"])) <= 1e-9 * float(g["loss"])
    loss.backward()
    for plist, ref in ((model.alpha, g["d_alpha"]), (model.n, g["d_n"]), (model.ksat, g["d_ksat"])):
        ref = np.nan_to_num(ref, nan=0.0)
        got = np.array([float(p.grad) for p in plist])
        assert np.abs(got - ref).max() <= 1e-6 * np.abs(ref).max(), (got, ref)


def test_ensemble_gradients_config5_shape():
    """BASELINE configs[4] at a reduced size: per-column (alpha, n, Ksat) ensemble, loss = mean runoff^2,
    one backward = 9 tangent launches; gradients are per column and finite."""
    from lgar_py_amd import workloads as W
    from lgar_py_amd.autograd import lgar_series
    N = 2048
    E = W.ensemble_columns(N, seed=0)
    f = W.synth1_forcing()
    T = f.shape[0]
    pr = torch.tensor(f[:, 0:1], device="cuda").expand(T, N).contiguous()
    pe = torch.zeros_like(pr)
    P = {k: torch.tensor(v, device="cuda") for k, v in E.items()}
    for k in ("alpha", "n", "ksat"):
        P[k].requires_grad_(True)
    with pytest.raises(ValueError):  # this wide ensemble leaves the reference's domain of validity in some columns
        lgar_series(P["alpha"], P["n"], P["ksat"], P["theta_e"], P["theta_r"], P["thickness"], pr, pe,
                    dt_h=300.0 / 3600.0, ponded_depth_max=0.0, dtype=torch.float64)
    st = []
    runoff, _ = lgar_series(P["alpha"], P["n"], P["ksat"], P["theta_e"], P["theta_r"], P["thickness"], pr, pe,
                            dt_h=300.0 / 3600.0, ponded_depth_max=0.0, dtype=torch.float64, check=False, status_out=st)
    ok = st[0] == 0
    assert 0.3 < float(ok.double().mean()) < 1.0
    loss = torch.mean(runoff[:, ok] ** 2)  # faulted columns are masked out of the loss
    loss.backward()
    assert len(st) == 2  # the backward pass appended the tangent status: columns whose gradient integration faulted
    tok = st[1] == 0
    assert float(tok.double().mean()) > 0.9
    for k in ("alpha", "n", "ksat"):
        gk = P[k].grad
        assert gk.shape == (3, N) and bool(torch.isfinite(gk).all())
        assert float(gk[:, ~ok].abs().sum()) == 0.0 and float(gk[:, ~tok].abs().sum()) == 0.0
    assert float(P["ksat"].grad[0].abs().sum()) > 0
    # per-column gradients equal the single-column gradients of the same member (columns are independent): spot-check
    # three members against the reference-pinned single-column path
    from lgar_py_amd.autograd import lgar_series as series
    for c in [int(i) for i in torch.nonzero(ok & tok).flatten()[:3]]:
        Q = {k: P[k].detach()[:, c:c + 1].clone() for k in P}
        for k in ("alpha", "n", "ksat"):
            Q[k].requires_grad_(True)
        r1, _ = series(Q["alpha"], Q["n"], Q["ksat"], Q["theta_e"], Q["theta_r"], Q["thickness"], pr[:, c:c + 1].contiguous(),
                       pe[:, c:c + 1].contiguous(), dt_h=300.0 / 3600.0, ponded_depth_max=0.0, dtype=torch.float64)
        (torch.sum(r1 ** 2) / (T * int(ok.sum()))).backward()
        for k in ("alpha", "n", "ksat"):
            assert torch.allclose(Q[k].grad[:, 0], P[k].grad[:, c], rtol=1e-9, atol=1e-18), (c, k)


@pytest.mark.timeout(900)
def test_ensemble_gradients_config5_full_size():
    """BASELINE configs[4] at its real size: 100 000 ensemble columns x 9 parameter directions = 900 000 lanes, which takes the
    shared-trapezoid layout (tangent_share = 9) on the library's own threshold -- nothing is patched; a spy on
    LgarEngine.tangent only records what autograd asked for.  Three members are checked against the single-column path (the
    one the reference's own gradient fixtures pin), no tangent integration faults, and the fraction of the ensemble inside the
    reference's domain of validity is the one bench.py reports."""
    import lgar_py_amd as lg
    from lgar_py_amd import autograd as AG
    from lgar_py_amd import workloads as W
    N = 100_000
    E = W.ensemble_columns(N, seed=0)
    f = W.synth1_forcing()
    T = f.shape[0]
    pr = torch.tensor(f[:, 0:1], device="cuda").expand(T, N).contiguous()
    pe = torch.zeros_like(pr)
    P = {k: torch.tensor(v, device="cuda") for k, v in E.items()}
    for k in ("alpha", "n", "ksat"):
        P[k].requires_grad_(True)
    shares = []
    real = lg.LgarEngine.tangent

    def spy(self, *a, **kw):
        shares.append((self.N, int(kw.get("share", 0))))
        return real(self, *a, **kw)

    lg.LgarEngine.tangent = spy
    try:
        st = []
        runoff, _ = AG.lgar_series(P["alpha"], P["n"], P["ksat"], P["theta_e"], P["theta_r"], P["thickness"], pr, pe,
                                   dt_h=300.0 / 3600.0, ponded_depth_max=0.0, dtype=torch.float64, check=False, status_out=st)
        ok = st[0] == 0
        loss = torch.mean(runoff[:, ok] ** 2)
        loss.backward()
    finally:
        lg.LgarEngine.tangent = real
    assert shares == [(9 * N, 9)], shares  # ONE launch, nine lanes per column sharing the trapezoid
    assert 9 * N >= AG.SHARE_MIN_LANES
    valid = float(ok.double().mean())
    assert 0.955 <= valid <= 0.972, valid  # bench.py's configs4_autograd.valid_fraction (0.9636 on this seed)
    assert len(st) == 2 and int((st[1] != 0).sum()) == 0  # tangent_faulted_fraction == 0
    for k in ("alpha", "n", "ksat"):
        gk = P[k].grad
        assert gk.shape == (3, N) and bool(torch.isfinite(gk).all())
        assert float(gk[:, ~ok].abs().sum()) == 0.0
    assert float(P["ksat"].grad[0].abs().sum()) > 0
    gmax = max(float(P[k].grad.abs().max()) for k in ("alpha", "n", "ksat"))
    idx = torch.nonzero(ok).flatten()
    for c in [int(idx[0]), int(idx[len(idx) // 2]), int(idx[-1])]:
        Q = {k: P[k].detach()[:, c:c + 1].clone() for k in P}
        for k in ("alpha", "n", "ksat"):
            Q[k].requires_grad_(True)
        r1, _ = AG.lgar_series(Q["alpha"], Q["n"], Q["ksat"], Q["theta_e"], Q["theta_r"], Q["thickness"],
                               pr[:, c:c + 1].contiguous(), pe[:, c:c + 1].contiguous(), dt_h=300.0 / 3600.0,
                               ponded_depth_max=0.0, dtype=torch.float64)
        assert torch.equal(r1[:, 0], runoff[:, c].detach())
        (torch.sum(r1 ** 2) / (T * int(ok.sum()))).backward()
        for k in ("alpha", "n", "ksat"):
            # shared vs plain trapezoid: the same sums in another order; 1e-6 of the column's largest
            # gradient entry is the bar of the reference's own gradient fixtures
            scale = max(float(Q[kk].grad.abs().max()) for kk in ("alpha", "n", "ksat"))
            assert float((Q[k].grad[:, 0] - P[k].grad[:, c]).abs().max()) <= 1e-6 * scale, (c, k)
    assert gmax > 0


def test_tangent_faults_are_reported_not_swallowed():
    """A column whose tangent integration faults (here: more than 32 fronts) has no gradient: parameter_vjp raises
    (check=True) or zeroes that column's entries and reports the status (check=False); clean columns are unaffected."""
    import lgar_py_amd as lg
    from lgar_py_amd.autograd import parameter_vjp
    g = np.load(os.path.join(GOLDEN, "manyfronts_pulse_84.npz"))
    P, _, _, ekw = _setup(g, 2)
    pulses = np.concatenate([g["forcing"][:, 0], np.tile([0.02, 0.0], 30)])
    pr = torch.tensor(np.stack([pulses, np.where(np.arange(len(pulses)) < 40, pulses, 0.0)], axis=1), device="cuda")
    pe = torch.zeros_like(pr)
    eng = lg.LgarEngine(P["alpha"], P["n"], P["ksat"], P["theta_e"], P["theta_r"], P["thickness"], **ekw)
    w = torch.ones_like(pr)
    with pytest.raises(lg.LgarStatusError, match="tangent"):
        parameter_vjp(eng, pr, pe, w, None, [("ksat", 0), ("n", 0)])
    vj, st = parameter_vjp(eng, pr, pe, w, None, [("ksat", 0), ("n", 0)], check=False)
    assert int(st[0]) & 8 and int(st[1]) == 0
    assert float(vj[("ksat", 0)][0]) == 0.0 and float(vj[("ksat", 0)][1]) != 0.0
    with pytest.raises(lg.LgarError, match=r"\[T, N\]"):
        eng.tangent({"ksat": torch.ones(3, 2)}, pr, pe, w_runoff=w[:5])


def test_agent_twin_experiment_reduces_loss(tmp_path):
    """Agent counterpart (agents/DifferentiableLGAR.py:94-172): synthetic-truth runoff, perturbed Ksat, a few Adam epochs."""
    from lgar_py_amd import config
    from lgar_py_amd import workloads as W
    from lgar_py_amd.agent import DifferentiableLGAR, RangeBoundLoss
    from lgar_py_amd.model import dpLGAR
    f = W.synth1_forcing()
    os.makedirs(tmp_path / "data", exist_ok=True)
    soil = write_soil_dat(str(tmp_path / "data" / "soil.dat"))
    forcing = write_forcing(str(tmp_path / "data" / "f.csv"), f, step_min=5)
    ov = {"data.forcing_file": forcing, "data.soil_params_file": soil, "models.hyperparameters.epochs": 6,
          "models.hyperparameters.learning_rate": 0.02, "models.hyperparameters.warmup": 0}
    cfg = config.load_config(data="synth_1", models="five_minute", cwd=str(tmp_path), overrides=ov)
    with torch.no_grad():
        truth = dpLGAR(cfg)
        obs, _ = truth(torch.tensor(f)[:, None, :])
        obs = obs[:, 0].cpu()
    assert float(obs.sum()) > 0.1
    for stepwise in (False, True):
        agent = DifferentiableLGAR(cfg, observations=obs, stepwise=stepwise, log=lambda s: None)
        with torch.no_grad():
            agent.model.ksat[0].mul_(0.6)  # start from a wrong top-layer Ksat
        for p in list(agent.model.alpha) + list(agent.model.n):
            p.requires_grad_(False)        # Adam moves every parameter by ~lr per step: only Ksat is trained here
        agent.model.set_internal_states()
        agent.cfg.models.hyperparameters.epochs = 6 if not stepwise else 2
        agent.run()
        h = agent.history
        assert all(np.isfinite(e["loss"]) for e in h)
        assert h[-1]["loss"] < h[0]["loss"], h
        assert float(agent.model.ksat[0]) > 0.27
    rb = RangeBoundLoss([0.0015, 1.0, 1e-6, 0.0], [0.015, 5.0, 30, 10.0])
    m = agent.model
    assert float(rb([m.alpha, m.n, m.ksat, m.ponded_depth_max])) == 0.0
    with torch.no_grad():
        m.alpha[0].fill_(0.02)
    assert abs(float(rb([m.alpha, m.n, m.ksat, m.ponded_depth_max])) - 0.005) < 1e-12


def test_fp32_gradients_close_to_reference():
    """The fp32 tangent kernel on the same case as the reference's autograd fixture: gradients within 2 % of fp64's."""
    from lgar_py_amd.autograd import lgar_series
    g = np.load(os.path.join(GOLDEN, "grad_synth0_12h.npz"))
    P, pr, pe, ekw = _setup(g, 2, dtype=torch.float32)
    for k in ("alpha", "n", "ksat"):
        P[k].requires_grad_(True)
    runoff, _ = lgar_series(P["alpha"], P["n"], P["ksat"], P["theta_e"], P["theta_r"], P["thickness"], pr, pe, **ekw)
    loss = torch.mean(runoff[:, 0] ** 2)
    assert abs(float(loss) - float(g["loss"])) <= 1e-3 * float(g["loss"])
    loss.backward()
    for k, ref in (("alpha", g["d_alpha"]), ("n", g["d_n"]), ("ksat", g["d_ksat"])):
        ref = np.nan_to_num(ref, nan=0.0)
        got = P[k].grad[:, 0].double().cpu().numpy()
        assert np.abs(got - ref).max() <= 2e-2 * np.abs(ref).max(), (k, got, ref)


@pytest.mark.parametrize("width", [9, 8, 3])
def test_shared_tangent_launch_equals_plain_launch_and_rejects_mixed_groups(width):
    """LgarDims.tangent_share = W: the W direction-lanes of a column share the Geff trapezoid (W = 9: all 3 x L directions of a
    three-layer column, seven groups and one idle lane per wavefront).  Values -- and so the status words -- are bit-identical to
    the plain launch; the tangents are summed in another order: equal to rounding (median difference 0, 99.5 % of the entries
    within 1e-9 of the largest gradient), except where the gradient itself is ill-conditioned: alpha h does not depend on alpha
    (h = f(Se) / alpha), so the alpha direction's d(alpha h) is pure cancellation noise in BOTH launches (and in the reference's
    autograd), which a near-saturated column multiplies by ~1e9: those entries (1-2 of 4500 here) agree to 1e-3 of their own
    size, 1e-6 of the largest gradient -- the bar of the reference fixtures.  The wrapper refuses groups whose columns are not
    one soil column."""
    import lgar_py_amd as lg
    from lgar_py_amd import workloads as W
    N = 500  # 500 x 9 = 4500 columns: ragged last wavefront
    E = W.ensemble_columns(N, seed=3)
    f = W.synth1_forcing()
    T = f.shape[0]
    pr = torch.tensor(f[:, 0:1], device="cuda")
    pe = torch.zeros_like(pr)
    w = torch.rand(T, 1, device="cuda", dtype=torch.float64)
    rep = {k: np.repeat(v, width, axis=1) for k, v in E.items()}
    eng = lg.LgarEngine(rep["alpha"], rep["n"], rep["ksat"], rep["theta_e"], rep["theta_r"], rep["thickness"],
                        dt_h=300.0 / 3600.0, ponded_depth_max=0.0, dtype=torch.float64, with_state=False)
    dirs = {k: torch.zeros(3, width * N, dtype=torch.float64, device="cuda") for k in ("alpha", "n", "ksat")}
    basis = [(kind, l) for kind in ("alpha", "n", "ksat") for l in range(3)]
    for b in range(width):
        kind, l = basis[b % 9]
        dirs[kind][l, b::width] = 1.0
    g0, _, s0 = eng.tangent(dirs, pr, pe, w_runoff=w, forcing_group=width)
    g1, _, s1 = eng.tangent(dirs, pr, pe, w_runoff=w, forcing_group=width, share=width)
    assert torch.equal(s0, s1)
    ok = (s0 & 0x7F) == 0
    scale = float(g0[ok].abs().max())
    d = (g0 - g1)[ok].abs()
    assert scale > 0 and float(d.max()) <= 1e-6 * scale
    assert float(d.median()) <= 1e-12 * scale and float((d > 1e-9 * scale).double().mean()) <= 5e-3
    mixed = rep["ksat"].copy()
    mixed[0, 3 if width > 3 else 1] *= 1.01
    bad = lg.LgarEngine(rep["alpha"], rep["n"], mixed, rep["theta_e"], rep["theta_r"], rep["thickness"],
                        dt_h=300.0 / 3600.0, ponded_depth_max=0.0, dtype=torch.float64, with_state=False)
    with pytest.raises(lg.LgarError, match="identical soil parameters"):
        bad.tangent(dirs, pr, pe, w_runoff=w, forcing_group=width, share=width)
