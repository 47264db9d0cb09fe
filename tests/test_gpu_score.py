"""GPU (-m gpu): catchment scores -- lgar_catchment_moments / lgar_catchment_moments_grad through scores.CatchmentScore and
scores.catchment_moments (autograd).

moments[.][b] and grad_sim[.][b] are pure functions of column b of the inputs (include/lgar.h), so the
kernels are held BIT FOR BIT to the numpy statement of the definition (tests/score_host: moments_ref and grad_ref, plain loops
over blocks and rows), the one tests/test_score_host.py holds the host build of the same header to.  Where the kernels are
compared with torch autograd of the masked plain statement -- another evaluation order -- the bar is score_host.gradient_bar,
whose docstring derives it."""
import os

import numpy as np
import pytest

from _golden import engine_keywords
from conftest import GOLDEN

import score_host as SH

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GRID_CAP = 4096  # LGAR_SCORE_GRID_CAP (csrc/lgar_score.hip): workgroups of a launch; the rest by stride


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _score(obs, window=1, warmup=0):
    from lgar_py_amd.scores import CatchmentScore
    return CatchmentScore(obs, window=window, warmup=warmup)


def _both(sim, obs, window, coef):
    """(moments, grad_sim) of the kernels, as numpy arrays; the gradient on the kernels' own moments."""
    score = _score(obs, window)
    dsim = _cuda(sim)
    m = score.moments(dsim)
    return m.cpu().numpy(), score.moments_grad(dsim, m, _cuda(coef)).cpu().numpy()


@pytest.mark.parametrize("B", SH.SHAPE_B)
def test_kernels_equal_the_numpy_definition_bit_for_bit(B):
    """To in {0, 1, 63, 64, 65, 129} x window in {1, 3, 12} x the gap patterns (none, 20 % random, a catchment wholly missing, a
    catchment with exactly one valid row, one whole block missing in one catchment, +inf and -inf as gaps), mixed signs and -0.0
    in sim: the moments and the gradient."""
    rng = np.random.default_rng(1000 + B)
    for To in SH.SHAPE_TO:
        for window in SH.SHAPE_WINDOW:
            for gaps in SH.GAPS:
                sim, obs, coef = SH.mixed_data(rng, To, B, window, gaps)
                m, g = _both(sim, obs, window, coef)
                ref = SH.moments_ref(sim, obs, window)
                what = (B, To, window, gaps)
                assert SH.same_bits(m, ref), what
                assert SH.same_bits(g, SH.grad_ref(sim, obs, window, ref, coef)), what


def test_a_nan_in_sim_poisons_its_catchment_only():
    rng = np.random.default_rng(4)
    To, B, window = 129, 65, 3
    sim, obs, coef = SH.mixed_data(rng, To, B, window, "random")
    obs[70, 7] = 1.5
    clean, _ = _both(sim, obs, window, coef)
    sim[70 * window + 1, 7] = np.nan
    got, _ = _both(sim, obs, window, coef)
    others = np.arange(B) != 7
    assert SH.same_bits(got, SH.moments_ref(sim, obs, window))
    assert SH.same_bits(got[:, others], clean[:, others]) and np.isnan(got[[2, 4, 5, 6], 7]).all() and not np.isnan(got[[0, 1, 3], 7]).any()


def test_the_capped_grid_strides():
    """A launch has at most 4096 workgroups.  The partial kernels' workgroups are (four blocks of 64 rows, 64 catchments): To = 7,
    B = 4097 x 64 - 63 is 4097 of them along the catchments; To = 257 (five blocks: two groups of four), B = 2049 x 64 - 63 is
    2 x 2049 = 4098 along both axes.  The gradient kernel's are (four rows, 64 catchments): the first shape is 2 x 4097 of them,
    and To = 8200, B = 65 is 2050 x 2 = 4100 along the rows.  The fold kernels' are 256 catchments: To = 1,
    B = 4096 x 256 + 1 is 4097.  All against the numpy definition, bit for bit."""
    rng = np.random.default_rng(8)
    for To, B, window in ((7, (GRID_CAP + 1) * 64 - 63, 1), (257, (GRID_CAP // 2 + 1) * 64 - 63, 1), (8200, 65, 2), (1, GRID_CAP * 256 + 1, 1)):
        blocks = (To + 63) // 64
        assert max(((blocks + 3) // 4) * ((B + 63) // 64), ((To + 3) // 4) * ((B + 63) // 64), (B + 255) // 256) > GRID_CAP
        sim, obs, coef = rng.standard_normal((To * window, B)), rng.standard_normal((To, B)), rng.standard_normal((4, B))
        obs[rng.random((To, B)) < 0.1] = np.nan
        m, g = _both(sim, obs, window, coef)
        ref = SH.moments_ref(sim, obs, window)
        assert SH.same_bits(m, ref), (To, B)
        assert SH.same_bits(g, SH.grad_ref(sim, obs, window, ref, coef)), (To, B)


def test_repeated_calls_and_a_permuted_subset_give_the_same_bits():
    """B = 257 catchments twice on one object (the workspace is reused), then a permuted subset of 100 of their columns alone,
    and column 0 of a B = 65 job as a job of its own (B = 1): the same bits for moments and gradient."""
    rng = np.random.default_rng(21)
    To, B, window = 129, 257, 3
    sim, obs, coef = SH.mixed_data(rng, To, B, window, "missing")
    score = _score(obs, window)
    dsim, dcoef = _cuda(sim), _cuda(coef)
    m = score.moments(dsim)
    g = score.moments_grad(dsim, m, dcoef)
    same = lambda a, b: SH.same_bits(a.cpu().numpy(), b.cpu().numpy())  # (an empty catchment has NaN means: torch.equal would refuse it)
    assert same(score.moments(dsim), m) and same(score.moments_grad(dsim, m, dcoef), g)
    pick = rng.permutation(B)[:100]
    mp, gp = _both(sim[:, pick], obs[:, pick], window, coef[:, pick])
    assert SH.same_bits(m.cpu().numpy()[:, pick], mp) and SH.same_bits(g.cpu().numpy()[:, pick], gp)
    m65, g65 = _both(sim[:, :65], obs[:, :65], window, coef[:, :65])
    m1, g1 = _both(sim[:, :1], obs[:, :1], window, coef[:, :1])
    assert SH.same_bits(m65[:, :1], m1) and SH.same_bits(g65[:, :1], g1) and float(np.abs(g1).max()) > 0


def test_one_long_catchment():
    """B = 1 with To = 10 000 rows (the agent's one basin): 157 blocks, each a wave's, not one serial walk -- and the same bits."""
    rng = np.random.default_rng(5)
    To = 10000
    sim, obs, coef = rng.random((To, 1)), rng.random((To, 1)), rng.standard_normal((4, 1))
    obs[rng.random((To, 1)) < 0.1] = np.nan
    m, g = _both(sim, obs, 1, coef)
    ref = SH.moments_ref(sim, obs, 1)
    assert SH.same_bits(m, ref) and SH.same_bits(g, SH.grad_ref(sim, obs, 1, ref, coef))


def test_entry_points_refuse_bad_arguments():
    """LGAR_E_ARG from the library itself: negative sizes, window < 1, To x window beyond int32, a null pointer the sizes say
    will be read or written, a null workspace where one is needed.  Nothing is launched by a refused call."""
    from lgar_py_amd import _capi
    lib = _capi.load()
    buf = torch.zeros(1024, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    assert lib.lgar_catchment_moments_workspace(129, 65) == 3 * 4 * 65 * 8 and lib.lgar_catchment_moments_workspace(0, 65) == 0
    assert lib.lgar_catchment_moments_workspace(-1, 1) == -1 and lib.lgar_catchment_moments_workspace(1, -1) == -1
    call = lambda **kw: lib.lgar_catchment_moments(*[kw.get(k, d) for k, d in (("sim", p), ("obs", p), ("To", 2), ("B", 2), ("window", 1), ("moments", p), ("ws", p))], None)
    for bad in (dict(To=-1), dict(B=-1), dict(window=0), dict(To=2 ** 30, window=4), dict(sim=None), dict(obs=None), dict(moments=None), dict(ws=None)):
        assert call(**bad) == -1, bad
    assert call(B=0, moments=None, sim=None, obs=None, ws=None) == 0
    grad = lambda **kw: lib.lgar_catchment_moments_grad(*[kw.get(k, d) for k, d in (("sim", p), ("obs", p), ("To", 2), ("B", 2), ("window", 1), ("moments", p), ("coef", p), ("grad", p))], None)
    for bad in (dict(To=-1), dict(B=-1), dict(window=0), dict(To=2 ** 30, window=4), dict(sim=None), dict(obs=None), dict(moments=None), dict(coef=None), dict(grad=None)):
        assert grad(**bad) == -1, bad
    assert grad(To=0, sim=None, obs=None, moments=None, coef=None, grad=None) == 0
    torch.cuda.synchronize()


def test_gradients_end_to_end():
    """lgar_series -> catchment_sum -> catchment_route -> catchment_moments -> loss("nse") (24 columns of grad_synth0_12h's soil in
    3 catchments, per-catchment hydrographs; observations = the routed sums of a perturbed parameter set with 15 % gaps) against
    the same chain with the masked torch statement (score_host.plain_moments) in place of the kernels.  Ahead of the scores both
    chains are the same deterministic kernels, so they hand the scores the same routed matrix; the gradient with respect to it
    is within score_host.gradient_bar (the forward error of the sums times the metric's sensitivity at these inputs, plus the
    rounding of the gradient formula; F = the mean over the three catchments of 1 - nse).  Behind the scores both chains run the
    same deterministic linear tail (CatchmentRouting.adjoint, CatchmentMap.spread, the tangent kernels): fed with the kernel
    chain's own gradient of the routed matrix it reproduces the parameter gradients bit for bit, which is how the bar reaches
    the parameters."""
    import lgar_py_amd as lg
    from lgar_py_amd import workloads as W
    from lgar_py_amd.autograd import lgar_series, parameter_vjp
    from lgar_py_amd.catchments import CatchmentMap, CatchmentRouting, catchment_route, catchment_sum
    from lgar_py_amd.scores import catchment_moments
    g = np.load(os.path.join(GOLDEN, "grad_synth0_12h.npz"))
    n, B, K = 24, 3, 5
    base = {k: g[k] for k in W.PARAM_KEYS + ("thickness",)}
    Pn = W.perturbed_columns(n, frac=0.05, seed=21, base=base)
    Pobs = W.perturbed_columns(n, frac=0.05, seed=22, base=base)
    f = torch.tensor(g["forcing"], device="cuda")
    Tn = f.shape[0]
    pr, pe = f[:, 0:1].expand(Tn, n).contiguous(), f[:, 1:2].expand(Tn, n).contiguous()
    ekw = dict(engine_keywords(g), dtype=torch.float64)
    ids = np.array([0] * 9 + [2] * 5 + [-1] + [1] * 9)[np.random.default_rng(1).permutation(n)]
    cmap = CatchmentMap(ids, weights=np.random.default_rng(2).random(n) + 0.5)
    rng = np.random.default_rng(3)
    routing = CatchmentRouting(g["giuh_ordinates"][None, :] * (1.0 + 0.2 * rng.random((B, K))))

    def routed_of(Pdict, grad):
        P = {k: torch.tensor(val, device="cuda") for k, val in Pdict.items()}
        for k in ("alpha", "n", "ksat"):
            P[k].requires_grad_(grad)
        statuses = []
        runoff, _ = lgar_series(P["alpha"], P["n"], P["ksat"], P["theta_e"], P["theta_r"], P["thickness"], pr, pe, check=False,
                                status_out=statuses, **ekw)
        return P, statuses[0], catchment_route(catchment_sum(runoff, cmap, statuses[0]), routing)

    with torch.no_grad():
        obs = routed_of(Pobs, False)[2].clone()
    assert tuple(obs.shape) == (Tn, B) and float(obs.abs().max()) > 0
    obs[torch.tensor(rng.random((Tn, B)) < 0.15, device="cuda")] = float("nan")
    score = lg.CatchmentScore(obs)
    grads = {}
    for chain in ("kernel", "plain"):
        P, status, routed = routed_of(Pn, True)
        routed.retain_grad()
        if chain == "kernel":
            loss = score.loss(catchment_moments(routed, score), "nse")
        else:
            loss = (1.0 - score.metrics(SH.plain_moments(routed, obs, 1))["nse"]).mean()
        loss.backward()
        grads[chain] = dict(P=P, status=status, routed=routed.detach(), d_routed=routed.grad, loss=float(loss.detach()))
    k_, p_ = grads["kernel"], grads["plain"]
    assert torch.equal(k_["routed"], p_["routed"]) and float(k_["routed"].abs().max()) > 0
    m = score.moments(k_["routed"]).cpu()
    assert SH.same_bits(m.numpy(), SH.moments_ref(k_["routed"].cpu().numpy(), obs.cpu().numpy())) and float(m[0].min()) >= 2 and float(m[3].min()) > 0
    bar = SH.gradient_bar(lambda mom: (1.0 - score.metrics(mom)["nse"]) / B, k_["routed"].cpu(), obs.cpu(), 1, m)
    err = (k_["d_routed"] - p_["d_routed"]).abs().cpu().numpy()
    live = bar > 0
    print("d loss / d routed, kernel chain vs plain chain: worst error / bar = %.3g (largest entry %.3g); loss %.6g vs %.6g"
          % (float((err[live] / bar[live]).max()), float(k_["d_routed"].abs().max()), k_["loss"], p_["loss"]))
    assert (err <= bar).all() and float(k_["d_routed"].abs().max()) > 0
    assert not k_["d_routed"][~torch.isfinite(obs)].any()
    # the linear tail: the kernel chain's parameter gradients are the tangent kernels on spread(adjoint(d loss / d routed)), bit for bit
    status = k_["status"]
    faulted = (status & 0x7F) != 0
    P = k_["P"]
    eng = lg.LgarEngine(P["alpha"].detach(), P["n"].detach(), P["ksat"].detach(), P["theta_e"], P["theta_r"], P["thickness"], **ekw)
    wr = cmap.spread(routing.adjoint(k_["d_routed"]), torch.float64, status=status)
    wanted = [(kind, l) for kind in ("alpha", "n", "ksat") for l in range(eng.L)]
    vj, _ = parameter_vjp(eng, pr, pe, wr, torch.zeros_like(wr), wanted, check=False)
    for kind in ("alpha", "n", "ksat"):
        want = torch.stack([vj[(kind, l)] for l in range(eng.L)])
        want = torch.where(faulted[None, :], torch.zeros_like(want), want)
        assert torch.equal(P[kind].grad, want) and float(want.abs().max()) > 0 and bool(torch.isfinite(want).all()), kind
        assert p_["P"][kind].grad is not None and bool(torch.isfinite(p_["P"][kind].grad).all())
