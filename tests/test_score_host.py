"""CPU: catchment scores (lgar_catchment_moments / lgar_catchment_moments_grad, include/lgar.h).

The aggregated simulation, the block partials, the fold of the partials and the gradient element the GPU kernels run
(lgar_py_amd/csrc/lgar_score.hpp) are compiled for the host into a small stand-alone program (tests/score_host).  It is held BIT
FOR BIT to the numpy statement of the definition (score_host.moments_ref / grad_ref: plain loops over blocks and rows); the same
program built with AddressSanitizer + UBSan runs the same cases.  The same header as a shared library stands behind
lgar_py_amd.scores.CatchmentScore (score_host.SimCatchmentScore), so the host logic of scores.py -- warm-up, autograd, metrics,
loss -- runs here too: against the reference's own recorded calculate_nse and MSE_loss of every committed trajectory fixture, and
against torch autograd of the masked plain statement."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import score_host as SH
from score_host import SimCatchmentScore

U = 2.0 ** -53  # unit roundoff of fp64
RUNOFF, GIUH_RUNOFF = 4, 6  # ACC_NAMES


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u): the relative error bound of a sum of k + 1 non-negative terms in ANY order (4.4)."""
    return k * U / (1.0 - k * U)


# ---- the host build against the numpy definition ---------------------------------------------------------------------------
def _definition_cases(B):
    """To in {0, 1, 63, 64, 65, 129} x window in {1, 3, 12} x the six gap patterns for one B: mixed signs and -0.0 in sim.  Each
    shape gives a moments case and a gradient case (on the reference's moments).  (cases, references)."""
    rng = np.random.default_rng(1000 + B)
    cases, refs = [], []
    for To in SH.SHAPE_TO:
        for window in SH.SHAPE_WINDOW:
            for gaps in SH.GAPS:
                sim, obs, coef = SH.mixed_data(rng, To, B, window, gaps)
                m = SH.moments_ref(sim, obs, window)
                cases += [("moments", sim, obs, window), ("grad", sim, obs, window, m, coef)]
                refs += [m, SH.grad_ref(sim, obs, window, m, coef)]
    return cases, refs


@pytest.fixture(scope="module")
def definition_cases():
    return {B: _definition_cases(B) for B in SH.SHAPE_B}


def _check(cases, refs, got):
    assert len(got) == len(refs) == len(cases)
    for c, r, o in zip(cases, refs, got):
        assert SH.same_bits(o, r), (c[0], c[2].shape, c[3])


def test_host_build_equals_the_numpy_definition_bit_for_bit(definition_cases):
    for B, (cases, refs) in definition_cases.items():
        _check(cases, refs, SH.run(cases))
    # what the definition says about the corners, on the references themselves
    for B, (cases, refs) in definition_cases.items():
        for c, m in zip(cases, refs):
            if c[0] != "moments":
                continue
            obs = c[2]
            n = np.isfinite(obs).sum(axis=0)
            assert (m[0] == n).all()
            empty = n == 0
            assert np.isnan(m[1:3, empty]).all() and not np.isnan(m[1:3, ~empty]).any()  # n = 0: NaN means
            assert SH.same_bits(m[3:, empty], np.zeros_like(m[3:, empty]))  # ... and +0.0 sums
            one = n == 1
            assert SH.same_bits(m[3:6, one], np.zeros_like(m[3:6, one]))  # one valid row: it is its own mean
    # every pattern did occur
    seen = [c for cases, _ in definition_cases.values() for c in cases if c[0] == "moments" and c[2].shape[0] == 129]
    assert any(np.isposinf(c[2]).any() and np.isneginf(c[2]).any() for c in seen)
    assert any((~np.isfinite(c[2][64:128])).all(axis=0).any() and np.isfinite(c[2][:64]).all(axis=0).any() for c in seen)
    assert any((np.isfinite(c[2]).sum(axis=0) == 1).any() for c in seen) and any((np.isfinite(c[2]).sum(axis=0) == 0).any() for c in seen)


def test_gradient_is_zero_under_gaps_and_constant_over_a_window(definition_cases):
    cases, refs = definition_cases[65]
    for c, g in zip(cases, refs):
        if c[0] != "grad":
            continue
        obs, window = c[2], c[3]
        under_gap = np.repeat(~np.isfinite(obs), window, axis=0)
        assert SH.same_bits(g[under_gap], np.zeros(int(under_gap.sum())))
        rows = g.reshape(obs.shape[0], window, obs.shape[1])
        assert SH.same_bits(rows, np.repeat(rows[:, :1], window, axis=1))


def test_a_nan_in_sim_poisons_its_catchment_only():
    """One NaN in sim on a valid row: ms, sss, sos and see of that catchment are NaN (n, mo and soo do not read sim), every other
    catchment keeps its bits; on an INVALID row it changes nothing."""
    rng = np.random.default_rng(4)
    To, B, window = 129, 65, 3
    sim, obs, _ = SH.mixed_data(rng, To, B, window, "random")
    obs[70, 7], obs[71, 9] = 1.5, np.nan
    clean = SH.moments_ref(sim, obs, window)
    bad = sim.copy()
    bad[70 * window + 1, 7] = np.nan
    bad[71 * window, 9] = np.nan
    ref = SH.moments_ref(bad, obs, window)
    got, = SH.run([("moments", bad, obs, window)])
    assert SH.same_bits(got, ref)
    others = np.arange(B) != 7
    assert SH.same_bits(got[:, others], clean[:, others]) and SH.same_bits(got[[0, 1, 3], 7], clean[[0, 1, 3], 7])
    assert np.isnan(got[[2, 4, 5, 6], 7]).all()


def test_a_catchment_does_not_depend_on_the_others():
    """B = 257 catchments, then a permuted subset of 100 of their columns alone: the same bits for moments and gradient."""
    rng = np.random.default_rng(21)
    To, B, window = 129, 257, 3
    sim, obs, coef = SH.mixed_data(rng, To, B, window, "missing")
    pick = rng.permutation(B)[:100]
    full, part = SH.run([("moments", sim, obs, window), ("moments", sim[:, pick], obs[:, pick], window)])
    assert SH.same_bits(full[:, pick], part)
    gfull, gpart = SH.run([("grad", sim, obs, window, full, coef), ("grad", sim[:, pick], obs[:, pick], window, part, coef[:, pick])])
    assert SH.same_bits(gfull[:, pick], gpart) and float(np.abs(gpart).max()) > 0


def test_sanitizer_build_on_the_same_cases(definition_cases):
    """AddressSanitizer + UBSan build of the same program (a stand-alone executable: nothing is loaded into python; every array,
    the workspace included, is allocated at its exact size) over the same cases: clean, with the same bits.  Any finding aborts
    the program."""
    for B, (cases, refs) in definition_cases.items():
        _check(cases, refs, SH.run(cases, sanitize=True))


def test_entry_points_refuse_bad_arguments():
    """The refusals of the C-ABI wrappers, as the host launchers restate them (LGAR_E_ARG = -1)."""
    lib = SH.library()
    import ctypes as C
    a = C.create_string_buffer(8 * 64 * 8)
    p = C.addressof(a)
    assert lib.scorehost_catchment_moments_workspace(129, 65) == 3 * 4 * 65 * 8 and lib.scorehost_catchment_moments_workspace(0, 65) == 0
    assert lib.scorehost_catchment_moments_workspace(-1, 1) == -1 and lib.scorehost_catchment_moments_workspace(1, -1) == -1
    ok = lambda **kw: lib.scorehost_catchment_moments(*[kw.get(k, d) for k, d in (("sim", p), ("obs", p), ("To", 2), ("B", 2), ("window", 1), ("moments", p), ("ws", p))])
    assert ok() == 0
    for bad in (dict(To=-1), dict(B=-1), dict(window=0), dict(To=2 ** 30, window=4), dict(sim=None), dict(obs=None), dict(moments=None), dict(ws=None)):
        assert ok(**bad) == -1, bad
    assert ok(B=0, moments=None, sim=None, obs=None, ws=None) == 0 and ok(To=0, sim=None, obs=None, ws=None) == 0
    okg = lambda **kw: lib.scorehost_catchment_moments_grad(*[kw.get(k, d) for k, d in (("sim", p), ("obs", p), ("To", 2), ("B", 2), ("window", 1), ("moments", p), ("coef", p), ("grad", p))])
    assert okg() == 0
    for bad in (dict(To=-1), dict(B=-1), dict(window=0), dict(To=2 ** 30, window=4), dict(sim=None), dict(obs=None), dict(moments=None), dict(coef=None), dict(grad=None)):
        assert okg(**bad) == -1, bad
    assert okg(To=0, sim=None, obs=None, moments=None, coef=None, grad=None) == 0


# ---- the reference's own scores --------------------------------------------------------------------------------------------
def test_reference_parity():
    """nse and mse from the moments of the recorded giuh_runoff (modeled) and runoff (observed) columns of every committed
    trajectory fixture with >= 100 completed rows and some runoff, warm-up 0 and 24 (no gaps, window 1), against what the
    reference's calculate_nse and MSE_loss returned (tests/golden/scores/reference_scores.npz, make_score_golden.py).

    The bound.  u = 2^-53, gamma_k = k u / (1 - k u).  Both sides form the same n terms t_j = (s_j - o_j)^2 >= 0: the difference
    is rounded once (and its sign does not matter to the square); the reference squares with np.power(x, 2), libm's pow, within
    1 ulp = 2 u of x^2 where the kernel's product is within u: the terms agree to 3 u relative.  Each side then adds n
    non-negative terms in an order of its own (blocks of 64 here, numpy's pairwise sum there), which is within gamma_{n-1} of
    the exact sum whatever the order (Higham 4.4).  So see = N (1 + a), |a| <= dN = 2 gamma_n + 3 u, N the reference's numerator.
    The denominators are sums of (o_j - mean)^2 about two means.  Each mean is a sum of n non-negative o_j within gamma_{n-1}
    of exact and one division: within e = (gamma_n + u) mean_o of the exact mean.  About a point d away from the exact mean the
    exact sum of squares is larger by n d^2 only: the two exact denominators differ by at most 2 n e^2, relatively
    dM = 2 n e^2 / soo.  The terms are again rounded alike up to 3 u (+ 2 u: the rounded subtraction of each side, squared) and
    summed in two orders: soo = D (1 + b), |b| <= dD = 2 gamma_n + 5 u + dM.  With q = see / soo,
        |nse - nse_ref| <= q ((dN + dD) / (1 - dD) + 2 u) + 2 u |nse|          (the two divisions, the two subtractions from 1)
    and for the mean squared error (torch's own sum of the same squares, then / n on both sides)
        |mse - mse_ref| <= mse (2 gamma_n + 2 u + 2 u).
    Where the observed series is constant (soo = 0 = see: a fixture whose runoff ends before the warm-up does) both give 0 / 0.
    The bound is tight enough to refuse a warm-up offset wrong by one row and obs and sim swapped (asserted below; the swap
    leaves mse as it is -- it is symmetric -- so it is nse that must refuse it)."""
    rec = np.load(os.path.join(GOLDEN, "scores", "reference_scores.npz"))
    names, warmups = [str(s) for s in rec["name"]], rec["warmup"]
    assert len(names) >= 40 and set(warmups.tolist()) == {0, 24}
    i = names.index("synth1_phil")
    assert warmups[i] == 0 and abs(rec["nse"][i] - 0.88683572) < 1e-8 and abs(rec["mse"][i] - 1.46057e-5) < 1e-10

    def scores(modeled, observed, warmup):
        score = SimCatchmentScore(observed[warmup:, None], warmup=warmup)
        mom = score.moments(torch.from_numpy(np.ascontiguousarray(modeled[:, None])))
        m = score.metrics(mom)
        return float(m["nse"][0]), float(m["mse"][0]), mom.numpy()[:, 0]

    def bounds(nse, mse, mom):
        n, mo, soo, see = mom[0], mom[1], mom[3], mom[6]
        dN = 2 * gamma(n) + 3 * U
        dD = 2 * gamma(n) + 5 * U + 2 * n * ((gamma(n) + U) * mo) ** 2 / soo
        q = see / soo
        return q * ((dN + dD) / (1 - dD) + 2 * U) + 2 * U * abs(nse), mse * (2 * gamma(n) + 4 * U)

    worst, refused, compared = 0.0, [0, 0], 0
    for nm, w, T, nse_ref, mse_ref in zip(names, warmups, rec["rows"], rec["nse"], rec["mse"]):
        g = np.load(os.path.join(GOLDEN, nm + ".npz"))
        modeled, observed = g["acc"][:T, GIUH_RUNOFF].astype(np.float64), g["acc"][:T, RUNOFF].astype(np.float64)
        nse, mse, mom = scores(modeled, observed, int(w))
        assert mom[0] == T - w
        if np.isnan(nse_ref):
            assert np.isnan(nse) and mom[3] == 0 and mse == mse_ref == 0, nm
            continue
        b_nse, b_mse = bounds(nse, mse, mom)
        ratio = max(abs(nse - nse_ref) / b_nse, abs(mse - mse_ref) / b_mse)
        worst, compared = max(worst, ratio), compared + 1
        assert abs(nse - nse_ref) <= b_nse and abs(mse - mse_ref) <= b_mse, (nm, w, nse, nse_ref, mse, mse_ref, ratio)
        # a warm-up wrong by one row, and obs and sim swapped, are refused
        nse1, mse1, _ = scores(modeled[1:], observed[1:], int(w))
        refused[0] += not (abs(nse1 - nse_ref) <= b_nse and abs(mse1 - mse_ref) <= b_mse)
        nse2, _, _ = scores(observed, modeled, int(w))
        refused[1] += not abs(nse2 - nse_ref) <= b_nse
    print("reference parity: %d scores compared, worst error / bound = %.3g; refused: %d offsets, %d swaps" % (compared, worst, refused[0], refused[1]))
    assert compared >= 40 and refused == [compared, compared]


# ---- gradients through the product's host logic -----------------------------------------------------------------------------
def _gradient_job():
    rng = np.random.default_rng(77)
    To, window, B = 130, 3, 5
    obs = 0.5 + rng.random((To, B)) * (1.0 + np.arange(B))[None, :]
    sim = np.repeat(obs, window, axis=0) * (1.0 + 0.3 * rng.standard_normal((To * window, B))) + 0.05
    obs[rng.random((To, B)) < 0.2] = np.nan
    obs[5, 1], obs[9, 2] = np.inf, -np.inf
    obs[:, 3] = np.nan  # the empty catchment
    return To, window, B, sim, obs


@pytest.mark.parametrize("metric", ["nse", "kge", "mse"])
def test_gradients_against_autograd_of_the_plain_statement(metric):
    """F = the sum of `metric` over the catchments with a record; d F / d sim through catchment_moments + metrics (the host
    build of the kernels behind SimCatchmentScore) against torch autograd of the masked plain statement.  To = 130, window = 3,
    B = 5, 20 % gaps, one empty catchment.

    The bar is computed from the data by score_host.gradient_bar, whose docstring derives it: the forward error of the sums
    (two orders of the same n terms) times the metric's sensitivity d g / d moment at these inputs, plus the rounding of the
    gradient formula itself.
    The empty catchment gets exact zeros."""
    from lgar_py_amd.scores import catchment_moments
    To, window, B, sim_np, obs_np = _gradient_job()
    keep = [0, 1, 2, 4]
    score = SimCatchmentScore(obs_np, window=window)
    sim = torch.from_numpy(sim_np).requires_grad_(True)
    m = catchment_moments(sim, score)
    assert SH.same_bits(m.detach().numpy(), SH.moments_ref(sim_np, obs_np, window))
    score.metrics(m[:, keep])[metric].sum().backward()
    got = sim.grad.numpy()
    assert SH.same_bits(got[:, 3], np.zeros(To * window)) and float(np.abs(got[:, keep]).max(axis=0).min()) > 0
    # the plain statement on the catchments with a record
    sim2 = torch.from_numpy(sim_np[:, keep].copy()).requires_grad_(True)
    obs_t = torch.from_numpy(obs_np[:, keep].copy())
    pm = SH.plain_moments(sim2, obs_t, window)
    score.metrics(pm)[metric].sum().backward()
    want = sim2.grad.numpy()
    bar = SH.gradient_bar(lambda mom: score.metrics(mom)[metric], sim2.detach(), obs_t, window, m.detach()[:, keep])
    err = np.abs(got[:, keep] - want)
    live = bar > 0
    assert (err[~live] == 0).all() and (want[~live] == 0).all()
    print("d %s / d sim, kernels vs autograd of the plain statement: worst error / bar = %.3g (largest entry %.3g, largest bar %.3g)"
          % (metric, float((err[live] / bar[live]).max()), float(np.abs(want).max()), float(bar.max())))
    assert (err <= bar).all()


def test_metrics_and_loss():
    from lgar_py_amd import LgarError
    from lgar_py_amd.scores import catchment_moments
    To, window, B, sim_np, obs_np = _gradient_job()
    obs_np[:, 4] = np.nan
    obs_np[17, 4] = 2.0  # one valid row: n = 1 < min_count, soo = 0
    score = SimCatchmentScore(obs_np, window=window)
    sim = torch.from_numpy(sim_np).requires_grad_(True)
    mt = score.metrics(sim)
    assert set(mt) == {"n", "mse", "rmse", "nse", "r", "alpha", "beta", "kge", "bias"} and all(tuple(v.shape) == (B,) for v in mt.values())
    m = score.moments(sim.detach())
    n, mo, ms, soo, sss, sos, see = m.unbind(0)
    same = lambda a, b: SH.same_bits(a.detach().numpy(), b.detach().numpy())  # (the empty catchment holds NaN: torch.equal would refuse it)
    assert same(mt["n"], n) and same(mt["mse"], see / n) and same(mt["bias"], ms - mo) and same(mt["beta"], ms / mo)
    assert torch.equal(mt["nse"][:3], (1.0 - see / soo)[:3]) and torch.equal(mt["rmse"][:3], torch.sqrt(see / n)[:3])
    r, alpha, beta = sos / torch.sqrt(sss * soo), torch.sqrt(sss / soo), ms / mo
    assert torch.equal(mt["kge"][:3], (1.0 - torch.sqrt((r - 1.0) ** 2 + (alpha - 1.0) ** 2 + (beta - 1.0) ** 2))[:3])
    assert bool((mt["r"][:3].abs() <= 1.0).all()) and torch.equal(score.metrics(m)["kge"][:3], mt["kge"][:3])
    for metric in ("nse", "kge", "r", "mse"):
        sim.grad = None
        loss = score.loss(sim, metric=metric)
        want = (mt[metric][:3] if metric == "mse" else 1.0 - mt[metric][:3]).mean()
        assert float(loss.detach()) == float(want.detach()), metric
        loss.backward()
        g = sim.grad
        assert bool(torch.isfinite(g).all()) and float(g[:, :3].abs().max()) > 0
        assert not g[:, 3:].any()  # no usable record: neither value nor gradient -- exact zeros
    with pytest.raises(LgarError, match="nothing to score"):
        score.loss(sim, min_count=To + 1)
    with pytest.raises(LgarError, match="nothing to score"):
        SimCatchmentScore(np.full((To, B), np.nan), window=window).loss(sim)
    with pytest.raises(LgarError):
        score.loss(sim, metric="rmsle")
    with pytest.raises(LgarError):
        catchment_moments(sim, "score")


def test_warmup_rows_are_skipped_and_get_zero_gradient():
    from lgar_py_amd.scores import catchment_moments
    To, window, B, sim_np, obs_np = _gradient_job()
    warm = 4 * window
    head = np.random.default_rng(1).standard_normal((warm, B))
    score, plain = SimCatchmentScore(obs_np, window=window, warmup=warm), SimCatchmentScore(obs_np, window=window)
    assert (score.T, score.To, score.B, score.window, score.warmup) == (warm + To * window, To, B, window, warm)
    sim = torch.from_numpy(np.concatenate([head, sim_np])).requires_grad_(True)
    short = torch.from_numpy(sim_np).requires_grad_(True)
    m = catchment_moments(sim, score)
    assert SH.same_bits(m.detach().numpy(), plain.moments(short.detach()).numpy())
    score.loss(m, "kge").backward()
    plain.loss(short, "kge").backward()
    assert not sim.grad[:warm].any() and SH.same_bits(sim.grad[warm:].numpy(), short.grad.numpy())
    coef = torch.from_numpy(np.random.default_rng(2).standard_normal((4, B)))
    assert SH.same_bits(score.moments_grad(sim.detach(), m.detach(), coef)[warm:].numpy(),
                        SH.grad_ref(sim_np, obs_np, window, m.detach().numpy(), coef.numpy()))


def test_host_logic_rejections():
    import lgar_py_amd as lg
    from lgar_py_amd import LgarError
    from lgar_py_amd.scores import CatchmentScore
    assert lg.CatchmentScore is CatchmentScore and callable(lg.catchment_moments)
    obs = np.zeros((6, 3))
    for bad in (dict(observations=np.zeros(6)), dict(observations=np.zeros((2, 3, 4))), dict(observations="gauge"),
                dict(observations=obs, window=0), dict(observations=obs, window=-2), dict(observations=obs, window=1.5),
                dict(observations=obs, window=True), dict(observations=obs, warmup=-1), dict(observations=obs, window=4, warmup=6),
                dict(observations=obs, warmup=2.0), dict(observations=np.zeros((2 ** 20, 1)), window=2 ** 11)):
        with pytest.raises(LgarError):
            CatchmentScore(device="cpu", **bad)
    score = SimCatchmentScore(obs, window=2, warmup=4)
    assert score.observations.dtype == torch.float64 and tuple(score.observations.shape) == (6, 3) and score.T == 16
    good = torch.zeros(16, 3, dtype=torch.float64)
    assert tuple(score.moments(good).shape) == (7, 3)
    for bad in (torch.zeros(15, 3, dtype=torch.float64), torch.zeros(16, 2, dtype=torch.float64), torch.zeros(16, 3), torch.zeros(48, dtype=torch.float64),
                torch.zeros(16, 3, dtype=torch.float64, device="meta"), good.numpy()):
        with pytest.raises(LgarError, match=r"\[16, 3\]"):
            score.moments(bad)
    m, coef = score.moments(good), torch.zeros(4, 3, dtype=torch.float64)
    for args in ((good[:15], m, coef), (good, m[:6], coef), (good, m, coef[:3]), (good, m.float(), coef), (good, m, coef.to("meta"))):
        with pytest.raises(LgarError):
            score.moments_grad(*args)
    # a score on the CPU holds the host logic only: the kernels have no CPU fallback
    cpu = CatchmentScore(obs, window=2, warmup=4, device="cpu")
    for call in (lambda: cpu.moments(good), lambda: cpu.moments_grad(good, m, coef), lambda: cpu.loss(good)):
        with pytest.raises(LgarError, match="no CPU fallback"):
            call()
