"""CPU: the forward-mode tangent of the catchment snowpack (lgar_catchment_snow_tangent, CatchmentSnow.tangent,
catchment_snow_directions) on the host build of the kernel's own header (tests/snow_tangent_host): bit for bit against the numpy
statement of the recurrence, the adjoint identity against the existing adjoint (pinned to mpmath by tests/test_snow_host.py)
evaluated exactly, chunked calls, NaN confinement, the refusals."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import snow_host as SH
import snow_tangent_host as ST
from _hostbuild import same_bits

U = 2.0 ** -53


def gamma(m):
    """Higham's gamma_m = m u / (1 - m u)"""
    return m * U / (1.0 - m * U)


_directions = ST.directions


@pytest.mark.parametrize("B", ST.SHAPE_B)
def test_host_build_equals_the_numpy_statement_bit_for_bit(B):
    """The full product of snow_tangent_host.statement_product: for this B, T in {0, 1, 9, 17} x D in {1, 3, 7} x every
    combination of NULL inputs and wanted outputs x two (ld, k0), and all of it with and without the value state: 3072 calls.  At
    every B that holds the cells of all eight kinds every regime is counted > 0, and where cells 16 .. 21 exist the six ties."""
    calls, reg, tie = ST.statement_product(ST.call, B)
    assert calls == 12 * 64 * 2 * 2
    if B >= 63:
        assert all(v > 0 for v in reg.values()) and all(v > 0 for v in tie.values()), (reg, tie)


def test_sanitizer_build_on_the_same_recurrence():
    rng = np.random.default_rng(7)
    cases, wants = [], []
    for B, T, D in ((65, 17, 3), (2, 9, 7), (64, 0, 1), (1, 1, 1)):
        p, ta, _, _, _, par, state, dt = SH.case_data(rng, T, B)
        dp, dta, dpar, dst = _directions(rng, D, T, B)
        cases.append((p, ta, par, dt, state, D, dp, None, dpar, dst, D + 1, 1))
        wants.append(ST.snow_tangent_ref(p, ta, par, dt, state, D, dp, None, dpar, dst))
    for (dw, dice, dliq, dso), want in zip(ST.run_program(cases, sanitize=True), wants):
        assert same_bits(dw[:, :, 1:], want[0]) and (dw[:, :, 0] == 0.0).all()
        assert same_bits(dso, want[3]) and (dice.size == 0 or (same_bits(dice, want[1]) and same_bits(dliq, want[2])))


def _identity(p, ta, par, dt, state, D, dirs, g, tangent):
    """Both sides of <gw, dw> + <gice, dice> + <gliq, dliq> = <gp, dp> + <gta, dta> + <gpar, dpar> + <gstate, dstate> per
    direction, exactly (fractions.Fraction of the floats), with the adjoint of tests/snow_host's host library."""
    gw, gice, gliq = g
    _, ice, liq, _ = SH.snow_ref(p, ta, par, dt, state)
    (gp, gta, gpar, gstate), = SH.run([("grad", gw, gice, gliq, p, ta, ice, liq, par, dt, state, True, True, True)])
    dw, dice, dliq, _ = tangent
    dp, dta, dpar, dst = dirs
    F = lambda a: [Fraction(float(v)) for v in np.asarray(a).ravel()]
    dot = lambda a, b: sum(x * y for x, y in zip(F(a), F(b)))
    out = []
    for k in range(D):
        left = dot(gw, dw[:, :, k]) + dot(gice, dice[k]) + dot(gliq, dliq[k])
        right = dot(gp, dp[k]) + dot(gta, dta[k]) + dot(gpar, dpar[k]) + dot(gstate, dst[k])
        out.append((left, right))
    return out


def test_the_tangent_is_the_transpose_of_the_adjoint():
    """The identity, both sides exact.  The two sides are the same bilinear form of (g, d) with the forward's rounded values as
    coefficients (both walks re-form them through sn_step: the same bits), so in exact arithmetic they are equal and what is left
    is the rounding of the two walks.  Counting roundings on the longest path of a row of the tangent: pd' 1, fr' 4 (two
    differences, a product, a quotient), rain' 3, dry' 1, snow' 3, ice1' 1, ice2' 2, liq1' 3 (pm' and pr', 3 each, stand in the place
    of ice1' / liq' on their branches), cap' 3, out' 1: at most 22 per row on top of what ice', liq' carried in, so after T rows
    (1 + u)^(22 T), plus cd' 1, cr' 3 once and the division of dw: m = 22 T + 5.  The adjoint's rows are shorter (at most 16
    roundings: section 19 counts them), so the same m covers it.  The magnitude each side's error is relative to is the same form
    on absolute values, every difference a sum -- <|g|, T_abs |d|>, T_abs the recurrence of snow_tangent_ref(absolute=True), which
    by transposition is the adjoint's own form on absolute values too.  Held: |left - right| <= gamma_m <|g|, T_abs |d|>.
    The bound refuses a dropped cwh * ice2', a wrong sign on refr' and a missing fr': the factors are printed and recorded in
    profiles/r18/error_bound.txt."""
    rng = np.random.default_rng(1906)
    worst, wrong_worst = 0.0, {"no_cwh_ice2": 0.0, "refr_sign": 0.0, "no_fr": 0.0}
    for B, T, D in ((8, 17, 3), (22, 9, 7), (24, 1, 2)):
        p, ta, gw, gice, gliq, par, state, dt = SH.case_data(rng, T, B)
        dirs = _directions(rng, D, T, B)
        m = 22 * T + 5
        rc, dw, dice, dliq, dso = ST.call(p, ta, par, dt, state, D, *dirs)
        aw, ai, al, _ = ST.snow_tangent_ref(p, ta, par, dt, state, D, *dirs, absolute=True)
        F = lambda a: [Fraction(float(v)) for v in np.asarray(a).ravel()]
        dot = lambda a, b: sum(x * y for x, y in zip(F(a), F(b)))
        bounds = [Fraction(gamma(m)) * (dot(np.abs(gw), aw[:, :, k]) + dot(np.abs(gice), ai[k]) + dot(np.abs(gliq), al[k])) for k in range(D)]
        for (left, right), bar in zip(_identity(p, ta, par, dt, state, D, dirs, (gw, gice, gliq), (dw, dice, dliq, dso)), bounds):
            assert bar > 0 and abs(left - right) <= bar, (B, T, float(abs(left - right) / bar))
            worst = max(worst, float(abs(left - right) / bar))
        for variant in wrong_worst:
            bad = ST.snow_tangent_ref(p, ta, par, dt, state, D, *dirs, variant=variant)
            ratios = [float(abs(l - r) / bar) for (l, r), bar in zip(_identity(p, ta, par, dt, state, D, dirs, (gw, gice, gliq), bad), bounds)]
            wrong_worst[variant] = max(wrong_worst[variant], max(ratios))
    print("snow tangent, adjoint identity: worst |left - right| / bound = %.3g; wrong tangents: %s"
          % (worst, ", ".join("%s %.3g" % kv for kv in wrong_worst.items())))
    assert all(v > 1.0 for v in wrong_worst.values()), wrong_worst


def test_chunked_calls_carrying_dstate_equal_one_call_in_bits():
    rng = np.random.default_rng(5)
    B, T, D = 65, 17, 3
    p, ta, _, _, _, par, state, dt = SH.case_data(rng, T, B)
    dp, dta, dpar, dst = _directions(rng, D, T, B)
    _, dw, dice, dliq, dso = ST.call(p, ta, par, dt, state, D, dp, dta, dpar, dst)
    _, _, _, states = SH.snow_ref(p, ta, par, dt, state)
    s, ds, parts = state, dst, []
    for lo, hi in ((0, 1), (1, 8), (8, 9), (9, 17), (17, 17)):
        c = np.ascontiguousarray
        _, w2, i2, l2, ds2 = ST.call(p[lo:hi], ta[lo:hi], par, dt, s, D, c(dp[:, lo:hi]), c(dta[:, lo:hi]), dpar, ds)
        parts.append((w2, i2, l2))
        s, ds = SH.snow_ref(p[lo:hi], ta[lo:hi], par, dt, s)[3], ds2
    assert same_bits(np.concatenate([x[0] for x in parts]), dw) and same_bits(ds, dso)
    assert same_bits(np.concatenate([x[1] for x in parts], axis=1), dice) and same_bits(np.concatenate([x[2] for x in parts], axis=1), dliq)


@pytest.mark.parametrize("which", ["dp", "dta", "dpar", "dstate"])
def test_a_nan_stays_in_its_cell_and_its_direction(which):
    ST.nan_confinement(ST.call, which)


def test_entry_point_refuses_bad_arguments():
    rng = np.random.default_rng(3)
    B, T, D = 4, 3, 2
    p, ta, _, _, _, par, state, dt = SH.case_data(rng, T, B)
    lib, E = ST.library(), -1
    dw, dice, dliq = np.zeros((T, B, D)), np.zeros((D, T, B)), np.zeros((D, T, B))
    a = lambda x: None if x is None else x.ctypes.data

    def call(p=p, ta=ta, T=T, B=B, par=par, dt=dt, D=D, dw=dw, ld=D, k0=0, dice=None, dliq=None):
        return lib.snowtanhost_catchment_snow_tangent(a(p), a(ta), T, B, a(par), dt, None, D, None, None, None, None, a(dw), ld, k0, a(dice), a(dliq), None)

    assert call() == 0 and call(dice=dice, dliq=dliq) == 0
    assert call(T=-1) == E and call(B=-1) == E and call(D=-1) == E and call(k0=-1) == E
    assert call(ld=D - 1) == E and call(ld=D, k0=1) == E
    assert call(dt=0.0) == E and call(dt=float("nan")) == E and call(dt=float("inf")) == E
    assert call(dice=dice) == E and call(dliq=dliq) == E
    assert call(p=None) == E and call(ta=None) == E and call(par=None) == E and call(dw=None) == E
    assert call(B=0, p=None) == 0 and call(D=0, dw=None, ld=0) == 0 and call(T=0, p=None, dw=None) == 0  # nothing to do


def test_catchment_snow_directions_through_the_host_build():
    """One direction per parameter that requires grad: d water / d parameter against the existing adjoint, column by column of
    the identity (gw one-hot is too many launches: a random gw instead), and the shape of what comes back."""
    import lgar_py_amd as lg
    rng = np.random.default_rng(11)
    B, T = 5, 17
    p, ta, gw, _, _, par, state, dt = SH.case_data(rng, T, B)
    par[1] = np.maximum(par[1], par[0] + 0.5)
    t = lambda x: torch.tensor(x)
    pars = [t(par[j]) for j in range(7)]
    for j in (2, 3, 4):
        pars[j].requires_grad_(True)
    water, fd = lg.catchment_snow_directions(t(p), t(ta), *pars, dt, state=t(np.abs(state)), owner=ST.SimSnow)
    assert fd.K == 3 and fd.d_pet is None and tuple(fd.d_precip.shape) == (3, T, B) and all(a is b for a, b in zip(fd.params, pars[2:5]))
    w, _, _, _ = SH.snow_ref(p, ta, par, dt, np.abs(state))
    assert same_bits(water.numpy(), w) and not water.requires_grad
    out = SH.SimCatchmentSnow.function(t(p), t(ta), *pars, dt, state=t(np.abs(state)))
    (out * t(gw)).sum().backward()
    for k, j in enumerate((2, 3, 4)):
        got = (fd.d_precip[k] * t(gw)).sum(0)
        assert torch.allclose(got, pars[j].grad, rtol=1e-9, atol=1e-12 * float(pars[j].grad.abs().max())), j
