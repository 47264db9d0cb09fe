"""CPU: the catchment snowpack (lgar_catchment_snow / lgar_catchment_snow_grad, include/lgar.h).

The per-cell walks the GPU kernels run (lgar_py_amd/csrc/lgar_snow.hpp) are compiled for the host into a small stand-alone
program (tests/snow_host).  It is held BIT FOR BIT to the numpy statement of the definition (snow_host.snow_ref /
snow_grad_ref); the same program built with AddressSanitizer + UBSan runs the same cases.  Independently of the statement the
definition is held to statements that do not come from it: the warm identity, a degree-day recurrence without the liquid store,
the mass balance as an exact sum, and the adjoint to derivatives of the real-arithmetic statement taken in mpmath.  The same
header as a shared library stands behind lgar_py_amd.snow.CatchmentSnow (snow_host.SimCatchmentSnow), so the host logic of
snow.py -- validation, carry, autograd -- runs here too."""
import itertools
from fractions import Fraction

import mpmath
import numpy as np
import pytest
import torch

import snow_host as SH
from snow_host import SimCatchmentSnow

U = 2.0 ** -53  # unit roundoff of fp64


def gamma(m):
    """Higham's gamma_m = m u / (1 - m u): (1 + d_1) .. (1 + d_m) = 1 + theta, |theta| <= gamma_m, for |d_i| <= u (3.1)."""
    return m * U / (1.0 - m * U)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---- 1. the host build against the numpy definition ------------------------------------------------------------------------
FWD_WANTS = tuple(itertools.product((True, False), repeat=2))   # pack, state_out
GRAD_WANTS = tuple(itertools.product((True, False), repeat=4))  # gice / gliq given, gta, gpar, gstate


def _grid(shape_t=SH.SHAPE_T):
    """B in {1, 2, 63, 64, 65, 257} x T x state_in present or NULL: the forward with every combination of pack and state_out
    wanted; the adjoint with every combination of gta, gpar and gstate wanted, with gice / gliq given and NULL.
    (cases, references, the count of rows per regime, the count of rows per exact tie)."""
    rng = np.random.default_rng(19)
    cases, refs = [], []
    rows, ties = {k: 0 for k in SH.REGIMES}, {k: 0 for k in SH.TIES}
    for B in SH.SHAPE_B:
        for T in shape_t:
            p, ta, gw, gi, gl, par, state, dt = SH.case_data(rng, T, B)
            for st in (None, state):
                w, ice, liq, so = SH.snow_ref(p, ta, par, dt, st)
                n_rows, n_ties, _, _ = SH.regimes(p, ta, par, dt, st)
                for k in rows:
                    rows[k] += n_rows[k]
                for k in ties:
                    ties[k] += n_ties[k]
                for pack, state_out in FWD_WANTS:
                    cases.append(("fwd", p, ta, par, dt, st, pack, state_out))
                    refs.append((w, ice if pack else None, liq if pack else None, so if state_out else None))
                full = SH.snow_grad_ref(gw, gi, gl, p, ta, ice, liq, par, dt, st)
                bare = SH.snow_grad_ref(gw, None, None, p, ta, ice, liq, par, dt, st)
                for gpack, want_ta, want_par, want_state in GRAD_WANTS:
                    ref = full if gpack else bare
                    cases.append(("grad", gw, gi if gpack else None, gl if gpack else None, p, ta, ice, liq, par, dt, st, want_ta, want_par, want_state))
                    refs.append((ref[0], ref[1] if want_ta else None, ref[2] if want_par else None, ref[3] if want_state else None))
    return cases, refs, rows, ties


@pytest.fixture(scope="module")
def grid():
    return _grid()


def _shape(c):
    return np.asarray(c[1]).shape


def _check(cases, refs, got):
    assert len(got) == len(refs) == len(cases)
    for c, r, o in zip(cases, refs, got):
        for want, have in zip(r, o):
            # (an output of no elements is not there at all: the host program hands a null pointer for it)
            assert (want is None or want.size == 0) == (have is None or have.size == 0), (c[0], _shape(c))
            assert want is None or want.size == 0 or SH.same_bits(have, want), (c[0], _shape(c))


def test_host_build_equals_the_numpy_definition_bit_for_bit(grid):
    cases, refs, rows, ties = grid
    _check(cases, refs, SH.run(cases))
    # every regime of the walk is taken somewhere in the case set, and every exact tie occurs
    print("rows per regime:", rows)
    print("rows per exact tie:", ties)
    assert set(rows) == set(SH.REGIMES) and all(n > 0 for n in rows.values()), rows
    assert set(ties) == set(SH.TIES) and all(n > 0 for n in ties.values()), ties
    # what the definition says about the corners, on the references themselves
    for c, r in zip(cases, refs):
        T, B = _shape(c)
        if c[0] == "fwd" and T == 0 and r[3] is not None:  # T = 0 copies the state, or writes zeros
            assert SH.same_bits(r[3], np.zeros((2, B)) if c[5] is None else np.asarray(c[5]))
        if c[0] == "grad" and T == 0:  # T = 0: zeros
            assert all(a is None or not a.any() for a in r)
    assert {_shape(c) for c in cases if c[0] == "fwd"} == {(T, B) for T in SH.SHAPE_T for B in SH.SHAPE_B}
    assert len(cases) == len(SH.SHAPE_B) * len(SH.SHAPE_T) * 2 * (len(FWD_WANTS) + len(GRAD_WANTS))


def test_the_planted_ties_sit_where_they_were_planted_and_go_where_the_selects_send_them():
    """case_data plants, in row 0 of cells 16 .. 21 with the state given, Ta == tlo (lo), Ta == thi (hi), d == 0 (not warm),
    pm == ice1 (melt free: melt = pm), pr == liq (refreeze free: refr = pr), liq1 == cap (hold)."""
    p, ta, _, _, _, par, state, dt = SH.case_data(np.random.default_rng(5), 9, 65)
    for dt_h in (dt, 1.0, 0.25, 24.0):
        if dt_h != dt:  # the planted state is in units of dt_h: cd = 2 dt_h, cr = dt_h, exactly
            state = state.copy()
            for k in SH.TIE_CELLS.values():
                state[:, k] = state[:, k] * (dt_h / dt)
            dt = dt_h
        _, _, reg, tie = SH.regimes(p, ta, par, dt, state)
        for name, went in (("Ta==tlo", "lo"), ("Ta==thi", "hi"), ("d==0", "refreeze_free"), ("pm==ice1", "melt_free"), ("pr==liq", "refreeze_free"),
                           ("liq1==cap", "hold")):
            assert tie[name][0, SH.TIE_CELLS[name]] and reg[went][0, SH.TIE_CELLS[name]], (name, dt)
        assert not reg["mid"][0, SH.TIE_CELLS["Ta==tlo"]] and not reg["mid"][0, SH.TIE_CELLS["Ta==thi"]]


def test_sanitizer_build_on_the_same_cases(grid):
    """AddressSanitizer + UBSan build of the same program (a stand-alone executable: nothing is loaded into python; every array is
    allocated at its exact size) over the same cases: clean, with the same bits.  Any finding aborts the program."""
    cases, refs, _, _ = grid
    _check(cases, refs, SH.run(cases, sanitize=True))


# ---- 2. independent of the statement ----------------------------------------------------------------------------------------
def test_warm_identity():
    """A zero state, every Ta > max(thi, tm), dt_h a power of two: fr = 1, rain = pd, dry = pd - pd = 0, no ice ever, melt limited
    by an ice1 of 0, cap = 0: w has the bits of p where p > 0 and is +0.0 where p == 0 -- whatever the other parameters are."""
    rng = np.random.default_rng(2)
    T, B = 17, 65
    _, _, _, _, _, par, _, _ = SH.case_data(rng, T, B)
    p = rng.random((T, B)) * 10.0 ** rng.integers(-6, 3, (T, B)) * (rng.random((T, B)) < 0.7)
    ta = np.maximum(par[SH.THI], par[SH.TM])[None, :] + 10.0 ** rng.uniform(-3, 1.5, (T, B))
    assert (p == 0).sum() > 50 and (p > 0).sum() > 500
    cases = [("fwd", p, ta, par, dt, st, True, True) for dt in (1.0, 0.25, 32.0, 2.0 ** -7) for st in (None, np.zeros((2, B)))]
    for w, ice, liq, so in SH.run(cases):
        assert SH.same_bits(w, p)  # (+0.0 where p == +0.0: the same bits too)
        assert not ice.any() and not liq.any() and not so.any()


def test_degree_day_recurrence_without_the_liquid_store():
    """cwh = 0 and cfr = 0 leave no liquid store: the pack is the plain degree-day recurrence
        ice1 = ice + sfcf (pd - pd fr);   melt = Ta > tm ? min(cd (Ta - tm), ice1) : 0;   ice = ice1 - melt;   w = (pd fr + melt) / dt
    written here without it (p >= 0, the state's liq = 0).  Equal values (a zero's sign aside)."""
    rng = np.random.default_rng(6)
    T, B = 17, 65
    p, ta, _, _, _, par, state, dt = SH.case_data(rng, T, B)
    p, par[SH.CWH], par[SH.CFR], state[1] = np.abs(p), 0.0, 0.0, 0.0
    (w, ice, liq, _), = SH.run([("fwd", p, ta, par, dt, state, True, False)])
    tlo, thi, tm, sfcf = par[SH.TLO], par[SH.THI], par[SH.TM], par[SH.SFCF]
    cd, s = par[SH.CFMAX] * dt, state[0].copy()
    with np.errstate(all="ignore"):
        for t in range(T):
            pd = p[t] * dt
            fr = np.where(ta[t] <= tlo, 0.0, np.where(ta[t] >= thi, 1.0, (ta[t] - tlo) / (thi - tlo)))
            ice1 = s + sfcf * (pd - pd * fr)
            melt = np.where(ta[t] > tm, np.minimum(cd * (ta[t] - tm), ice1), 0.0)
            s = ice1 - melt
            assert np.array_equal(ice[t], s) and np.array_equal(w[t], (pd * fr + melt) / dt), t
    assert not liq.any() and float(w.sum()) > 0 and float(ice.max()) > 0


def test_mass_closes_per_cell():
    """ice_T + liq_T + dt sum w = ice_0 + liq_0 + dt sum (fr + sfcf (1 - fr)) p per cell over 17 rows, the difference taken exactly
    (fractions.Fraction of the floats, fr the exact quotient), within gamma_22T M, M = ice_0 + liq_0 + sum (1 + sfcf) p dt.
    With p >= 0 and a state >= 0 no store goes negative (asserted), so every intermediate of a row is at most the mass that has
    entered, M_t <= M.  Per row: the water that enters is rain + snow, where pd rounds once, fr three times (two differences of
    inputs and a quotient), rain = pd fr once more (5), dry = pd - rain once more on |pd| + |rain| (6), snow = sfcf dry once
    more (7): off by at most 5 u pd + 7 u sfcf (2 pd) <= 14 u M_t.  Melt and refreeze move one and the same float between the
    stores.  The stores round in ice + snow, ice1 - melt, + refr, liq + rain, + melt, - refr, liq1 - cap and out / dt_h: 8
    roundings of quantities <= M_t.  22 roundings of M_t per row, T rows.
    Measured: worst |miss| 1.08e-14, worst miss / bound 0.00896."""
    rng = np.random.default_rng(4)
    T, B = 17, 257
    p, ta, _, _, _, par, state, dt = SH.case_data(rng, T, B)
    p, state = np.abs(p), np.abs(state)
    (w, ice, liq, so), = SH.run([("fwd", p, ta, par, dt, state, True, True)])
    assert float(ice.min()) >= 0 and float(liq.min()) >= 0 and float(w.min()) >= 0  # the pack never goes negative
    F = lambda v: Fraction(float(v))
    worst, worst_abs = 0.0, 0.0
    for b in range(B):
        tlo, thi, sfcf = F(par[SH.TLO, b]), F(par[SH.THI, b]), F(par[SH.SFCF, b])
        entered, M = F(0), F(state[0, b]) + F(state[1, b])
        for t in range(T):
            Ta = F(ta[t, b])
            fr = F(0) if Ta <= tlo else (F(1) if Ta >= thi else (Ta - tlo) / (thi - tlo))
            entered += F(dt) * F(p[t, b]) * (fr + sfcf * (1 - fr))
            M += (1 + sfcf) * F(p[t, b]) * F(dt)
        miss = abs(F(so[0, b]) + F(so[1, b]) + F(dt) * sum(F(v) for v in w[:, b]) - F(state[0, b]) - F(state[1, b]) - entered)
        bar = Fraction(gamma(22 * T)) * M
        assert miss <= bar, b
        worst, worst_abs = max(worst, float(miss / bar)), max(worst_abs, float(miss))
    print("snow mass closure: worst |miss| %.3g, worst miss / bound %.3g (gamma_%d M), %d cells x %d rows" % (worst_abs, worst, 22 * T, B, T))
    assert 0.0 < worst <= 1.0 and float(w.sum()) > 0


# ---- 3. the adjoint is the true derivative ------------------------------------------------------------------------------------
def _derivative_data():
    """B = 7, T = 9, dt_h = 1, p > 0 everywhere: ordinary packs (0, 1, 5), a pack under tlo == thi (2), a large cfmax on a thin pack
    that melts away and is snowed on again (3: melt limited), a large cfr (4: refreeze limited), a deep cold pack (6)."""
    rng = np.random.default_rng(77)
    T, B = 9, 7
    jit = lambda: 1.0 + 0.05 * rng.random(B)
    tlo = np.array([-1.0, -1.5, 0.4, -1.0, -0.5, -2.0, -1.0]) * jit()
    thi = np.array([2.0, 1.5, 0.4, 2.5, 2.0, 1.0, 3.0]) * jit()
    thi[2] = tlo[2]
    tm = np.array([0.3, 0.5, 0.2, 0.1, 0.6, -0.3, 0.4]) * jit()
    sfcf = np.array([1.1, 0.9, 1.2, 1.0, 1.05, 0.95, 1.15]) * jit()
    cfmax = np.array([0.15, 0.2, 0.1, 3.0, 0.12, 0.25, 0.1]) * jit()
    cfr = np.array([0.05, 0.08, 0.05, 0.05, 5.0, 0.1, 0.05]) * jit()
    cwh = np.array([0.1, 0.05, 0.08, 0.1, 0.12, 0.06, 0.1]) * jit()
    state = np.stack([np.array([3.0, 2.0, 1.5, 0.8, 2.5, 4.0, 6.0]) * jit(), np.array([0.1, 0.05, 0.1, 0.05, 0.2, 0.1, 0.3]) * jit()])
    ta = np.array([[-4.0, -0.3, 1.1, 3.5, 0.7, -2.5, 1.7, 4.2, -1.4]] * B).T * (1.0 + 0.2 * rng.random((T, B))) + rng.normal(0.0, 0.4, (T, B))
    ta[:, 6] -= 3.0
    p = 0.2 + 1.5 * rng.random((T, B))
    mixed = lambda: (rng.random((T, B)) - 0.4) * 2.0
    return p, ta, mixed(), 0.5 * mixed(), 0.5 * mixed(), np.stack([tlo, thi, tm, sfcf, cfmax, cfr, cwh]), state, 1.0


def _mp_cell(p, ta, par, ice, liq, dt, gw, gi, gl, detail=False):
    """One cell of the definition in REAL arithmetic (mpmath at the working precision): the loss sum gw w + gi ice + gl liq and,
    with detail, every value and flag of every row."""
    tlo, thi, tm, sfcf, cfmax, cfr, cwh = par
    cd = cfmax * dt
    cr = cfr * cd
    loss, rows, Z, ONE = mpmath.mpf(0), [], mpmath.mpf(0), mpmath.mpf(1)
    for t in range(len(p)):
        Ta, pd = ta[t], p[t] * dt
        lo = Ta <= tlo
        hi = (not lo) and Ta >= thi
        fr = Z if lo else (ONE if hi else (Ta - tlo) / (thi - tlo))
        rain = pd * fr
        dry = pd - rain
        d = Ta - tm
        warm = d > 0
        ice1 = ice + sfcf * dry
        pm, pr = cd * d, cr * (-d)
        ml, rl = pm > ice1, pr > liq
        melt = (ice1 if ml else pm) if warm else Z
        refr = Z if warm else (liq if rl else pr)
        ice2 = (ice1 - melt) + refr
        liq1 = ((liq + rain) + melt) - refr
        cap = cwh * ice2
        over = liq1 > cap
        out = liq1 - cap if over else Z
        rows.append(dict(Ta=Ta, pd=pd, lo=lo, hi=hi, mid=not lo and not hi, fr=fr, rain=rain, dry=dry, d=d, warm=warm, ice_in=ice, liq_in=liq, ice1=ice1,
                         pm=pm, pr=pr, ml=ml, rl=rl, melt=melt, refr=refr, ice2=ice2, liq1=liq1, cap=cap, over=over))
        ice, liq = ice2, (cap if over else liq1)
        loss += gw[t] * (out / dt) + gi[t] * ice + gl[t] * liq
    return (loss, rows) if detail else loss


OUTPUTS = ("gp", "gta", "gpar", "gstate")


@pytest.fixture(scope="module")
def derivative():
    """The data of the derivative tests, the derivatives of the real-arithmetic statement by central differences in mpmath, the
    adjoint on absolute values and the operation counts m (test_the_adjoint_is_the_true_derivative has the derivation)."""
    mpmath.mp.dps = 60
    p, ta, gw, gi, gl, par, state, dt = _derivative_data()
    T, B = p.shape
    M = mpmath.mpf
    h = M(10) ** -20
    grid = lambda rows: [[None] * B for _ in range(rows)]
    want, mag = dict(gp=grid(T), gta=grid(T), gpar=grid(7), gstate=grid(2)), dict(gp=grid(T), gta=grid(T), gpar=grid(7), gstate=grid(2))
    n_rows, _, reg, _ = SH.regimes(p, ta, par, dt, state)
    cond = dict(n_ice=0.0, margin=np.inf)
    for b in range(B):
        x = [M(float(v)) for v in p[:, b]] + [M(float(v)) for v in ta[:, b]] + [M(float(par[k, b])) for k in range(7)] + [M(float(state[k, b])) for k in range(2)]
        g = [[M(float(v)) for v in a[:, b]] for a in (gw, gi, gl)]
        cell = lambda v, **kw: _mp_cell(v[:T], v[T:2 * T], v[2 * T:2 * T + 7], v[2 * T + 7], v[2 * T + 8], M(dt), g[0], g[1], g[2], **kw)
        _, rows = cell(x, detail=True)
        # no row within a relative 1e-6 of a switch (Ta against tlo and thi, d against 0, pm against ice1 where warm, pr against liq
        # where not, liq1 against cap), and the float walk takes the real walk's branches
        for t, row in enumerate(rows):
            rel = lambda a, c: abs(a - c) / max(abs(a), abs(c), M(10) ** -300)
            margins = [rel(row["Ta"], x[2 * T]), rel(row["Ta"], x[2 * T + 2]), rel(row["liq1"], row["cap"]),
                       rel(row["pm"], row["ice1"]) if row["warm"] else rel(row["pr"], row["liq_in"])]
            if x[2 * T] != x[2 * T + 1]:
                margins.append(rel(row["Ta"], x[2 * T + 1]))
            cond["margin"] = min(cond["margin"], float(min(margins)))
            for k, v in (("lo", row["lo"]), ("hi", row["hi"]), ("melt_limited", row["warm"] and row["ml"]), ("melt_free", row["warm"] and not row["ml"]),
                         ("refreeze_limited", not row["warm"] and row["rl"]), ("refreeze_free", not row["warm"] and not row["rl"]), ("over", row["over"])):
                assert bool(v) == bool(reg[k][t, b]), (k, t, b)
        for i in range(2 * T + 9):
            xp, xm = list(x), list(x)
            hi_ = h * abs(x[i])  # relative to the variable; no variable is 0
            assert hi_ > 0
            xp[i], xm[i] = x[i] + hi_, x[i] - hi_
            if b == 2 and i in (2 * T, 2 * T + 1):
                # tlo == thi: a step.  Ta is held off it (above), so the loss does not depend on where it is: both derivatives are 0,
                # and moving one of the two alone would open a transition of width h
                xp[2 * T] = xp[2 * T + 1] = x[i] + hi_
                xm[2 * T] = xm[2 * T + 1] = x[i] - hi_
            dv = (cell(xp) - cell(xm)) / (2 * hi_)
            if i < T:
                want["gp"][i][b] = dv
            elif i < 2 * T:
                want["gta"][i - T][b] = dv
            elif i < 2 * T + 7:
                want["gpar"][i - 2 * T][b] = dv
            else:
                want["gstate"][i - 2 * T - 7][b] = dv
        # the adjoint on absolute values (every difference a sum, dry as |pd| + |rain|), and the forward error of ice2 in units of u
        tlo, thi, tm, sfcf, cfmax, cfr, cwh = x[2 * T:2 * T + 7]
        cd = cfmax * M(dt)
        cr = cfr * cd
        span = thi - tlo
        e_i, e_l, e_ice2 = M(0), M(0), []
        for row in rows:
            wm, wf = row["warm"] and row["ml"], row["warm"] and not row["ml"]
            cl, cf = not row["warm"] and row["rl"], not row["warm"] and not row["rl"]
            e_rain = 5 * abs(row["rain"])
            e_snow = 7 * sfcf * (abs(row["pd"]) + abs(row["rain"]))
            e_ice1 = e_i + e_snow + abs(row["ice1"])
            e_melt = e_ice1 if wm else (3 * abs(row["pm"]) if wf else M(0))
            e_refr = e_l if cl else (4 * abs(row["pr"]) if cf else M(0))
            e_2 = M(0) if wm else e_ice1 + e_melt + abs(row["ice1"] - row["melt"]) + e_refr + abs(row["ice2"])
            e_liq1 = (e_l + e_rain + abs(row["liq_in"] + row["rain"]) + e_melt + abs(row["liq_in"] + row["rain"] + row["melt"]) + e_refr
                      + abs(row["liq1"]))
            e_i, e_l = e_2, (cwh * e_2 + abs(row["cap"]) if row["over"] else e_liq1)
            e_ice2.append(e_2)
            if row["over"] and row["ice2"] != 0:
                cond["n_ice"] = max(cond["n_ice"], float(e_2 / abs(row["ice2"])))
        li, ll = M(0), M(0)
        acc = dict(tlo=M(0), thi=M(0), tm=M(0), sfcf=M(0), cd=M(0), cr=M(0), cwh=M(0))
        for t in range(T - 1, -1, -1):
            row = rows[t]
            wm, wf = row["warm"] and row["ml"], row["warm"] and not row["ml"]
            cl, cf = not row["warm"] and row["rl"], not row["warm"] and not row["rl"]
            li, ll, go = li + abs(g[1][t]), ll + abs(g[2][t]), abs(g[0][t]) / M(dt)
            dl1 = go if row["over"] else ll
            dcap = ll + go if row["over"] else M(0)
            di2 = li + cwh * dcap
            acc["cwh"] += dcap * abs(row["ice2"])
            dmelt = drefr = dl1 + di2
            di1 = di2 + dmelt if wm else di2
            dliq = dl1 + drefr if cl else dl1
            gd = dmelt * cd if wf else (drefr * cr if cf else M(0))
            if wf:
                acc["cd"] += dmelt * abs(row["d"])
            if cf:
                acc["cr"] += drefr * abs(row["d"])
            acc["tm"] += gd
            acc["sfcf"] += di1 * (abs(row["pd"]) + abs(row["rain"]))
            sd = sfcf * di1
            drain = dl1 + sd
            dfr = drain * abs(row["pd"])
            mag["gp"][t][b] = (sd + drain * row["fr"]) * M(dt)
            mag["gta"][t][b] = gd + dfr / span if row["mid"] else gd
            if row["mid"]:
                acc["tlo"] += dfr * abs(row["Ta"] - thi) / span ** 2
                acc["thi"] += dfr * abs(row["Ta"] - tlo) / span ** 2
            li, ll = di1, dliq
        mag["gstate"][0][b], mag["gstate"][1][b] = li, ll
        for k, v in enumerate((acc["tlo"], acc["thi"], acc["tm"], acc["sfcf"], M(dt) * (acc["cd"] + cfr * acc["cr"]), cd * acc["cr"], acc["cwh"])):
            mag["gpar"][k][b] = v
    assert cond["margin"] > 1e-6, cond
    m = dict(gstate=6 * T, gp=6 * T + 8, gta=6 * T + 7, gpar=int(np.ceil(6 * T + T + 16 + cond["n_ice"])))
    return dict(data=(p, ta, gw, gi, gl, par, state, dt), want=want, mag=mag, m=m, cond=cond, rows=n_rows)


def _ratios(d, got):
    """per output, error / bound of every element against the mpmath derivative (inf where the bound is 0 and the error is not)"""
    out = {}
    for k, arr in zip(OUTPUTS, got):
        r = np.zeros(arr.shape)
        for i in range(arr.shape[0]):
            for j in range(arr.shape[1]):
                err, bar = abs(mpmath.mpf(float(arr[i, j])) - d["want"][k][i][j]), mpmath.mpf(gamma(d["m"][k])) * d["mag"][k][i][j]
                r[i, j] = float(err / bar) if bar else (0.0 if err == 0 else np.inf)
        out[k] = r
    return out


def test_the_adjoint_is_the_true_derivative(derivative):
    """gp, gta, gpar and gstate of the host build against the derivatives of L = sum gw w + sum gice ice + sum gliq liq of the
    definition's REAL-arithmetic statement, taken in mpmath at 60 digits by central differences with h = 1e-20 |x| (L is piecewise
    polynomial-rational in every variable: the quotient misses the derivative by h^2 L''' / 6 ~ 1e-40 between switches, and no row
    lies within a relative 1e-6 of one -- asserted, with the float walk taking the real walk's branch in every row).  B = 7,
    T = 9, p > 0; rows in lo, mid and hi, melt limited and free, refreeze limited and free, over and hold, and a cell with
    tlo == thi all occur (asserted).

    The bound is gamma_m x (the same adjoint on absolute values: every difference a sum, dry taken as |pd| + |rain|), to first order
    in u.  Derivation, with figures from the real-arithmetic walk (never from the code under test):
      the state adjoint.  li and ll pass a row through li + gice, ll + gliq, gw / dt_h (1 rounding each), ll - go (2 on its path),
        cwh dcap (3), li + that (4), dmelt or drefr (5), di2 + dmelt or dl1 + drefr (6).  The factors are 1 and cwh, an input: no
        forward value enters but through the flags, which are the real walk's.  A path of the expansion passes a row once:
        m_gstate = 6 T.
      gp.  sd = sfcf di1 (7), drain = dl1 - sd (8), drain fr (fr: two differences of inputs and a quotient, 3: 12), sd + that
        (13), times dt_h (14): 8 on top of the row's 6: m_gp = 6 T + 8.
      gta.  gd = dmelt cd (cd rounds once: 7) or -(drefr cr) (cr twice: 8); dfr = drain pd (pd once: 10), / span (span once:
        12), gd + that (13): m_gta = 6 T + 7.
      gpar.  A term is a cotangent of the row (<= 8 roundings with the row's 6) times forward values: (Ta - thi) / span^2 behind dfr
        (16 in all, the largest of the input-only factors), d (1), dry (6 relative to |pd| + |rain|: pd once, rain 5 times, the
        difference once), or ice2.  ice2 is the one STATE a term holds.  Its forward error, in u, from the recurrence over the rows
        (e_i, e_l: the errors of ice and liq behind the row, 0 before row 0):
            e_snow = 7 sfcf (|pd| + |rain|);  e_ice1 = e_i + e_snow + |ice1|
            e_melt = e_ice1 (limited) | 3 |pm| (free) | 0;   e_refr = e_l (limited) | 4 |pr| (free) | 0
            e_ice2 = 0 where the melt is limited (ice1 - ice1 + 0.0 is exactly 0), else
                     e_ice1 + e_melt + |ice1 - melt| + e_refr + |ice2|
            e_liq1 = e_l + 5 |rain| + |liq + rain| + e_melt + |liq + rain + melt| + e_refr + |liq1|
            e_l'   = cwh e_ice2 + |cap| (over) | e_liq1 (hold);   e_i' = e_ice2
        n_ice = the largest e_ice2 / |ice2| of a row that is over (where gcwh takes its term).  Each accumulator adds <= T terms,
        and gcfmax = dt_h (gcd + cfr gcr) adds 3:  m_gpar = 6 T + T + 16 + n_ice.
    It refuses, on every output the change reaches: dcap dropped from di2 (all four), the refreeze cotangent with the wrong sign
    (all four), gice added after the row instead of before (all four), the mid quotient missing from gta (gta alone).
    Measured: worst error / bound = 0.0147 (gp), 0.0171 (gta), 0.00546 (gpar), 0.0224 (gstate), with m = 54 (gstate), 62 (gp),
    61 (gta), 172 (gpar; n_ice = 92.9); the nearest switch is a relative 0.0030 away; the wrong adjoints miss by 1e12 - 1e14
    bounds on every output they reach (profiles/r16/error_bound.txt)."""
    p, ta, gw, gi, gl, par, state, dt = derivative["data"]
    rows = derivative["rows"]
    assert all(rows[k] > 0 for k in SH.REGIMES), rows
    assert rows["mid"] >= 7 and rows["melt_limited"] >= 3 and rows["refreeze_limited"] >= 3 and float(p.min()) > 0
    _, ice, liq, _ = SH.snow_ref(p, ta, par, dt, state)
    got, = SH.run([("grad", gw, gi, gl, p, ta, ice, liq, par, dt, state, True, True, True)])
    assert all(SH.same_bits(a, b) for a, b in zip(got, SH.snow_grad_ref(gw, gi, gl, p, ta, ice, liq, par, dt, state)))
    rt = _ratios(derivative, got)
    print("snow adjoint vs mpmath derivative: worst error / bound = %s; m = %r; %r; rows per regime %r"
          % (", ".join("%.3g (%s)" % (rt[k].max(), k) for k in OUTPUTS), derivative["m"], derivative["cond"], rows))
    assert all(v.max() <= 1.0 for v in rt.values()), {k: v.max() for k, v in rt.items()}
    assert all(v.max() > 0 for v in rt.values())  # (the data are general: something does round)
    for variant, reached in (("no_dcap", OUTPUTS), ("refr_sign", OUTPUTS), ("gice_late", OUTPUTS), ("no_mid", ("gta",))):
        wrong = _ratios(derivative, SH.snow_grad_ref(gw, gi, gl, p, ta, ice, liq, par, dt, state, variant=variant))
        print("  wrong adjoint %-9s: worst error / bound = %s" % (variant, ", ".join("%.3g (%s)" % (wrong[k].max(), k) for k in OUTPUTS)))
        assert all(wrong[k].max() > 1.0 for k in reached), (variant, {k: v.max() for k, v in wrong.items()})
        assert all(wrong[k].max() <= 1.0 for k in wrong if k not in reached), variant


# ---- 4. behaviour -------------------------------------------------------------------------------------------------------------
def test_chunked_repeated_and_permuted_calls_give_the_same_bits():
    """One call against calls cut at 1 row, at T - 1 rows and in the middle (carry=True keeps the [2, B] pack per key), from no pack
    and from a given state; a repeated call; reset(); a permutation of the cells gives the permuted bits."""
    rng = np.random.default_rng(23)
    T, B = 17, 65
    p, ta, gw, gi, gl, par, state, dt = SH.case_data(rng, T, B)  # (its parameters are ones the Python layer takes)
    store = SimCatchmentSnow(*par, dt)
    tp, tt = _t(p), _t(ta)
    for st in (None, state):
        want = SH.snow_ref(p, ta, par, dt, st)
        ts = None if st is None else _t(st)
        w, ice, liq = store.run(tp, tt, carry=False, state=ts, pack=True)
        assert all(SH.same_bits(a.numpy(), b) for a, b in zip((w, ice, liq), want))
        assert SH.same_bits(store.run(tp, tt, carry=False, state=ts).numpy(), want[0]) and store.state_of() is None
        for cut in (1, T - 1, T // 2):
            key = ("cut", cut, st is None)
            a = store.run(tp[:cut], tt[:cut], key=key, state=ts, pack=True)
            b = store.run(tp[cut:], tt[cut:], key=key, pack=True)
            assert all(SH.same_bits(torch.cat([x, y]).numpy(), z) for x, y, z in zip(a, b, want)), cut
            assert SH.same_bits(store.state_of(key).numpy(), want[3])
            assert tuple(store.run(tp[:0], tt[:0], key=key).shape) == (0, B) and SH.same_bits(store.state_of(key).numpy(), want[3])  # T = 0
    assert store.state_of("nobody") is None
    store.reset()
    assert store.state_of(("cut", 1, True)) is None
    perm = rng.permutation(B)
    w, ice, liq, so = SH.snow_ref(p, ta, par, dt, state)
    got, = SH.run([("fwd", p[:, perm], ta[:, perm], par[:, perm], dt, state[:, perm], True, True)])
    assert all(SH.same_bits(a, b[:, perm]) for a, b in zip(got, (w, ice, liq, so)))
    want = SH.snow_grad_ref(gw, gi, gl, p, ta, ice, liq, par, dt, state)
    got, = SH.run([("grad", gw[:, perm], gi[:, perm], gl[:, perm], p[:, perm], ta[:, perm], ice[:, perm], liq[:, perm], par[:, perm], dt,
                    state[:, perm], True, True, True)])
    assert all(SH.same_bits(a, b[:, perm]) for a, b in zip(got, want))


@pytest.mark.parametrize("which", ["p", "ta"])
def test_a_nan_stays_in_its_cell_from_its_row_on(which):
    """A NaN in p[t][b] or ta[t][b] is in ice and liq of cell b from row t on and in state_out, and in no other cell: every other
    cell has the clean run's bits.  (w of cell b from that row on is what the selects give a NaN: `over` is false, and its last
    alternative is the constant 0.0 -- the pack, not w, carries the NaN; the rows before it have the clean bits.)"""
    rng = np.random.default_rng(41)
    T, B = 9, 65
    p, ta, _, _, _, par, state, dt = SH.case_data(rng, T, B)
    clean = SH.snow_ref(p, ta, par, dt, state)
    t0, b = 4, 17
    (p if which == "p" else ta)[t0, b] = np.nan
    got, = SH.run([("fwd", p, ta, par, dt, state, True, True)])
    assert all(SH.same_bits(a, r) for a, r in zip(got, SH.snow_ref(p, ta, par, dt, state)))
    hit = np.zeros((T, B), dtype=bool)
    hit[t0:, b] = True
    for have, was in zip(got[1:3], clean[1:3]):
        assert (np.isnan(have) == hit).all() and SH.same_bits(have[~hit], was[~hit])
    assert SH.same_bits(got[0][~hit], clean[0][~hit]) and not got[0][hit].any() and not np.signbit(got[0][hit]).any()
    assert np.isnan(got[3][:, b]).all() and np.isnan(got[3]).sum() == 2


def test_autograd_through_the_host_build(derivative):
    """catchment_snow on the host build (SimCatchmentSnow.function) on the data of the derivative test: precip, temp, the seven
    parameters and the initial pack receive the bits of snow_grad_ref.  Scalar parameters receive the sum over the cells; without
    return_pack no gice / gliq is passed; a temp or a state that requires no gradient gets none."""
    p, ta, gw, gi, gl, par, state, dt = derivative["data"]
    leaf = lambda a: _t(a).clone().requires_grad_(True)
    tp, tt, ts = leaf(p), leaf(ta), leaf(state)
    tpar = [leaf(par[k]) for k in range(7)]
    w, ice, liq = SimCatchmentSnow.function(tp, tt, *tpar, dt, state=ts, return_pack=True)
    ref = SH.snow_ref(p, ta, par, dt, state)
    assert all(SH.same_bits(a.detach().numpy(), b) for a, b in zip((w, ice, liq), ref))
    ((w * _t(gw)).sum() + (ice * _t(gi)).sum() + (liq * _t(gl)).sum()).backward()
    g_ref = SH.snow_grad_ref(gw, gi, gl, p, ta, ref[1], ref[2], par, dt, state)
    mine = (tp.grad.numpy(), tt.grad.numpy(), np.stack([v.grad.numpy() for v in tpar]), ts.grad.numpy())
    assert all(SH.same_bits(a, b) for a, b in zip(mine, g_ref))
    assert all(float(np.abs(g_ref[2][k]).max()) > 0 for k in range(7)) and float(np.abs(g_ref[3]).min()) > 0
    # without the pack: no gice / gliq; scalar parameters: summed gradients; a constant temp and state
    scal = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (-1.0, 2.0, 0.3, 1.1, 0.15, 0.05, 0.1)]
    tp2 = leaf(p)
    w2 = SimCatchmentSnow.function(tp2, _t(ta), *scal, dt, state=_t(state))
    (w2 * _t(gw)).sum().backward()
    par2 = np.stack([np.full(7, float(v.detach())) for v in scal])
    ref2 = SH.snow_ref(p, ta, par2, dt, state)
    g2 = SH.snow_grad_ref(gw, None, None, p, ta, ref2[1], ref2[2], par2, dt, state)
    assert SH.same_bits(w2.detach().numpy(), ref2[0]) and SH.same_bits(tp2.grad.numpy(), g2[0])
    for k, v in enumerate(scal):
        assert SH.same_bits(v.grad.numpy().reshape(1), _t(g2[2][k]).sum().numpy().reshape(1)), k
    assert float(np.abs(g2[2]).sum(axis=1).min()) > 0
    # temp alone
    tt3 = leaf(ta)
    w3, i3, l3 = SimCatchmentSnow.function(_t(p), tt3, *[_t(par[k]) for k in range(7)], dt, return_pack=True)
    ref3 = SH.snow_ref(p, ta, par, dt)
    ((i3 + l3) * _t(gi)).sum().backward()
    g3 = SH.snow_grad_ref(np.zeros_like(gw), gi, gi, p, ta, ref3[1], ref3[2], par, dt)
    assert SH.same_bits(tt3.grad.numpy(), g3[1])
    with torch.no_grad():
        assert SH.same_bits(SimCatchmentSnow.function(_t(p), _t(ta), *[_t(par[k]) for k in range(7)], dt).numpy(), ref3[0])


def test_construction_and_rejections():
    import lgar_py_amd as lg
    from lgar_py_amd import LgarError, _capi
    from lgar_py_amd.snow import CatchmentSnow, catchment_snow
    assert lg.CatchmentSnow is CatchmentSnow and lg.catchment_snow is catchment_snow
    assert {"CatchmentSnow", "catchment_snow"} <= set(lg.__all__)
    assert _capi.ABI_VERSION == 4
    assert {"lgar_catchment_snow", "lgar_catchment_snow_grad"} <= set(_capi.EXPORTS)
    make = lambda *a, **kw: CatchmentSnow(*a, device="cpu", **kw)
    ok = [[-1.0, -0.5, 0.0], torch.tensor([1.0, 2.0, 0.0], dtype=torch.float64), np.array([0.0, 0.5, -0.2]), 1.0, [0.1, 0.2, 0.0], 0.05, 0.1]
    st = make(*ok, 1.0)
    assert st.B == 3 and tuple(st.par.shape) == (7, 3) and st.par.dtype == torch.float64 and st.par[1].tolist() == [1.0, 2.0, 0.0]
    assert st.par[3].tolist() == [1.0] * 3 and st.dt_h == 1.0
    assert make(-1.0, 1.0, 0.0, 1.0, 0.1, 0.05, 0.1, 0.5, n_catchments=4).par.tolist() == [[v] * 4 for v in (-1.0, 1.0, 0.0, 1.0, 0.1, 0.05, 0.1)]
    assert make([], [], [], [], [], [], [], 1.0).B == 0

    def but(k, v, dt=1.0, **kw):
        args = list(ok)
        args[k] = v
        return lambda: make(*args, dt, **kw)

    for call, word in ((but(0, [-1.0, 0.0]), "agree"), (lambda: make(-1.0, 1.0, 0.0, 1.0, 0.1, 0.05, 0.1, 1.0), "agree"), (but(0, -1.0, n_catchments=4), "agree"),
                       (but(0, [[-1.0]]), r"\[B\]"), (but(0, [2.0, -0.5, 0.0]), "tlo <= thi"), (but(0, [-1.0, -0.5, 1e-9]), "tlo <= thi"),
                       (but(3, -1.0), "sfcf"), (but(4, [0.1, -0.2, 0.0]), "cfmax"), (but(5, -0.05), "cfr"), (but(6, -0.1), "cwh"),
                       (but(0, [np.nan, -0.5, 0.0]), "finite"), (but(1, [np.inf, 2.0, 0.0]), "finite"), (but(2, [0.0, np.nan, 0.0]), "finite"),
                       (but(6, np.inf), "finite"), (but(0, ok[0], dt=0.0), "dt_h"), (but(0, ok[0], dt=np.nan), "dt_h"), (but(0, ok[0], dt=-1.0), "dt_h"),
                       (but(0, ok[0], dt="hour"), "dt_h"), (but(0, torch.tensor([-1.0, -0.5, 0.0])), "fp64"), (but(2, ["a", 0.0, 0.0]), "numbers")):
        with pytest.raises(LgarError, match=word):
            call()
    # calls: shapes, dtypes, devices
    sim = SimCatchmentSnow(*ok, 1.0)
    x, y = torch.ones(4, 3, dtype=torch.float64), torch.zeros(4, 3, dtype=torch.float64)
    assert tuple(sim.run(x, y).shape) == (4, 3) and tuple(sim.state_of().shape) == (2, 3)
    assert all(tuple(a.shape) == (4, 3) for a in sim.run(x, y, pack=True))
    for args in ((x[:, :2], y), (x.float(), y), (x.numpy(), y), (x.to("meta"), y), (x[0], y), (x, y[:3]), (x, y.float()), (x, y[:, :2]),
                 (x, y, True, None, x), (x, y, True, None, x[:2].float()), (x, y, True, None, x[0])):
        with pytest.raises(LgarError, match=r"3\] tensor"):
            sim.run(*args)
    q = [torch.ones(3, dtype=torch.float64) for _ in range(7)]
    f = SimCatchmentSnow.function
    for call in (lambda: f(x.float(), y, *q, 1.0), lambda: f(x, y[:3], *q, 1.0), lambda: f(x, y.float(), *q, 1.0), lambda: f(x, y, q[0][:2], *q[1:], 1.0),
                 lambda: f(x, y, q[0].float(), *q[1:], 1.0), lambda: f(x, y, "a", *q[1:], 1.0), lambda: f(x, y, *q, 0.0), lambda: f(x, y, *q, 1.0, state=x),
                 lambda: f(x, y, *q[:6], q[6].to("meta"), 1.0), lambda: f(x[0], y[0], *q, 1.0)):
        with pytest.raises(LgarError):
            call()
    # a store on the CPU holds the host logic only: the kernels have no CPU fallback
    cpu = make(*ok, 1.0)
    for call in (lambda: cpu.run(x, y), lambda: cpu.run(x, y, carry=False, pack=True), lambda: catchment_snow(x, y, *q, 1.0)):
        with pytest.raises(LgarError, match="no CPU fallback"):
            call()
    # the docstrings say what the store does not do
    for doc in (lg.snow.__doc__, catchment_snow.__doc__):
        assert "PET under snow" in doc and "(ice + liq) == 0" in doc and "does not exist yet" in " ".join(doc.split())


def test_entry_points_refuse_bad_arguments():
    """The refusals of the C-ABI wrappers (lgar_snow.hpp's own checks, which the host launchers call as the library does):
    LGAR_E_ARG = -1 for negative sizes, a dt_h that is not finite or <= 0, a null pointer the sizes say will be read or written,
    exactly one of ice / liq, the adjoint without ice / liq with T > 0."""
    lib = SH.library()
    buf = np.ones(512)
    a = buf.ctypes.data
    T, B = 2, 4
    fwd = (("p", a), ("ta", a), ("T", T), ("B", B), ("par", a), ("dt", 1.0), ("state_in", None), ("state_out", a + 512), ("w", a + 1024),
           ("ice", a + 1536), ("liq", a + 2048))
    run = lambda **kw: lib.snowhost_catchment_snow(*[kw.get(k, d) for k, d in fwd])
    assert run() == 0
    for bad in (dict(T=-1), dict(B=-1), dict(p=None), dict(ta=None), dict(par=None), dict(w=None), dict(ice=None), dict(liq=None), dict(dt=0.0),
                dict(dt=-1.0), dict(dt=float("nan")), dict(dt=float("inf")), dict(B=0, dt=0.0), dict(B=0, ice=None), dict(T=0, liq=None)):
        assert run(**bad) == -1, bad
    assert run(ice=None, liq=None) == 0 and run(state_out=None) == 0 and run(state_in=a) == 0
    assert run(B=0, p=None, ta=None, par=None, w=None) == 0 and run(T=0, p=None, ta=None, par=None, w=None) == 0
    assert run(T=0, p=None, ta=None, w=None, state_out=None) == 0
    buf[64:72] = 7.0
    assert run(T=0, p=None, ta=None, par=None, w=None, ice=None, liq=None) == 0 and buf[64:72].tolist() == [0.0] * 8  # T = 0, no state_in: zeros
    grd = (("gw", a), ("gice", a), ("gliq", a), ("p", a), ("ta", a), ("ice", a), ("liq", a), ("T", T), ("B", B), ("par", a), ("dt", 1.0),
           ("state_in", None), ("gp", a + 512), ("gta", a + 1024), ("gpar", a + 1536), ("gstate", a + 2048))
    grad = lambda **kw: lib.snowhost_catchment_snow_grad(*[kw.get(k, d) for k, d in grd])
    assert grad() == 0
    for bad in (dict(T=-1), dict(B=-1), dict(gw=None), dict(p=None), dict(ta=None), dict(ice=None), dict(liq=None), dict(ice=None, liq=None),
                dict(par=None), dict(gp=None), dict(dt=0.0), dict(dt=float("nan")), dict(dt=float("-inf")), dict(ice=None, liq=None, gpar=None, gstate=None),
                dict(T=0, ice=None), dict(B=0, liq=None)):
        assert grad(**bad) == -1, bad
    assert grad(gice=None, gliq=None) == 0 and grad(gice=None) == 0 and grad(gta=None) == 0 and grad(gpar=None) == 0 and grad(gstate=None) == 0
    assert grad(gta=None, gpar=None, gstate=None) == 0
    assert grad(B=0, gw=None, p=None, ta=None, ice=None, liq=None, par=None, gp=None) == 0
    buf[192:220] = 7.0
    buf[256:264] = 7.0
    assert grad(T=0, gw=None, gice=None, gliq=None, p=None, ta=None, ice=None, liq=None, par=None, gp=None, gta=None) == 0
    assert buf[192:220].tolist() == [0.0] * 28 and buf[256:264].tolist() == [0.0] * 8  # T = 0: gpar and gstate are zeros
    assert grad(T=0, gpar=None, gstate=None, gw=None, ice=None, liq=None) == 0
