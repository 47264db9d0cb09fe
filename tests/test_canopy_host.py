"""CPU: the catchment canopy (lgar_catchment_canopy / _grad / _tangent, include/lgar.h).

The per-cell walks the GPU kernels run (lgar_py_amd/csrc/lgar_canopy.hpp) are compiled for the host into a small stand-alone
program and a shared library (tests/canopy_host).  Both are held BIT FOR BIT to the numpy statement of the definition
(canopy_host.canopy_ref / canopy_grad_ref / canopy_tangent_ref); the same program built with AddressSanitizer + UBSan runs the
program's cases.  Independently of the statement the definition is held to statements that do not come from it: bare ground, a
store that never fills, the water balance as an exact sum, the energy bound, the adjoint against derivatives of the
real-arithmetic statement taken in mpmath, and the tangent against the adjoint through the transposition identity.  The same
header as a shared library stands behind lgar_py_amd.canopy.CatchmentCanopy (canopy_host.SimCatchmentCanopy), so the host logic
of canopy.py -- validation, carry, autograd, directions -- and the new upstream= of catchment_snow_directions run here too."""
from fractions import Fraction

import mpmath
import numpy as np
import pytest
import torch

import canopy_host as CH
import snow_host as SH
import snow_tangent_host as ST
from canopy_host import SimCatchmentCanopy

U = 2.0 ** -53  # unit roundoff of fp64
PROGRAM_TANGENT_EVERY = 32  # the stand-alone program runs every 32nd tangent case of the grid (the library runs all of them)


def gamma(m):
    """Higham's gamma_m = m u / (1 - m u): (1 + d_1) .. (1 + d_m) = 1 + theta, |theta| <= gamma_m, for |d_i| <= u (3.1)."""
    return m * U / (1.0 - m * U)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


F = lambda v: Fraction(float(v))
_fr = lambda a: [Fraction(float(v)) for v in np.asarray(a).ravel()]
dot = lambda a, b: sum(x * y for x, y in zip(_fr(a), _fr(b)))


# ---- 1. the host build against the numpy definition ------------------------------------------------------------------------
@pytest.mark.parametrize("B", CH.SHAPE_B)
def test_host_library_equals_the_numpy_statement_bit_for_bit(B):
    """canopy_host.grid(B) in full through the host library: T in {0, 1, 9, 17} x state present / NULL x lai present / NULL, and at
    each of these points every combination of optional inputs and wanted outputs of the forward (4), the adjoint (32) and the
    tangent (256; D in {1, 3} and two (ld, k0) rotating): 4672 calls.  The elements of dw / dpet outside k0 .. k0 + D keep what
    they held; T = 0 copies the state.  At every B that holds cells of all kinds every regime is counted > 0, and where cells
    16 .. 18 exist the three ties."""
    n = 0
    for case, want in CH.grid(B):
        CH.check(case, want, CH.host_call(case))
        n += 1
        if case[0] == "fwd" and np.asarray(case[1]).shape[0] == 0 and want[4] is not None:  # T = 0 copies the state, or writes zeros
            assert CH.same_bits(want[4], np.zeros((1, B)) if case[6] is None else np.asarray(case[6]))
        if case[0] == "tan" and np.asarray(case[1]).shape[0] == 0 and want[4] is not None:
            assert CH.same_bits(want[4], np.zeros((case[7], B)) if case[12] is None else np.asarray(case[12]))
    assert n == 16 * (4 + 32 + 256)
    rows, ties = CH.grid_counts(B)
    print("B = %d: rows per regime %r, rows per exact tie %r" % (B, rows, ties))
    if B >= 63:
        assert set(rows) == set(CH.REGIMES) and all(v > 0 for v in rows.values()), rows
        assert set(ties) == set(CH.TIES) and all(v > 0 for v in ties.values()), ties


def test_the_stated_draw_reaches_all_six_regimes():
    """cmax in [0, 0.2], fe in [0, 2.5], cover in [0, 1], lai in [0.5, 4.5], half the rows dry, dt_h = 1/4, T = 17, B = 65."""
    p, e, lai, par, state, dt = CH.case_data(np.random.default_rng(0), 17, 65, dt=0.25)
    rows = CH.regimes(p, e, lai, par, dt, state)[0]
    print("rows per regime:", rows)
    assert all(rows[k] > 0 for k in CH.REGIMES), rows
    assert float(par[0].max()) <= 0.2 and float(par[1].max()) <= 2.5 and 0.0 <= float(par[2].min()) and float(par[2].max()) <= 1.0
    assert 0.5 <= float(lai.min()) and float(lai.max()) <= 4.5 and 0.35 < float((p == 0).mean()) < 0.65


def _program_cases():
    cases, refs = [], []
    for B in CH.SHAPE_B:
        for case, want in CH.grid(B, tangent_every=PROGRAM_TANGENT_EVERY):
            cases.append(case)
            refs.append(want)
    return cases, refs


@pytest.fixture(scope="module")
def program_cases():
    return _program_cases()


def test_host_program_equals_the_numpy_statement_bit_for_bit(program_cases):
    """The stand-alone program over every forward and adjoint case of the grid at every B and every 32nd tangent case (the
    phase rotates, so each of the 256 tangent combinations is run): ONE run, under the host-program protocol."""
    cases, refs = program_cases
    kinds = [c[0] for c in cases]
    assert kinds.count("fwd") == 6 * 16 * 4 and kinds.count("grad") == 6 * 16 * 32 and kinds.count("tan") == 6 * 16 * 256 // PROGRAM_TANGENT_EVERY
    combos = {(tuple(a is not None for a in c[8:13]), c[15:18]) for c in cases if c[0] == "tan"}
    assert len(combos) == 256
    for case, want, got in zip(cases, refs, CH.run(cases)):
        CH.check(case, want, got)


def test_sanitizer_build_on_the_same_cases(program_cases):
    """AddressSanitizer + UBSan build of the same program (a stand-alone executable: nothing is loaded into python; every array is
    allocated at its exact size) over the program's cases: clean, with the same bits.  Any finding aborts the program."""
    cases, refs = program_cases
    for case, want, got in zip(cases, refs, CH.run(cases, sanitize=True)):
        CH.check(case, want, got)


def test_the_planted_ties_sit_where_they_were_planted_and_go_where_the_selects_send_them():
    """case_data plants, in row 0 of cells 16 .. 18 with the state given, s1 == cap (holds: no drip), dem == s2 (demand-limited:
    ei = dem, the store is left at +0.0) and ei == ed (a residual: r = +0.0) -- with and without leaf area, for every dt_h."""
    for dt_h in (0.25, 1.0, 24.0, 0.1):
        p, e, lai, par, state, dt = CH.case_data(np.random.default_rng(5), 9, 65, dt=dt_h)
        for la in (lai, None):
            _, _, reg, tie, _ = CH.regimes(p, e, la, par, dt, state)
            for name, went in (("s1==cap", "hold"), ("dem==s2", "free"), ("ei==ed", "pos")):
                assert tie[name][0, CH.TIE_CELLS[name]] and reg[went][0, CH.TIE_CELLS[name]], (name, dt)
            (w, pet, st, ev, _), = [CH.host_call(("fwd", p, e, la, par, dt, state, True, False))]
            assert w[0, 16] == 0.0 and st[0, 17] == 0.0 and pet[0, 18] == 0.0 and not np.signbit(pet[0, 18])
            assert ev[0, 17] * dt == pytest.approx(0.5 * e[0, 17] * dt, rel=1e-15) and ev[0, 18] == pytest.approx(e[0, 18], rel=1e-15)


@pytest.mark.parametrize("which", ["p", "e", "lai", "state"])
def test_a_nan_stays_in_its_cell(which):
    CH.nan_confinement(CH.host_call, which)


# ---- 2. independent of the statement ----------------------------------------------------------------------------------------
def test_bare_ground():
    """cover = 0, a zero state, dt_h a power of two: hit = 0 pd = 0, direct = pd, nothing is ever held or evaporated: w has p's
    bits and pet_out has e's bits (p, e >= 0), whatever cmax, fe and lai are."""
    rng = np.random.default_rng(2)
    T, B = 17, 65
    _, _, lai, par, _, _ = CH.case_data(rng, T, B)
    par[CH.COVER] = 0.0
    p = rng.random((T, B)) * 10.0 ** rng.integers(-6, 3, (T, B)) * (rng.random((T, B)) < 0.7)
    e = rng.random((T, B)) * 10.0 ** rng.integers(-6, 1, (T, B)) * (rng.random((T, B)) < 0.9)
    assert (p == 0).sum() > 50 and (p > 0).sum() > 500 and (e == 0).sum() > 20
    for dt in (1.0, 0.25, 32.0, 2.0 ** -7):
        for st, la in ((None, lai), (np.zeros((1, B)), lai), (None, None)):
            w, pet, store, evap, so = CH.host_call(("fwd", p, e, la, par, dt, st, True, True))
            assert CH.same_bits(w, p) and CH.same_bits(pet, e)
            assert not store.any() and not evap.any() and not so.any()


def test_never_full_and_no_evaporation():
    """fe = 0 and a huge cmax: the store is the running sum of cover * pd, written here as a cumulative sum, and w is direct / dt_h;
    nothing evaporates and pet_out is e."""
    rng = np.random.default_rng(6)
    T, B = 17, 65
    p, e, lai, par, state, dt = CH.case_data(rng, T, B)
    p, par[CH.FE], par[CH.CMAX], state = np.abs(p), 0.0, 1e30, np.abs(state)
    w, pet, store, evap, _ = CH.host_call(("fwd", p, e, lai, par, dt, state, True, False))
    pd = p * dt
    hit = par[CH.COVER][None, :] * pd
    run = state[0].copy()
    for t in range(T):
        run = run + hit[t]
        assert np.array_equal(store[t], run), t
    assert np.array_equal(w, (pd - hit) / dt) and not evap.any()
    assert np.array_equal(pet, (e * dt) / dt) and float(store[-1].max()) > 1.0


def test_water_balance_closes_per_cell():
    """sum pd = sum w dt_h + sum evap dt_h + s_end - s_0 per cell over 17 rows, the difference taken exactly (fractions.Fraction of
    the floats), within gamma_8 sum_t S_t.  In real arithmetic a row is pd = direct + hit, s1 = s + hit, s1 = drip + s2,
    s2 = ei + s': pd = (direct + drip) + ei + (s' - s), exactly.  hit and ei enter both sides of their two equations with one and
    the same float, so their own rounding does not disturb the balance.  The roundings that do, per row: pd = p dt_h, direct =
    pd - hit, s1 = s + hit, drip = s1 - cap, s' = s2 - ei, direct + drip, that sum / dt_h and ei / dt_h: m = 8, each relative to
    a value of the row that is at most S_t = |pd| + |direct| + |s1| + |drip| + |s'| + |direct + drip| + |ei|, the row on
    absolute values.
    Measured: worst |miss| 9.68e-16, worst miss / bound 0.027."""
    rng = np.random.default_rng(4)
    T, B = 17, 257
    p, e, lai, par, state, dt = CH.case_data(rng, T, B)
    w, pet, store, evap, so = CH.host_call(("fwd", p, e, lai, par, dt, state, True, True))
    worst, worst_abs = 0.0, 0.0
    for b in range(B):
        s, S = float(state[0, b]), Fraction(0)
        for t in range(T):
            pd = p[t, b] * dt
            hit = par[CH.COVER, b] * pd
            direct, s1 = pd - hit, s + hit
            tf, ei = w[t, b] * dt, evap[t, b] * dt  # (to the last bit or so: they only size the bound)
            drip = tf - direct
            S += sum(abs(F(v)) for v in (pd, direct, s1, drip, store[t, b], tf, ei))
            s = float(store[t, b])
        miss = abs(F(dt) * sum(F(v) for v in p[:, b]) - F(dt) * sum(F(v) for v in w[:, b]) - F(dt) * sum(F(v) for v in evap[:, b])
                   - F(so[0, b]) + F(state[0, b]))
        bar = Fraction(gamma(8)) * S
        assert miss <= bar, (b, float(miss), float(bar))
        if bar:
            worst, worst_abs = max(worst, float(miss / bar)), max(worst_abs, float(miss))
    print("canopy water balance: worst |miss| %.3g, worst miss / bound %.3g (gamma_8 sum S_t), %d cells x %d rows" % (worst_abs, worst, B, T))
    assert 0.0 < worst <= 1.0 and float(evap.sum()) > 0 and float(w.sum()) > 0


def test_energy():
    """pet_out >= 0 always, and pet_out + evap <= e wherever fe <= 1 (then fc = fe cover <= 1 and ei <= dem <= ed: the canopy
    cannot spend more than there is).  The second is held on the depths the walk forms, exactly: with ed = e dt_h as the walk
    rounds it, r = fl(ed - ei) and ei <= ed, so r + ei <= ed (1 + u); pet_out = fl(r / dt_h) and evap = fl(ei / dt_h) add a
    rounding each: (pet_out + evap) dt_h <= ed (1 + gamma_3), the sum and the products taken in Fraction."""
    rng = np.random.default_rng(8)
    T, B = 17, 257
    p, e, lai, par, state, dt = CH.case_data(rng, T, B)
    w, pet, store, evap, _ = CH.host_call(("fwd", np.abs(p), e, lai, par, dt, np.abs(state), True, False))
    assert float(pet.min()) >= 0.0 and float(evap.min()) >= 0.0
    cells = np.nonzero(par[CH.FE] <= 1.0)[0]
    assert cells.size > 50 and (par[CH.FE] > 1.0).sum() > 50
    slack = Fraction(1) + Fraction(gamma(3))
    for b in cells:
        for t in range(T):
            assert (F(pet[t, b]) + F(evap[t, b])) * F(dt) <= F(e[t, b] * dt) * slack, (t, b)
    over = (pet + evap > e * (1.0 + 1e-12))
    assert over.any() and not over[:, cells].any()  # (fc > 1 does spend more: the residual is cut at zero)


# ---- 3. the adjoint is the true derivative, the tangent its transpose ---------------------------------------------------------
def _derivative_data():
    """B = 6, T = 9, dt_h = 1/4, p > 0 and lai given: an ordinary canopy (0), a small capacity that spills in most rows (1), a
    large one that never spills (2), fc > 1 (3: rows with no residual), a weak evaporation that never empties the store (4), a
    sparse cover (5).  Values are jittered, so no row sits at a switch (asserted by the test)."""
    rng = np.random.default_rng(77)
    T, B = 9, 6
    jit = lambda: 1.0 + 0.05 * rng.random(B)
    cmax = np.array([0.12, 0.02, 5.0, 0.15, 0.2, 0.1]) * jit()
    fe = np.array([0.9, 1.0, 0.8, 2.4, 0.05, 1.2]) * jit()
    cover = np.array([0.7, 0.8, 0.6, 0.9, 0.75, 0.15]) * jit()
    lai = 0.5 + 4.0 * rng.random((T, B))
    p = (0.05 + 1.5 * rng.random((T, B))) * (1.0 + 3.0 * (rng.random((T, B)) < 0.4))
    e = 0.05 + 0.6 * rng.random((T, B))
    state = (np.array([0.1, 0.01, 0.5, 0.2, 0.3, 0.05]) * jit())[None, :]
    g = tuple((rng.random((T, B)) - 0.4) * 2.0 for _ in range(4))
    return p, e, lai, np.stack([cmax, fe, cover]), state, 0.25, g


def _mp_cell(p, e, lai, par, s, dt, g):
    """One cell of the definition in REAL arithmetic (mpmath at the working precision): the loss
    sum gw w + gpet pet_out + gstore store + gevap evap."""
    cmax, fe, cover = par
    fc = fe * cover
    loss, Z = mpmath.mpf(0), mpmath.mpf(0)
    for t in range(len(p)):
        pd, ed = p[t] * dt, e[t] * dt
        hit = cover * pd
        direct, cap, s1 = pd - hit, cmax * lai[t], s + hit
        full = s1 > cap
        drip, s2 = (s1 - cap, cap) if full else (Z, s1)
        dem = fc * ed
        ei = s2 if dem > s2 else dem
        s = s2 - ei
        r = Z if ei > ed else ed - ei
        loss += g[0][t] * ((direct + drip) / dt) + g[1][t] * (r / dt) + g[2][t] * s + g[3][t] * (ei / dt)
    return loss


OUTPUTS = ("gp", "ge", "glai", "gpar", "gstate")


def test_the_adjoint_is_the_true_derivative():
    """gp, ge, glai, gpar and gstate of the host build against the derivatives of L = sum gw w + gpet pet_out + gstore store +
    gevap evap of the definition's REAL-arithmetic statement, taken in mpmath at 60 digits by central differences with
    h = 1e-20 |x| (between switches L is a polynomial in every variable: the quotient misses the derivative by h^2 L''' / 6 ~ 1e-40;
    no row lies within a relative 1e-6 of a switch -- asserted on the float walk, whose values are within 1e-14 of the real
    walk's, so both take the same branches).  B = 6, T = 9; every regime occurs (asserted).

    The bound is gamma_m x (the same adjoint on absolute values, every difference a sum: canopy_grad_ref(absolute=True)), with m
    counted from the recurrence.  No forward STATE enters a term: store[t - 1] only decides the flags; the forward factors are
    pd and ed (one rounding each), fc (one), lai, cmax, cover, fe (inputs).  The adjoint of the store passes a row through
    ls + gstore (1), (gei - dr) - ls (2) and ls + dei (3): 3 T over the rows, and a cotangent enters with 2 (its division by dt_h
    and gei - dr).  On top: gp adds ds1 - gtf, dhit cover, gtf + ., . dt_h (4); ge adds fc's own rounding, ddem fc, dr + ., . dt_h
    (4); glai adds ds2 - gtf and dcap cmax (2); a parameter term adds its forward factor's rounding and the product (2), at most T
    additions into its accumulator, and gfc cover, gfc fe, gcover + . after row 0 (3).  m = 3 T + 2 + 2 + T + 3 = 4 T + 7 covers
    every output.
    Measured: worst error / bound = 0.00853 (gp), 0.0188 (ge), 0.0244 (glai), 0.0101 (gpar), 0.00926 (gstate), m = 43; the nearest
    switch is a relative 0.0056 away."""
    mpmath.mp.dps = 60
    p, e, lai, par, state, dt, g = _derivative_data()
    T, B = p.shape
    rows, _, _, _, margin = CH.regimes(p, e, lai, par, dt, state)
    assert all(rows[k] > 0 for k in CH.REGIMES) and margin > 1e-6, (rows, margin)
    _, _, store, _, _ = CH.canopy_ref(p, e, lai, par, dt, state)
    case = ("grad", *g, p, e, lai, store, par, dt, state, True, True, True)
    got = CH.host_call(case)
    CH.check(case, CH.reference(case), got)
    mag = CH.canopy_grad_ref(*g, p, e, lai, store, par, dt, state, absolute=True)
    M = mpmath.mpf
    h = M(10) ** -20
    m = 4 * T + 7
    worst = dict.fromkeys(OUTPUTS, 0.0)
    for b in range(B):
        x = ([M(float(v)) for v in p[:, b]] + [M(float(v)) for v in e[:, b]] + [M(float(v)) for v in lai[:, b]]
             + [M(float(par[k, b])) for k in range(3)] + [M(float(state[0, b]))])
        gb = [[M(float(v)) for v in a[:, b]] for a in g]
        cell = lambda v: _mp_cell(v[:T], v[T:2 * T], v[2 * T:3 * T], v[3 * T:3 * T + 3], v[3 * T + 3], M(dt), gb)
        for i in range(3 * T + 4):
            xp, xm = list(x), list(x)
            hi = h * abs(x[i])
            assert hi > 0
            xp[i], xm[i] = x[i] + hi, x[i] - hi
            want = (cell(xp) - cell(xm)) / (2 * hi)
            k, j = (i // T, i % T) if i < 3 * T else ((3, i - 3 * T) if i < 3 * T + 3 else (4, 0))
            err, bar = abs(M(float(got[k][j, b])) - want), M(gamma(m)) * M(float(mag[k][j, b]))
            assert err <= bar, (OUTPUTS[k], j, b, float(err), float(bar))
            if bar:
                worst[OUTPUTS[k]] = max(worst[OUTPUTS[k]], float(err / bar))
    print("canopy adjoint vs mpmath derivative: worst error / bound = %s; m = %d; nearest switch %.3g; rows %r"
          % (", ".join("%.3g (%s)" % (worst[k], k) for k in OUTPUTS), m, margin, rows))
    assert all(v > 0 for v in worst.values())  # (the data are general: something does round)


def _identity(g, dirs, adj, tan, D):
    """Both sides of <gw, dw> + <gpet, dpet> + <gstore, dstore> + <gevap, devap> = <gp, dp> + <ge, de> + <glai, dlai> + <gpar, dpar>
    + <gstate, dstate> per direction, exactly (fractions.Fraction of the floats)."""
    gw, gpet, gstore, gevap = g
    dp, de, dlai, dpar, dst = dirs
    gp, ge, glai, gpar, gstate = adj
    dw, dpet, dstore, devap = tan[:4]
    return [(dot(gw, dw[:, :, k]) + dot(gpet, dpet[:, :, k]) + dot(gstore, dstore[k]) + dot(gevap, devap[k]),
             dot(gp, dp[k]) + dot(ge, de[k]) + dot(glai, dlai[k]) + dot(gpar, dpar[k]) + dot(gstate[0], dst[k])) for k in range(D)]


def test_the_tangent_is_the_transpose_of_the_adjoint():
    """The identity, both sides exact.  The two sides are the same bilinear form of (g, d) with the forward's rounded values as
    coefficients (both walks re-form the flags through cn_step: the same bits), so in exact arithmetic they are equal and what is
    left is the rounding of the two walks.  Counting roundings on the longest path of the tangent: s' passes a row through
    s' + hit' (1) and s2' - ei' (2): 2 T over the rows; a term enters with at most 5 (dem' = fc' ed + fc ed': fc' two products and
    a sum, 3 with fe cover' + fe' cover taken as one level each; times ed, itself rounded once, 4; the sum, 5; hit' and cap' are
    shorter) and leaves through direct' + drip' or ed' - ei', then / dt_h, with s1' - cap' before it: 3.  m_tangent = 2 T + 8.  The
    adjoint's count is 4 T + 7 (test_the_adjoint_is_the_true_derivative).  Each side's error is relative to the same form on
    absolute values, every difference a sum: <|g|, T_abs |d|>, T_abs the recurrence of canopy_tangent_ref(absolute=True), which
    by transposition is the adjoint's own form on absolute values too.  Held: |left - right| <= gamma_m <|g|, T_abs |d|> with
    m = (2 T + 8) + (4 T + 7) = 6 T + 15.
    The bound refuses a dropped cmax lai', a wrong sign on ei' and a missing fc': the ratios are printed and recorded in
    profiles/r19/error_bound.txt.
    Measured: worst |left - right| / bound = 0.00134; wrong tangents: no_cmax_dlai 7.84e+11, ei_sign 4.99e+13, no_dfc 6.16e+12."""
    rng = np.random.default_rng(1906)
    worst, wrong_worst = 0.0, {"no_cmax_dlai": 0.0, "ei_sign": 0.0, "no_dfc": 0.0}
    for B, T, D, with_lai in ((8, 17, 3, True), (22, 9, 3, True), (24, 1, 2, True), (19, 17, 1, False)):
        p, e, lai, par, state, dt = CH.case_data(rng, T, B)
        lai = lai if with_lai else None
        g = tuple(CH.mixed(rng, T, B) for _ in range(4))
        dirs = (CH.mixed(rng, D, T, B), CH.mixed(rng, D, T, B), CH.mixed(rng, D, T, B), CH.mixed(rng, D, 3, B), CH.mixed(rng, D, B))
        m = 6 * T + 15
        store = CH.canopy_ref(p, e, lai, par, dt, state)[2]
        adj = CH.host_call(("grad", *g, p, e, lai, store, par, dt, state, True, True, True))
        if lai is None:  # glai is still the derivative along lai' (lai = 1)
            assert CH.same_bits(adj[2], CH.canopy_grad_ref(*g, p, e, None, store, par, dt, state)[2])
        tan = CH.host_call(("tan", p, e, lai, par, dt, state, D, *dirs, D, 0, True, True, True))
        ab = CH.canopy_tangent_ref(p, e, lai, par, dt, state, D, *dirs, absolute=True)
        bounds = [Fraction(gamma(m)) * (dot(np.abs(g[0]), ab[0][:, :, k]) + dot(np.abs(g[1]), ab[1][:, :, k]) + dot(np.abs(g[2]), ab[2][k])
                                        + dot(np.abs(g[3]), ab[3][k])) for k in range(D)]
        for (left, right), bar in zip(_identity(g, dirs, adj, tan, D), bounds):
            assert bar > 0 and abs(left - right) <= bar, (B, T, float(abs(left - right) / bar))
            worst = max(worst, float(abs(left - right) / bar))
        for variant in wrong_worst:
            bad = CH.canopy_tangent_ref(p, e, lai, par, dt, state, D, *dirs, variant=variant)
            ratios = [float(abs(l - r) / bar) for (l, r), bar in zip(_identity(g, dirs, adj, bad, D), bounds)]
            wrong_worst[variant] = max(wrong_worst[variant], max(ratios))
    print("canopy tangent, adjoint identity: worst |left - right| / bound = %.3g; wrong tangents: %s"
          % (worst, ", ".join("%s %.3g" % kv for kv in wrong_worst.items())))
    assert 0.0 < worst <= 1.0
    assert all(v > 1.0 for v in wrong_worst.values()), wrong_worst


# ---- 4. behaviour through the Python layer ------------------------------------------------------------------------------------
def _taken(par):
    """parameters the Python layer takes (case_data's are)"""
    return [par[k] for k in range(3)]


def test_chunked_repeated_and_permuted_calls_give_the_same_bits():
    """One call against calls cut at 1 row, at T - 1 rows and in the middle (carry=True keeps the [1, B] store per key), from a dry
    canopy and from a given state, with and without leaf area; reset(); a permutation of the cells gives the permuted bits; the
    raw tangent in chunks carrying dstate."""
    rng = np.random.default_rng(23)
    T, B = 17, 65
    p, e, lai, par, state, dt = CH.case_data(rng, T, B)
    canopy = SimCatchmentCanopy(*_taken(par), dt)
    tp, te, tl = _t(p), _t(e), _t(lai)
    for st in (None, state):
        for la, tla in ((lai, tl), (None, None)):
            want = CH.canopy_ref(p, e, la, par, dt, st)
            ts = None if st is None else _t(st)
            got = canopy.run(tp, te, tla, carry=False, state=ts, store=True)
            assert len(got) == 4 and all(CH.same_bits(a.numpy(), b) for a, b in zip(got, want))
            two = canopy.run(tp, te, tla, carry=False, state=ts)
            assert len(two) == 2 and all(CH.same_bits(a.numpy(), b) for a, b in zip(two, want)) and canopy.state_of() is None
            for cut in (1, T - 1, T // 2):
                key = ("cut", cut, st is None, la is None)
                a = canopy.run(tp[:cut], te[:cut], None if la is None else tl[:cut], key=key, state=ts, store=True)
                b = canopy.run(tp[cut:], te[cut:], None if la is None else tl[cut:], key=key, store=True)
                assert all(CH.same_bits(torch.cat([x, y]).numpy(), z) for x, y, z in zip(a, b, want)), cut
                assert CH.same_bits(canopy.state_of(key).numpy(), want[4])
                empty = canopy.run(tp[:0], te[:0], key=key)  # T = 0
                assert tuple(empty[0].shape) == (0, B) and CH.same_bits(canopy.state_of(key).numpy(), want[4])
    assert canopy.state_of("nobody") is None
    canopy.reset()
    assert canopy.state_of(("cut", 1, True, True)) is None
    perm = rng.permutation(B)
    want = CH.canopy_ref(p, e, lai, par, dt, state)
    got = CH.host_call(("fwd", p[:, perm], e[:, perm], lai[:, perm], par[:, perm], dt, state[:, perm], True, True))
    assert all(CH.same_bits(a, b[:, perm]) for a, b in zip(got, want))
    # the raw tangent, in chunks that carry the value state and dstate
    D = 3
    dirs = [CH.mixed(rng, D, T, B), CH.mixed(rng, D, T, B), CH.mixed(rng, D, T, B), CH.mixed(rng, D, 3, B), CH.mixed(rng, D, B)]
    td = [_t(a) for a in dirs]
    whole = canopy.tangent(tp, te, D, lai=tl, dp=td[0], de=td[1], dlai=td[2], dpar=td[3], state=_t(state), dstate=td[4], store=True, want_state=True)
    ref = CH.canopy_tangent_ref(p, e, lai, par, dt, state, D, *dirs)
    assert all(CH.same_bits(a.numpy(), b) for a, b in zip(whole, ref))
    s, ds, parts = _t(state), td[4], []
    for lo, hi in ((0, 1), (1, 8), (8, 9), (9, 17), (17, 17)):
        cut = lambda x: x[:, lo:hi].contiguous()
        part = canopy.tangent(tp[lo:hi], te[lo:hi], D, lai=tl[lo:hi], dp=cut(td[0]), de=cut(td[1]), dlai=cut(td[2]), dpar=td[3], state=s, dstate=ds,
                              store=True, want_state=True)
        parts.append(part)
        ds = part[4]
        s = _t(CH.canopy_ref(p[lo:hi], e[lo:hi], lai[lo:hi], par, dt, s.numpy())[4])
    assert CH.same_bits(torch.cat([x[0] for x in parts]).numpy(), ref[0]) and CH.same_bits(torch.cat([x[1] for x in parts]).numpy(), ref[1])
    assert CH.same_bits(torch.cat([x[2] for x in parts], dim=1).numpy(), ref[2]) and CH.same_bits(ds.numpy(), ref[4])
    # the write into a wider block, without d pet_out
    block = torch.full((T, B, 6), 7.5, dtype=torch.float64)
    out, out_pet, dst, dev, dso = canopy.tangent(tp, te, D, lai=tl, dpar=td[3], state=_t(state), out=block, k0=2, want_pet=False)
    assert out is block and out_pet is None and dst is None and dev is None and dso is None
    want_w = CH.canopy_tangent_ref(p, e, lai, par, dt, state, D, dpar=dirs[3])[0]
    assert CH.same_bits(block[:, :, 2:5].numpy(), want_w) and bool((block[:, :, [0, 1, 5]] == 7.5).all())
    from lgar_py_amd import LgarError
    with pytest.raises(LgarError, match=r"ld >= k0 \+ D"):
        canopy.tangent(tp, te, D, out=block, k0=4)
    with pytest.raises(LgarError, match="one ld"):
        canopy.tangent(tp, te, D, out=block, out_pet=torch.zeros(T, B, 5, dtype=torch.float64), k0=2)
    with pytest.raises(LgarError, match="dpar must be a contiguous"):
        canopy.tangent(tp, te, D, dpar=td[3][:, :2])


def test_autograd_through_the_host_build():
    """catchment_canopy on the host build (SimCatchmentCanopy.function): precip, pet, lai, the three parameters and the initial
    store receive the bits of canopy_grad_ref.  Scalar parameters receive the sum over the cells; without return_store no
    gstore / gevap is passed; without lai none is read; an input that requires no gradient gets none."""
    p, e, lai, par, state, dt, g = _derivative_data()
    leaf = lambda a: _t(a).clone().requires_grad_(True)
    tp, te, tl, ts = leaf(p), leaf(e), leaf(lai), leaf(state)
    tpar = [leaf(par[k]) for k in range(3)]
    outs = SimCatchmentCanopy.function(tp, te, *tpar, dt, lai=tl, state=ts, return_store=True)
    ref = CH.canopy_ref(p, e, lai, par, dt, state)
    assert len(outs) == 4 and all(CH.same_bits(a.detach().numpy(), b) for a, b in zip(outs, ref))
    sum((o * _t(gk)).sum() for o, gk in zip(outs, g)).backward()
    g_ref = CH.canopy_grad_ref(*g, p, e, lai, ref[2], par, dt, state)
    mine = (tp.grad.numpy(), te.grad.numpy(), tl.grad.numpy(), np.stack([v.grad.numpy() for v in tpar]), ts.grad.numpy())
    assert all(CH.same_bits(a, b) for a, b in zip(mine, g_ref))
    assert all(float(np.abs(g_ref[3][k]).max()) > 0 for k in range(3)) and float(np.abs(g_ref[4]).min()) > 0
    # two outputs, no leaf area, scalar parameters: summed gradients; a constant pet and state
    scal = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (0.12, 0.9, 0.7)]
    tp2 = leaf(p)
    w2, pet2 = SimCatchmentCanopy.function(tp2, _t(e), *scal, dt, state=_t(state))
    ((w2 * _t(g[0])).sum() + (pet2 * _t(g[1])).sum()).backward()
    par2 = np.stack([np.full(p.shape[1], float(v.detach())) for v in scal])
    ref2 = CH.canopy_ref(p, e, None, par2, dt, state)
    g2 = CH.canopy_grad_ref(g[0], g[1], None, None, p, e, None, ref2[2], par2, dt, state)
    assert CH.same_bits(w2.detach().numpy(), ref2[0]) and CH.same_bits(pet2.detach().numpy(), ref2[1]) and CH.same_bits(tp2.grad.numpy(), g2[0])
    for k, v in enumerate(scal):
        assert CH.same_bits(v.grad.numpy().reshape(1), _t(g2[3][k]).sum().numpy().reshape(1)), k
    assert float(np.abs(g2[3]).sum(axis=1).min()) > 0
    # pet alone, through pet_out only
    te3 = leaf(e)
    _, pet3 = SimCatchmentCanopy.function(_t(p), te3, *[_t(par[k]) for k in range(3)], dt, lai=_t(lai))
    (pet3 * _t(g[1])).sum().backward()
    ref3 = CH.canopy_ref(p, e, lai, par, dt)
    g3 = CH.canopy_grad_ref(np.zeros_like(p), g[1], None, None, p, e, lai, ref3[2], par, dt)
    assert CH.same_bits(te3.grad.numpy(), g3[1])
    with torch.no_grad():
        plain = SimCatchmentCanopy.function(_t(p), _t(e), *[_t(par[k]) for k in range(3)], dt, lai=_t(lai))
        assert CH.same_bits(plain[0].numpy(), ref3[0]) and CH.same_bits(plain[1].numpy(), ref3[1])


def test_construction_and_rejections():
    import lgar_py_amd as lg
    from lgar_py_amd import LgarError, _capi
    from lgar_py_amd.canopy import CatchmentCanopy, catchment_canopy, catchment_canopy_directions
    assert lg.CatchmentCanopy is CatchmentCanopy and lg.catchment_canopy is catchment_canopy
    assert lg.catchment_canopy_directions is catchment_canopy_directions
    assert {"CatchmentCanopy", "catchment_canopy", "catchment_canopy_directions"} <= set(lg.__all__)
    assert _capi.ABI_VERSION == 4
    assert {"lgar_catchment_canopy", "lgar_catchment_canopy_grad", "lgar_catchment_canopy_tangent"} <= set(_capi.EXPORTS)
    make = lambda *a, **kw: CatchmentCanopy(*a, device="cpu", **kw)
    ok = [[0.1, 0.0, 0.2], torch.tensor([0.5, 2.0, 0.0], dtype=torch.float64), np.array([0.0, 0.5, 1.0])]
    st = make(*ok, 0.25)
    assert st.B == 3 and tuple(st.par.shape) == (3, 3) and st.par.dtype == torch.float64 and st.par[1].tolist() == [0.5, 2.0, 0.0]
    assert st.dt_h == 0.25
    assert make(0.1, 1.0, 0.5, 0.5, n_catchments=4).par.tolist() == [[v] * 4 for v in (0.1, 1.0, 0.5)]
    assert make([], [], [], 1.0).B == 0

    def but(k, v, dt=1.0, **kw):
        args = list(ok)
        args[k] = v
        return lambda: make(*args, dt, **kw)

    for call, word in ((but(0, [0.1, 0.0]), "agree"), (lambda: make(0.1, 1.0, 0.5, 1.0), "agree"), (but(0, 0.1, n_catchments=4), "agree"),
                       (but(0, [[0.1]]), r"\[B\]"), (but(0, [0.1, -0.01, 0.2]), r"cmax\[1\].*>= 0"), (but(1, -0.5), r"fe\[0\].*>= 0"),
                       (but(2, [0.0, 0.5, 1.0000001]), r"cover\[2\].*0 \.\. 1"), (but(2, [-1e-9, 0.5, 1.0]), r"cover\[0\].*0 \.\. 1"),
                       (but(0, [np.nan, 0.0, 0.2]), "finite"), (but(1, [np.inf, 2.0, 0.0]), "finite"), (but(2, [0.0, np.nan, 0.0]), "finite"),
                       (but(0, ok[0], dt=0.0), "dt_h"), (but(0, ok[0], dt=np.nan), "dt_h"), (but(0, ok[0], dt=-1.0), "dt_h"),
                       (but(0, ok[0], dt="hour"), "dt_h"), (but(0, torch.tensor([0.1, 0.0, 0.2])), "fp64"), (but(2, ["a", 0.0, 0.0]), "numbers")):
        with pytest.raises(LgarError, match=word):
            call()
    # calls: shapes, dtypes, devices
    sim = SimCatchmentCanopy(*ok, 1.0)
    x, y = torch.ones(4, 3, dtype=torch.float64), torch.full((4, 3), 0.1, dtype=torch.float64)
    w, pet = sim.run(x, y)
    assert tuple(w.shape) == (4, 3) and tuple(pet.shape) == (4, 3) and tuple(sim.state_of().shape) == (1, 3)
    assert len(sim.run(x, y, store=True)) == 4 and len(sim.run(x, y, x)) == 2
    for args in ((x[:, :2], y), (x.float(), y), (x.numpy(), y), (x.to("meta"), y), (x[0], y), (x, y[:3]), (x, y.float()), (x, y[:, :2]),
                 (x, y, x[:3]), (x, y, x.float()), (x, y, None, True, None, x), (x, y, None, True, None, x[:1].float()), (x, y, None, True, None, x[0])):
        with pytest.raises(LgarError, match=r"3\] tensor"):
            sim.run(*args)
    q = [torch.ones(3, dtype=torch.float64) for _ in range(3)]
    f = SimCatchmentCanopy.function
    for call in (lambda: f(x.float(), y, *q, 1.0), lambda: f(x, y[:3], *q, 1.0), lambda: f(x, y.float(), *q, 1.0), lambda: f(x, None, *q, 1.0),
                 lambda: f(x, y, q[0][:2], *q[1:], 1.0), lambda: f(x, y, q[0].float(), *q[1:], 1.0), lambda: f(x, y, "a", *q[1:], 1.0),
                 lambda: f(x, y, *q, 0.0), lambda: f(x, y, *q, 1.0, state=x), lambda: f(x, y, *q, 1.0, lai=x[:2]),
                 lambda: f(x, y, *q[:2], q[2].to("meta"), 1.0), lambda: f(x[0], y[0], *q, 1.0)):
        with pytest.raises(LgarError):
            call()
    # a store on the CPU holds the host logic only: the kernels have no CPU fallback
    cpu = make(*ok, 1.0)
    for call in (lambda: cpu.run(x, y), lambda: cpu.run(x, y, carry=False, store=True), lambda: cpu.tangent(x, y, 1),
                 lambda: catchment_canopy(x, y, *q, 1.0), lambda: catchment_canopy_directions(x, y, *[v.clone().requires_grad_(True) for v in q], 1.0)):
        with pytest.raises(LgarError, match="no CPU fallback"):
            call()
    with pytest.raises(LgarError, match=r"cover\[0\]"):  # the directions validate as the class does
        catchment_canopy_directions(x, y, q[0], q[1], q[2] * 2.0, 1.0, owner=SimCatchmentCanopy)


def test_entry_points_refuse_bad_arguments():
    """canopy_host.refusals on the host launchers, which call lgar_canopy.hpp's own checks as the library does."""
    lib = CH.library()
    buf = np.ones(1024)

    class Buffer:
        address = buf.ctypes.data
        get = staticmethod(lambda lo, hi: buf[lo:hi].tolist())

        @staticmethod
        def set(lo, hi, values):
            buf[lo:hi] = values
    CH.refusals(lambda name: getattr(lib, "canopyhost_" + name), Buffer)


def test_catchment_canopy_directions_through_the_host_build():
    """One direction per parameter that requires grad, in the order cmax, fe, cover, from one tangent launch: d_precip and d_pet have
    the bits of canopy_tangent_ref along one-hot dpar; contracted with a cotangent they agree with the autograd node's gradients."""
    import lgar_py_amd as lg
    p, e, lai, par, state, dt, g = _derivative_data()
    T, B = p.shape
    pars = [_t(par[k]).clone() for k in range(3)]
    pars[0].requires_grad_(True)
    pars[2].requires_grad_(True)
    launches = []

    class Counted(SimCatchmentCanopy):
        @classmethod
        def _open(cls, device):
            lib = SimCatchmentCanopy._open(device)

            class Count:
                def __getattr__(self, name):
                    launches.append(name)
                    return getattr(lib, name)
            return Count()
    water, pet_out, fd = lg.catchment_canopy_directions(_t(p), _t(e), *pars, dt, lai=_t(lai), state=_t(state), owner=Counted)
    assert launches == ["lgar_catchment_canopy", "lgar_catchment_canopy_tangent"]
    assert fd.K == 2 and fd.params[0] is pars[0] and fd.params[1] is pars[2]
    dpar = np.zeros((2, 3, B))
    dpar[0, 0], dpar[1, 2] = 1.0, 1.0
    want = CH.canopy_tangent_ref(p, e, lai, par, dt, state, 2, dpar=dpar)
    assert CH.same_bits(fd.d_precip.permute(1, 2, 0).numpy(), want[0]) and CH.same_bits(fd.d_pet.permute(1, 2, 0).numpy(), want[1])
    ref = CH.canopy_ref(p, e, lai, par, dt, state)
    assert CH.same_bits(water.numpy(), ref[0]) and CH.same_bits(pet_out.numpy(), ref[1]) and not water.requires_grad
    w2, pet2 = SimCatchmentCanopy.function(_t(p), _t(e), *pars, dt, lai=_t(lai), state=_t(state))
    ((w2 * _t(g[0])).sum() + (pet2 * _t(g[1])).sum()).backward()
    for k, j in enumerate((0, 2)):
        got = (fd.d_precip[k] * _t(g[0])).sum(0) + (fd.d_pet[k] * _t(g[1])).sum(0)
        assert torch.allclose(got, pars[j].grad, rtol=1e-9, atol=1e-12 * float(pars[j].grad.abs().max())), j
    none = lg.catchment_canopy_directions(_t(p), _t(e), *[v.detach() for v in pars], dt, owner=SimCatchmentCanopy)
    assert none[2].K == 0 and CH.same_bits(none[0].numpy(), CH.canopy_ref(p, e, None, par, dt)[0])


def test_snow_directions_behind_an_upstream_stage():
    """catchment_snow_directions(upstream=None) is the function as it was: the bits of the statement, one forward and one tangent
    launch over D directions with dp NULL.  With the canopy's directions upstream, ONE snow-tangent launch runs over K + D
    directions; its d_precip equals, in bits, two separate tangent calls chained by hand (the canopy's d water through dp with a
    zero dpar; the snow parameters through dpar with a zero dp); d_pet is the canopy's, padded with zero rows."""
    import lgar_py_amd as lg
    rng = np.random.default_rng(31)
    T, B = 17, 9
    p, ta, _, _, _, spar, sstate, dt = SH.case_data(rng, T, B)
    p, sstate = np.abs(p), np.abs(sstate)
    spar[1] = np.maximum(spar[1], spar[0] + 0.5)
    e = rng.random((T, B)) * 0.3 / dt
    lai = rng.uniform(0.5, 4.5, (T, B))
    cpar = np.stack([rng.uniform(0.02, 0.2, B) * dt, rng.uniform(0.2, 2.0, B), rng.uniform(0.2, 1.0, B)])
    launches = []

    class CountedSnow(ST.SimSnow):
        @classmethod
        def _open(cls, device):
            lib = ST.SimSnow._open(device)

            class Count:
                def __getattr__(self, name):
                    fn = getattr(lib, name)

                    def counted(*args):
                        launches.append((name, args))
                        return fn(*args)
                    return counted
            return Count()
    spars = [_t(spar[j]).clone() for j in range(7)]
    for j in (3, 4):
        spars[j].requires_grad_(True)
    sdpar = np.zeros((2, 7, B))
    sdpar[0, 3], sdpar[1, 4] = 1.0, 1.0
    # upstream=None: today's results and launches
    plain = lg.catchment_snow_directions(_t(p), _t(ta), *spars, dt, state=_t(sstate), owner=CountedSnow)
    first = list(launches)
    del launches[:]
    again = lg.catchment_snow_directions(_t(p), _t(ta), *spars, dt, state=_t(sstate), owner=CountedSnow, upstream=None)
    assert [n for n, _ in first] == [n for n, _ in launches] == ["lgar_catchment_snow", "lgar_catchment_snow_tangent"]
    assert first[1][1][7] == launches[1][1][7] == 2 and first[1][1][8] is None and launches[1][1][8] is None  # D = 2, dp NULL
    want = ST.snow_tangent_ref(p, ta, spar, dt, sstate, 2, dpar=sdpar)[0]
    for water, fd in (plain, again):
        assert fd.K == 2 and fd.d_pet is None and CH.same_bits(fd.d_precip.permute(1, 2, 0).numpy(), want)
        assert CH.same_bits(water.numpy(), SH.snow_ref(p, ta, spar, dt, sstate)[0])
    # canopy -> snow
    cpars = [_t(cpar[k]).clone().requires_grad_(True) for k in range(3)]
    water_c, pet_c, fd_c = lg.catchment_canopy_directions(_t(p), _t(e), *cpars, dt, lai=_t(lai), owner=SimCatchmentCanopy)
    del launches[:]
    water, fd = lg.catchment_snow_directions(water_c, _t(ta), *spars, dt, state=_t(sstate), owner=CountedSnow, upstream=fd_c)
    assert [n for n, _ in launches] == ["lgar_catchment_snow", "lgar_catchment_snow_tangent"] and launches[1][1][7] == 5
    assert fd.K == 5 and all(a is b for a, b in zip(fd.params, cpars + [spars[3], spars[4]]))
    wc = water_c.numpy()
    assert CH.same_bits(water.numpy(), SH.snow_ref(wc, ta, spar, dt, sstate)[0])
    up = ST.snow_tangent_ref(wc, ta, spar, dt, sstate, 3, dp=fd_c.d_precip.numpy(), dpar=np.zeros((3, 7, B)))[0]
    own = ST.snow_tangent_ref(wc, ta, spar, dt, sstate, 2, dp=np.zeros((2, T, B)), dpar=sdpar)[0]
    rc1, dw1, _, _, _ = ST.call(wc, ta, spar, dt, sstate, 3, dp=fd_c.d_precip.numpy(), dpar=np.zeros((3, 7, B)))
    rc2, dw2, _, _, _ = ST.call(wc, ta, spar, dt, sstate, 2, dp=np.zeros((2, T, B)), dpar=sdpar)
    assert rc1 == 0 and rc2 == 0 and CH.same_bits(dw1, up) and CH.same_bits(dw2, own)
    assert CH.same_bits(fd.d_precip.permute(1, 2, 0).numpy(), np.concatenate([dw1, dw2], axis=2))
    assert float(np.abs(dw1).max()) > 0 and float(np.abs(dw2).max()) > 0
    assert CH.same_bits(fd.d_pet[:3].numpy(), fd_c.d_pet.numpy()) and not fd.d_pet[3:].any() and tuple(fd.d_pet.shape) == (5, T, B)
    # an upstream without d_pet gives none; one without directions is no upstream at all; a misshapen one is refused
    from lgar_py_amd.forcing import ForcingDirections
    _, fd2 = lg.catchment_snow_directions(water_c, _t(ta), *spars, dt, state=_t(sstate), owner=ST.SimSnow,
                                          upstream=ForcingDirections(fd_c.params, d_precip=fd_c.d_precip))
    assert fd2.d_pet is None and CH.same_bits(fd2.d_precip.numpy(), fd.d_precip.numpy())
    _, fd3 = lg.catchment_snow_directions(water_c, _t(ta), *spars, dt, state=_t(sstate), owner=ST.SimSnow, upstream=ForcingDirections((), None, None))
    assert fd3.K == 2 and fd3.d_pet is None
    _, fd4 = lg.catchment_snow_directions(water_c, _t(ta), *[v.detach() for v in spars], dt, state=_t(sstate), owner=ST.SimSnow, upstream=fd_c)
    assert fd4.K == 3 and CH.same_bits(fd4.d_precip.permute(1, 2, 0).numpy(), ST.snow_tangent_ref(wc, ta, spar, dt, sstate, 3, dp=fd_c.d_precip.numpy(),
                                                                                                   dpar=np.zeros((3, 7, B)))[0])
    with pytest.raises(lg.LgarError, match="tangent of precip"):
        lg.catchment_snow_directions(water_c[:5], _t(ta)[:5], *spars, dt, owner=ST.SimSnow, upstream=fd_c)
    with pytest.raises(lg.LgarError, match="tangent of precip"):
        lg.catchment_snow_directions(water_c, _t(ta), *spars, dt, owner=ST.SimSnow, upstream=ForcingDirections(fd_c.params, d_pet=fd_c.d_pet))
