"""CPU: the catchment baseflow (lgar_catchment_baseflow / lgar_catchment_baseflow_grad, include/lgar.h).

The per-catchment walks the GPU kernels run (lgar_py_amd/csrc/lgar_baseflow.hpp) are compiled for the host into a small
stand-alone program (tests/baseflow_host).  It is held BIT FOR BIT to the numpy statement of the definition
(baseflow_host.baseflow_ref / baseflow_grad_ref / gw_exp_ref); the same program built with AddressSanitizer + UBSan runs the same
cases.  Independently of the recurrence the definition itself is held to statements that do not come from it: gw_exp to
mpmath.exp, the mass balance to an exact sum, and the adjoint to derivatives of the real-arithmetic statement taken in mpmath.
The same header as a shared library stands behind lgar_py_amd.baseflow.CatchmentBaseflow (baseflow_host.SimCatchmentBaseflow),
so the host logic of baseflow.py -- validation, carry, autograd -- runs here too."""
from fractions import Fraction

import mpmath
import numpy as np
import pytest
import torch

import baseflow_host as BH
from baseflow_host import SimCatchmentBaseflow

U = 2.0 ** -53  # unit roundoff of fp64


def gamma(m):
    """Higham's gamma_m = m u / (1 - m u): (1 + d_1) .. (1 + d_m) = 1 + theta, |theta| <= gamma_m, for |d_i| <= u (3.1)."""
    return m * U / (1.0 - m * U)


# ---- 1. the host build against the numpy definition ------------------------------------------------------------------------
def _grid(shape_t=BH.SHAPE_T):
    """B in {1, 2, 63, 64, 65, 257} x T x state_in present or NULL: the forward with s and state_out wanted and with neither; the
    adjoint with gs, gpar and gstate / without gs, gpar only / with gs, neither / without gs, gstate only.
    (cases, references, the count of rows per branch)."""
    rng = np.random.default_rng(15)
    cases, refs = [], []
    rows = dict(flux=0, flux_z_low=0, flux_z_high=0, z_low=0, emptied=0, zero=0)
    for B in BH.SHAPE_B:
        for T in shape_t:
            r, gq, gs, par, state, dt = BH.case_data(rng, T, B)
            for st in (None, state):
                q, s, so = BH.baseflow_ref(r, par, dt, st)
                reg, clamp = BH.regimes(r, par, dt, st)
                for name, hit in (("flux", (reg == BH.FLUX) & (clamp == 0)), ("flux_z_low", (reg == BH.FLUX) & (clamp < 0)),
                                  ("flux_z_high", (reg == BH.FLUX) & (clamp > 0)), ("z_low", clamp < 0), ("emptied", reg == BH.EMPTIED),
                                  ("zero", reg == BH.ZERO)):
                    rows[name] += int(hit.sum())
                cases += [("fwd", r, par, dt, st, True, True), ("fwd", r, par, dt, st, False, False)]
                refs += [(q, s, so), (q, None, None)]
                full = BH.baseflow_grad_ref(gq, gs, r, s, par, dt, st)
                bare = BH.baseflow_grad_ref(gq, None, r, s, par, dt, st)
                cases += [("grad", gq, gs, r, s, par, dt, st, True, True), ("grad", gq, None, r, s, par, dt, st, True, False),
                          ("grad", gq, gs, r, s, par, dt, st, False, False), ("grad", gq, None, r, s, par, dt, st, False, True)]
                refs += [full, (bare[0], bare[1], None), (full[0], None, None), (bare[0], None, bare[2])]
    return cases, refs, rows


@pytest.fixture(scope="module")
def grid():
    return _grid()


def _check(cases, refs, got):
    assert len(got) == len(refs) == len(cases)
    for c, r, o in zip(cases, refs, got):
        for want, have in zip(r, o):
            assert (want is None) == (have is None), (c[0], np.asarray(c[3]).shape)
            assert want is None or BH.same_bits(have, want), (c[0], np.asarray(c[3]).shape)


def test_host_build_equals_the_numpy_definition_bit_for_bit(grid):
    cases, refs, rows = grid
    _check(cases, refs, BH.run(cases))
    # every branch of the walk is taken somewhere in the case set: flux; flux with z clamped at each end (z > ZMAX from a tiny cgw
    # under a large expon; z < 0 under a positive A from a negative expon, which the raw entry points take); z < 0 from a negative A
    # (which the selects send to "zero": f = 0 > A, qq = A < 0); emptied; zero
    print("rows per branch:", rows)
    assert all(n > 0 for n in rows.values()), rows
    # what the definition says about the corners, on the references themselves
    for c, r in zip(cases, refs):
        if c[0] == "fwd" and np.asarray(c[1]).shape[0] == 0 and r[2] is not None:  # T = 0 copies the state, or writes zeros
            assert BH.same_bits(r[2], np.zeros(np.asarray(c[1]).shape[1]) if c[4] is None else np.asarray(c[4]))
        if c[0] == "grad" and np.asarray(c[3]).shape[0] == 0:  # T = 0: zeros
            assert all(a is None or not a.any() for a in r)
    assert {np.asarray(c[1]).shape for c in cases if c[0] == "fwd"} == {(T, B) for T in BH.SHAPE_T for B in BH.SHAPE_B}


def test_sanitizer_build_on_the_same_cases(grid):
    """AddressSanitizer + UBSan build of the same program (a stand-alone executable: nothing is loaded into python; every array is
    allocated at its exact size) over the same cases: clean, with the same bits.  Any finding aborts the program."""
    cases, refs, _ = grid
    _check(cases, refs, BH.run(cases, sanitize=True))


# ---- 2. gw_exp against mpmath -----------------------------------------------------------------------------------------------
def _exp_grid():
    ln2 = float(mpmath.log(2))
    pts = [np.linspace(0.0, BH.ZMAX, 4001), 10.0 ** -np.arange(3.0, 17.0), np.array([0.0, 5e-324, 1e-300, BH.ZMAX])]
    half = np.array([(k + 0.5) * ln2 for k in range(58)])  # where k = rint(z log2 e) changes
    pts += [half, np.nextafter(half, 0.0), np.nextafter(half, 100.0), half * (1 - 1e-9), half * (1 + 1e-9), np.arange(1, 58) * ln2]
    z = np.unique(np.concatenate(pts))
    return z[(z >= 0.0) & (z <= BH.ZMAX)]


def test_gw_exp_against_mpmath():
    """gw_exp of the host build (and gw_exp_ref, the same bits) against mpmath.exp at 40 digits on a fixed grid of [0, ZMAX]: 4001
    evenly spaced points, the half-integer multiples of ln 2 (where k changes; each with both neighbours and +- 1e-9 relative), the
    integer multiples, 1e-3 .. 1e-16, the smallest subnormal, 0 and ZMAX.

    The bar, derived: with k = rint(z log2 e), |r| <= ln2 / 2 (1 + a few u).  k LN2_HI is exact (k <= 58 has 6 bits, LN2_HI 21), and
    z - k LN2_HI is exact (Sterbenz: k LN2_HI is within a factor 2 of z for k >= 1); k LN2_LO and the second subtraction round
    once each, and LN2_HI + LN2_LO misses ln 2 by 1.2e-26: the reduced argument is off by at most 2 u |r| + 7e-25, a relative
    error of e^r of the same size, counted as 2 roundings.  The polynomial: each coefficient is a correctly rounded 1 / j! (1
    rounding), each of the 13 Horner steps rounds a product and a sum (26): the computed p is sum c_j r^j with every term
    carrying at most 27 factors (1 + d), so |p - sum r^j / j!| <= gamma_27 sum |r|^j / j! <= gamma_27 e^|r| <= gamma_27 e^(ln2 / 2).
    The truncation after j = 13 is at most (ln2 / 2)^14 / 14! (1 + |r| / 15 + ..) < 4.3e-18.  The scaling by 2^k is exact.  In all:
    gamma_29 e^(ln2 / 2) + 4.3e-18 = 4.56e-15.  (That is the bound on the ABSOLUTE error of p, which lies in [0.707, 1.415]; taken
    relative to e^r it is rigorous for r >= 0 only -- for r < 0 the rigorous relative figure is gamma_29 e^(2 |r|) <= 2 gamma_29 --
    and it is asserted for the RELATIVE error at every point, the tighter reading.)
    Measured: worst relative error 1.38 u (1.53e-16), 0.0336 of the bound, over 4364 points."""
    z = _exp_grid()
    assert len(z) > 4300 and (z < 1e-3).sum() >= 14
    (e,), = BH.run([("exp", z)])
    assert BH.same_bits(e, BH.gw_exp_ref(z))
    bound = gamma(29) * float(np.exp(np.log(2.0) / 2.0)) + 4.3e-18
    mpmath.mp.dps = 40
    worst = 0.0
    for zi, ei in zip(z, e):
        want = mpmath.exp(mpmath.mpf(float(zi)))
        worst = max(worst, float(abs(mpmath.mpf(float(ei)) - want) / want))
    print("gw_exp vs mpmath.exp: worst relative error %.3g = %.3g u, %.3g of the bound %.3g, %d points" % (worst, worst / U, worst / bound, bound, len(z)))
    assert worst <= bound
    assert e[0] == 1.0 and e[-1] == float(mpmath.nstr(mpmath.exp(40), 20))


# ---- 3. mass ------------------------------------------------------------------------------------------------------------------
def test_mass_closes_per_catchment():
    """state_in + sum r = sum q + state_out within gamma_2T (|state_in| + sum |r|), the left side minus the right taken exactly
    (fractions.Fraction of the floats).  Each row rounds twice, A = fl(S + r) and S' = fl(A - qq), and 0 <= qq <= max(A, 0) gives
    |S'| <= |A| <= (|state_in| + sum |r|)(1 + u)^2t: 2T roundings of quantities no larger than that."""
    rng = np.random.default_rng(4)
    T, B = 17, 257
    r, _, _, par, state, dt = BH.case_data(rng, T, B)
    (q, _, so), = BH.run([("fwd", r, par, dt, state, False, True)])
    F = lambda v: Fraction(float(v))
    worst = 0.0
    for b in range(B):
        miss = abs(F(state[b]) + sum(F(v) for v in r[:, b]) - sum(F(v) for v in q[:, b]) - F(so[b]))
        bar = Fraction(gamma(2 * T)) * (abs(F(state[b])) + sum(abs(F(v)) for v in r[:, b]))
        assert miss <= bar, b
        worst = max(worst, float(miss / bar))
    assert 0.0 < worst <= 1.0 and float(q.sum()) > 0


# ---- 4. the same bits ---------------------------------------------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _valid(rng, T, B):
    """case_data with parameters the Python layer accepts (expon > 0)"""
    r, gq, gs, par, state, dt = BH.case_data(rng, T, B)
    par[1] = np.abs(par[1])
    return r, gq, gs, par, state, dt


def test_chunked_repeated_and_permuted_calls_give_the_same_bits():
    """One call against calls cut at 1 row, at T - 1 rows and in the middle (carry=True keeps the [B] storage per key), from zeros
    and from a given state; a repeated call; reset(); a permutation of the catchments gives the permuted bits."""
    rng = np.random.default_rng(23)
    T, B = 17, 65
    r, _, _, par, state, dt = _valid(rng, T, B)
    store = SimCatchmentBaseflow(par[0], par[1], par[2], dt)
    tr = _t(r)
    for st in (None, state):
        want_q, want_s, want_state = BH.baseflow_ref(r, par, dt, st)
        ts = None if st is None else _t(st)
        q, s = store.run(tr, carry=False, state=ts, storage=True)
        assert BH.same_bits(q.numpy(), want_q) and BH.same_bits(s.numpy(), want_s)
        assert BH.same_bits(store.run(tr, carry=False, state=ts).numpy(), want_q) and store.state_of() is None
        for cut in (1, T - 1, T // 2):
            key = ("cut", cut, st is None)
            a, sa = store.run(tr[:cut], key=key, state=ts, storage=True)
            b, sb = store.run(tr[cut:], key=key, storage=True)
            assert BH.same_bits(torch.cat([a, b]).numpy(), want_q) and BH.same_bits(torch.cat([sa, sb]).numpy(), want_s), cut
            assert BH.same_bits(store.state_of(key).numpy(), want_state)
            assert tuple(store.run(tr[:0], key=key).shape) == (0, B) and BH.same_bits(store.state_of(key).numpy(), want_state)  # T = 0
    assert store.state_of("nobody") is None
    store.reset()
    assert store.state_of(("cut", 1, True)) is None
    perm = rng.permutation(B)
    q, s, so = BH.baseflow_ref(r, par, dt, state)
    (pq, ps, pso), = BH.run([("fwd", r[:, perm], par[:, perm], dt, state[perm], True, True)])
    assert BH.same_bits(pq, q[:, perm]) and BH.same_bits(ps, s[:, perm]) and BH.same_bits(pso, so[perm])
    _, gq, gs, _, _, _ = BH.case_data(rng, T, B)
    want = BH.baseflow_grad_ref(gq, gs, r, s, par, dt, state)
    got, = BH.run([("grad", gq[:, perm], gs[:, perm], r[:, perm], s[:, perm], par[:, perm], dt, state[perm], True, True)])
    assert BH.same_bits(got[0], want[0][:, perm]) and BH.same_bits(got[1], want[1][:, perm]) and BH.same_bits(got[2], want[2][perm])


def test_a_nan_stays_in_its_catchment_from_its_row_on():
    rng = np.random.default_rng(41)
    T, B = 9, 65
    r, _, _, par, state, dt = BH.case_data(rng, T, B)
    clean_q, clean_s, _ = BH.baseflow_ref(r, par, dt, state)
    t0, b = 4, 17
    r[t0, b] = np.nan
    (q, s, so), = BH.run([("fwd", r, par, dt, state, True, True)])
    hit = np.zeros((T, B), dtype=bool)
    hit[t0:, b] = True
    for got, clean in ((q, clean_q), (s, clean_s)):
        assert (np.isnan(got) == hit).all() and BH.same_bits(got[~hit], clean[~hit])
    assert np.isnan(so[b]) and np.isnan(so).sum() == 1


# ---- 5. the adjoint is the true derivative ------------------------------------------------------------------------------------
def _derivative_data():
    """B = 7, T = 9, dt_h = 1: ordinary stores (0, 1, 2, 6), a store with a large cgw that is emptied and then refills (3), a tiny
    cgw under a large expon (4: z > ZMAX), a negative initial storage that recharge brings back above zero (5)."""
    rng = np.random.default_rng(77)
    T, B = 9, 7
    cgw = np.array([0.05, 0.02, 0.1, 3.0, 1e-25, 0.05, 0.03]) * (1.0 + 0.1 * rng.random(B))
    expon = np.array([3.0, 5.0, 2.0, 3.0, 70.0, 4.0, 6.0]) * (1.0 + 0.1 * rng.random(B))
    smax = np.array([20.0, 30.0, 10.0, 20.0, 15.0, 8.0, 25.0]) * (1.0 + 0.1 * rng.random(B))
    state = np.array([10.0, 12.0, 6.0, 11.0, 12.0, -2.0, 9.0]) * (1.0 + 0.1 * rng.random(B))
    r = 0.4 + 1.2 * rng.random((T, B))
    gq, gs = (rng.random((T, B)) - 0.4) * 2.0, (rng.random((T, B)) - 0.4) * 0.5
    return r, gq, gs, np.stack([cgw, expon, smax]), state, 1.0


def _mp_column(r, cgw, expon, smax, dt, S0, gq, gs, detail=False):
    """One catchment of the definition in REAL arithmetic (mpmath at the working precision; exp is mpmath.exp): the loss
    sum gq q + sum gs s and, with detail, per row A, z, e, f, q, S, the regime and whether z is inside [0, ZMAX]."""
    S, loss, rows = S0, mpmath.mpf(0), []
    cd = cgw * dt
    for t in range(len(r)):
        A = S + r[t]
        z = expon * (A / smax)
        zc = mpmath.mpf(0) if z < 0 else (mpmath.mpf(BH.ZMAX) if z > BH.ZMAX else z)
        e = mpmath.exp(zc)
        f = cd * (e - 1)
        pre = A if f > A else f
        qq = mpmath.mpf(0) if pre < 0 else pre
        S = A - qq
        loss += gq[t] * qq + gs[t] * S
        rows.append(dict(Sprev=A - r[t], A=A, z=z, zc=zc, e=e, f=f, q=qq, S=S, regime=BH.ZERO if pre < 0 else (BH.EMPTIED if f > A else BH.FLUX),
                         inside=not (z < 0 or z > BH.ZMAX)))
    return (loss, rows) if detail else loss


@pytest.fixture(scope="module")
def derivative():
    """The data of the derivative tests, the derivatives of the real-arithmetic statement by central differences in mpmath, the
    adjoint on absolute values and the operation counts m (test_the_adjoint_is_the_true_derivative has the derivation)."""
    mpmath.mp.dps = 60
    r, gq, gs, par, state, dt = _derivative_data()
    T, B = r.shape
    M = mpmath.mpf
    h = M(10) ** -20
    want = dict(gr=[[None] * B for _ in range(T)], gpar=[[None] * B for _ in range(3)], gstate=[None] * B)
    mag = dict(gr=[[None] * B for _ in range(T)], gpar=[[None] * B for _ in range(3)], gstate=[None] * B)
    reg, clamp = BH.regimes(r, par, dt, state)
    cond = dict(K1=0.0, Z=0.0, n_e=0.0, R=0.0, margin=np.inf)
    for b in range(B):
        x = [M(float(v)) for v in r[:, b]] + [M(float(par[k, b])) for k in range(3)] + [M(float(state[b]))]
        g, gsb = [M(float(v)) for v in gq[:, b]], [M(float(v)) for v in gs[:, b]]
        col = lambda v, **kw: _mp_column(v[:T], v[T], v[T + 1], v[T + 2], M(dt), v[T + 3], g, gsb, **kw)
        _, rows = col(x, detail=True)
        # no row within a relative 1e-6 of a regime switch (f against A, the pre-clamp discharge against 0, z against 0 and ZMAX),
        # and the float walk takes the real walk's branches
        for t, row in enumerate(rows):
            scale = max(abs(row["A"]), abs(row["f"]))
            margins = [abs(row["f"] - row["A"]) / scale, abs(row["z"]) / max(1, abs(row["z"])), abs(row["z"] - BH.ZMAX) / BH.ZMAX]
            if row["f"] > row["A"]:  # the pre-clamp discharge is A = S + r: against 0 relative to its two terms
                margins.append(abs(row["A"]) / (abs(row["Sprev"]) + abs(x[t])))
            # (otherwise it is f = cd (e - 1), a product: it reaches 0 only where z does, which is held off above)
            cond["margin"] = min(cond["margin"], float(min(margins)))
            assert row["regime"] == reg[t, b] and row["inside"] == (clamp[t, b] == 0), (t, b)
        for i in range(T + 4):
            xp, xm = list(x), list(x)
            hi = h * abs(x[i])  # relative to the variable (cgw of catchment 4 is 1e-25); no variable is 0
            xp[i], xm[i] = x[i] + hi, x[i] - hi
            d = (col(xp) - col(xm)) / (2 * hi)
            if i < T:
                want["gr"][i][b] = d
            elif i < T + 3:
                want["gpar"][i - T][b] = d
            else:
                want["gstate"][b] = d
        # the adjoint on absolute values, and the condition figures of the derivation
        cd, expon, smax = x[T] * M(dt), x[T + 1], x[T + 2]
        lam, acc = M(0), [M(0)] * 3
        big = max(max(abs(row["A"]), abs(row["q"]), abs(row["S"])) for row in rows)
        K1 = max([float(row["e"] / (row["e"] - 1)) for row in rows if row["regime"] == BH.FLUX and row["z"] > 0] + [1.0])
        Z = max([float(row["z"]) for row in rows if row["regime"] == BH.FLUX and row["inside"]] + [0.0])
        for t in range(T - 1, -1, -1):
            row = rows[t]
            lam = lam + abs(gsb[t])
            w = abs(g[t]) + lam
            ce = cd * row["e"]
            flux, inside = row["regime"] == BH.FLUX, row["regime"] == BH.FLUX and row["inside"]
            dA = M(0) if row["regime"] == BH.ZERO else (M(1) if row["regime"] == BH.EMPTIED else (ce * (expon / smax) if inside else M(0)))
            assert 0 <= dA <= 1, (t, b)  # |dS / dA| = |1 - dA| <= 1: the forward walk does not amplify an error of A
            if flux:
                acc[0] = acc[0] + w * abs(M(dt) * (row["e"] - 1))
            if inside:
                acc[1] = acc[1] + w * abs(ce * (row["A"] / smax))
                acc[2] = acc[2] + w * abs(ce * row["zc"] / smax)
            lam = lam + w * abs(dA)
            mag["gr"][t][b] = lam
        mag["gstate"][b] = lam
        for k in range(3):
            mag["gpar"][k][b] = acc[k]
        E = (gamma(29) * 2.0 ** 0.5 + 4.3e-18) / U          # gw_exp's bound, in u
        rho = K1 * (2.0 * Z + E) + 3.0                      # the local relative error of qq of a flux row, in u
        delta = T * (2.0 + rho) * float(big)                # |dA_t| / u: T rows of (u |A| + rho u |q| + u |S|), not amplified
        n_e = E + 2.0 * Z + float(expon / smax) * delta     # the relative error of the factor e of a row, in u
        R = max([delta / float(abs(row["A"])) for row in rows if row["regime"] == BH.FLUX and row["inside"]] + [0.0])
        for k, v in (("K1", K1), ("Z", Z), ("n_e", n_e), ("R", R)):
            cond[k] = max(cond[k], v)
    assert cond["margin"] > 1e-6, cond
    m_gr = int(np.ceil(T * (8.0 + cond["n_e"])))
    m = dict(gr=m_gr, gstate=m_gr, gpar=int(np.ceil(m_gr + (cond["K1"] + 1.0) * cond["n_e"] + cond["R"] + T + 8)))
    return dict(data=(r, gq, gs, par, state, dt), want=want, mag=mag, m=m, cond=cond, regimes=(reg, clamp))


def _ratios(d, got):
    """per output, error / bound of every element against the mpmath derivative (inf where the bound is 0 and the error is not)"""
    out = {}
    for k, arr in zip(("gr", "gpar", "gstate"), got):
        a2, w2, m2 = np.atleast_2d(arr), d["want"][k], d["mag"][k]
        if arr.ndim == 1:
            w2, m2 = [w2], [m2]
        r = np.zeros(a2.shape)
        for i in range(a2.shape[0]):
            for j in range(a2.shape[1]):
                err, bar = abs(mpmath.mpf(float(a2[i, j])) - w2[i][j]), mpmath.mpf(gamma(d["m"][k])) * m2[i][j]
                r[i, j] = float(err / bar) if bar else (0.0 if err == 0 else np.inf)
        out[k] = r
    return out


def test_the_adjoint_is_the_true_derivative(derivative):
    """gr, gpar and gstate of the host build against the derivatives of L = sum gq q + sum gs s of the definition's REAL-arithmetic
    statement, taken in mpmath at 60 digits by central differences with h = 1e-20 |x| (the quotient misses the derivative by
    h^2 L''' / 6 ~ 1e-40: L is smooth between regime switches, and no row lies within a relative 1e-6 of one -- asserted, with the
    float walk taking the real walk's branch in every row).  B = 7, T = 9; rows in flux, flux with z > ZMAX, emptied and zero
    (with z < 0) all occur (asserted).

    The bound is gamma_m x (the same adjoint on absolute values: lam' = lam' + |gs|, w' = |gq| + lam', gr' = lam' + w' |dA|, the
    accumulators with |terms|), with the error of gw_exp counted inside m.  Derivation, to first order in u, per catchment, with
    figures taken from the real-arithmetic walk (never from the code under test):
      forward.  In a flux row z rounds twice, so e^z is off by 2 Z u relatively (Z = the largest z of an unclamped flux row) and
        gw_exp adds E = gamma_29 e^(ln2/2) + 4.3e-18 (its own derived bound); e - 1 amplifies that by K1 = max e / (e - 1) and
        rounds; cgw dt and the product round: qq is off by rho u = (K1 (2 Z + E / u) + 3) u relatively.  An emptied row gives
        qq = A, a zero row 0: no local error.  A = fl(S + r) and S = fl(A - qq) round once each.  dS / dA = 1 - dA lies in [0, 1]
        in every row (asserted), so errors of A are handed on without growth: |A_t - its real value| <= Delta =
        T (2 + rho) u max(|A|, |q|, |S|).
      a factor e in the adjoint is therefore off by n_e u = (E / u + 2 Z + (expon / smax) Delta / u) u; dA = (cd e)(expon / smax)
        adds 4 roundings (cd, ce, the quotient, the product); the row's own operations add 4 (lam + gs, gq - lam, w dA, lam + ..).
        A path of the expansion of gr passes a row at most once: m_gr = T (8 + n_e), and gstate is gr of a row before row 0.
      gpar: a term is w (<= m_gr) times a factor that holds e or e - 1 (<= K1 n_e), ce (n_e + 2), A or zc (R = the largest
        Delta / (u |A|) of an unclamped flux row, + 2) and at most 4 more roundings, added into an accumulator <= T times:
        m_gpar = m_gr + (K1 + 1) n_e + R + T + 8.
    n_e is dominated by (expon / smax) Delta / u, the forward error of A entering through e^z: the bound is of the order 1e-10
    relative to the absolute-value adjoint, far above the measured error and far below a wrong formula: it refuses, on every
    output the change reaches, dA without the factor e (gr, gpar, gstate), gs added after w instead of before (gr, gpar, gstate)
    and gsmax with the wrong sign (gpar).
    Measured: worst error / bound = 2.9e-06 (gr), 1.19e-06 (gpar), 1.47e-06 (gstate), with m = 422673 (gr, gstate), 1052266 (gpar)."""
    r, gq, gs, par, state, dt = derivative["data"]
    reg, clamp = derivative["regimes"]
    assert ((reg == BH.FLUX) & (clamp == 0)).sum() > 20 and ((reg == BH.FLUX) & (clamp > 0)).sum() > 0
    assert (reg == BH.EMPTIED).sum() > 0 and ((reg == BH.ZERO) & (clamp < 0)).sum() > 0
    _, s, _ = BH.baseflow_ref(r, par, dt, state)
    got, = BH.run([("grad", gq, gs, r, s, par, dt, state, True, True)])
    assert all(BH.same_bits(a, b) for a, b in zip(got, BH.baseflow_grad_ref(gq, gs, r, s, par, dt, state)))
    rt = _ratios(derivative, got)
    print("baseflow adjoint vs mpmath derivative: worst error / bound = %.3g (gr), %.3g (gpar), %.3g (gstate); m = %r; %r"
          % (rt["gr"].max(), rt["gpar"].max(), rt["gstate"].max(), derivative["m"], derivative["cond"]))
    assert all(v.max() <= 1.0 for v in rt.values())
    assert all(v.max() > 0 for v in rt.values())  # (the data are general: something does round)
    for variant, reached in (("no_e", ("gr", "gpar", "gstate")), ("gs_late", ("gr", "gpar", "gstate")), ("gsmax_sign", ("gpar",))):
        wrong = _ratios(derivative, BH.baseflow_grad_ref(gq, gs, r, s, par, dt, state, variant=variant))
        assert all(wrong[k].max() > 1.0 for k in reached), (variant, {k: v.max() for k, v in wrong.items()})
        assert all(wrong[k].max() <= 1.0 for k in wrong if k not in reached), variant


# ---- 6. autograd --------------------------------------------------------------------------------------------------------------
def _torch_statement(r, cgw, expon, smax, dt, state):
    """The plain torch statement of the recurrence (torch.exp, torch.where): q, s [T, B]."""
    S, qs, ss = state, [], []
    for t in range(r.shape[0]):
        A = S + r[t]
        z = expon * (A / smax)
        zc = torch.where(z < 0, torch.zeros_like(z), torch.where(z > BH.ZMAX, torch.full_like(z, BH.ZMAX), z))
        f = (cgw * dt) * (torch.exp(zc) - 1.0)
        pre = torch.where(f > A, A, f)
        qq = torch.where(pre < 0, torch.zeros_like(pre), pre)
        S = A - qq
        qs.append(qq)
        ss.append(S)
    return torch.stack(qs), torch.stack(ss)


def test_autograd_through_the_host_build(derivative):
    """catchment_baseflow on the host build (SimCatchmentBaseflow.function) on the data of the derivative test: recharge, the three
    parameters and the initial storage receive the bits of baseflow_grad_ref; against torch autograd of the plain torch statement
    the gradients agree within the bound of test_the_adjoint_is_the_true_derivative (the torch statement performs the same
    operations with libm's exp, whose error is below gw_exp's bound E: the derivation covers it as it stands).  Scalar
    parameters receive the sum over the catchments; without return_storage no gs is passed; a state that requires no gradient
    gets none."""
    r, gq, gs, par, state, dt = derivative["data"]
    leaf = lambda a: _t(a).clone().requires_grad_(True)
    tr, tc, te, tm, ts = leaf(r), leaf(par[0]), leaf(par[1]), leaf(par[2]), leaf(state)
    q, s = SimCatchmentBaseflow.function(tr, tc, te, tm, dt, state=ts, return_storage=True)
    q_ref, s_ref, _ = BH.baseflow_ref(r, par, dt, state)
    assert BH.same_bits(q.detach().numpy(), q_ref) and BH.same_bits(s.detach().numpy(), s_ref)
    ((q * _t(gq)).sum() + (s * _t(gs)).sum()).backward()
    gr_ref, gpar_ref, gstate_ref = BH.baseflow_grad_ref(gq, gs, r, s_ref, par, dt, state)
    mine = (tr.grad.numpy(), np.stack([tc.grad.numpy(), te.grad.numpy(), tm.grad.numpy()]), ts.grad.numpy())
    assert BH.same_bits(mine[0], gr_ref) and BH.same_bits(mine[1], gpar_ref) and BH.same_bits(mine[2], gstate_ref)
    assert float(np.abs(gpar_ref[0]).min()) > 0 and float(np.abs(np.delete(gpar_ref, 4, axis=1)).min()) > 0  # (4: z > ZMAX in every row)
    # torch autograd of the torch statement
    ar, ac, ae, am, as_ = leaf(r), leaf(par[0]), leaf(par[1]), leaf(par[2]), leaf(state)
    q2, s2 = _torch_statement(ar, ac, ae, am, dt, as_)
    ((q2 * _t(gq)).sum() + (s2 * _t(gs)).sum()).backward()
    theirs = (ar.grad.numpy(), np.stack([ac.grad.numpy(), ae.grad.numpy(), am.grad.numpy()]), as_.grad.numpy())
    rt = _ratios(derivative, theirs)
    assert all(v.max() <= 1.0 for v in rt.values()), {k: v.max() for k, v in rt.items()}
    for k, a, b in zip(("gr", "gpar", "gstate"), mine, theirs):
        bars = np.array([[float(gamma(derivative["m"][k]) * v) for v in row] for row in
                         (derivative["mag"][k] if a.ndim == 2 else [derivative["mag"][k]])]).reshape(a.shape)
        assert (np.abs(a - b) <= bars).all() and float(np.abs(q2.detach().numpy() - q_ref).max()) < 1e-12, k
    # without storage: no gs; scalar parameters: summed gradients; a constant state
    sc, se = torch.tensor(0.05, dtype=torch.float64, requires_grad=True), torch.tensor(3.0, dtype=torch.float64, requires_grad=True)
    tr2 = leaf(r)
    q3 = SimCatchmentBaseflow.function(tr2, sc, se, 20.0, dt, state=_t(state))
    (q3 * _t(gq)).sum().backward()
    par3 = np.stack([np.full(7, 0.05), np.full(7, 3.0), np.full(7, 20.0)])
    q3_ref, s3_ref, _ = BH.baseflow_ref(r, par3, dt, state)
    g3 = BH.baseflow_grad_ref(gq, None, r, s3_ref, par3, dt, state)
    assert BH.same_bits(q3.detach().numpy(), q3_ref) and BH.same_bits(tr2.grad.numpy(), g3[0])
    assert BH.same_bits(sc.grad.numpy().reshape(1), _t(g3[1][0]).sum().numpy().reshape(1)) and BH.same_bits(se.grad.numpy().reshape(1), _t(g3[1][1]).sum().numpy().reshape(1))
    with torch.no_grad():
        assert BH.same_bits(SimCatchmentBaseflow.function(_t(r), _t(par[0]), _t(par[1]), _t(par[2]), dt).numpy(), BH.baseflow_ref(r, par, dt)[0])


# ---- 7. host logic ------------------------------------------------------------------------------------------------------------
def test_construction_and_rejections():
    import lgar_py_amd as lg
    from lgar_py_amd import LgarError, _capi
    from lgar_py_amd.baseflow import CatchmentBaseflow, catchment_baseflow
    assert lg.CatchmentBaseflow is CatchmentBaseflow and lg.catchment_baseflow is catchment_baseflow
    assert {"CatchmentBaseflow", "catchment_baseflow"} <= set(lg.__all__)
    assert _capi.ABI_VERSION == 4 and _capi.GW_ZMAX == BH.ZMAX
    assert {"lgar_catchment_baseflow", "lgar_catchment_baseflow_grad"} <= set(_capi.EXPORTS)
    make = lambda *a, **kw: CatchmentBaseflow(*a, device="cpu", **kw)
    st = make([0.1, 0.0, 0.2], torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64), np.array([5.0, 6.0, 7.0]), 1.0)
    assert st.B == 3 and tuple(st.par.shape) == (3, 3) and st.par.dtype == torch.float64 and st.par[1].tolist() == [1.0, 2.0, 3.0]
    assert make(0.1, 2.0, 10.0, 0.5, n_catchments=4).par.tolist() == [[0.1] * 4, [2.0] * 4, [10.0] * 4]
    assert make(0.1, [2.0, 3.0], 10.0, 1.0).B == 2 and make([], [], [], 1.0).B == 0
    for args, kw, word in ((([0.1, 0.2], [1.0] * 3, [5.0] * 3, 1.0), {}, "agree"), ((0.1, 2.0, 10.0, 1.0), {}, "agree"),
                           (([0.1] * 3, [1.0] * 3, [5.0] * 3, 1.0), dict(n_catchments=4), "agree"),
                           (([[0.1]], [1.0], [5.0], 1.0), {}, r"\[B\]"), (([-0.1], [1.0], [5.0], 1.0), {}, "cgw"),
                           (([0.1], [0.0], [5.0], 1.0), {}, "expon"), (([0.1], [1.0], [0.0], 1.0), {}, "smax"),
                           (([0.1], [1.0], [-5.0], 1.0), {}, "smax"), (([np.nan], [1.0], [5.0], 1.0), {}, "finite"),
                           (([0.1], [np.inf], [5.0], 1.0), {}, "finite"), (([0.1], [1.0], [5.0], 0.0), {}, "dt_h"),
                           (([0.1], [1.0], [5.0], np.nan), {}, "dt_h"), (([0.1], [1.0], [5.0], -1.0), {}, "dt_h"),
                           (([0.1], [1.0], [5.0], "hour"), {}, "dt_h"), ((torch.tensor([0.1]), [1.0], [5.0], 1.0), {}, "fp64"),
                           ((["a"], [1.0], [5.0], 1.0), {}, "numbers")):
        with pytest.raises(LgarError, match=word):
            make(*args, **kw)
    # calls: shapes, dtypes, devices
    sim = SimCatchmentBaseflow([0.1, 0.05, 0.2], 2.0, [5.0, 6.0, 7.0], 1.0)
    x = torch.ones(4, 3, dtype=torch.float64)
    assert tuple(sim.run(x).shape) == (4, 3) and tuple(sim.state_of().shape) == (3,)
    for args in ((x[:, :2],), (x.float(),), (x.numpy(),), (x.to("meta"),), (x[0],), (x, True, None, x), (x, True, None, x[0].float())):
        with pytest.raises(LgarError, match=r"3\] tensor"):
            sim.run(*args)
    p = torch.ones(3, dtype=torch.float64)
    for call in (lambda: SimCatchmentBaseflow.function(x.float(), p, p, p, 1.0), lambda: SimCatchmentBaseflow.function(x, p[:2], p, p, 1.0),
                 lambda: SimCatchmentBaseflow.function(x, p.float(), p, p, 1.0), lambda: SimCatchmentBaseflow.function(x, p, "a", p, 1.0),
                 lambda: SimCatchmentBaseflow.function(x, p, p, p, 0.0), lambda: SimCatchmentBaseflow.function(x, p, p, p, 1.0, state=x),
                 lambda: SimCatchmentBaseflow.function(x, p, p, p.to("meta"), 1.0), lambda: SimCatchmentBaseflow.function(x[0], p, p, p, 1.0)):
        with pytest.raises(LgarError):
            call()
    # a store on the CPU holds the host logic only: the kernels have no CPU fallback
    cpu = make([0.1] * 3, [2.0] * 3, [5.0] * 3, 1.0)
    for call in (lambda: cpu.run(x), lambda: cpu.run(x, carry=False, storage=True), lambda: catchment_baseflow(x, p, p, p, 1.0)):
        with pytest.raises(LgarError, match="no CPU fallback"):
            call()


def test_entry_points_refuse_bad_arguments():
    """The refusals of the C-ABI wrappers (lgar_baseflow.hpp's own checks, which the host launchers call as the library does):
    LGAR_E_ARG = -1 for negative sizes, a dt_h that is not finite or <= 0, a null pointer the sizes say will be read or written,
    gpar or gstate wanted without s."""
    lib = BH.library()
    buf = np.ones(256)
    p = buf.ctypes.data
    T, B = 2, 4
    fwd = (("r", p), ("T", T), ("B", B), ("par", p), ("dt", 1.0), ("state_in", None), ("state_out", p + 512), ("q", p + 1024), ("s", p + 1536))
    run = lambda **kw: lib.baseflowhost_catchment_baseflow(*[kw.get(k, d) for k, d in fwd])
    assert run() == 0
    for bad in (dict(T=-1), dict(B=-1), dict(r=None), dict(par=None), dict(q=None), dict(dt=0.0), dict(dt=-1.0), dict(dt=float("nan")),
                dict(dt=float("inf")), dict(B=0, dt=0.0)):
        assert run(**bad) == -1, bad
    assert run(s=None) == 0 and run(state_out=None) == 0 and run(state_in=p) == 0
    assert run(B=0, r=None, par=None, q=None) == 0 and run(T=0, r=None, par=None, q=None) == 0 and run(T=0, r=None, q=None, state_out=None) == 0
    buf[64:68] = 7.0
    assert run(T=0, r=None, par=None, q=None, s=None) == 0 and buf[64:68].tolist() == [0.0] * 4  # T = 0, no state_in: zeros
    grd = (("gq", p), ("gs", p), ("r", p), ("s", p), ("T", T), ("B", B), ("par", p), ("dt", 1.0), ("state_in", None), ("gr", p + 512),
           ("gpar", p + 1024), ("gstate", p + 1536))
    grad = lambda **kw: lib.baseflowhost_catchment_baseflow_grad(*[kw.get(k, d) for k, d in grd])
    assert grad() == 0
    for bad in (dict(T=-1), dict(B=-1), dict(gq=None), dict(r=None), dict(s=None), dict(par=None), dict(gr=None), dict(dt=0.0),
                dict(dt=float("nan")), dict(dt=float("-inf")), dict(s=None, gpar=None), dict(s=None, gstate=None), dict(s=None, gpar=None, gstate=None)):
        assert grad(**bad) == -1, bad
    assert grad(gs=None) == 0 and grad(gpar=None) == 0 and grad(gstate=None) == 0 and grad(gpar=None, gstate=None) == 0
    assert grad(B=0, gq=None, r=None, s=None, par=None, gr=None) == 0
    buf[128:140] = 7.0
    buf[192:196] = 7.0
    assert grad(T=0, gq=None, gs=None, r=None, s=None, par=None, gr=None) == 0
    assert buf[128:140].tolist() == [0.0] * 12 and buf[192:196].tolist() == [0.0] * 4  # T = 0: gpar and gstate are zeros
    assert grad(T=0, gpar=None, gstate=None, gq=None, s=None) == 0
