"""CPU: the Muskingum-Cunge catchment network (lgar_network_route_mc / lgar_network_route_mc_grad, include/lgar.h; DESIGN.md
section 17).

The per-reach walks the GPU kernels run (lgar_py_amd/csrc/lgar_network_mc.hpp) are compiled for the host into a small stand-alone
program (tests/network_mc_host).  It is held BIT FOR BIT to the numpy statement of the definition (network_mc_host.route_mc_ref /
route_mc_grad_ref / mc_ln_ref); the same program built with AddressSanitizer + UBSan runs the same cases.  Independently of the
statement the definition is held to statements that do not come from it: beta = 0 to the linear route with torch's Muskingum
coefficients, mc_ln to mpmath.log, a steady flow to itself, and the adjoint to derivatives of the real-arithmetic statement
taken in mpmath.  The same header as a shared library stands behind lgar_py_amd.network.CatchmentNetwork
(network_mc_host.SimCatchmentNetworkMC overrides _open() only), so the host logic of route_mc / network_route_mc runs here too."""
import mpmath
import numpy as np
import pytest
import torch

import network_host as NH
import network_mc_host as MH
from network_mc_host import SimCatchmentNetworkMC

U = 2.0 ** -53  # unit roundoff of fp64
REGIMES = ("inside", "low", "low_negative", "high", "tau_pos", "tau_neg", "big", "tie_low", "tie_high")


def gamma(m):
    """Higham's gamma_m = m u / (1 - m u)."""
    return m * U / (1.0 - m * U)


LN_BOUND = gamma(9) + 7e-19  # mc_ln's relative error (derived in csrc/lgar_network_mc.hpp)
EXP_BOUND = gamma(29) * 2.0 ** 0.5 + 4.3e-18  # gw_exp's (derived in tests/test_baseflow_host.py)


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


# ---- 1. the host build against the numpy definition ------------------------------------------------------------------------
def _grid():
    """Every topology x T in {0, 1, 2, 7, 8, 9, 17} (the default range and the widest taking turns) x state_in present or NULL:
    the forward with and without state_out, the adjoint with gpar and gstate / gpar / gstate / neither.
    (cases, references, the count of rows per regime)."""
    rng = np.random.default_rng(17)
    cases, refs = [], []
    count = dict.fromkeys(REGIMES, 0)
    for name, down in NH.topologies().items():
        topo = NH.Topology(down)
        for i, T in enumerate(MH.SHAPE_T):
            x, gy, par, state, dt, rr = MH.case_data(rng, T, topo.B, wide=bool(i % 2))
            for st in (None, state):
                y, so = MH.route_mc_ref(topo, x, par, dt, *rr, st)
                for k, v in MH.regimes(topo, x, par, dt, *rr, st).items():
                    count[k] += v
                cases += [("route", topo, x, par, dt, rr, st, True), ("route", topo, x, par, dt, rr, st, False)]
                refs += [(y, so), (y, None)]
                gx, gpar, gstate = MH.route_mc_grad_ref(topo, gy, x, y, par, dt, *rr, st)
                for wp, ws in ((True, True), (True, False), (False, True), (False, False)):
                    cases.append(("grad", topo, gy, x, y, par, dt, rr, st, wp, ws))
                    refs.append((gx, gpar if wp else None, gstate if ws else None))
    return cases, refs, count


@pytest.fixture(scope="module")
def grid():
    return _grid()


def _check(cases, refs, got):
    assert len(got) == len(refs) == len(cases)
    for c, r, o in zip(cases, refs, got):
        for want, have in zip(r, o):
            assert (want is None) == (have is None), (c[0], c[1].B, np.asarray(c[2]).shape)
            assert want is None or MH.same_bits(have, want), (c[0], c[1].B, np.asarray(c[2]).shape)


def test_host_build_equals_the_numpy_definition_bit_for_bit(grid):
    cases, refs, count = grid
    _check(cases, refs, MH.run(cases))
    # every regime of the row is taken somewhere: inside; rho < rmin, also from a negative Oprev (mixed-sign x); rho > rmax; tau of
    # either sign; ta > ZMAX (a large beta, which the raw entry points take whatever the range); the exact ties
    print("rows per regime:", count)
    assert all(count[k] > 0 for k in REGIMES), count
    for c, r in zip(cases, refs):
        T = np.asarray(c[2]).shape[0]
        if c[0] == "route" and T == 0 and r[1] is not None:  # T = 0 copies the state, or writes zeros
            assert MH.same_bits(r[1], np.zeros((2, c[1].B)) if c[6] is None else np.asarray(c[6]))
        if c[0] == "grad" and T == 0:  # T = 0: zeros
            assert all(a is None or not a.any() for a in r)
    sizes = {c[1].B for c in cases}
    assert {1, 2, 63, 64, 65, 127, 257} <= sizes
    widths = {int(w) for c in cases for w in np.diff(c[1].level_ptr)}
    assert 64 in widths and 65 in widths and 256 in widths and max(c[1].n_levels for c in cases) == 65
    assert {np.asarray(c[2]).shape[0] for c in cases} == set(MH.SHAPE_T)


def test_sanitizer_build_on_the_same_cases(grid):
    """AddressSanitizer + UBSan build of the same program (a stand-alone executable: nothing is loaded into python; every array is
    allocated at its exact size) over the same cases: clean, with the same bits.  Any finding aborts the program."""
    cases, refs, _ = grid
    _check(cases, refs, MH.run(cases, sanitize=True))


def test_a_corrupt_topology_stays_inside_the_arrays():
    """order, up_idx and down far outside 0 .. B - 1, up_ptr outside 0 .. E and decreasing: the sanitizer build runs clean (wrong
    numbers, no access out of bounds -- every index read from device memory is clamped).  The forward does not read `down`: with
    only that array corrupt it still gives the definition's bits.  Host build only: this is never run on a GPU."""
    rng = np.random.default_rng(3)
    good = NH.Topology(NH.random_forest(65, 5))
    T, B = 9, good.B
    x, gy, par, state, dt, rr = MH.case_data(rng, T, B)
    y, _ = MH.route_mc_ref(good, x, par, dt, *rr, state)
    cases = []
    for field, values in (("order", (10 ** 6, -5, B)), ("up_idx", (10 ** 6, -5, B)), ("down", (10 ** 6, B, -7)),
                          ("up_ptr", (10 ** 6, -5, 2 ** 31 - 1))):
        bad = good.copy()
        arr = getattr(bad, field)
        arr[rng.permutation(len(arr))[:9]] = np.resize(np.array(values, dtype=np.int64), 9).astype(np.int32)
        cases += [("route", bad, x, par, dt, rr, state, True), ("grad", bad, gy, x, y, par, dt, rr, state, True, True),
                  ("grad", bad, gy, x, y, par, dt, rr, None, False, False)]
    bad = good.copy()
    bad.up_ptr = bad.up_ptr[::-1].copy()
    cases += [("route", bad, x, par, dt, rr, state, True), ("grad", bad, gy, x, y, par, dt, rr, state, True, True)]
    got = MH.run(cases, sanitize=True)
    assert len(got) == len(cases) and all(g[0].shape == (T, B) for g in got)
    assert MH.same_bits(got[6][0], y)  # corrupt `down` entries touch the adjoint only


# ---- 2. independent of the statement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(NH.topologies()))
def test_beta_zero_is_the_linear_route(name):
    """beta = 0: tau = 0, e = 1, K = kref exactly, and the row's coefficient formulas have the association of
    network.muskingum_coefficients: y equals lgar_network_route (tests/network_host's host build, and its numpy statement) with
    muskingum_coefficients(kref, X, dt_h) computed by torch on the CPU, bit for bit."""
    from lgar_py_amd.network import muskingum_coefficients
    topo = NH.Topology(NH.topologies()[name])
    net = SimCatchmentNetworkMC(topo.down)
    rng = np.random.default_rng(2900 + topo.B)
    for T in (9, 17):
        x, _, par, state, dt, rr = MH.case_data(rng, T, topo.B)
        par[1] = 0.0
        coef = muskingum_coefficients(_t(par[0]), _t(par[2]), dt)
        for st in (None, state):
            want = net.route(_t(x), coef, carry=False, state=_t(st))
            got = net.route_mc(_t(x), _t(par[0]), 0.0, _t(par[2]), _t(par[3]), dt, carry=False, state=_t(st))
            assert torch.equal(got, want) and float(got.abs().max()) > 0, (name, T)
            assert MH.same_bits(got.numpy(), NH.route_ref(topo, x, coef.numpy(), st)[0]), (name, T)
            assert MH.same_bits(got.numpy(), MH.route_mc_ref(topo, x, par, dt, *rr, st)[0]), (name, T)


def _ln_grid():
    rng = np.random.default_rng(14)
    pts = [2.0 ** rng.uniform(-60.0, 60.0, 4000), 1.0 + rng.uniform(-1e-3, 1e-3, 500), np.array([2.0 ** -60, 2.0 ** 60, 1.0, 1.0 / 64.0, 64.0])]
    brk = np.array([MH.SQRT_HALF * 2.0 ** k for k in range(-60, 61)])  # where the reduction switches
    pts += [brk, np.nextafter(brk, 0.0), np.nextafter(brk, np.inf), np.nextafter(1.0, 0.0).reshape(1), np.nextafter(1.0, 2.0).reshape(1)]
    v = np.unique(np.concatenate(pts))
    return v[(v >= 2.0 ** -60) & (v <= 2.0 ** 60)]


def test_mc_ln_against_mpmath():
    """mc_ln of the host build (and mc_ln_ref, the same bits) against mpmath.log at 40 digits over [2^-60, 2^60], the widest range
    rmin .. rmax may span: 4000 points log-uniform over it, 500 within 1e-3 of 1, the break points sqrt(1/2) 2^k with both
    neighbours, the neighbours of 1, the ends and the default rmin / rmax.  The bar is the bound derived in the header,
    gamma_9 + 7e-19 = 1.0e-15 relative (ln 1 = 0 must be exact).
    Measured: worst relative error 2.93 u (3.26e-16), 0.326 of the bound, over 4867 points."""
    v = _ln_grid()
    assert len(v) > 4800 and (np.abs(v - 1.0) < 1e-3).sum() >= 500
    (got,), = MH.run([("ln", v)])
    assert MH.same_bits(got, MH.mc_ln_ref(v))
    mpmath.mp.dps = 40
    worst = 0.0
    for xi, li in zip(v, got):
        want = mpmath.log(mpmath.mpf(float(xi)))
        if want == 0:
            assert li == 0.0
            continue
        worst = max(worst, float(abs(mpmath.mpf(float(li)) - want) / abs(want)))
    print("mc_ln vs mpmath.log: worst relative error %.3g = %.3g u, %.3g of the bound %.3g, %d points" % (worst, worst / U, worst / LN_BOUND, LN_BOUND, len(v)))
    assert worst <= LN_BOUND


def test_a_steady_flow_stays():
    """From state_in = (v, v) with constant inflow v on a single reach, y stays at v over 17 rows.  Variable-K Muskingum does NOT
    conserve volume exactly in transients (K changes between the row that stores and the row that releases), so no mass closure
    is asserted for them; what the row does keep is a steady flow, because c0 + c1 + c2 = 1 whatever K is.

    The bar, derived.  With the floats KX, u = fl(K - KX) and half the three numerators sum to u + half exactly, and
    D = fl(u + half) = (u + half)(1 + d): each numerator and each quotient round once, so |c0 + c1 + c2 - 1| <= u + gamma_2 S,
    S = |c0| + |c1| + |c2|, and S = c0 + c1 + c2 <= 1 + 3 u for the non-negative coefficients of these cases (asserted on the numpy
    statement).  O = (c0 I + c1 Ip) + c2 Op rounds each product once and passes at most two sums: with I = Ip = v and
    |Op - v| = d_(t-1), |O - v| <= |c2| d_(t-1) + (u + gamma_2 + gamma_3)(1 + 3 u) max(|v|, |Op|) <= d_(t-1) + gamma_7 |v| to first
    order: d_17 <= 17 gamma_7 |v|.
    Measured: worst miss / bound = 0.0168."""
    topo = NH.Topology(NH.single())
    T = 17
    cases, vs = [], []
    for v, kref, beta, X, qref, dt in ((1.0, 2.0, 0.4, 0.1, 1.7, 1.0), (0.37, 3.0, 0.6, 0.05, 0.1, 1.0), (123.456, 1.0, 0.4, 0.2, 500.0, 1.0),
                                       (3.3e-4, 0.2, 0.9, 0.02, 1.0, 2.0), (7.7, 2.0, 0.0, 0.1, 1.0, 1.0)):
        par = np.array([[kref], [beta], [X], [qref]])
        x, state = np.full((T, 1), v), np.full((2, 1), v)
        r = MH._row(np.array([v]), *par, 0.5 * dt, *MH.NARROW)
        assert min(r["c0"][0], r["c1"][0], r["c2"][0]) >= 0.0, (v, r)
        cases.append(("route", topo, x, par, dt, MH.NARROW, state, True))
        vs.append(v)
    worst = 0.0
    for v, (y, so) in zip(vs, MH.run(cases)):
        miss = float(np.abs(y - v).max())
        worst = max(worst, miss / (T * gamma(7) * v))
        assert miss <= T * gamma(7) * v and abs(so[1, 0] - v) <= T * gamma(7) * v and so[0, 0] == v, (v, miss)
    print("steady flow: worst miss / bound = %.3g" % worst)


# ---- 3. the same bits ---------------------------------------------------------------------------------------------------------
def test_chunked_repeated_and_relabelled_calls_give_the_same_bits():
    """One call against calls cut at 1 row, at T - 1 rows and in the middle (carry=True keeps the [2, B] state per key, in a key
    space of its own), from zeros and from a given state; a repeated call; reset(); an order-preserving relabelling into a
    larger network gives the relabelled bits, forward and adjoint."""
    rng = np.random.default_rng(23)
    topo = NH.Topology(NH.random_forest(65, 12))
    T, B = 17, topo.B
    x, gy, par, state, dt, rr = MH.case_data(rng, T, B)
    net = SimCatchmentNetworkMC(topo.down)
    tx, tp = _t(x), [_t(p) for p in par]
    for st in (None, state):
        want, want_state = MH.route_mc_ref(topo, x, par, dt, *rr, st)
        y = net.route_mc(tx, *tp, dt, carry=False, state=_t(st))
        assert MH.same_bits(y.numpy(), want) and net.mc_state_of() is None
        assert torch.equal(net.route_mc(tx, *tp, dt, carry=False, state=_t(st)), y)
        for cut in (1, T - 1, T // 2):
            key = ("cut", cut, st is None)
            a = net.route_mc(tx[:cut], *tp, dt, key=key, state=_t(st))
            b = net.route_mc(tx[cut:], *tp, dt, key=key)
            assert MH.same_bits(torch.cat([a, b]).numpy(), want) and MH.same_bits(net.mc_state_of(key).numpy(), want_state), cut
            assert tuple(net.route_mc(tx[:0], *tp, dt, key=key).shape) == (0, B) and MH.same_bits(net.mc_state_of(key).numpy(), want_state)
            assert net.state_of(key) is None  # the linear route's keys are another space
    net.reset()
    assert net.mc_state_of(("cut", 1, True)) is None
    M = 100
    down2, slots = MH.embed(rng, topo, M)
    x2, gy2, par2, state2, _, _ = MH.case_data(rng, T, M)
    x2[:, slots], gy2[:, slots], par2[:, slots], state2[:, slots] = x, gy, par, state
    topo2 = NH.Topology(down2)
    want, want_state = MH.route_mc_ref(topo, x, par, dt, *rr, state)
    (y2, so2), = MH.run([("route", topo2, x2, par2, dt, rr, state2, True)])
    assert MH.same_bits(y2[:, slots], want) and MH.same_bits(so2[:, slots], want_state)
    got, = MH.run([("grad", topo2, gy2, x2, y2, par2, dt, rr, state2, True, True)])
    ref = MH.route_mc_grad_ref(topo, gy, x, want, par, dt, *rr, state)
    assert all(MH.same_bits(a[:, slots], b) for a, b in zip(got, ref))


def test_a_nan_reaches_exactly_its_downstream_closure_from_its_row_on():
    rng = np.random.default_rng(41)
    topo = NH.Topology(NH.random_forest(65, 3))
    T, B = 9, topo.B
    x, _, par, state, dt, rr = MH.case_data(rng, T, B)
    clean, _ = MH.route_mc_ref(topo, x, par, dt, *rr, state)
    b = int(topo.order[0])
    while topo.down[b] < 0 or topo.down[topo.down[b]] < 0:  # a headwater with two reaches below it
        b = int(topo.order[list(topo.order).index(b) + 1])
    t0 = 4
    x[t0, b] = np.nan
    (y, so), = MH.run([("route", topo, x, par, dt, rr, state, True)])
    hit = np.zeros((T, B), dtype=bool)
    hit[t0:, topo.closure()[:, b]] = True
    assert hit[t0].sum() >= 3 and not hit[:t0].any()
    assert (np.isnan(y) == hit).all() and MH.same_bits(y[~hit], clean[~hit])
    assert (np.isnan(so[1]) == hit[-1]).all()


# ---- 4. the adjoint is the true derivative ------------------------------------------------------------------------------------
def _derivative_data():
    """B = 7, T = 9, dt_h = 1, the default range: a random forest of three levels or more; ordinary reaches whose rho stays inside
    (0, 1, 3, 4, 6), a reach with a large qref (2: rho < rmin in every row) and one with a tiny qref (5: rho > rmax)."""
    rng = np.random.default_rng(77)
    T, B = 9, 7
    topo = NH.Topology(NH.random_forest(B, 4, roots=0.0))
    kref = np.array([2.0, 1.5, 0.4, 2.2, 1.0, 3.0, 1.8]) * (1.0 + 0.1 * rng.random(B))
    beta = rng.uniform(0.3, 0.6, B)
    X = rng.uniform(0.03, 0.08, B)
    qref = np.array([2.0, 2.0, 1e3, 2.0, 2.0, 1e-3, 2.0]) * (1.0 + 0.1 * rng.random(B))
    x = 0.5 + 1.5 * rng.random((T, B))
    state = 0.5 + 1.5 * rng.random((2, B))
    gy = (rng.random((T, B)) - 0.4) * 2.0
    return topo, x, gy, np.stack([kref, beta, X, qref]), state, 1.0, MH.NARROW


def _mp_network(topo, x, par, state, gy, dt, rmin, rmax, detail=False):
    """The definition in REAL arithmetic (mpmath at the working precision; ln and exp are mpmath's): the loss sum gy y and, with
    detail, per (t, b) the row's I, Ip, Op, rho, L, tau, K, D, c0, c1, c2 and regime."""
    T, B = len(x), topo.B
    M = mpmath.mpf
    half, zmax = dt / 2, M(MH.ZMAX)
    y = [[None] * B for _ in range(T)]
    rows, loss = {}, M(0)
    for b in (int(v) for v in topo.order):
        kref, beta, X, qref = (par[k][b] for k in range(4))
        Ip, Op = state[0][b], state[1][b]
        for t in range(T):
            I = x[t][b]
            for u in topo.ups[b]:
                I = I + y[t][u]
            rho = Op / qref
            lo, hi = rho < rmin, rho > rmax
            rc = rmin if lo else (rmax if hi else rho)
            L = mpmath.log(rc)
            tau = beta * L
            big = abs(tau) > zmax
            K = kref * mpmath.exp(-(mpmath.sign(tau) * zmax if big else tau))
            KX = K * X
            uu = K - KX
            D = uu + half
            c0, c1, c2 = (half - KX) / D, (half + KX) / D, (uu - half) / D
            O = c0 * I + c1 * Ip + c2 * Op
            y[t][b] = O
            loss += gy[t][b] * O
            if detail:
                rows[t, b] = dict(I=I, Ip=Ip, Op=Op, O=O, rho=rho, L=L, tau=tau, K=K, D=D, c0=c0, c1=c1, c2=c2, lo=lo, hi=hi, big=big,
                                  inside=not (lo or hi or big), X=X, beta=beta, kref=kref)
            Ip, Op = I, O
    return (loss, rows) if detail else loss


@pytest.fixture(scope="module")
def derivative():
    """The data of the derivative tests, the derivatives of the real-arithmetic statement by central differences in mpmath, the
    adjoint on absolute values and the operation counts m (test_the_adjoint_is_the_true_derivative has the derivation)."""
    mpmath.mp.dps = 60
    topo, x, gy, par, state, dt, (rmin, rmax) = _derivative_data()
    T, B = x.shape
    assert topo.n_levels >= 3 and topo.E == B - 1
    M = mpmath.mpf
    mp2 = lambda a: [[M(float(v)) for v in row] for row in a]
    X0, P0, S0, G = mp2(x), mp2(par), mp2(state), mp2(gy)
    net = lambda xx, pp, ss, **kw: _mp_network(topo, xx, pp, ss, G, M(dt), M(rmin), M(rmax), **kw)
    _, rows = net(X0, P0, S0, detail=True)
    # the float walk takes the real walk's branches, and no row lies within a relative 1e-6 of a regime switch -- both walks
    flt = {k: np.zeros((T, B), dtype=(bool if k in ("lo", "hi", "big") else np.float64)) for k in ("rho", "tau", "lo", "hi", "big")}
    MH._walk(topo, x, par, dt, rmin, rmax, state, flt)
    margin = np.inf
    for (t, b), r in rows.items():
        assert (bool(r["lo"]), bool(r["hi"]), bool(r["big"])) == (flt["lo"][t, b], flt["hi"][t, b], flt["big"][t, b]), (t, b)
        for rho, tau in ((float(r["rho"]), float(r["tau"])), (flt["rho"][t, b], flt["tau"][t, b])):
            margin = min(margin, abs(rho - rmin) / rmin, abs(rho - rmax) / rmax, abs(abs(tau) - MH.ZMAX) / MH.ZMAX)
    assert margin > 1e-6, margin
    # central differences, h = 1e-20 |x|
    h = M(10) ** -20
    want = dict(gx=[[None] * B for _ in range(T)], gpar=[[None] * B for _ in range(3)], gstate=[[None] * B for _ in range(2)])
    for name, base, n in (("gx", X0, T), ("gpar", P0, 3), ("gstate", S0, 2)):
        for i in range(n):
            for b in range(B):
                v = base[i][b]
                assert v != 0
                vals = []
                for sgn in (1, -1):
                    base[i][b] = v + sgn * h * abs(v)
                    vals.append(net(X0, P0, S0))
                base[i][b] = v
                want[name][i][b] = (vals[0] - vals[1]) / (2 * h * abs(v))
    # the forward error figure: the linearised forward on absolute values, in units of u
    n_loc = max(float(r["beta"] * (LN_BOUND / U * abs(r["L"]) + 2) + abs(r["tau"]) + EXP_BOUND / U + 1) for r in rows.values())
    dy, di, delta, kappa = {}, {}, 0.0, 0.0
    for b in (int(v) for v in topo.order):
        for t in range(T):
            r = rows[t, b]
            omx, KD = 1 - r["X"], r["K"] / r["D"]
            parts = ((r["X"] + abs(r["c0"]) * omx) * KD, (r["X"] + abs(r["c1"]) * omx) * KD, omx * (1 + abs(r["c2"])) * KD)
            A = abs(r["c0"] * r["I"]) + abs(r["c1"] * r["Ip"]) + abs(r["c2"] * r["Op"])
            W = parts[0] * abs(r["I"]) + parts[1] * abs(r["Ip"]) + parts[2] * abs(r["Op"])
            di[t, b] = sum(dy[t, u] for u in topo.ups[b]) + len(topo.ups[b]) * (abs(X0[t][b]) + sum(abs(rows[t, u]["O"]) for u in topo.ups[b]))
            g = abs(r["c2"]) + (W * r["beta"] / abs(r["Op"]) if r["inside"] else 0)
            dy[t, b] = 11 * A + (n_loc + 6) * W + g * dy.get((t - 1, b), 0) + abs(r["c0"]) * di[t, b] + abs(r["c1"]) * di.get((t - 1, b), 0)
            delta = max(delta, float(dy[t, b] / abs(r["O"])), float(di[t, b] / abs(r["I"])))
            kappa = max(kappa, *(float(p / abs(c)) for p, c in zip(parts, (r["c0"], r["c1"], r["c2"]))))
    Lmax, Z, bmax = (max(float(abs(r[k])) for r in rows.values()) for k in ("L", "tau", "beta"))
    n_K = bmax * (LN_BOUND / U * Lmax + 2.0 + delta) + Z + EXP_BOUND / U + 1.0
    n_f = kappa * n_K + delta + 12.0
    m_gx = int(np.ceil((T + topo.n_levels) * (2.0 * n_f + n_K + delta + 8.0)))
    m = dict(gx=m_gx, gstate=m_gx, gpar=int(np.ceil(m_gx + 2.0 * n_f + n_K + LN_BOUND / U + T + 8.0)))
    # the adjoint on absolute values
    mag = dict(gx=[[None] * B for _ in range(T)], gpar=[[None] * B for _ in range(3)], gstate=[[None] * B for _ in range(2)])
    for b in (int(v) for v in topo.order[::-1]):
        pI, pO, acc = M(0), M(0), [M(0)] * 3
        for t in range(T - 1, -1, -1):
            r = rows[t, b]
            omx, KD = 1 - r["X"], r["K"] / r["D"]
            lam = abs(G[t][b]) + (mag["gx"][t][int(topo.down[b])] if topo.down[b] >= 0 else 0) + pO
            mag["gx"][t][b] = abs(r["c0"]) * lam + pI
            dK = ((r["X"] + abs(r["c0"]) * omx) * abs(r["I"]) + (r["X"] + abs(r["c1"]) * omx) * abs(r["Ip"]) + omx * (1 + abs(r["c2"])) * abs(r["Op"])) / r["D"]
            dX = ((1 + abs(r["c0"])) * abs(r["I"]) + (1 + abs(r["c1"])) * abs(r["Ip"]) + (1 + abs(r["c2"])) * abs(r["Op"])) * KD
            GK = lam * dK
            acc[0] += GK * r["K"] / r["kref"]
            if not r["big"]:
                acc[1] += GK * r["K"] * abs(r["L"])
            acc[2] += lam * dX
            pI = abs(r["c1"]) * lam
            pO = abs(r["c2"]) * lam + (GK * r["beta"] * r["K"] / abs(r["Op"]) if r["inside"] else 0)
        mag["gstate"][0][b], mag["gstate"][1][b] = pI, pO
        for k in range(3):
            mag["gpar"][k][b] = acc[k]
    cond = dict(margin=float(margin), n_loc=n_loc, delta=delta, kappa=kappa, Lmax=Lmax, Z=Z, n_K=n_K, n_f=n_f)
    return dict(data=(topo, x, gy, par, state, dt, (rmin, rmax)), want=want, mag=mag, m=m, cond=cond, rows=rows)


def _ratios(d, got):
    """per output, error / bound of every element against the mpmath derivative (inf where the bound is 0 and the error is not)"""
    out = {}
    for k, arr in zip(("gx", "gpar", "gstate"), got):
        r = np.zeros(arr.shape)
        for i in range(arr.shape[0]):
            for j in range(arr.shape[1]):
                err, bar = abs(mpmath.mpf(float(arr[i, j])) - d["want"][k][i][j]), mpmath.mpf(gamma(d["m"][k])) * d["mag"][k][i][j]
                r[i, j] = float(err / bar) if bar else (0.0 if err == 0 else np.inf)
        out[k] = r
    return out


def test_the_adjoint_is_the_true_derivative(derivative):
    """gx, gpar and gstate of the host build against the derivatives of L = sum gy y of the definition's REAL-arithmetic statement
    over the whole network, taken in mpmath at 60 digits by central differences with h = 1e-20 |x| (the quotient misses the
    derivative by h^2 L''' / 6 ~ 1e-40: L is smooth between regime switches, and no row lies within a relative 1e-6 of one --
    asserted on the numpy statement and on the real walk, the float walk taking the real walk's branch in every row).  B = 7,
    T = 9, a random forest; rows inside, clamped low and clamped high all occur (asserted).

    The bound is gamma_m x (the same adjoint on absolute values: |gy|, |c_i|, the three terms of dK and dX each by its absolute
    value, |beta K / Op|), with the errors of mc_ln and gw_exp counted inside m.  Derivation, to first order in u, with figures
    taken from the real-arithmetic walk (never from the code under test):
      K of a row.  rho rounds once; rc carries the forward error of Oprev, delta u relatively (inside rows; a clamped rc is exact).
        L = mc_ln(rc) is off by (E_ln |L| + 1 + delta) u absolutely (E_ln = (gamma_9 + 7e-19) / u, the header's bound), tau = beta L
        by beta times that plus |tau| u; e = gw_exp(|tau|) turns the absolute error of tau into a relative one and adds
        E_exp = (gamma_29 e^(ln2/2) + 4.3e-18) / u; kref / e or kref e rounds once:
        n_K = beta (E_ln |L| + 2 + delta) + |tau| + E_exp + 1, with the largest beta, |L| and |tau| of the walk; n_loc is n_K
        without delta (what one row adds by itself).
      forward.  A row's own error of O is at most (11 A + (n_loc + 6) W) u: A = |c0 I| + |c1 Ip| + |c2 Op| (five roundings of the
        recurrence and six of the coefficients' own operations relative to their terms), W = the terms of K |dO / dK| by absolute
        value (what a relative error of K does to O, and what the cancelling numerators half - KX and u - half lose).  The error
        of Oprev is handed on with |c2| + W beta / |Op| (the second term through K, inside rows only), that of the inflow with
        |c0| and |c1|; the inflow collects the errors of the upstream discharges and deg roundings of its fold.  This recurrence
        is run on the real walk; delta = the largest resulting error / u relative to |O| or |I|.
      a factor of the adjoint row -- c_i, one of the three terms of dK or of dX -- is its real value at the real walk's point but
        for n_f u relatively: n_f = kappa n_K + delta + 12, kappa = the largest K |dc_i / dK| / |c_i| with the terms by absolute
        value (how a relative error of K shows in a coefficient), delta for the I, Ip or Op in it, 12 for its own operations.
        The product GK dK/dO = lam dK (beta K / Op) holds two such factors, K again and Op.  A path of the expansion of gx
        passes a row at most once and at most T + n_levels rows: m_gx = (T + n_levels)(2 n_f + n_K + delta + 8); gstate is gx of a
        row before row 0.  A term of gpar is lam (<= m_gx) times one more factor, K, kref or L (E_ln), added into an accumulator
        <= T times: m_gpar = m_gx + 2 n_f + n_K + E_ln + T + 8.
    m is dominated by delta, the forward error handed down the network and on from row to row, through kappa n_K: the
    bound is of the order 1e-10 relative to the absolute-value adjoint, far above the measured error and far below a wrong
    formula: it refuses, on every output the change reaches, the GK dK/dO term dropped (gx, gpar, gstate), c1 of row t where c1 of
    row t + 1 belongs (gx, and gpar and gstate of the reaches upstream) and gbeta with the wrong sign (gpar).
    Measured: worst error / bound = 1.9e-06 (gx), 6.2e-08 (gpar), 4.72e-07 (gstate), with m = 861556 (gx, gstate), 919174 (gpar);
    delta = 8674, kappa = 3.75, n_K = 4727, n_f = 26432, the nearest regime switch at a relative 0.92."""
    topo, x, gy, par, state, dt, rr = derivative["data"]
    rows = derivative["rows"]
    assert sum(r["inside"] for r in rows.values()) > 30 and sum(bool(r["lo"]) for r in rows.values()) == 9 and sum(bool(r["hi"]) for r in rows.values()) == 9
    y, _ = MH.route_mc_ref(topo, x, par, dt, *rr, state)
    got, = MH.run([("grad", topo, gy, x, y, par, dt, rr, state, True, True)])
    assert all(MH.same_bits(a, b) for a, b in zip(got, MH.route_mc_grad_ref(topo, gy, x, y, par, dt, *rr, state)))
    rt = _ratios(derivative, got)
    print("MC adjoint vs mpmath derivative: worst error / bound = %.3g (gx), %.3g (gpar), %.3g (gstate); m = %r; %r"
          % (rt["gx"].max(), rt["gpar"].max(), rt["gstate"].max(), derivative["m"], derivative["cond"]))
    assert all(v.max() <= 1.0 for v in rt.values())
    assert all(v.max() > 0 for v in rt.values())  # (the data are general: something does round)
    for variant, reached in (("no_gk", ("gx", "gpar", "gstate")), ("c1_now", ("gx", "gpar", "gstate")), ("gbeta_sign", ("gpar",))):
        wrong = _ratios(derivative, MH.route_mc_grad_ref(topo, gy, x, y, par, dt, *rr, state, variant=variant))
        assert all(wrong[k].max() > 1.0 for k in reached), (variant, {k: v.max() for k, v in wrong.items()})
        assert all(wrong[k].max() <= 1.0 for k in wrong if k not in reached), variant


# ---- 5. autograd --------------------------------------------------------------------------------------------------------------
def test_autograd_through_the_host_build(derivative):
    """network_route_mc on a CatchmentNetwork whose _open() alone is overridden (the host build in the library's place), on the
    data of the derivative test: x, kref, beta, X and state receive the bits of route_mc_grad_ref from one backward; qref gets
    none.  Scalar parameters receive the sum over the reaches; a state that requires no gradient gets none."""
    from lgar_py_amd.network import network_route_mc
    topo, x, gy, par, state, dt, rr = derivative["data"]
    net = SimCatchmentNetworkMC(topo.down)
    leaf = lambda a: _t(a).clone().requires_grad_(True)
    tx, tk, tb, tX, ts = leaf(x), leaf(par[0]), leaf(par[1]), leaf(par[2]), leaf(state)
    tq = leaf(par[3])
    y = network_route_mc(tx, net, tk, tb, tX, tq, dt, state=ts)
    y_ref, _ = MH.route_mc_ref(topo, x, par, dt, *rr, state)
    assert MH.same_bits(y.detach().numpy(), y_ref)
    (y * _t(gy)).sum().backward()
    gx, gpar, gstate = MH.route_mc_grad_ref(topo, gy, x, y_ref, par, dt, *rr, state)
    assert MH.same_bits(tx.grad.numpy(), gx) and MH.same_bits(np.stack([tk.grad.numpy(), tb.grad.numpy(), tX.grad.numpy()]), gpar)
    assert MH.same_bits(ts.grad.numpy(), gstate) and tq.grad is None
    assert float(np.abs(gpar).min()) > 0 and float(np.abs(gstate).min()) > 0
    # scalar parameters: summed gradients; a constant state; another range
    sk, sb = torch.tensor(1.7, dtype=torch.float64, requires_grad=True), torch.tensor(0.4, dtype=torch.float64, requires_grad=True)
    tx2 = leaf(x)
    y2 = network_route_mc(tx2, net, sk, sb, 0.1, 2.0, dt, rmin=0.25, rmax=4.0, state=_t(state))
    (y2 * _t(gy)).sum().backward()
    par2 = np.stack([np.full(7, 1.7), np.full(7, 0.4), np.full(7, 0.1), np.full(7, 2.0)])
    y2_ref, _ = MH.route_mc_ref(topo, x, par2, dt, 0.25, 4.0, state)
    g2 = MH.route_mc_grad_ref(topo, gy, x, y2_ref, par2, dt, 0.25, 4.0, state)
    assert MH.same_bits(y2.detach().numpy(), y2_ref) and MH.same_bits(tx2.grad.numpy(), g2[0])
    assert MH.same_bits(sk.grad.numpy().reshape(1), _t(g2[1][0]).sum().numpy().reshape(1))
    assert MH.same_bits(sb.grad.numpy().reshape(1), _t(g2[1][1]).sum().numpy().reshape(1))
    with torch.no_grad():
        assert MH.same_bits(network_route_mc(_t(x), net, _t(par[0]), _t(par[1]), _t(par[2]), _t(par[3]), dt).numpy(),
                            MH.route_mc_ref(topo, x, par, dt, *rr)[0])


# ---- 6. host logic ------------------------------------------------------------------------------------------------------------
def test_python_layer_names_and_rejections():
    import lgar_py_amd as lg
    from lgar_py_amd import LgarError, _capi
    from lgar_py_amd.network import CatchmentNetwork, manning_reach_parameters, network_route_mc
    assert lg.network_route_mc is network_route_mc and lg.manning_reach_parameters is manning_reach_parameters
    assert {"network_route_mc", "manning_reach_parameters"} <= set(lg.__all__)
    assert _capi.ABI_VERSION == 4 and {"lgar_network_route_mc", "lgar_network_route_mc_grad"} <= set(_capi.EXPORTS)
    net = SimCatchmentNetworkMC([1, 2, -1])
    x = torch.ones(4, 3, dtype=torch.float64)
    p = torch.ones(3, dtype=torch.float64)
    assert tuple(net.route_mc(x, p, 0.4, 0.2, p, 1.0).shape) == (4, 3) and tuple(net.mc_state_of().shape) == (2, 3)
    ok = dict(kref=p, beta=0.4, X=0.2, qref=1.0, dt_h=1.0)
    for change, word in ((dict(kref=0.0), "kref"), (dict(kref=-p), "kref"), (dict(kref=float("nan")), "finite"), (dict(beta=-0.1), "beta"),
                         (dict(beta=float("inf")), "finite"), (dict(X=0.6), "X"), (dict(X=-0.1), "X"), (dict(qref=0.0), "qref"),
                         (dict(qref=torch.tensor([1.0, -1.0, 1.0], dtype=torch.float64)), r"qref\[1\]"), (dict(dt_h=0.0), "dt_h"),
                         (dict(dt_h=float("nan")), "dt_h"), (dict(dt_h="hour"), "numbers"), (dict(rmin=0.0), "rmin"), (dict(rmax=2.0 ** 61), "rmin"),
                         (dict(rmin=8.0, rmax=4.0), "rmin"), (dict(rmin=float("nan")), "rmin"), (dict(kref=p[:2]), r"fp64 \[3\]"),
                         (dict(kref=p.float()), r"fp64 \[3\]"), (dict(beta="a"), "scalar"), (dict(X=p.to("meta")), r"fp64 \[3\]")):
        with pytest.raises(LgarError, match=word):
            net.route_mc(x, **dict(ok, **change))
    for bad in (x[:, :2], x.float(), x.numpy(), x[0]):
        with pytest.raises(LgarError, match=r"3\] tensor"):
            net.route_mc(bad, **ok)
    with pytest.raises(LgarError, match=r"\[2, 3\]"):
        net.route_mc(x, state=x, **ok)
    # the differentiable entry: no value validation (beta < 0 runs), shapes and the network are checked
    assert tuple(network_route_mc(x, net, p, -0.1, 0.2, p, 1.0).shape) == (4, 3)
    for call in (lambda: network_route_mc(x, "net", p, 0.4, 0.2, p, 1.0), lambda: network_route_mc(x.float(), net, p, 0.4, 0.2, p, 1.0),
                 lambda: network_route_mc(x, net, p[:2], 0.4, 0.2, p, 1.0), lambda: network_route_mc(x, net, p, 0.4, 0.2, p, 0.0),
                 lambda: network_route_mc(x, net, p, 0.4, 0.2, p, 1.0, rmin=0.0), lambda: network_route_mc(x, net, p, 0.4, 0.2, p, 1.0, state=x)):
        with pytest.raises(LgarError):
            call()
    # a network on the CPU holds the host logic only: the kernels have no CPU fallback
    cpu = CatchmentNetwork([1, 2, -1], device="cpu")
    for call in (lambda: cpu.route_mc(x, **ok), lambda: network_route_mc(x, cpu, p, 0.4, 0.2, p, 1.0)):
        with pytest.raises(LgarError, match="no CPU fallback"):
            call()


def test_manning_reach_parameters():
    """kref = length / (3600 (5/3) n^(-3/5) S^(3/10) W^(-2/5) Q^(2/5)) against the same formula in mpmath, beta = 0.4; differentiable;
    kref falls as qref^(-2/5), so the routing's K = kref (Q / qref)^(-beta) does not depend on the qref chosen."""
    from lgar_py_amd.network import manning_reach_parameters
    length, slope, n, width, qref = 12000.0, 0.002, 0.035, 25.0, 40.0
    kref, beta = manning_reach_parameters(length, slope, n, width, qref)
    mpmath.mp.dps = 40
    M = mpmath.mpf
    c = M(5) / 3 * M(n) ** (M(-3) / 5) * M(slope) ** (M(3) / 10) * M(width) ** (M(-2) / 5) * M(qref) ** (M(2) / 5)
    assert abs(float(kref) - float(M(length) / (3600 * c))) <= 1e-13 * float(kref) and float(beta) == 0.4 and kref.dtype == torch.float64
    assert 1.0 < float(kref) < 3.0  # 12 km at about 1.9 m/s
    L = torch.tensor([12000.0, 5000.0], dtype=torch.float64, requires_grad=True)
    k2, b2 = manning_reach_parameters(L, slope, n, torch.tensor([25.0, 10.0], dtype=torch.float64), qref)
    k2.sum().backward()
    assert tuple(k2.shape) == (2,) and b2.tolist() == [0.4, 0.4] and torch.allclose(L.grad, k2.detach() / L.detach())
    k3, _ = manning_reach_parameters(length, slope, n, width, 4.0 * qref)
    assert abs(float(k3) * 4.0 ** 0.4 / float(kref) - 1.0) < 1e-14


def test_entry_points_refuse_bad_arguments():
    """The refusals of the C-ABI wrappers (lgar_network_mc.hpp's own checks, which the host launchers call as the library does):
    LGAR_E_ARG = -1 for everything lgar_network_route refuses, a dt_h that is not finite or <= 0, rmin / rmax not finite or outside
    2^-60 <= rmin <= rmax <= 2^60, a null par, the adjoint's null x, y, up_ptr, gx, down, or a null up_idx with E > 0."""
    lib = MH.library()
    buf = np.ones(256)
    ibuf = np.zeros(16, dtype=np.int32)
    p, q = buf.ctypes.data, ibuf.ctypes.data
    level_ptr, bad_levels = np.array([0, 4], dtype=np.int32), np.array([0, 3], dtype=np.int32)
    fwd = (("x", p), ("T", 2), ("B", 4), ("par", p), ("dt", 1.0), ("rmin", 1 / 64), ("rmax", 64.0), ("up_ptr", q), ("up_idx", q), ("E", 1),
           ("order", q), ("level_ptr", level_ptr.ctypes.data), ("L", 1), ("state_in", None), ("state_out", p + 512), ("y", p + 1024))
    run = lambda **kw: lib.networkmchost_network_route_mc(*[kw.get(k, d) for k, d in fwd])
    assert run() == 0
    nan, inf = float("nan"), float("inf")
    scalars = (dict(dt=0.0), dict(dt=-1.0), dict(dt=nan), dict(dt=inf), dict(rmin=nan), dict(rmax=nan), dict(rmax=inf), dict(rmin=-inf),
               dict(rmin=2.0 ** -61), dict(rmax=2.0 ** 61), dict(rmin=65.0), dict(rmin=0.0), dict(B=0, dt=0.0))
    for bad in (dict(T=-1), dict(B=-1), dict(E=-1), dict(L=-1), dict(x=None), dict(par=None), dict(T=0, par=None), dict(y=None), dict(up_ptr=None), dict(up_idx=None),
                dict(order=None), dict(level_ptr=None), dict(level_ptr=bad_levels.ctypes.data)) + scalars:
        assert run(**bad) == -1, bad
    assert run(rmin=2.0 ** -60, rmax=2.0 ** 60) == 0 and run(rmin=3.0, rmax=3.0) == 0 and run(E=0, up_idx=None) == 0
    assert run(B=0, x=None, par=None, y=None, level_ptr=None) == 0 and run(T=0, state_out=None, x=None, y=None) == 0
    buf[64:72] = 7.0
    assert run(T=0, x=None, y=None) == 0 and buf[64].tolist() == 0.0  # T = 0, no state_in: zeros (every lane is reach 0 here)
    grd = (("gy", p), ("T", 2), ("B", 4), ("par", p), ("dt", 1.0), ("rmin", 1 / 64), ("rmax", 64.0), ("down", q), ("order", q),
           ("level_ptr", level_ptr.ctypes.data), ("L", 1), ("gx", p + 512), ("x", p), ("y", p), ("up_ptr", q), ("up_idx", q), ("E", 1),
           ("state_in", None), ("gpar", p + 1024), ("gstate", p + 1536))
    grad = lambda **kw: lib.networkmchost_network_route_mc_grad(*[kw.get(k, d) for k, d in grd])
    assert grad() == 0
    for bad in (dict(T=-1), dict(B=-1), dict(E=-1), dict(L=-1), dict(gy=None), dict(par=None), dict(T=0, par=None), dict(down=None), dict(order=None), dict(gx=None),
                dict(x=None), dict(y=None), dict(up_ptr=None), dict(up_idx=None), dict(level_ptr=None), dict(level_ptr=bad_levels.ctypes.data),
                dict(x=None, gpar=None, gstate=None)) + scalars:
        assert grad(**bad) == -1, bad
    assert grad(gpar=None) == 0 and grad(gstate=None) == 0 and grad(gpar=None, gstate=None) == 0 and grad(E=0, up_idx=None) == 0
    assert grad(B=0, gy=None, gx=None, level_ptr=None) == 0 and grad(T=0, gpar=None, gstate=None, gy=None, x=None) == 0
    buf[128] = buf[192] = 7.0
    assert grad(T=0, gy=None, gx=None, x=None, y=None) == 0 and buf[128] == 0.0 and buf[192] == 0.0  # T = 0: zeros
