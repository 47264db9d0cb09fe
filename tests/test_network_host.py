"""CPU: the catchment network (lgar_network_route / lgar_network_route_grad, include/lgar.h).

The per-reach walks the GPU kernels run (lgar_py_amd/csrc/lgar_network.hpp) are compiled for the host into a small stand-alone
program (tests/network_host).  It is held BIT FOR BIT to the numpy statement of the definition (network_host.route_ref /
adjoint_ref / coef_grad_ref); the same program built with AddressSanitizer + UBSan runs the same cases, and a corrupt topology.
Independently of the recurrence the definition itself is held to exact statements: the upstream-closure matrix, the shifted
partial sums of a chain, and rational arithmetic (fractions.Fraction) for the forward, the adjoint and the coefficient
gradient.  The same header as a shared library stands behind lgar_py_amd.network.CatchmentNetwork
(network_host.SimCatchmentNetwork), so the host logic of network.py -- validation, levels, carry, autograd -- runs here too."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import network_host as NH
from network_host import SimCatchmentNetwork

U = 2.0 ** -53  # unit roundoff of fp64


def gamma(m):
    """Higham's gamma_m = m u / (1 - m u): (1 + d_1) .. (1 + d_m) = 1 + theta, |theta| <= gamma_m, for |d_i| <= u (3.1)."""
    return m * U / (1.0 - m * U)


# ---- 1. the host build against the numpy definition ------------------------------------------------------------------------
def _grid():
    """Every topology x T in {0, 1, 2, 7, 8, 9, 17} x the four coefficient sets x state_in present or NULL: a forward case (state
    wanted), an adjoint with the coefficient gradient and one without.  (cases, references)."""
    rng = np.random.default_rng(14)
    cases, refs = [], []
    for name, down in NH.topologies().items():
        topo = NH.Topology(down)
        for T in NH.SHAPE_T:
            for kind in NH.COEFS:
                x, gy, coef, state = NH.case_data(rng, T, topo.B, kind)
                for st in (None, state):
                    y, so = NH.route_ref(topo, x, coef, st)
                    gx = NH.adjoint_ref(topo, gy, coef)
                    cases += [("route", topo, x, coef, st, True), ("grad", topo, gy, coef, x, y, st), ("grad", topo, gy, coef, None, None, None)]
                    refs += [(y, so), (gx, NH.coef_grad_ref(topo, x, y, gy, coef, st)), (gx, None)]
    return cases, refs


@pytest.fixture(scope="module")
def grid():
    return _grid()


def _check(cases, refs, got):
    assert len(got) == len(refs) == len(cases)
    for c, r, o in zip(cases, refs, got):
        for want, have in zip(r, o):
            assert (want is None) == (have is None), (c[0], c[1].B)
            assert want is None or NH.same_bits(have, want), (c[0], c[1].B, np.asarray(c[2]).shape)


def test_host_build_equals_the_numpy_definition_bit_for_bit(grid):
    cases, refs = grid
    _check(cases, refs, NH.run(cases))
    # what the definition says about the corners, on the references themselves
    for c, r in zip(cases, refs):
        if c[0] == "route" and np.asarray(c[2]).shape[0] == 0:  # T = 0 copies the state, or writes zeros
            assert NH.same_bits(r[1], np.zeros((2, c[1].B)) if c[4] is None else np.asarray(c[4]))
    sizes = {c[1].B for c in cases}
    assert {1, 2, 63, 64, 65, 127, 257} <= sizes
    widths = {int(w) for c in cases for w in np.diff(c[1].level_ptr)}
    assert 64 in widths and 65 in widths and 256 in widths and max(c[1].n_levels for c in cases) == 65
    assert any((c[1].order != np.arange(c[1].B)).any() and (c[1].down > np.arange(c[1].B)).any()
               and ((c[1].down >= 0) & (c[1].down < np.arange(c[1].B))).any() for c in cases)


def test_sanitizer_build_on_the_same_cases(grid):
    """AddressSanitizer + UBSan build of the same program (a stand-alone executable: nothing is loaded into python; every array is
    allocated at its exact size) over the same cases: clean, with the same bits.  Any finding aborts the program."""
    cases, refs = grid
    _check(cases, refs, NH.run(cases, sanitize=True))


def test_a_corrupt_topology_stays_inside_the_arrays():
    """order, up_idx and down far outside 0 .. B - 1, up_ptr outside 0 .. E and decreasing: the sanitizer build runs clean (wrong
    numbers, no access out of bounds -- every index read from device memory is clamped).  The forward does not read `down`: with
    only that array corrupt it still gives the definition's bits.  Host build only: this is never run on a GPU."""
    rng = np.random.default_rng(3)
    good = NH.Topology(NH.random_forest(65, 5))
    T, B = 9, good.B
    x, gy, coef, state = NH.case_data(rng, T, B, "muskingum")
    y, _ = NH.route_ref(good, x, coef, state)
    cases = []
    for field, values in (("order", (10 ** 6, -5, B)), ("up_idx", (10 ** 6, -5, B)), ("down", (10 ** 6, B, -7)),
                          ("up_ptr", (10 ** 6, -5, 2 ** 31 - 1))):
        bad = good.copy()
        arr = getattr(bad, field)
        arr[rng.permutation(len(arr))[:9]] = np.resize(np.array(values, dtype=np.int64), 9).astype(np.int32)
        cases += [("route", bad, x, coef, state, True), ("grad", bad, gy, coef, x, y, state), ("grad", bad, gy, coef, None, None, None)]
    bad = good.copy()
    bad.up_ptr = bad.up_ptr[::-1].copy()
    cases += [("route", bad, x, coef, state, True), ("grad", bad, gy, coef, x, y, state)]
    got = NH.run(cases, sanitize=True)
    assert len(got) == len(cases) and all(g[0].shape == (T, B) for g in got)
    # corrupt `down` entries touch the adjoint only: the forward of that topology is still the definition's
    assert NH.same_bits(got[6][0], y)


# ---- 2. independent of the recurrence, and exact ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["chain65", "star257", "tree63", "forest65", "random64", "random257", "wide65"])
def test_accumulation_is_the_upstream_closure(name):
    """coef = (1, 0, 0) and small-integer x: every sum is exact, so y = x R^T bit for bit, R the upstream-closure matrix (b itself
    and everything upstream), built by repeated boolean matrix products -- no recurrence, no levels."""
    topo = NH.Topology(NH.topologies()[name])
    rng = np.random.default_rng(2)
    x = rng.integers(-9, 10, (9, topo.B)).astype(np.float64)
    net = SimCatchmentNetwork(topo.down)
    y = net.accumulate(torch.from_numpy(x)).numpy()
    R = topo.closure()
    assert R.sum() > topo.B or topo.E == 0
    assert NH.same_bits(y + 0.0, x @ R.T.astype(np.float64) + 0.0)  # (+ 0.0: an exact zero sum may carry either sign)
    (got, _), = NH.run([("route", topo, x, NH.coefficients(rng, "accumulate", topo.B), None, False)])
    assert NH.same_bits(got, y)


def test_a_chain_of_lags_is_the_shifted_partial_sums():
    """The chain with coef = (0, 1, 0): y[t][b] = I[t - 1][b] and I[t][b] = x[t][b] + y[t][b - 1], so
    y[t][b] = x[t - 1][b] + x[t - 2][b - 1] + ... : a diagonal partial sum, exact for small integers."""
    B, T = 65, 17
    topo = NH.Topology(NH.chain(B))
    rng = np.random.default_rng(6)
    x = rng.integers(-9, 10, (T, B)).astype(np.float64)
    want = np.zeros((T, B))
    for t in range(T):
        for b in range(B):
            want[t, b] = sum(x[t - 1 - k, b - k] for k in range(min(b, t - 1) + 1)) if t >= 1 else 0.0
    (got, _), = NH.run([("route", topo, x, NH.coefficients(rng, "lag", B), None, False)])
    assert NH.same_bits(got + 0.0, want + 0.0) and float(np.abs(got[:, B - 1]).max()) > 0


# ---- 3./4. rational arithmetic ----------------------------------------------------------------------------------------------
def exact(topo, x, coef, gy, state=None, seen=None, absolute=False):
    """y, gx, gc of the definition in fractions.Fraction from float inputs (each float is a rational number, exactly).
    seen: a list that receives every intermediate.  absolute: the same operator on the absolute values of x, coef, gy, state
    -- what the error bounds are multiples of."""
    F = (lambda v: abs(Fraction(float(v)))) if absolute else (lambda v: Fraction(float(v)))
    T, B = np.asarray(x).shape
    note = (lambda v: (seen.append(v), v)[1]) if seen is not None else (lambda v: v)
    X = [[F(x[t][b]) for b in range(B)] for t in range(T)]
    G = [[F(gy[t][b]) for b in range(B)] for t in range(T)]
    c = [[F(coef[k][b]) for b in range(B)] for k in range(3)]
    st = [[F(0 if state is None else state[k][b]) for b in range(B)] for k in range(2)]
    y = [[None] * B for _ in range(T)]
    I = [[None] * B for _ in range(T)]
    for b in [int(v) for v in topo.order]:
        Iprev, Oprev = st[0][b], st[1][b]
        for t in range(T):
            acc = X[t][b]
            for u in topo.ups[b]:
                acc = note(acc + y[t][u])
            O = note(note(note(c[0][b] * acc) + note(c[1][b] * Iprev)) + note(c[2][b] * Oprev))
            y[t][b], I[t][b], Iprev, Oprev = O, acc, acc, O
    gx = [[None] * B for _ in range(T)]
    gc = [[Fraction(0)] * B for _ in range(3)]
    for b in [int(v) for v in topo.order[::-1]]:
        lam_next = Fraction(0)
        for t in range(T - 1, -1, -1):
            a = G[t][b]
            if topo.down[b] >= 0:
                a = note(a + gx[t][topo.down[b]])
            lam = note(a + note(c[2][b] * lam_next))
            gx[t][b] = note(note(c[0][b] * lam) + note(c[1][b] * lam_next))
            gc[0][b] = note(gc[0][b] + note(lam * I[t][b]))
            gc[1][b] = note(gc[1][b] + note(lam * (I[t - 1][b] if t else st[0][b])))
            gc[2][b] = note(gc[2][b] + note(lam * (y[t - 1][b] if t else st[1][b])))
            lam_next = lam
    return y, gx, gc


def _floats(rows):
    return np.array([[float(v) for v in row] for row in rows], dtype=np.float64).reshape(len(rows), -1)


def _host(topo, x, coef, gy, state=None):
    """y, gx, gc of the host build"""
    (y, _), = NH.run([("route", topo, x, coef, state, False)])
    (gx, gc), = NH.run([("grad", topo, gy, coef, x, y, state)])
    return y, gx, gc


def test_the_definitions_adjoint_is_the_true_adjoint_exactly():
    """Coefficients that are multiples of 1/4, small-integer x, gy and state, B = 6, T = 5: y, gx and gc in rational arithmetic.
    The test first asserts that its data are exactly representable and that NO operation rounds (every Fraction intermediate
    converts to float and back unchanged), so the float results must equal the rational ones exactly.  The rational gx and gc
    are themselves held to the derivatives of L = sum(gy * y): L is linear in x, so L(x + unit impulse) - L(x) IS gx[t][b]; L is
    a polynomial in every coefficient, so the central difference (L(c + h) - L(c - h)) / 2h at h = 2^-20, in rational arithmetic,
    misses dL/dc by its cubic term only."""
    topo = NH.Topology([2, 2, 4, 4, 5, -1])
    T, B = 5, topo.B
    rng = np.random.default_rng(9)
    x = rng.integers(-3, 4, (T, B)).astype(np.float64)
    gy = rng.integers(-3, 4, (T, B)).astype(np.float64)
    state = rng.integers(-2, 3, (2, B)).astype(np.float64)
    coef = rng.integers(-2, 4, (3, B)).astype(np.float64) / 4.0
    assert topo.n_levels == 4 and (coef * 4 == np.round(coef * 4)).all() and float(np.abs(coef).max()) > 0.5
    seen = []
    y, gx, gc = exact(topo, x, coef, gy, state, seen=seen)
    assert len(seen) > 500 and all(Fraction(float(v)) == v for v in seen), "an operation of this case rounds"
    hy, hgx, hgc = _host(topo, x, coef, gy, state)
    assert NH.same_bits(hy + 0.0, _floats(y) + 0.0) and NH.same_bits(hgx + 0.0, _floats(gx) + 0.0) and NH.same_bits(hgc + 0.0, _floats(gc) + 0.0)
    assert float(np.abs(hgc).min(axis=1).max()) > 0 and float(np.abs(hgx).max()) > 0
    # the true adjoint: <gy, route(x + e) - route(x)> = gx[e] for every unit impulse e (linear: exact)
    loss = lambda yy: sum(Fraction(float(gy[t][b])) * yy[t][b] for t in range(T) for b in range(B))
    base = loss(y)
    for t in range(T):
        for b in range(B):
            xe = x.copy()
            xe[t, b] += 1.0
            assert loss(exact(topo, xe, coef, gy, state)[0]) - base == gx[t][b], (t, b)
    # the coefficient gradient: central difference in exact arithmetic, h = 2^-20; L is a polynomial of degree <= T + n_levels in
    # one coefficient with all else fixed, so the quotient misses dL/dc by O(h^2) times its third derivative
    h = 2.0 ** -20
    for k in range(3):
        for b in range(B):
            cp, cm = coef.copy(), coef.copy()
            cp[k, b] += h
            cm[k, b] -= h
            quot = (loss(exact(topo, x, cp, gy, state)[0]) - loss(exact(topo, x, cm, gy, state)[0])) / Fraction(2 * h)
            assert abs(quot - gc[k][b]) <= Fraction(1, 2 ** 24), (k, b, float(quot), float(gc[k][b]))


def _neighbour_down(topo):
    """down with every entry replaced by the neighbour of the old one in `order` inside its level, where it has one."""
    pos = np.empty(topo.B, dtype=np.int64)
    pos[topo.order] = np.arange(topo.B)
    down = topo.down.copy()
    for b in range(topo.B):
        d = topo.down[b]
        if d < 0:
            continue
        l = topo.level[d]
        lo, hi = topo.level_ptr[l], topo.level_ptr[l + 1]
        if hi - lo > 1:
            p = pos[d] + 1 if pos[d] + 1 < hi else pos[d] - 1
            down[b] = topo.order[p]
    return down


def test_general_data_against_the_exact_rational_result():
    """B = 7, T = 9, a random forest, Muskingum coefficients, general data: y, gx and gc of the host build against the EXACT
    rational result of the same float inputs.

    The bound is gamma_m x (the same operator applied to absolute values), gamma_m = m u / (1 - m u), u = 2^-53, m the count of
    rounded operations on the longest chain into that output.  Every output is a sum over paths of products of inputs; a
    computed value carries one factor (1 + d), |d| <= u, per rounded operation along its path, so it errs by at most gamma_m
    times the sum of the paths' absolute values (Higham 3.1, 3.4), which is the operator on |x|, |coef|, |gy|.
      y:  a path into y[t][b] walks the grid of (row, level): each step goes one row back in the same reach or to an upstream
          reach in the same row, at most T + n_levels cells; a cell costs at most maxdeg adds of the inflow fold, three
          products and two adds: m_y = (T + n_levels)(maxdeg + 5).
      gx: the same walk forward in time and downstream; a cell costs the add of gx[t][down], three products and two adds, and
          gx does not read the forward at all: m_gx = 6 (T + n_levels).
      gc: a term is lam * I (or lam * y): lam with m_gx, I or y with m_y (the forward error of I and y comes in here), one
          product, and at most T adds of the accumulator: m_gc = m_gx + m_y + T + 1.
    The bound must be worth something: it refuses, on every output the change reaches, c0 and c1 swapped (y, gx, gc), gy shifted
    by one row (gx, gc: y does not read gy) and down replaced by its level-neighbour (y, gx, gc).
    Measured: worst error / bound = 0.0164 (y), 0.0291 (gx), 0.0124 (gc), with m = 91, 78, 179."""
    rng = np.random.default_rng(17)
    for seed in range(40):  # the first random forest of 7 with three levels and a level of two or more
        topo = NH.Topology(NH.random_forest(7, 100 + seed, roots=0.1))
        if topo.n_levels >= 3 and (np.diff(topo.level_ptr) >= 2).sum() >= 2 and (_neighbour_down(topo) != topo.down).any():
            break
    T, B = 9, topo.B
    x, gy, _, state = NH.case_data(rng, T, B, "muskingum")
    coef = NH.muskingum_np(0.5 + 5.0 * rng.random(B), 0.5 * rng.random(B), 1.0)
    maxdeg = int(np.diff(topo.up_ptr).max())
    m_y, m_gx = (T + topo.n_levels) * (maxdeg + 5), 6 * (T + topo.n_levels)
    m = dict(y=m_y, gx=m_gx, gc=m_gx + m_y + T + 1)
    want = dict(zip(("y", "gx", "gc"), exact(topo, x, coef, gy, state)))
    mag = dict(zip(("y", "gx", "gc"), exact(topo, x, coef, gy, state, absolute=True)))

    def ratios(got):
        """per output, error / bound of every element (inf where the bound is 0 and the error is not)"""
        out = {}
        for k, arr in zip(("y", "gx", "gc"), got):
            r = np.zeros(arr.shape)
            for i in range(arr.shape[0]):
                for j in range(arr.shape[1]):
                    err, bar = abs(Fraction(float(arr[i, j])) - want[k][i][j]), Fraction(gamma(m[k])) * mag[k][i][j]
                    r[i, j] = float(err / bar) if bar else (0.0 if err == 0 else np.inf)
            out[k] = r
        return out

    r = ratios(_host(topo, x, coef, gy, state))
    print("network vs exact rational: worst error / bound = %.3g (y), %.3g (gx), %.3g (gc); m = %r" % (r["y"].max(), r["gx"].max(), r["gc"].max(), m))
    assert all(v.max() <= 1.0 for v in r.values())
    assert all(v.max() > 0 for v in r.values())  # (the data are general: something does round)
    swapped = ratios(_host(topo, x, coef[[1, 0, 2]], gy, state))
    assert all(swapped[k].max() > 1.0 for k in ("y", "gx", "gc"))
    shifted = ratios(_host(topo, x, coef, np.roll(gy, 1, axis=0), state))
    assert shifted["y"].max() <= 1.0 and all(shifted[k].max() > 1.0 for k in ("gx", "gc"))
    moved = ratios(_host(NH.Topology(_neighbour_down(topo)), x, coef, gy, state))
    assert all(moved[k].max() > 1.0 for k in ("y", "gx", "gc"))


# ---- 5. the same bits --------------------------------------------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_chunked_and_repeated_calls_give_the_same_bits():
    """One call against calls cut at 1 row, at T - 1 rows and in the middle (carry=True keeps the [2, B] state per key), from
    zeros and from a given state; a repeated call; reset()."""
    rng = np.random.default_rng(23)
    topo = NH.Topology(NH.random_forest(65, 9))
    T, B = 17, topo.B
    x, _, coef, state = NH.case_data(rng, T, B, "muskingum")
    net = SimCatchmentNetwork(topo.down)
    tx, tc = _t(x), _t(coef)
    for st in (None, state):
        want, want_state = NH.route_ref(topo, x, coef, st)
        one = net.route(tx, tc, carry=False, state=None if st is None else _t(st))
        assert NH.same_bits(one.numpy(), want) and NH.same_bits(net.route(tx, tc, carry=False, state=None if st is None else _t(st)).numpy(), want)
        for cut in (1, T - 1, T // 2):
            key = ("cut", cut, st is None)
            a = net.route(tx[:cut], tc, key=key, state=None if st is None else _t(st))
            b = net.route(tx[cut:], tc, key=key)
            assert NH.same_bits(torch.cat([a, b]).numpy(), want), cut
            assert NH.same_bits(net.state_of(key).numpy(), want_state)
            assert tuple(net.route(tx[:0], tc, key=key).shape) == (0, B) and NH.same_bits(net.state_of(key).numpy(), want_state)  # T = 0
    assert net.state_of("nobody") is None
    net.reset()
    assert net.state_of(("cut", 1, True)) is None


def test_unrelated_reaches_leave_a_subtree_alone():
    """The upstream closure S of one reach of a random forest, moved into a larger network between unrelated reaches under an
    ORDER-PRESERVING relabelling: y of S keeps its bits.  Only order-preserving: the inflow fold adds the
    upstream discharges in ascending index, so a relabelling that reorders the upstream of a reach reorders a floating-point
    sum.  (gx of S depends on what is DOWNSTREAM of S, which is not moved; it is compared for the whole network instead.)"""
    rng = np.random.default_rng(31)
    big = NH.Topology(NH.random_forest(65, 12))
    root = int(big.order[-1])  # a reach of the highest level
    S = np.nonzero(big.closure()[root])[0]
    assert 3 <= len(S) < big.B
    T = 9
    x, gy, coef, state = NH.case_data(rng, T, big.B, "mixed")
    y_big, _ = NH.route_ref(big, x, coef, state)
    M = 100
    slots = np.sort(rng.permutation(M)[:len(S)])  # S[i] -> slots[i], increasing
    new_of = {int(s): int(n) for s, n in zip(S, slots)}
    others = np.setdiff1d(np.arange(M), slots)
    down = np.full(M, -1, dtype=np.int64)
    for s in S:
        if s != root:
            down[new_of[int(s)]] = new_of[int(big.down[s])]
    for i, o in enumerate(others[1:], 1):  # the unrelated reaches: a random forest among themselves
        down[o] = others[rng.integers(0, i)] if rng.random() > 0.2 else -1
    x2, c2, s2 = NH.mixed(rng, T, M), NH.coefficients(rng, "mixed", M), NH.mixed(rng, 2, M)
    x2[:, slots], c2[:, slots], s2[:, slots] = x[:, S], coef[:, S], state[:, S]
    net = SimCatchmentNetwork(down)
    y2 = net.route(_t(x2), _t(c2), carry=False, state=_t(s2)).numpy()
    assert NH.same_bits(y2[:, slots], y_big[:, S]) and float(np.abs(y2[:, slots]).max()) > 0
    # the whole network under an order-preserving relabelling into the same larger network: the adjoint and gc keep their bits too
    slots = np.sort(rng.permutation(M)[:big.B])
    others = np.setdiff1d(np.arange(M), slots)
    down = np.full(M, -1, dtype=np.int64)
    down[slots] = np.where(big.down >= 0, slots[np.maximum(big.down, 0)], -1)
    for i, o in enumerate(others[1:], 1):
        down[o] = others[rng.integers(0, i)] if rng.random() > 0.2 else -1
    x2, g2, c2 = NH.mixed(rng, T, M), NH.mixed(rng, T, M), NH.coefficients(rng, "mixed", M)
    x2[:, slots], g2[:, slots], c2[:, slots] = x, gy, coef
    net = SimCatchmentNetwork(down)
    y2 = net.route(_t(x2), _t(c2), carry=False)
    y1, _ = NH.route_ref(big, x, coef)
    assert NH.same_bits(y2.numpy()[:, slots], y1)
    assert NH.same_bits(net.adjoint(_t(g2), _t(c2)).numpy()[:, slots], NH.adjoint_ref(big, gy, coef))
    assert NH.same_bits(net.coef_grad(_t(x2), y2, _t(g2), _t(c2)).numpy()[:, slots], NH.coef_grad_ref(big, x, y1, gy, coef))


# ---- 6. NaN ------------------------------------------------------------------------------------------------------------------
def test_a_nan_reaches_exactly_its_downstream_closure_from_its_row_on():
    rng = np.random.default_rng(41)
    topo = NH.Topology(NH.random_forest(65, 3))
    T, B = 9, topo.B
    x, _, coef, _ = NH.case_data(rng, T, B, "muskingum")
    b = int(topo.order[0])
    while topo.down[b] < 0 or topo.down[topo.down[b]] < 0:  # a headwater with two reaches below it
        b = int(topo.order[int(np.nonzero(topo.order == b)[0][0]) + 1])
    t0 = 4
    clean, _ = NH.route_ref(topo, x, coef)
    x[t0, b] = np.nan
    (got, _), = NH.run([("route", topo, x, coef, None, False)])
    hit = np.zeros((T, B), dtype=bool)
    hit[t0:, topo.closure()[:, b]] = True  # R[d, b]: b is d or upstream of d
    assert hit[:, b].any() and hit.sum() >= 3 * (T - t0) and hit.sum() < T * B // 2
    assert (np.isnan(got) == hit).all() and NH.same_bits(got[~hit], clean[~hit])


# ---- 7. host logic -----------------------------------------------------------------------------------------------------------
def test_network_construction_and_rejections():
    import lgar_py_amd as lg
    from lgar_py_amd import LgarError
    from lgar_py_amd.network import CatchmentNetwork
    assert lg.CatchmentNetwork is CatchmentNetwork and callable(lg.network_route) and callable(lg.muskingum_coefficients)
    assert {"CatchmentNetwork", "network_route", "muskingum_coefficients"} <= set(lg.__all__)
    for name, down in NH.topologies().items():
        topo, net = NH.Topology(down), CatchmentNetwork(down, device="cpu")
        assert (net.B, net.n_levels, net.n_edges) == (topo.B, topo.n_levels, topo.E), name
        for mine, theirs in ((net.levels, topo.level), (net.order_host, topo.order), (net.level_ptr, topo.level_ptr),
                             (net.up_ptr_host, topo.up_ptr), (net.up_idx_host, topo.up_idx), (net.down.numpy(), topo.down)):
            assert np.array_equal(mine, theirs) and mine.dtype == np.int32, name
        assert all(np.array_equal(net.upstream_of(b), topo.ups[b]) for b in range(0, topo.B, 7))
        assert net.order.dtype == torch.int32 and net.level_ptr.flags["C_CONTIGUOUS"]
    levels = lambda down: CatchmentNetwork(down, device="cpu")
    assert levels(NH.single()).n_levels == 1 and levels(NH.chain(65)).n_levels == 65 and levels(NH.star(257)).n_levels == 2
    assert levels(NH.binary_tree(127)).n_levels == 7 and levels(NH.wide(65)).levels.tolist().count(0) == 65
    assert np.array_equal(levels(NH.chain(5)).levels, np.arange(5)) and levels(NH.forest(64)).levels[3:8].tolist() == [0] * 5
    empty = levels(np.zeros(0, dtype=np.int64))
    assert (empty.B, empty.n_levels, empty.level_ptr.tolist()) == (0, 0, [0])
    assert levels(torch.tensor([1, -1])).n_levels == 2
    for bad, word in (([1, 2, 0], "cycle through catchment"), ([-1, 2, 3, 1, 0], "cycle through catchment [123]"), ([0], "into itself"),
                      ([1, 1], "into itself"), ([2, -1], "no catchment"), ([-2, -1], "no catchment"), ([0.5, -1], "integers"),
                      ([[1, -1]], r"\[B\]"), ("river", "integers")):
        with pytest.raises(LgarError, match=word):
            levels(bad)
    with pytest.raises(LgarError):
        levels([1, -1]).upstream_of(2)
    # calls: shapes, dtypes, devices
    net = SimCatchmentNetwork([1, 2, -1])
    x, coef = torch.zeros(4, 3, dtype=torch.float64), torch.zeros(3, 3, dtype=torch.float64)
    assert tuple(net.route(x, coef).shape) == (4, 3) and tuple(net.route(x, coef[:, 0]).shape) == (4, 3)
    for args in ((x[:, :2], coef), (x.float(), coef), (x, coef[:2]), (x, coef.float()), (x.numpy(), coef), (x.to("meta"), coef), (x, coef, True, None, x)):
        with pytest.raises(LgarError, match=r"3\] tensor"):
            net.route(*args)
    for call in (lambda: net.adjoint(x[:, :2], coef), lambda: net.coef_grad(x, x[:3], x, coef), lambda: net.coef_grad(x[:3], x, x, coef),
                 lambda: net.coef_grad(x, x, x, coef, state=x), lambda: lg.network_route(x, "net", coef), lambda: lg.network_route(x, net, [1, 0, 0])):
        with pytest.raises(LgarError):
            call()
    # a network on the CPU holds the host logic only: the kernels have no CPU fallback
    cpu = CatchmentNetwork([1, 2, -1], device="cpu")
    for call in (lambda: cpu.route(x, coef), lambda: cpu.adjoint(x, coef), lambda: cpu.coef_grad(x, x, x, coef), lambda: cpu.accumulate(x)):
        with pytest.raises(LgarError, match="no CPU fallback"):
            call()


def test_muskingum_coefficients():
    from lgar_py_amd.network import muskingum_coefficients
    rng = np.random.default_rng(5)
    K, X, dt = 0.5 + 5.0 * rng.random(9), 0.5 * rng.random(9), 1.0
    c = muskingum_coefficients(torch.from_numpy(K), torch.from_numpy(X), dt)
    assert tuple(c.shape) == (3, 9) and c.dtype == torch.float64
    assert np.allclose(c.numpy(), NH.muskingum_np(K, X, dt), rtol=4 * U, atol=0) and float((c.sum(dim=0) - 1.0).abs().max()) <= 8 * U
    assert tuple(muskingum_coefficients(2.0, 0.2, 1.0).shape) == (3,) and tuple(muskingum_coefficients(torch.from_numpy(K), 0.2, 1.0).shape) == (3, 9)
    # non-negative iff 2 K X <= dt <= 2 K (1 - X); not enforced
    assert float(muskingum_coefficients(2.0, 0.2, 1.0).min()) >= 0 and float(muskingum_coefficients(2.0, 0.4, 1.0)[0]) < 0 and float(muskingum_coefficients(0.5, 0.2, 1.0)[2]) < 0
    Kt, Xt = torch.from_numpy(K).requires_grad_(True), torch.from_numpy(X).requires_grad_(True)
    muskingum_coefficients(Kt, Xt, dt)[0].sum().backward()
    D = K - K * X + 0.5 * dt
    assert np.allclose(Xt.grad.numpy(), (-K * D + (0.5 * dt - K * X) * K) / D ** 2, rtol=1e-12) and float(Kt.grad.abs().min()) > 0


def test_autograd_through_the_host_build():
    """network_route gives x the adjoint and coef its gradient -- the bits of adjoint_ref and coef_grad_ref -- an explicit state
    is a constant, and the gradient reaches K and X through muskingum_coefficients as torch autograd fed the same gc."""
    from lgar_py_amd.network import muskingum_coefficients, network_route
    rng = np.random.default_rng(8)
    topo = NH.Topology(NH.random_forest(7, 104, roots=0.1))
    T, B = 9, topo.B
    x_np, gy_np, _, st_np = NH.case_data(rng, T, B, "muskingum")
    net = SimCatchmentNetwork(topo.down)
    K = torch.from_numpy(0.5 + 5.0 * rng.random(B)).requires_grad_(True)
    X = torch.from_numpy(0.5 * rng.random(B)).requires_grad_(True)
    coef = muskingum_coefficients(K, X, 1.0)
    coef.retain_grad()
    x, state = _t(x_np).requires_grad_(True), _t(st_np).requires_grad_(True)
    y = network_route(x, net, coef, state)
    c_np = coef.detach().numpy()
    y_ref, _ = NH.route_ref(topo, x_np, c_np, st_np)
    assert NH.same_bits(y.detach().numpy(), y_ref) and net.state_of() is None
    (y * _t(gy_np)).sum().backward()
    gc_ref = NH.coef_grad_ref(topo, x_np, y_ref, gy_np, c_np, st_np)
    assert NH.same_bits(x.grad.numpy(), NH.adjoint_ref(topo, gy_np, c_np)) and NH.same_bits(coef.grad.numpy(), gc_ref) and state.grad is None
    K2, X2 = K.detach().clone().requires_grad_(True), X.detach().clone().requires_grad_(True)
    muskingum_coefficients(K2, X2, 1.0).backward(_t(gc_ref))
    assert torch.equal(K.grad, K2.grad) and torch.equal(X.grad, X2.grad) and float(K.grad.abs().min()) > 0
    # x alone: no coefficient gradient is computed, the same gx
    x2 = _t(x_np).requires_grad_(True)
    (network_route(x2, net, coef.detach(), state.detach()) * _t(gy_np)).sum().backward()
    assert torch.equal(x2.grad, x.grad)


def test_entry_points_refuse_bad_arguments():
    """The refusals of the C-ABI wrappers (lgar_network.hpp's own checks, which the host launchers call as the library does):
    LGAR_E_ARG = -1 for negative sizes, n_levels < 0, a level_ptr that does not start at 0, end at B and never decrease, a null
    pointer the sizes say will be read or written, gc wanted without x, y, up_ptr, up_idx."""
    lib = NH.library()
    topo = NH.Topology([1, 2, -1, 2])
    B, E, L, T = topo.B, topo.E, topo.n_levels, 2
    buf = np.zeros(64)
    p = buf.ctypes.data
    ints = {k: np.ascontiguousarray(getattr(topo, k), dtype=np.int32) for k in ("up_ptr", "up_idx", "order", "level_ptr", "down")}
    ip = {k: v.ctypes.data for k, v in ints.items()}
    fwd = (("x", p), ("T", T), ("B", B), ("coef", p), ("up_ptr", ip["up_ptr"]), ("up_idx", ip["up_idx"]), ("E", E), ("order", ip["order"]),
           ("level_ptr", ip["level_ptr"]), ("L", L), ("state_in", None), ("state_out", p + 256), ("y", p + 128))
    route = lambda **kw: lib.networkhost_network_route(*[kw.get(k, d) for k, d in fwd])
    assert route() == 0
    bad_ptrs = [np.array(v, dtype=np.int32) for v in ([1, 2, 3, 4], [0, 2, 3, 5], [0, 3, 2, 4], [0, 2, 3, 3])]
    bad_args = [dict(T=-1), dict(B=-1), dict(E=-1), dict(L=-1), dict(x=None), dict(y=None), dict(coef=None), dict(up_ptr=None), dict(up_idx=None),
                dict(order=None), dict(level_ptr=None), dict(L=2)] + [dict(level_ptr=v.ctypes.data) for v in bad_ptrs]
    for bad in bad_args:
        assert route(**bad) == -1, bad
    assert route(B=0, x=None, y=None, coef=None, order=None, level_ptr=None, up_ptr=None) == 0
    assert route(T=0, x=None, y=None, coef=None, up_ptr=None, up_idx=None) == 0 and route(T=0, state_out=None, order=None) == 0
    assert route(T=0, order=None) == -1 and route(E=0, up_idx=None) == 0 and route(state_out=None) == 0
    grd = (("gy", p), ("T", T), ("B", B), ("coef", p), ("down", ip["down"]), ("order", ip["order"]), ("level_ptr", ip["level_ptr"]), ("L", L),
           ("gx", p + 128), ("x", p), ("y", p), ("up_ptr", ip["up_ptr"]), ("up_idx", ip["up_idx"]), ("E", E), ("state_in", None), ("gc", p + 256))
    grad = lambda **kw: lib.networkhost_network_route_grad(*[kw.get(k, d) for k, d in grd])
    assert grad() == 0
    for bad in [dict(T=-1), dict(B=-1), dict(E=-1), dict(L=-1), dict(gy=None), dict(gx=None), dict(coef=None), dict(down=None), dict(order=None),
                dict(level_ptr=None), dict(x=None), dict(y=None), dict(up_ptr=None), dict(up_idx=None), dict(L=2)] + [dict(level_ptr=v.ctypes.data) for v in bad_ptrs]:
        assert grad(**bad) == -1, bad
    assert grad(gc=None, x=None, y=None, up_ptr=None, up_idx=None) == 0 and grad(B=0, gy=None, gx=None, level_ptr=None) == 0
    buf[32:44] = 7.0
    assert grad(T=0, gy=None, gx=None, x=None, y=None, coef=None, down=None) == 0 and buf[32:44].tolist() == [0.0] * 12  # T = 0: gc = zeros
    assert grad(T=0, gc=None, order=None) == 0
