"""CPU: the catchment network with reaches and level-pool reservoirs (lgar_network_route_pool / lgar_network_route_pool_grad,
include/lgar.h).

The per-node walks the GPU kernels run (lgar_py_amd/csrc/lgar_network_pool.hpp, with lgar_network_mc.hpp's for the reaches) are
compiled for the host into a small stand-alone program (tests/network_pool_host).  It is held BIT FOR BIT to the numpy statement
of the definition (network_pool_host.route_pool_ref / route_pool_grad_ref); the same program built with AddressSanitizer + UBSan
runs the same cases.  Independently of the statement the definition is held to statements that do not come from it: P = 0 to the
Muskingum-Cunge route, m = 0 to a recurrence without logarithm or exponential, the volume to its closure, the release law to
mpmath.power and the adjoint to derivatives of the real-arithmetic statement taken in mpmath.  The same header as a shared library
stands behind lgar_py_amd.network.CatchmentNetwork (network_pool_host.SimCatchmentNetworkPool overrides _open() only), so the
host logic of NetworkPools / route_pool / network_route_pool runs here too."""
from fractions import Fraction

import mpmath
import numpy as np
import pytest
import torch

import network_host as NH
import network_mc_host as MH
import network_pool_host as PH
from network_pool_host import SimCatchmentNetworkPool

U = 2.0 ** -53  # unit roundoff of fp64


def gamma(m):
    """Higham's gamma_m = m u / (1 - m u)."""
    return m * U / (1.0 - m * U)


LN_BOUND = gamma(9) + 7e-19  # mc_ln's relative error (derived in csrc/lgar_network_mc.hpp)
EXP_BOUND = gamma(29) * 2.0 ** 0.5 + 4.3e-18  # gw_exp's (derived in tests/test_baseflow_host.py)
WANTS = ((True, True, True), (True, False, False), (False, True, False), (False, False, True), (False, False, False))


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _pools(net, pt):
    """The product's NetworkPools of pt's pools, held to pt's arrays (built by plain loops)."""
    from lgar_py_amd.network import NetworkPools
    pools = NetworkPools(net, pt.nodes)
    assert pools.P == pt.P and (pools.order_host == pt.order).all() and (pools.pool_ptr == pt.pool_ptr).all()
    assert (pools.pool_slot_host == pt.pool_slot).all() and (net.order_host == pt.base.order).all()  # the network's own order is untouched
    return pools


# ---- 1. the host build against the numpy definition ------------------------------------------------------------------------
def _grid():
    """Every topology x every pool placement x T in {0, 1, 2, 7, 8, 9, 17}; state_in present or NULL, the default and the widest
    ranges and which of state_out / storage / gpar_mc / gpool / gstate are wanted take turns from case to case, at periods
    (2, 4, 8, 16 and 5 cases) that differ from the 7 row counts of a placement.  (cases, references, the count of pool rows per regime)."""
    rng = np.random.default_rng(18)
    cases, refs = [], []
    count = dict.fromkeys(PH.POOL_REGIMES, 0)
    k = 0
    for name, down in NH.topologies().items():
        topo = NH.Topology(down)
        for kind in PH.PLACEMENTS:
            pt = PH.PoolTopology(topo, PH.placement(topo, kind, rng))
            for T in PH.SHAPE_T:
                k += 1
                x, gy, pm, pp, state, dt, rr, prr = PH.case_data(rng, pt, T, wide=bool(k % 2))
                st = state if (k // 2) % 2 else None
                y, so, sg = PH.route_pool_ref(pt, x, pm, pp, dt, rr, prr, st)
                for key, v in PH.pool_regimes(pt, x, pm, pp, dt, rr, prr, st).items():
                    count[key] += v
                ws, wg = bool((k // 4) % 2), bool((k // 8) % 2)
                cases.append(("route", pt, x, pm, pp, dt, rr, prr, st, ws, wg))
                refs.append((y, so if ws else None, sg if wg else None))
                g = PH.route_pool_grad_ref(pt, gy, x, y, sg, pm, pp, dt, rr, prr, st)
                for wp, wl, wt in (WANTS[k % 5], WANTS[(k + 2) % 5]):
                    cases.append(("grad", pt, gy, x, y, sg, pm, pp, dt, rr, prr, st, wp, wl, wt))
                    refs.append((g[0], g[1] if wp else None, g[2] if wl else None, g[3] if wt else None))
    return cases, refs, count


@pytest.fixture(scope="module")
def grid():
    return _grid()


def _check(cases, refs, got):
    assert len(got) == len(refs) == len(cases)
    for c, r, o in zip(cases, refs, got):
        for want, have in zip(r, o):
            assert (want is None) == (have is None), (c[0], c[1].B, c[1].P, np.asarray(c[2]).shape)
            assert want is None or PH.same_bits(have, want), (c[0], c[1].B, c[1].P, np.asarray(c[2]).shape)


def test_host_build_equals_the_numpy_definition_bit_for_bit(grid):
    cases, refs, count = grid
    _check(cases, refs, PH.run(cases))
    # every regime of the pool row is taken somewhere: inside; clamped low and high; |tau| > ZMAX; the release law, the limited
    # release and the release cut to zero (from mixed-sign x, and from S < s0 in state_in); the spill; smax = +inf; the exact ties
    print("pool rows per regime:", count)
    assert all(count[k] > 0 for k in PH.POOL_REGIMES), count
    for c, r in zip(cases, refs):
        T = np.asarray(c[2]).shape[0]
        if c[0] == "route" and T == 0 and r[1] is not None:  # T = 0 copies the state, or writes zeros
            assert PH.same_bits(r[1], np.zeros((2, c[1].B)) if c[8] is None else np.asarray(c[8]))
        if c[0] == "grad" and T == 0:  # T = 0: zeros
            assert all(a is None or not a.any() for a in r)
        if c[0] == "grad" and r[1] is not None:  # a reach parameter receives +0.0 at a pool
            assert not r[1][:, c[1].is_pool].any() and not np.signbit(r[1][:, c[1].is_pool]).any()
    assert {1, 2, 63, 64, 65, 127, 257} <= {c[1].B for c in cases} and {np.asarray(c[2]).shape[0] for c in cases} == set(PH.SHAPE_T)
    pools_in_level = {int(n) for c in cases for n in (c[1].level_ptr[1:] - c[1].pool_ptr)}
    assert {0, 64, 65} <= pools_in_level
    assert any((c[1].pool_ptr == c[1].level_ptr[:-1]).any() and c[1].P < c[1].B and c[1].P for c in cases)  # a level of only pools
    assert {c[1].P for c in cases} >= {0, 1} and any(c[1].P == c[1].B > 1 for c in cases)


def test_sanitizer_build_on_the_same_cases(grid):
    """AddressSanitizer + UBSan build of the same program (a stand-alone executable: nothing is loaded into python; every array is
    allocated at its exact size, and with P = 0 par_pool, pool_slot and storage are null pointers) over the same cases: clean,
    with the same bits.  Any finding aborts the program."""
    cases, refs, _ = grid
    _check(cases, refs, PH.run(cases, sanitize=True))


def test_corrupt_topology_pool_slot_and_order_stay_inside_the_arrays():
    """order, up_idx, down and pool_slot far outside their ranges, up_ptr outside 0 .. E, and an `order` that is consistent with
    pool_ptr but sends reaches to the pool kernel and pools to the reach kernel (the level's two parts swapped): the sanitizer
    build runs clean (wrong numbers, no access out of bounds -- every index read from device memory is clamped).  Host build
    only: this is never run on a GPU."""
    rng = np.random.default_rng(3)
    good = PH.PoolTopology(NH.Topology(NH.random_forest(65, 5)), rng.permutation(65)[:20])
    T, B = 9, good.B
    x, gy, pm, pp, state, dt, rr, prr = PH.case_data(rng, good, T)
    y, _, sg = PH.route_pool_ref(good, x, pm, pp, dt, rr, prr, state)
    cases = []
    for field, values in (("order", (10 ** 6, -5, B)), ("up_idx", (10 ** 6, -5, B)), ("down", (10 ** 6, B, -7)),
                          ("up_ptr", (10 ** 6, -5, 2 ** 31 - 1)), ("pool_slot", (10 ** 6, -5, good.P, -1))):
        bad = good.copy()
        arr = getattr(bad, field)
        arr[rng.permutation(len(arr))[:9]] = np.resize(np.array(values, dtype=np.int64), 9).astype(np.int32)
        cases += [("route", bad, x, pm, pp, dt, rr, prr, state, True, True), ("grad", bad, gy, x, y, sg, pm, pp, dt, rr, prr, state, True, True, True),
                  ("grad", bad, gy, x, y, sg, pm, pp, dt, rr, prr, None, False, False, False)]
    bad = good.copy()
    for l in range(bad.n_levels):  # every level: pools first, reaches after them, pool_ptr as it was
        a, b = bad.level_ptr[l], bad.level_ptr[l + 1]
        bad.order[a:b] = np.concatenate([good.pools(l), good.reaches(l)])
    cases += [("route", bad, x, pm, pp, dt, rr, prr, state, True, True), ("grad", bad, gy, x, y, sg, pm, pp, dt, rr, prr, state, True, True, True)]
    got = PH.run(cases, sanitize=True)
    assert len(got) == len(cases) and all(g[0].shape == (T, B) for g in got)
    assert PH.same_bits(got[6][0], y)  # corrupt `down` entries touch the adjoint only


# ---- 2. independent of the statement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(NH.topologies()))
def test_without_pools_it_is_the_muskingum_cunge_route(name):
    """P = 0 (null par_pool, pool_slot and storage; pool_ptr[l] = level_ptr[l + 1]): y, state_out, gx, gpar_mc and gstate of the
    host build equal lgar_network_route_mc's host build (tests/network_mc_host) and its numpy statement, bit for bit."""
    topo = NH.Topology(NH.topologies()[name])
    pt = PH.PoolTopology(topo, [])
    assert (pt.order == topo.order).all() and (pt.pool_ptr == topo.level_ptr[1:]).all()
    rng = np.random.default_rng(3100 + topo.B)
    mine, theirs = [], []
    for T in (0, 9, 17):
        x, gy, par, state, dt, rr = MH.case_data(rng, T, topo.B, wide=(T == 17))
        for st in (None, state):
            y = MH.route_mc_ref(topo, x, par, dt, *rr, st)[0]
            none = np.zeros((5, 0))
            mine += [("route", pt, x, par, none, dt, rr, PH.PNARROW, st, True, False),
                     ("grad", pt, gy, x, y, np.zeros((T, 0)), par, none, dt, rr, PH.PNARROW, st, True, False, True)]
            theirs += [("route", topo, x, par, dt, rr, st, True), ("grad", topo, gy, x, y, par, dt, rr, st, True, True)]
    for a, b in zip(PH.run(mine), MH.run(theirs)):
        if len(a) == 3:
            assert PH.same_bits(a[0], b[0]) and PH.same_bits(a[1], b[1]) and a[2] is None
        else:
            assert PH.same_bits(a[0], b[0]) and PH.same_bits(a[1], b[1]) and PH.same_bits(a[3], b[2]) and a[2] is None


def _m_zero_recurrence(pt, x, cq, s0, smax, dt, state):
    """Every node a pool with m = 0, written without the row function, a logarithm or an exponential: the release law is cq."""
    T, B = x.shape
    y, storage = np.zeros((T, B)), np.zeros((T, B))
    half = 0.5 * np.float64(dt)
    with np.errstate(all="ignore"):
        for b in pt.order.astype(np.int64):
            c, z, cap = cq[pt.pool_slot[b]], s0[pt.pool_slot[b]], smax[pt.pool_slot[b]] - s0[pt.pool_slot[b]]
            Iprev, S = (state[0, b], state[1, b]) if state is not None else (0.0, 0.0)
            for t in range(T):
                I = x[t, b]
                for u in pt.ups[b]:
                    I = I + y[t, u]
                av = (S - z) + half * (I + Iprev)
                qa = av / dt
                Q = c if c < qa else qa
                Q = 0.0 if Q < 0.0 else Q
                r = av - dt * Q
                ex = r - cap
                O, S = (Q + ex / dt, cap + z) if ex > 0.0 else (Q, r + z)
                y[t, b], storage[t, pt.pool_slot[b]], Iprev = O, S, I
    return y, storage


@pytest.mark.parametrize("name", ("single", "chain65", "tree63", "random65", "star257"))
def test_m_zero_is_a_recurrence_without_logarithm_or_exponential(name):
    """m = 0: tau = 0, e = 1, Ql = cq exactly whatever rc is (also clamped).  y and storage of the host build equal a plain
    recurrence with Ql = cq, bit for bit, with every node a pool."""
    topo = NH.Topology(NH.topologies()[name])
    rng = np.random.default_rng(3300 + topo.B)
    pt = PH.PoolTopology(topo, rng.permutation(topo.B))
    cases, wants = [], []
    for T, wide in ((9, False), (17, True)):
        x, _, pm, pp, state, dt, rr, prr = PH.case_data(rng, pt, T, wide)
        pp[1] = 0.0
        for st in (None, state):
            cases.append(("route", pt, x, pm, pp, dt, rr, prr, st, False, True))
            wants.append(_m_zero_recurrence(pt, x, pp[0], pp[2], pp[4], dt, st))
    for (y, _, sg), (wy, wsg) in zip(PH.run(cases), wants):
        assert PH.same_bits(y, wy) and PH.same_bits(sg, wsg) and float(np.abs(y).max()) > 0


def test_the_volume_closes():
    """S_T - S_0 = sum vin_t - dt_h sum O_t per pool over 17 rows, with vin_t = half (I_t + I_(t-1)) taken exactly (Fractions) from
    the floats I the walk formed, O and S the floats it stored.

    The bar, derived from the row's operations before the first run.  Between S_(t-1) and S_t the row rounds: I + Iprev and its
    product with half (2), a = S - s0 (1), av = a + vin (1), qa = av / dt_h where the release is limited (1), dt_h * Q (1),
    r = av - that (1), and then either S = r + s0 (1) or, where the pool spills, ex = r - cap, ex / dt_h, O = Q + that and
    S = cap + s0 (4): at most 11 roundings, each of a value that is at most 2 W_t in magnitude, W_t = |S_(t-1)| + |s0| + |vin_t| +
    dt_h |O_t| + |S_t| + (|cap| where the pool spills) (|a| <= |S| + |s0|, |av| <= |a| + |vin|, |r| <= |av| + dt_h |Q|, Q <= O,
    |ex| <= |r| + |cap|).  The release law's own error does not enter: whatever Q is, the row removes dt_h Q and reports O.  So
    |S_T - S_0 - sum vin + dt_h sum O| <= gamma_22 sum_t W_t, k = 22.
    Measured: worst miss / bound = 0.0299."""
    rng = np.random.default_rng(51)
    worst, seen = 0.0, dict.fromkeys(("spill", "limited", "empty", "free"), 0)
    F = Fraction
    for name in ("random65", "tree63"):
        topo = NH.Topology(NH.topologies()[name])
        pt = PH.PoolTopology(topo, rng.permutation(topo.B))
        T = 17
        x, _, pm, pp, state, dt, rr, prr = PH.case_data(rng, pt, T)
        (y, so, sg), = PH.run([("route", pt, x, pm, pp, dt, rr, prr, state, True, True)])
        rows = PH.pool_rows(pt, x, pm, pp, dt, rr, prr, state)
        for k in seen:
            seen[k] += int((~rows["free"] & ~rows["empty"]).sum()) if k == "limited" else int(rows[k].sum())
        for s, b in enumerate(pt.nodes):
            S = [F(state[1, b])] + [F(v) for v in sg[:, s]]
            vin = [F(dt) / 2 * (F(rows["I"][t, s]) + F(rows["Iprev"][t, s])) for t in range(T)]
            O = [F(v) for v in y[:, b]]
            cap = F(pp[4, s]) - F(pp[2, s]) if np.isfinite(pp[4, s]) else F(0)
            miss = abs(S[T] - S[0] - sum(vin) + F(dt) * sum(O))
            W = sum(abs(S[t]) + abs(F(pp[2, s])) + abs(vin[t]) + F(dt) * abs(O[t]) + abs(S[t + 1]) + (abs(cap) if rows["spill"][t, s] else 0)
                    for t in range(T))
            bar = F(gamma(22)) * W
            assert miss <= bar, (name, s, float(miss / bar))
            worst = max(worst, float(miss / bar))
            assert so[1, b] == sg[T - 1, s]
    print("pool volume closure: worst miss / bound = %.3g (k = 22); rows %r" % (worst, seen))
    assert 0.0 < worst <= 1.0 and all(v > 0 for v in seen.values())


def test_release_law_against_mpmath():
    """Ql of the row for cq = 1 (rc^m as the row forms it: mc_ln, one product, gw_exp, a product or a quotient) against
    mpmath.power at 40 digits: 3000 points with rc log-uniform over the default range 2^-20 .. 2^20 and m uniform in [0, 2.8]
    (|tau| <= 38.9 < ZMAX), 300 with rc within 1e-3 of 1, and m = 0.  The bound is the header's (csrc/lgar_network_pool.hpp):
    |tau| (LN_BOUND + u) + EXP_BOUND + u per point, from mc_ln's and gw_exp's stated bounds.
    Measured: worst relative error 2.97e-15 at a bound of 2.28e-14 there; worst error / bound = 0.13 over 3302 points."""
    rng = np.random.default_rng(15)
    rc = np.concatenate([2.0 ** rng.uniform(-20.0, 20.0, 3000), 1.0 + rng.uniform(-1e-3, 1e-3, 300), [2.0 ** -20, 2.0 ** 20]])
    m = np.concatenate([rng.uniform(0.0, 2.8, 3000), rng.uniform(0.0, 2.8, 300), [2.8, 2.8]])
    m[:50] = 0.0
    (q,), = PH.run([("release", rc, m, PH.PNARROW)])
    with np.errstate(all="ignore"):
        ref = PH._pool_row(rc, np.zeros(len(rc)), np.ones(len(rc)), m, 0.0, 1.0, 1.0, 1.0, *PH.PNARROW)
    assert PH.same_bits(q, ref["Ql"]) and (q[:50] == 1.0).all() and not ref["big"].any() and ref["inside"].all()
    mpmath.mp.dps = 40
    worst, worst_rel, at = 0.0, 0.0, 0.0
    for r, e, got in zip(rc, m, q):
        want = mpmath.power(mpmath.mpf(float(r)), mpmath.mpf(float(e)))
        rel = float(abs(mpmath.mpf(float(got)) - want) / want)
        tau = float(abs(mpmath.mpf(float(e)) * mpmath.log(mpmath.mpf(float(r)))))
        bound = (tau * (LN_BOUND + U) + EXP_BOUND + U) * (1.0 + 1e-9)
        assert rel <= bound, (r, e, rel, bound)
        if rel / bound > worst:
            worst, worst_rel, at = rel / bound, rel, bound
    print("release law vs mpmath.power: worst relative error %.3g at a bound of %.3g there; worst error / bound = %.3g over %d points"
          % (worst_rel, at, worst, len(rc)))
    assert worst > 0.0


# ---- 3. the same bits ---------------------------------------------------------------------------------------------------------
def test_chunked_repeated_and_relabelled_calls_give_the_same_bits():
    """One call against calls cut at 1 row, at T - 1 rows and in the middle (carry=True keeps the [2, B] state per key, in a key
    space of its own), from zeros and from a given state; a repeated call; reset(); an order-preserving relabelling into a
    larger network gives the relabelled bits, forward and adjoint."""
    rng = np.random.default_rng(23)
    topo = NH.Topology(NH.random_forest(65, 12))
    pt = PH.PoolTopology(topo, rng.permutation(65)[:21])
    T, B = 17, topo.B
    x, gy, pm, pp, state, dt, rr, prr = PH.case_data(rng, pt, T)
    pp[1] = np.minimum(pp[1], 2.5)  # what route_pool validates holds for every m; the large ones only slow nothing down
    net = SimCatchmentNetworkPool(topo.down)
    pools = _pools(net, pt)
    tx, reach, pool = _t(x), tuple(_t(p) for p in pm), tuple(_t(p) for p in pp)
    for st in (None, state):
        want, want_state, want_storage = PH.route_pool_ref(pt, x, pm, pp, dt, rr, prr, st)
        y, sg = net.route_pool(tx, pools, reach, pool, dt, carry=False, state=_t(st), return_storage=True)
        assert PH.same_bits(y.numpy(), want) and PH.same_bits(sg.numpy(), want_storage) and net.pool_state_of() is None
        assert torch.equal(net.route_pool(tx, pools, reach, pool, dt, carry=False, state=_t(st)), y)
        for cut in (1, T - 1, T // 2):
            key = ("cut", cut, st is None)
            a = net.route_pool(tx[:cut], pools, reach, pool, dt, key=key, state=_t(st))
            b, sb = net.route_pool(tx[cut:], pools, reach, pool, dt, key=key, return_storage=True)
            assert PH.same_bits(torch.cat([a, b]).numpy(), want) and PH.same_bits(net.pool_state_of(key).numpy(), want_state), cut
            assert PH.same_bits(sb.numpy(), want_storage[cut:])
            assert tuple(net.route_pool(tx[:0], pools, reach, pool, dt, key=key).shape) == (0, B)
            assert PH.same_bits(net.pool_state_of(key).numpy(), want_state)
            assert net.state_of(key) is None and net.mc_state_of(key) is None  # the other routes' keys are other spaces
    net.reset()
    assert net.pool_state_of(("cut", 1, True)) is None
    M = 100
    down2, slots = MH.embed(rng, topo, M)
    topo2 = NH.Topology(down2)
    others = np.setdiff1d(np.arange(M), slots)
    extra = others[:5]
    pt2 = PH.PoolTopology(topo2, np.concatenate([extra, slots[pt.nodes]]))  # the old pools keep their order behind five new ones
    x2, gy2, pm2, pp2, state2, _, _, _ = PH.case_data(rng, pt2, T)
    x2[:, slots], gy2[:, slots], pm2[:, slots], state2[:, slots], pp2[:, 5:] = x, gy, pm, state, pp
    want, want_state, want_storage = PH.route_pool_ref(pt, x, pm, pp, dt, rr, prr, state)
    (y2, so2, sg2), = PH.run([("route", pt2, x2, pm2, pp2, dt, rr, prr, state2, True, True)])
    assert PH.same_bits(y2[:, slots], want) and PH.same_bits(so2[:, slots], want_state) and PH.same_bits(sg2[:, 5:], want_storage)
    got, = PH.run([("grad", pt2, gy2, x2, y2, sg2, pm2, pp2, dt, rr, prr, state2, True, True, True)])
    ref = PH.route_pool_grad_ref(pt, gy, x, want, want_storage, pm, pp, dt, rr, prr, state)
    assert PH.same_bits(got[0][:, slots], ref[0]) and PH.same_bits(got[1][:, slots], ref[1]) and PH.same_bits(got[3][:, slots], ref[3])
    assert PH.same_bits(got[2][:, 5:], ref[2])


@pytest.mark.parametrize("at_pool", (True, False))
def test_a_nan_reaches_exactly_its_downstream_closure_from_its_row_on(at_pool):
    """A NaN in x[t0][b], b a pool / b a reach above a pool: y is NaN exactly at the downstream closure of b from row t0 on (every
    select of the pool row takes its last alternative and the storage is arithmetic), and so is the storage of the pools in it."""
    rng = np.random.default_rng(41)
    topo = NH.Topology(NH.random_forest(65, 3))
    b = int(topo.order[0])
    while topo.down[b] < 0 or topo.down[topo.down[b]] < 0:  # a headwater with two nodes below it
        b = int(topo.order[list(topo.order).index(b) + 1])
    below = int(topo.down[b])
    nodes = [n for n in rng.permutation(65)[:20] if n not in (b, below)] + ([b] if at_pool else [below])
    pt = PH.PoolTopology(topo, nodes)
    assert pt.is_pool[b] == at_pool and (at_pool or pt.is_pool[below])
    T, B = 9, topo.B
    x, _, pm, pp, state, dt, rr, prr = PH.case_data(rng, pt, T)
    clean, _, clean_sg = PH.route_pool_ref(pt, x, pm, pp, dt, rr, prr, state)
    t0 = 4
    x[t0, b] = np.nan
    (y, so, sg), = PH.run([("route", pt, x, pm, pp, dt, rr, prr, state, True, True)])
    hit = np.zeros((T, B), dtype=bool)
    hit[t0:, topo.closure()[:, b]] = True
    assert hit[t0].sum() >= 3 and not hit[:t0].any()
    assert (np.isnan(y) == hit).all() and PH.same_bits(y[~hit], clean[~hit])
    assert (np.isnan(sg) == hit[:, pt.nodes]).all() and PH.same_bits(sg[~hit[:, pt.nodes]], clean_sg[~hit[:, pt.nodes]])
    assert (np.isnan(so[1]) == hit[-1]).all()


# ---- 4. the adjoint is the true derivative ------------------------------------------------------------------------------------
def _derivative_data():
    """B = 7, T = 9, dt_h = 1, the default ranges.  0 -> 1 -> 2 -> 4 -> 6, 3 -> 4, 5 -> 6: five levels.  Pools, in slot order, 4
    (level 3: small smax, it spills in most rows), 1 (level 1: an ordinary pool, inside and free, below reach 0), 5 (level 0: a
    huge sref, so rho < prmin, and S below s0 at the start, so its first rows are empty) and 2 (level 2: a huge cq and a tiny m,
    limited in every row); reaches 0, 3 and 6 (the outlet, below pools 4 and 5)."""
    rng = np.random.default_rng(78)
    T, B = 9, 7
    topo = NH.Topology([1, 2, 4, 4, 6, 6, -1])
    pt = PH.PoolTopology(topo, [4, 1, 5, 2])
    kref = np.array([2.0, 1.5, 0.4, 2.2, 1.0, 3.0, 1.8]) * (1.0 + 0.1 * rng.random(B))
    pm = np.stack([kref, rng.uniform(0.3, 0.6, B), rng.uniform(0.03, 0.08, B), 2.0 * (1.0 + 0.1 * rng.random(B))])
    x = 0.5 + 1.5 * rng.random((T, B))
    state = 0.5 + 1.5 * rng.random((2, B))
    gy = (rng.random((T, B)) - 0.4) * 2.0
    #                  pool 4  pool 1  pool 5  pool 2
    pp = np.array([[0.9, 0.7, 0.8, 500.0],     # cq
                   [1.5, 1.3, 1.2, 0.01],      # m
                   [0.4, 0.3, 3.1, 0.2],       # s0
                   [2.3, 1.7, 4e8, 1.9],       # sref
                   [6.7, 90.0, 80.0, 70.0]]) * (1.0 + 0.05 * rng.random((5, 4)))
    state[1, pt.nodes] = np.array([5.2, 2.9, 1.6, 1.4]) * (1.0 + 0.05 * rng.random(4))
    return pt, x, gy, pm, pp, state, 1.0, MH.NARROW, PH.PNARROW


def _mp_network(pt, x, pm, pp, state, gy, dt, rr, prr, detail=False):
    """The definition in REAL arithmetic (mpmath at the working precision; ln and exp are mpmath's) over the whole mixed network:
    the loss sum gy y and, with detail, the values and the regime of every row."""
    T, B = len(x), pt.B
    M = mpmath.mpf
    half, zmax = dt / 2, M(MH.ZMAX)
    y = [[None] * B for _ in range(T)]
    rows, loss = {}, M(0)
    for b in (int(v) for v in pt.order):
        Ip, Op = state[0][b], state[1][b]
        s = int(pt.pool_slot[b])
        for t in range(T):
            I = x[t][b]
            for u in pt.ups[b]:
                I = I + y[t][u]
            if s < 0:
                kref, beta, X, qref = (pm[k][b] for k in range(4))
                rho = Op / qref
                lo, hi = rho < rr[0], rho > rr[1]
                rc = rr[0] if lo else (rr[1] if hi else rho)
                L = mpmath.log(rc)
                tau = beta * L
                big = abs(tau) > zmax
                K = kref * mpmath.exp(-(mpmath.sign(tau) * zmax if big else tau))
                KX = K * X
                uu = K - KX
                D = uu + half
                c0, c1, c2 = (half - KX) / D, (half + KX) / D, (uu - half) / D
                O = c0 * I + c1 * Ip + c2 * Op
                if detail:
                    rows[t, b] = dict(pool=False, I=I, Ip=Ip, Op=Op, O=O, rho=rho, L=L, tau=tau, K=K, D=D, c0=c0, c1=c1, c2=c2, lo=lo, hi=hi,
                                      big=big, inside=not (lo or hi or big), X=X, beta=beta, kref=kref)
                Ip, Op = I, O
            else:
                cq, m, s0, sref, smax = (pp[k][s] for k in range(5))
                cap, S = smax - s0, Op
                vin = half * (I + Ip)
                a = S - s0
                rho = a / sref
                lo, hi = rho < prr[0], rho > prr[1]
                rc = prr[0] if lo else (prr[1] if hi else rho)
                L = mpmath.log(rc)
                tau = m * L
                big = abs(tau) > zmax
                pw = mpmath.exp(mpmath.sign(tau) * zmax if big else tau)
                Ql = cq * pw
                av = a + vin
                qa = av / dt
                free = Ql < qa
                Q0 = Ql if free else qa
                empty = Q0 < 0
                Q = M(0) if empty else Q0
                r = av - dt * Q
                ex = r - cap
                spill = ex > 0
                O = Q + ex / dt if spill else Q
                Sn = (cap if spill else r) + s0
                if detail:
                    rows[t, b] = dict(pool=True, I=I, Ip=Ip, Sp=S, O=O, S=Sn, vin=vin, a=a, rho=rho, L=L, tau=tau, pw=pw, Ql=Ql, av=av, qa=qa,
                                      Q0=Q0, Q=Q, r=r, ex=ex, cap=cap, lo=lo, hi=hi, big=big, inside=not (lo or hi or big), free=free,
                                      empty=empty, spill=spill, cq=cq, m=m, s0=s0, sref=sref)
                Ip, Op = I, Sn
            y[t][b] = O
            loss += gy[t][b] * O
    return (loss, rows) if detail else loss


@pytest.fixture(scope="module")
def derivative():
    """The data of the derivative tests, the derivatives of the real-arithmetic statement by central differences in mpmath, the
    adjoint on absolute values and the operation counts m (test_the_adjoint_is_the_true_derivative has the derivation)."""
    mpmath.mp.dps = 60
    pt, x, gy, pm, pp, state, dt, rr, prr = _derivative_data()
    T, B = x.shape
    P = pt.P
    assert pt.n_levels >= 3 and len({int(pt.level[b]) for b in pt.nodes}) >= 2
    M = mpmath.mpf
    mp2 = lambda a: [[M(float(v)) for v in row] for row in a]
    X0, PM0, PP0, S0, G = mp2(x), mp2(pm), mp2(pp), mp2(state), mp2(gy)
    net = lambda **kw: _mp_network(pt, X0, PM0, PP0, S0, G, M(dt), [M(v) for v in rr], [M(v) for v in prr], **kw)
    _, rows = net(detail=True)
    # the float walk takes the real walk's branches, and no row lies within a relative 1e-6 of a regime switch -- both walks
    flt = PH.pool_rows(pt, x, pm, pp, dt, rr, prr, state)
    y_flt = PH.route_pool_ref(pt, x, pm, pp, dt, rr, prr, state)[0]
    rflt = {}  # the reach rows of the float walk, from the Oprev it stored
    for b in np.nonzero(~pt.is_pool)[0]:
        with np.errstate(all="ignore"):
            rflt[b] = MH._row(np.concatenate([state[1, b:b + 1], y_flt[:-1, b]]), *pm[:, b], 0.5 * dt, *rr)
    margin = np.inf
    ZM = MH.ZMAX

    def switch_margin(rho, tau, lo_hi, Ql=None, qa=None, free=None, av=None, av_scale=None, ex=None, ex_scale=None):
        """the relative distance to the nearest switch: rho against the range, |tau| against ZMAX, Ql against qa, av against 0
        where the release is qa (Ql is cq rc^m > 0: its sign cannot switch), ex against 0"""
        out = min(abs(rho - lo_hi[0]) / lo_hi[0], abs(rho - lo_hi[1]) / lo_hi[1], abs(abs(tau) - ZM) / ZM)
        if Ql is not None:
            out = min(out, abs(Ql - qa) / max(abs(Ql), abs(qa)), abs(ex) / ex_scale, 1.0 if free else abs(av) / av_scale)
        return out

    for (t, b), r in rows.items():
        if r["pool"]:
            s = int(pt.pool_slot[b])
            flags = tuple(bool(flt[k][t, s]) for k in ("lo", "hi", "big", "free", "empty", "spill"))
            assert tuple(bool(r[k]) for k in ("lo", "hi", "big", "free", "empty", "spill")) == flags, (t, b)
            cap = float(r["cap"])
            fscale = abs(flt["a"][t, s]) + 0.5 * dt * (abs(flt["I"][t, s]) + abs(flt["Iprev"][t, s]))
            margin = min(margin, switch_margin(float(r["rho"]), float(r["tau"]), prr, float(r["Ql"]), float(r["qa"]), bool(r["free"]), float(r["av"]),
                                               float(abs(r["a"]) + abs(r["vin"])), float(r["ex"]), abs(float(r["r"])) + cap),
                         switch_margin(flt["rho"][t, s], flt["tau"][t, s], prr, flt["Ql"][t, s], flt["qa"][t, s], flags[3], flt["av"][t, s],
                                       fscale, flt["ex"][t, s], abs(flt["ex"][t, s] + cap) + cap))
        else:
            f = rflt[b]
            assert (bool(r["lo"]), bool(r["hi"]), bool(r["big"])) == (bool(f["lo"][t]), bool(f["hi"][t]), bool(f["big"][t])), (t, b)
            margin = min(margin, switch_margin(float(r["rho"]), float(r["tau"]), rr), switch_margin(f["rho"][t], f["tau"][t], rr))
    assert margin > 1e-6, margin
    # central differences, h = 1e-20 |x|; a reach parameter at a pool is not read: its derivative is 0
    h = M(10) ** -20
    want = dict(gx=[[None] * B for _ in range(T)], gpar=[[M(0)] * B for _ in range(3)], gpool=[[None] * P for _ in range(4)],
                gstate=[[None] * B for _ in range(2)])
    for name, base, idx, cols in (("gx", X0, range(T), range(B)), ("gpar", PM0, range(3), [b for b in range(B) if not pt.is_pool[b]]),
                                  ("gpool", PP0, (0, 1, 2, 4), range(P)), ("gstate", S0, range(2), range(B))):
        for o, i in enumerate(idx):
            for b in cols:
                v = base[i][b]
                assert v != 0
                vals = []
                for sgn in (1, -1):
                    base[i][b] = v + sgn * h * abs(v)
                    vals.append(net())
                base[i][b] = v
                want[name][o][b] = (vals[0] - vals[1]) / (2 * h * abs(v))
    # ---- the forward error recurrence on the real walk, in units of u (absolute errors)
    EL, EE = LN_BOUND / U, EXP_BOUND / U
    n_loc = max(float(r["beta"] * (EL * abs(r["L"]) + 2) + abs(r["tau"]) + EE + 1) for r in rows.values() if not r["pool"])
    dy, di, ds, delta, kappa, dlt_a, nq = {}, {}, {}, 0.0, 0.0, 0.0, 0.0
    dtm = M(dt)
    for b in (int(v) for v in pt.order):
        for t in range(T):
            r = rows[t, b]
            di[t, b] = sum(dy[t, u] for u in pt.ups[b]) + len(pt.ups[b]) * (abs(X0[t][b]) + sum(abs(rows[t, u]["O"]) for u in pt.ups[b]))
            delta = max(delta, float(di[t, b] / abs(r["I"])))
            if not r["pool"]:
                omx, KD = 1 - r["X"], r["K"] / r["D"]
                parts = ((r["X"] + abs(r["c0"]) * omx) * KD, (r["X"] + abs(r["c1"]) * omx) * KD, omx * (1 + abs(r["c2"])) * KD)
                A = abs(r["c0"] * r["I"]) + abs(r["c1"] * r["Ip"]) + abs(r["c2"] * r["Op"])
                W = parts[0] * abs(r["I"]) + parts[1] * abs(r["Ip"]) + parts[2] * abs(r["Op"])
                g = abs(r["c2"]) + (W * r["beta"] / abs(r["Op"]) if r["inside"] else 0)
                dy[t, b] = 11 * A + (n_loc + 6) * W + g * dy.get((t - 1, b), 0) + abs(r["c0"]) * di[t, b] + abs(r["c1"]) * di.get((t - 1, b), 0)
                delta = max(delta, float(dy[t, b] / abs(r["O"])))
                kappa = max(kappa, *(float(p / abs(c)) for p, c in zip(parts, (r["c0"], r["c1"], r["c2"]))))
                continue
            dvin = 2 * abs(r["vin"]) + (dtm / 2) * (di[t, b] + di.get((t - 1, b), 0))
            da = ds.get((t - 1, b), 0) + abs(r["a"])
            rel_a = da / abs(r["a"]) if r["a"] != 0 else 0  # (used in inside rows only, where a > 0)
            n_q = r["m"] * (EL * abs(r["L"]) + 1 + (rel_a + 1 if r["inside"] else 0)) + abs(r["tau"]) + EE + 1
            dav = da + dvin + abs(r["av"])
            dQ = 0 if r["empty"] else (n_q * abs(r["Ql"]) if r["free"] else dav / dtm + abs(r["qa"]))
            dr = dav + dtm * dQ + dtm * abs(r["Q"]) + abs(r["r"])
            if r["spill"]:
                dex = dr + abs(r["ex"])
                dy[t, b], ds[t, b] = dQ + dex / dtm + abs(r["ex"] / dtm) + abs(r["O"]), abs(r["S"])
            else:
                dy[t, b], ds[t, b] = dQ, dr + abs(r["S"])
            if r["O"] != 0:
                delta = max(delta, float(dy[t, b] / abs(r["O"])))
            if r["free"] and not r["empty"]:
                nq = max(nq, float(n_q))
                if r["inside"]:
                    dlt_a = max(dlt_a, float(rel_a))
    reach_rows = [r for r in rows.values() if not r["pool"]]
    Lmax, Z, bmax = (max(float(abs(r[k])) for r in reach_rows) for k in ("L", "tau", "beta"))
    n_K = bmax * (EL * Lmax + 2.0 + delta) + Z + EE + 1.0
    n_f = kappa * n_K + delta + 12.0
    n_reach = 2.0 * n_f + n_K + delta + 8.0
    n_pool = nq + dlt_a + delta + 12.0
    m_gx = int(np.ceil((T + pt.n_levels) * max(n_reach, n_pool)))
    m = dict(gx=m_gx, gstate=m_gx, gpar=int(np.ceil(m_gx + 2.0 * n_f + n_K + EL + T + 8.0)), gpool=int(np.ceil(m_gx + nq + dlt_a + EL + T + 8.0)))
    # ---- the adjoint on absolute values
    mag = dict(gx=[[None] * B for _ in range(T)], gpar=[[M(0)] * B for _ in range(3)], gpool=[[None] * P for _ in range(4)],
               gstate=[[None] * B for _ in range(2)])
    for b in (int(v) for v in pt.order[::-1]):
        s = int(pt.pool_slot[b])
        pI, pO, acc = M(0), M(0), [M(0)] * 4
        for t in range(T - 1, -1, -1):
            r = rows[t, b]
            av = abs(G[t][b]) + (mag["gx"][t][int(pt.down[b])] if pt.down[b] >= 0 else 0)
            if s < 0:
                omx, KD = 1 - r["X"], r["K"] / r["D"]
                lam = av + pO
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
                continue
            lamO, lamS = av, pO
            q = lamO / dtm
            gr = q if r["spill"] else lamS
            gcap = lamS + q
            gQ = 0 if r["empty"] else lamO + dtm * gr
            gav = gr if r["free"] else gr + gQ / dtm
            ga = gav + (gQ * r["m"] * abs(r["Ql"] / r["a"]) if r["free"] and r["inside"] else 0)
            if r["free"]:
                acc[0] += gQ * r["pw"]
                if not r["big"]:
                    acc[1] += gQ * abs(r["Ql"] * r["L"])
            acc[2] += (lamS + gcap if r["spill"] else lamS) + ga
            if r["spill"]:
                acc[3] += gcap
            hg = (dtm / 2) * gav
            mag["gx"][t][b] = hg + pI
            pI, pO = hg, ga
        mag["gstate"][0][b], mag["gstate"][1][b] = pI, pO
        if s < 0:
            for k in range(3):
                mag["gpar"][k][b] = acc[k]
        else:
            for k in range(4):
                mag["gpool"][k][s] = acc[k]
    cond = dict(margin=float(margin), delta=delta, kappa=kappa, n_K=n_K, n_f=n_f, nq=nq, delta_a=dlt_a, n_reach=n_reach, n_pool=n_pool)
    return dict(data=(pt, x, gy, pm, pp, state, dt, rr, prr), want=want, mag=mag, m=m, cond=cond, rows=rows)


def _ratios(d, got):
    """per output, error / bound of every element against the mpmath derivative (inf where the bound is 0 and the error is not)"""
    out = {}
    for k, arr in zip(("gx", "gpar", "gpool", "gstate"), got):
        r = np.zeros(arr.shape)
        for i in range(arr.shape[0]):
            for j in range(arr.shape[1]):
                err, bar = abs(mpmath.mpf(float(arr[i, j])) - d["want"][k][i][j]), mpmath.mpf(gamma(d["m"][k])) * d["mag"][k][i][j]
                r[i, j] = float(err / bar) if bar else (0.0 if err == 0 else np.inf)
        out[k] = r
    return out


def test_the_adjoint_is_the_true_derivative(derivative):
    """gx, gpar_mc, gpool and gstate of the host build against the derivatives of L = sum gy y of the definition's REAL-arithmetic
    statement over the whole mixed network, taken in mpmath at 60 digits by central differences with h = 1e-20 |x| (L is smooth
    between regime switches, and no row lies within a relative 1e-6 of one: rho against prmin and prmax, |tau| against ZMAX, Ql
    against qa, the smaller of the two against 0, ex against 0 -- asserted on the numpy statement and on the real walk, the float
    walk taking the real walk's branch in every row).  B = 7, T = 9, five levels, pools on four of them, one above the other and
    reaches above and below them; pool rows inside, clamped low, limited, empty and spilling all occur (asserted).

    The bound is gamma_m x (the same adjoint on absolute values: every factor and every term of a sum or difference by its
    absolute value), with the errors of mc_ln and gw_exp counted inside m.  Derivation, to first order in u, with figures taken
    from the real-arithmetic walk (never from the code under test):
      reach rows: tests/test_network_mc_host.py's derivation as it is -- the row's own forward error 11 A + (n_loc + 6) W, handed
        on with |c2| + W beta / |Op|; n_K, kappa, n_f = kappa n_K + delta + 12; a path pays 2 n_f + n_K + delta + 8 per reach
        row (n_reach).
      pool rows, forward.  vin rounds twice and takes half the errors of I and Iprev; a = S - s0 carries the error of S and one
        rounding (relative to |a| that is rel_a: the subtraction is where a forward error is magnified); rho and an unclamped
        rc carry rel_a + 1, a clamped rc is exact.  L = mc_ln(rc) is off by (E_ln |L| + rel_a + 1) u absolutely, tau = m L by m
        times that plus |tau| u, gw_exp adds E_exp and the product or quotient with cq one more:
        n_q = m (E_ln |L| + 1 + [inside](rel_a + 1)) + |tau| + E_exp + 1 relative to Ql.  av = a + vin, qa = av / dt, dt Q and
        r = av - dt Q round once each; Q carries n_q |Ql| (free), the error of qa (limited) or nothing (empty); a spill adds the
        roundings of ex, ex / dt and the sum to O and leaves S = cap + s0 with one rounding; else S = r + s0.  Every error is
        handed on by absolute value, so cancellation between av and dt Q is not relied on.  The recurrence runs on the real walk
        together with the reaches'; delta = the largest resulting error / u relative to |O| or |I| anywhere.
      pool rows, adjoint.  A path through a pool row passes at most the factors 1 / dt, dt, 1 / dt, m, Ql and 1 / a and four sums:
        12 roundings, the relative error n_q of Ql (the largest over the free rows: nq), that of a (the largest rel_a over the
        inside free rows: delta_a) and delta for the I in vin's place of the regime: n_pool = nq + delta_a + delta + 12.
      a path of the expansion of gx passes a row at most once and at most T + n_levels rows:
        m_gx = (T + n_levels) max(n_reach, n_pool); gstate is gx of a row before row 0.  A term of gpar_mc is as in the reach test:
        m_gx + 2 n_f + n_K + E_ln + T + 8.  A term of gpool is a path (<= m_gx) times one more factor -- rc^m (n_q), Ql L (n_q and
        E_ln) -- added into an accumulator <= T times: m_gpool = m_gx + nq + delta_a + E_ln + T + 8.
    The bound refuses, on every output the change reaches: the gQ m Ql / a term dropped (gx, gpar_mc, gpool, gstate), the limited
    branch's gQ / dt dropped (the same four), gcap with the wrong sign (gpool) and the row's own half gav in gx where the row
    above's belongs (the same four).
    Measured: worst error / bound = 2.82e-07 (gx), 6.73e-09 (gpar_mc), 7.16e-08 (gpool), 1.27e-08 (gstate), with m = 6177762 (gx,
    gstate), 6553588 (gpar_mc), 6201910 (gpool); delta = 65461, kappa = 2.86, n_reach = 441269, n_pool = 89595 (nq = 13946,
    delta_a = 10176), the nearest regime switch at a relative 0.032."""
    pt, x, gy, pm, pp, state, dt, rr, prr = derivative["data"]
    rows = [r for r in derivative["rows"].values() if r["pool"]]
    n = lambda f: sum(1 for r in rows if f(r))
    assert n(lambda r: r["inside"] and r["free"]) >= 9 and n(lambda r: r["lo"]) >= 9 and n(lambda r: not r["free"] and not r["empty"]) >= 9
    assert n(lambda r: r["empty"]) >= 1 and n(lambda r: r["spill"]) >= 3 and n(lambda r: not r["spill"]) >= 9
    y, _, sg = PH.route_pool_ref(pt, x, pm, pp, dt, rr, prr, state)
    got, = PH.run([("grad", pt, gy, x, y, sg, pm, pp, dt, rr, prr, state, True, True, True)])
    assert all(PH.same_bits(a, b) for a, b in zip(got, PH.route_pool_grad_ref(pt, gy, x, y, sg, pm, pp, dt, rr, prr, state)))
    got = (got[0], got[1], got[2][[0, 1, 2, 3]], got[3])
    rt = _ratios(derivative, got)
    print("pool adjoint vs mpmath derivative: worst error / bound = %.3g (gx), %.3g (gpar_mc), %.3g (gpool), %.3g (gstate); m = %r; %r"
          % (rt["gx"].max(), rt["gpar"].max(), rt["gpool"].max(), rt["gstate"].max(), derivative["m"], derivative["cond"]))
    assert all(v.max() <= 1.0 for v in rt.values()), {k: v.max() for k, v in rt.items()}
    assert all(v.max() > 0 for v in rt.values())  # (the data are general: something does round)
    everything = ("gx", "gpar", "gpool", "gstate")
    for variant, reached in (("no_dqda", everything), ("no_limited", everything), ("gcap_sign", ("gpool",)), ("pI_row", everything)):
        wrong = _ratios(derivative, PH.route_pool_grad_ref(pt, gy, x, y, sg, pm, pp, dt, rr, prr, state, variant=variant))
        assert all(wrong[k].max() > 1.0 for k in reached), (variant, {k: v.max() for k, v in wrong.items()})
        assert all(wrong[k].max() <= 1.0 for k in wrong if k not in reached), variant


# ---- 5. autograd --------------------------------------------------------------------------------------------------------------
def test_autograd_through_the_host_build(derivative):
    """network_route_pool on a CatchmentNetwork whose _open() alone is overridden, on the data of the derivative test: x, kref,
    beta, X, cq, m, s0, smax and state receive the bits of route_pool_grad_ref from one backward; qref and sref get none.  Scalar
    parameters receive the sum over the nodes; a state that requires no gradient gets none."""
    from lgar_py_amd.network import network_route_pool
    pt, x, gy, pm, pp, state, dt, rr, prr = derivative["data"]
    net = SimCatchmentNetworkPool(pt.down)
    pools = _pools(net, pt)
    leaf = lambda a: _t(a).clone().requires_grad_(True)
    tx, ts = leaf(x), leaf(state)
    reach, pool = [leaf(p) for p in pm], [leaf(p) for p in pp]
    y = network_route_pool(tx, net, pools, reach, pool, dt, state=ts)
    y_ref, _, sg = PH.route_pool_ref(pt, x, pm, pp, dt, rr, prr, state)
    assert PH.same_bits(y.detach().numpy(), y_ref)
    (y * _t(gy)).sum().backward()
    gx, gpar, gpool, gstate = PH.route_pool_grad_ref(pt, gy, x, y_ref, sg, pm, pp, dt, rr, prr, state)
    assert PH.same_bits(tx.grad.numpy(), gx) and PH.same_bits(np.stack([p.grad.numpy() for p in reach[:3]]), gpar)
    assert PH.same_bits(np.stack([pool[k].grad.numpy() for k in (0, 1, 2, 4)]), gpool) and PH.same_bits(ts.grad.numpy(), gstate)
    assert reach[3].grad is None and pool[3].grad is None
    assert float(np.abs(gpar[:, ~pt.is_pool]).min()) > 0 and float(np.abs(gpool).max(axis=1).min()) > 0
    # scalar parameters: summed gradients; a constant state; other ranges
    sc = lambda v: torch.tensor(v, dtype=torch.float64, requires_grad=True)
    sk, scq, ssm = sc(1.7), sc(0.8), sc(7.5)
    tx2 = leaf(x)
    y2 = network_route_pool(tx2, net, pools, (sk, 0.4, 0.1, 2.0), (scq, 1.5, 0.5, 2.0, ssm), dt, rmin=0.25, rmax=4.0, prmin=0.125, prmax=2.0,
                            state=_t(state))
    (y2 * _t(gy)).sum().backward()
    pm2 = np.stack([np.full(7, v) for v in (1.7, 0.4, 0.1, 2.0)])
    pp2 = np.stack([np.full(4, v) for v in (0.8, 1.5, 0.5, 2.0, 7.5)])
    y2_ref, _, sg2 = PH.route_pool_ref(pt, x, pm2, pp2, dt, (0.25, 4.0), (0.125, 2.0), state)
    g2 = PH.route_pool_grad_ref(pt, gy, x, y2_ref, sg2, pm2, pp2, dt, (0.25, 4.0), (0.125, 2.0), state)
    assert PH.same_bits(y2.detach().numpy(), y2_ref) and PH.same_bits(tx2.grad.numpy(), g2[0])
    for leaf_, want in ((sk, g2[1][0]), (scq, g2[2][0]), (ssm, g2[2][3])):
        assert PH.same_bits(leaf_.grad.numpy().reshape(1), _t(want).sum().numpy().reshape(1))
    with torch.no_grad():
        assert PH.same_bits(network_route_pool(_t(x), net, pools, [_t(p) for p in pm], [_t(p) for p in pp], dt).numpy(),
                            PH.route_pool_ref(pt, x, pm, pp, dt, rr, prr)[0])


# ---- 6. host logic ------------------------------------------------------------------------------------------------------------
def test_python_layer_names_and_rejections():
    import lgar_py_amd as lg
    from lgar_py_amd import LgarError, _capi
    from lgar_py_amd.network import CatchmentNetwork, NetworkPools, network_route_pool, weir_pool_parameters
    assert lg.network_route_pool is network_route_pool and lg.NetworkPools is NetworkPools and lg.weir_pool_parameters is weir_pool_parameters
    assert {"network_route_pool", "NetworkPools", "weir_pool_parameters"} <= set(lg.__all__)
    assert _capi.ABI_VERSION == 4 and {"lgar_network_route_pool", "lgar_network_route_pool_grad"} <= set(_capi.EXPORTS)
    net = SimCatchmentNetworkPool([1, 2, -1])
    for nodes, word in (([3], "no catchment"), ([-1], "no catchment"), ([1, 1], "twice"), ([[1]], r"\[P\]"), ([0.5], "integers"), ("a", "integers")):
        with pytest.raises(LgarError, match=word):
            NetworkPools(net, nodes)
    with pytest.raises(LgarError, match="CatchmentNetwork"):
        NetworkPools("net", [1])
    pools = NetworkPools(net, [1])
    assert pools.P == 1 and pools.order_host.tolist() == [0, 1, 2] and pools.pool_ptr.tolist() == [1, 1, 3] and pools.pool_slot_host.tolist() == [-1, 0, -1]
    assert NetworkPools(net, []).P == 0 and NetworkPools(net, torch.tensor([2, 0])).pool_slot_host.tolist() == [1, -1, 0]
    x = torch.ones(4, 3, dtype=torch.float64)
    p = torch.ones(3, dtype=torch.float64)
    one = torch.ones(1, dtype=torch.float64)
    reach, pool = (p, 0.4, 0.2, 1.0), (0.5, 1.5, 0.0, one, 10.0)
    y, sg = net.route_pool(x, pools, reach, pool, 1.0, return_storage=True)
    assert tuple(y.shape) == (4, 3) and tuple(sg.shape) == (4, 1) and tuple(net.pool_state_of().shape) == (2, 3)
    assert tuple(net.route_pool(x, NetworkPools(net, []), reach, (0.5, 1.5, 0.0, 1.0, 10.0), 1.0, carry=False).shape) == (4, 3)
    # a value is validated only where it is read: a bad reach parameter at the pool, a fine one elsewhere
    bad_at_pool = torch.tensor([1.0, -1.0, 1.0], dtype=torch.float64)
    assert tuple(net.route_pool(x, pools, (bad_at_pool, 0.4, 0.2, 1.0), pool, 1.0, carry=False).shape) == (4, 3)
    call = lambda reach=reach, pool=pool, pools=pools, x=x, dt_h=1.0, **kw: net.route_pool(x, pools, reach, pool, dt_h, **kw)
    inf, nan = float("inf"), float("nan")
    assert tuple(call(pool=(0.5, 1.5, 0.0, 1.0, inf), carry=False).shape) == (4, 3) and tuple(call(pool=(0.0, 0.0, 1.0, 1.0, 1.0), carry=False).shape) == (4, 3)
    for change, word in ((dict(reach=(torch.tensor([-1.0, 1.0, 1.0], dtype=torch.float64), 0.4, 0.2, 1.0)), r"kref\[0\]"),
                         (dict(reach=(p, 0.4, 0.6, 1.0)), "X"), (dict(reach=(p, 0.4, 0.2)), "reach must be"), (dict(pool=(0.5, 1.5, 0.0, 1.0)), "pool"),
                         (dict(pool=(-0.5, 1.5, 0.0, 1.0, 10.0)), "cq"), (dict(pool=(inf, 1.5, 0.0, 1.0, 10.0)), "cq"),
                         (dict(pool=(0.5, -1.0, 0.0, 1.0, 10.0)), r"m\[0\]"), (dict(pool=(0.5, 1.5, nan, 1.0, 10.0)), "s0"),
                         (dict(pool=(0.5, 1.5, 0.0, 0.0, 10.0)), "sref"), (dict(pool=(0.5, 1.5, 2.0, 1.0, 1.0)), "smax"),
                         (dict(pool=(0.5, 1.5, 0.0, 1.0, nan)), "smax"), (dict(pool=(0.5, 1.5, 0.0, 1.0, -inf)), r"pool at catchment 1"),
                         (dict(pool=(p, 1.5, 0.0, 1.0, 10.0)), r"fp64 \[1\]"), (dict(pool=("a", 1.5, 0.0, 1.0, 10.0)), "scalar"),
                         (dict(pools="pools"), "NetworkPools"), (dict(pools=NetworkPools(SimCatchmentNetworkPool([1, 2, -1]), [1])), "of this network"),
                         (dict(dt_h=0.0), "dt_h"), (dict(rmin=0.0), "rmin"), (dict(prmin=0.0), "prmin"), (dict(prmax=2.0 ** 61), "prmin"),
                         (dict(prmin=8.0, prmax=4.0), "prmin"), (dict(prmax="x"), "numbers"), (dict(x=x[:, :2]), r"3\] tensor"),
                         (dict(state=x), r"\[2, 3\]")):
        with pytest.raises(LgarError, match=word):
            call(**change)
    # the differentiable entry: no value validation (cq < 0 runs), shapes, the network and the pools are checked
    assert tuple(network_route_pool(x, net, pools, reach, (-0.5, 1.5, 0.0, 1.0, 10.0), 1.0).shape) == (4, 3)
    for bad in (lambda: network_route_pool(x, "net", pools, reach, pool, 1.0), lambda: network_route_pool(x.float(), net, pools, reach, pool, 1.0),
                lambda: network_route_pool(x, net, "pools", reach, pool, 1.0), lambda: network_route_pool(x, net, pools, reach[:3], pool, 1.0),
                lambda: network_route_pool(x, net, pools, reach, pool, 0.0), lambda: network_route_pool(x, net, pools, reach, pool, 1.0, prmin=0.0)):
        with pytest.raises(LgarError):
            bad()
    cpu = CatchmentNetwork([1, 2, -1], device="cpu")
    with pytest.raises(LgarError, match="no CPU fallback"):
        cpu.route_pool(x, NetworkPools(cpu, [1]), reach, pool, 1.0)


def test_weir_pool_parameters():
    """cq = Cw L href^1.5, m = 1.5, sref = area href / 3600 against the same formulas in mpmath; differentiable; the release of a
    pool with these parameters at head h is Cw L h^1.5 whatever href was chosen."""
    from lgar_py_amd.network import weir_pool_parameters
    area, length, cw, href = 2.5e6, 40.0, 1.7, 0.8
    cq, m, sref = weir_pool_parameters(area, length, cw, href)
    mpmath.mp.dps = 40
    M = mpmath.mpf
    assert abs(float(cq) - float(M(cw) * M(length) * M(href) ** M(1.5))) <= 1e-14 * float(cq) and float(m) == 1.5 and cq.dtype == torch.float64
    assert abs(float(sref) - float(M(area) * M(href) / 3600)) <= 1e-14 * float(sref)
    c1, m1, s1 = weir_pool_parameters(area, length, cw)
    assert float(c1) == cw * length and abs(float(s1) - area / 3600.0) <= 1e-12 * float(s1)
    h = 0.37  # Ql = cq (a / sref)^m with a = area h / 3600
    for c, s in ((cq, sref), (c1, s1)):
        assert abs(float(c) * (area * h / 3600.0 / float(s)) ** 1.5 / (cw * length * h ** 1.5) - 1.0) < 1e-14
    A = torch.tensor([2.5e6, 1.0e5], dtype=torch.float64, requires_grad=True)
    c2, m2, s2 = weir_pool_parameters(A, torch.tensor([40.0, 5.0], dtype=torch.float64), cw, href)
    s2.sum().backward()
    assert tuple(c2.shape) == (2,) and m2.tolist() == [1.5, 1.5] and torch.allclose(A.grad, torch.full((2,), href / 3600.0, dtype=torch.float64))


def test_entry_points_refuse_bad_arguments():
    """The refusals of the C-ABI wrappers (lgar_network_pool.hpp's own checks, which the host launchers call as the library does):
    LGAR_E_ARG = -1 for everything lgar_network_route_mc(_grad) refuses, prmin / prmax outside 2^-60 <= prmin <= prmax <= 2^60,
    P < 0, a null pool_ptr with n_levels > 0, a pool_ptr[l] outside its level, a pool segment with P = 0, with P > 0 a null
    par_pool or pool_slot, and the adjoint's null storage with T > 0 and P > 0.  The scalars are checked first."""
    lib = PH.library()
    buf = np.ones(512)
    ibuf = np.zeros(16, dtype=np.int32)
    p, q = buf.ctypes.data, ibuf.ctypes.data
    arr = lambda *v: np.array(v, dtype=np.int32)
    level_ptr, bad_levels, pool_ptr, no_pools, below, above = arr(0, 4), arr(0, 3), arr(2), arr(4), arr(-1), arr(5)
    fwd = (("x", p), ("T", 2), ("B", 4), ("par", p), ("par_pool", p), ("P", 2), ("dt", 1.0), ("rmin", 1 / 64), ("rmax", 64.0), ("prmin", 2.0 ** -20),
           ("prmax", 2.0 ** 20), ("up_ptr", q), ("up_idx", q), ("E", 1), ("order", q), ("level_ptr", level_ptr.ctypes.data),
           ("pool_ptr", pool_ptr.ctypes.data), ("L", 1), ("pool_slot", q), ("state_in", None), ("state_out", p + 512), ("y", p + 1024),
           ("storage", p + 2048))
    run = lambda **kw: lib.networkpoolhost_network_route_pool(*[kw.get(k, d) for k, d in fwd])
    assert run() == 0
    nan, inf = float("nan"), float("inf")
    scalars = (dict(dt=0.0), dict(dt=-1.0), dict(dt=nan), dict(dt=inf), dict(rmin=nan), dict(rmax=inf), dict(rmin=2.0 ** -61), dict(rmin=65.0),
               dict(prmin=nan), dict(prmax=nan), dict(prmax=inf), dict(prmin=-inf), dict(prmin=2.0 ** -61), dict(prmax=2.0 ** 61),
               dict(prmin=2.0 ** 21), dict(prmin=0.0), dict(B=0, prmin=0.0), dict(B=0, dt=0.0))
    pool_args = (dict(P=-1), dict(B=0, P=-1), dict(pool_ptr=None), dict(pool_ptr=below.ctypes.data), dict(pool_ptr=above.ctypes.data),
                 dict(P=0), dict(P=0, par_pool=None, pool_slot=None), dict(par_pool=None), dict(pool_slot=None))
    for bad in (dict(T=-1), dict(B=-1), dict(E=-1), dict(L=-1), dict(x=None), dict(par=None), dict(T=0, par=None), dict(y=None), dict(up_ptr=None),
                dict(up_idx=None), dict(order=None), dict(level_ptr=None), dict(level_ptr=bad_levels.ctypes.data)) + scalars + pool_args:
        assert run(**bad) == -1, bad
    assert run(prmin=2.0 ** -60, prmax=2.0 ** 60) == 0 and run(prmin=3.0, prmax=3.0) == 0 and run(E=0, up_idx=None) == 0 and run(storage=None) == 0
    assert run(P=0, par_pool=None, pool_slot=None, storage=None, pool_ptr=no_pools.ctypes.data) == 0
    assert run(B=0, x=None, par=None, y=None, level_ptr=None, pool_ptr=None) == 0 and run(T=0, state_out=None, x=None, y=None) == 0
    assert run(L=0, B=0, pool_ptr=None, level_ptr=arr(0).ctypes.data) == 0
    buf[64:72] = 7.0
    assert run(T=0, x=None, y=None) == 0 and buf[64].tolist() == 0.0  # T = 0, no state_in: zeros (every lane is node 0 here)
    grd = (("gy", p), ("T", 2), ("B", 4), ("par", p), ("par_pool", p), ("P", 2), ("dt", 1.0), ("rmin", 1 / 64), ("rmax", 64.0), ("prmin", 2.0 ** -20),
           ("prmax", 2.0 ** 20), ("down", q), ("order", q), ("level_ptr", level_ptr.ctypes.data), ("pool_ptr", pool_ptr.ctypes.data), ("L", 1),
           ("pool_slot", q), ("gx", p + 512), ("x", p), ("y", p), ("storage", p), ("up_ptr", q), ("up_idx", q), ("E", 1), ("state_in", None),
           ("gpar", p + 1024), ("gpool", p + 1536), ("gstate", p + 2048))
    grad = lambda **kw: lib.networkpoolhost_network_route_pool_grad(*[kw.get(k, d) for k, d in grd])
    assert grad() == 0
    for bad in (dict(T=-1), dict(B=-1), dict(E=-1), dict(L=-1), dict(gy=None), dict(par=None), dict(T=0, par=None), dict(down=None), dict(order=None),
                dict(gx=None), dict(x=None), dict(y=None), dict(up_ptr=None), dict(up_idx=None), dict(level_ptr=None),
                dict(level_ptr=bad_levels.ctypes.data), dict(x=None, gpar=None, gpool=None, gstate=None), dict(storage=None)) + scalars + pool_args:
        assert grad(**bad) == -1, bad
    assert grad(gpar=None) == 0 and grad(gpool=None) == 0 and grad(gstate=None) == 0 and grad(gpar=None, gpool=None, gstate=None) == 0
    assert grad(E=0, up_idx=None) == 0 and grad(T=0, storage=None) == 0
    assert grad(P=0, par_pool=None, pool_slot=None, storage=None, gpool=None, pool_ptr=no_pools.ctypes.data) == 0
    assert grad(B=0, gy=None, gx=None, level_ptr=None, pool_ptr=None) == 0 and grad(T=0, gpar=None, gpool=None, gstate=None, gy=None, x=None) == 0
    buf[128] = buf[192] = buf[256] = 7.0
    assert grad(T=0, gy=None, gx=None, x=None, y=None, storage=None) == 0 and buf[128] == 0.0 and buf[192] == 0.0 and buf[256] == 0.0  # T = 0: zeros
    buf[192] = 7.0
    assert grad(T=0, gpar=None, gstate=None, gy=None, gx=None, x=None, y=None) == 0 and buf[192] == 0.0  # gpool alone is wanted: written
