"""TEST INFRASTRUCTURE ONLY: what the host test and the GPU test of the fp32 leaves share -- running a leaf op over the fixture's
points through either backend, the bound check, the exact edges; further down the same for the tangent leaves
(lgar_leaf_tangent_batch against tests/golden/leaf_tangent/leaf_tangent_ref.npz).  numpy only.

A backend is a function batch(op, x, y, z, alpha=, n=, ksat=, theta_e=, theta_r=, nint=) -> fp32 numpy array: leaf_host.leaf_batch for
the host build, lgar_py_amd.leaf_batch(dtype=float32) behind a small wrapper for the hardware."""
import numpy as np

import leaf_ref as R

F = np.float32
NINT = 120
LOG2_1EM12 = F(-39.863137)  # the trapezoid's own literal (lgar_geff.hpp)


def soil_kw(S, idx):
    return dict(alpha=S[idx, 0], n=S[idx, 1], ksat=S[idx, 2], theta_e=S[idx, 3], theta_r=S[idx, 4])


def run(batch, op, S, d):
    """The op over the points d (a function's dict of the fixture): one call per distinct z."""
    got = np.empty(len(d["x"]), dtype=F)
    for z in np.unique(d["z"]):
        w = d["z"] == z
        got[w] = batch(op, d["x"][w], d["y"][w], float(z), nint=NINT, **soil_kw(S, d["soil"][w]))
    return got


def ulp_of(ref):
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.floor(np.log2(np.abs(ref)))
    e = np.where(np.isfinite(e), e, -126.0)
    return np.exp2(np.maximum(e, -126.0) - 23.0)


def same_class(got, ref):
    """NaN where the reference is NaN, the same infinity where it is infinite, finite where it is finite."""
    g = got.astype(np.float64)
    return (np.isnan(g) == np.isnan(ref)) & (np.isposinf(g) == np.isposinf(ref)) & (np.isneginf(g) == np.isneginf(ref))


def against_fixture(name, op, got, d, units, soil_names):
    """Assert |got - ref| <= FACTOR sum_k coef_k u_k at every point, the class rule for NaN / inf and its 2 % cap; returns the line
    of the table: worst error in ulp, worst error / bound and where."""
    ref, g = d["ref"], got.astype(np.float64)
    finite = np.isfinite(ref)
    cls = same_class(got, ref)
    assert cls.all(), "%s op %d: %d points of another class than the statement's, first: soil %s x %r got %r ref %r" % (
        name, op, int((~cls).sum()), soil_names[d["soil"][~cls][0]], d["x"][~cls][0], got[~cls][0], ref[~cls][0])
    assert (~finite).sum() <= 0.02 * len(ref), (name, int((~finite).sum()), len(ref))
    b = R.FACTOR * R.bound(d["coef"], units)
    with np.errstate(invalid="ignore"):
        err = np.where(finite, np.abs(g - ref), 0.0)
        ratio = np.where(finite & np.isfinite(b) & (b > 0), err / np.where(b > 0, b, 1.0), 0.0)
        ratio = np.where(finite & (b == 0) & (err > 0), np.inf, ratio)
        ulps = np.where(finite & np.isfinite(b), err / ulp_of(ref), 0.0)
    i, j = int(np.argmax(ratio)), int(np.argmax(ulps))
    where = lambda k: "%s x=%.9g y=%.9g" % (soil_names[d["soil"][k]], d["x"][k], d["y"][k])
    line = "%-16s op %2d: %4d points, %3d inf/NaN, %3d unbounded; worst %.1f ulp (%s); worst error / bound %.3f (%s)" % (
        name, op, len(ref), int((~finite).sum()), int((finite & np.isinf(b)).sum()), ulps[j], where(j), ratio[i], where(i))
    print(line)
    assert ratio[i] <= 1.0, "outside the bound: " + line + " got %r ref %r bound %r" % (got[i], ref[i], b[i])
    return line


def exact_edges(batch, S, soil_names):
    """The equalities the kernels rest on, for every soil of the fixture and both policies.  IEEE operations (the layer's m, Se =
    (theta - theta_r) / (theta_e - theta_r), sums and products) are restated in numpy fp32; the platform's own pow and exp2 come
    from leaf ops 9 and 8."""
    n = len(S)
    kw = soil_kw(S, np.arange(n))
    te, tr, ksat = S[:, 3], S[:, 4], S[:, 2]
    m = F(1) - F(1) / S[:, 1]
    call = lambda op, x, y=None, z=0.0: batch(op, np.asarray(x, dtype=F), None if y is None else np.asarray(y, dtype=F), z, nint=NINT, **kw)
    full = lambda v: np.full(n, v, dtype=F)
    for op_theta, op_k, op_h in ((0, 2, 3), (17, 19, 20)):
        # theta_from_h(0): the pow part contributes exactly 1
        assert np.array_equal(call(op_theta, full(0.0)), (te - tr) + tr), op_theta
        # an overflowed (alpha h)^n gives exactly theta_r, not NaN
        assert np.array_equal(call(op_theta, full(np.finfo(F).max)), tr), op_theta
        # k_from_se(1) is k_from_se_one: Ksat sqrt(1) (1 - (1e-12)^m)^2 with the platform's pow
        t = F(1) - call(9, full(1e-12), m)
        assert np.array_equal(call(op_k, full(1.0)), (ksat * F(1)) * (t * t)), op_k
    # Se(theta_e) == 1 exactly: the trapezoid up to theta_e ends at the head of Se = 1 and no other (a Se of 1 - 2^-24 has a head
    # a thousand times larger)
    t1 = np.minimum((tr + F(0.5) * (te - tr)).astype(F), te)
    se_i = ((t1 - tr) / (te - tr)).astype(F)
    assert np.array_equal(call(4, t1, te), call(22, call(3, se_i), call(3, full(1.0))))
    # geff(theta, theta) == 0
    assert np.array_equal(call(4, t1, t1), full(0.0)) and np.array_equal(call(4, te, te), full(0.0))
    assert np.array_equal(call(22, full(50.0), full(50.0)), full(0.0))
    # a node below the cut contributes K_r(1) = (1 - 2^(m log2(1e-12)))^2: with both heads under it every node does
    tsat = F(1) - call(8, (m * LOG2_1EM12).astype(F))
    ksat1 = (tsat * tsat).astype(F)
    h_i, h_f = F(0.05), F(0.01)
    dh = F(F(h_f - h_i) * F(F(1) / F(NINT)))
    acc = np.zeros((2, 2, n), dtype=F)
    for p in range((NINT - 1) >> 1):
        acc[p & 1] = acc[p & 1] + ksat1
    a = acc[0] + acc[1]
    total = (a[0] + a[1]) + ksat1  # (nint - 1 is odd: one more node)
    want = np.abs((F(0.5) * dh) * ((ksat1 + ksat1) + F(2) * total)).astype(F)
    assert np.array_equal(call(22, full(h_i), full(h_f)), want)


def theta_stays_in_the_domain(batch, S, d, soil_names):
    """theta(h) > theta_e for some h >= 0 would be Se > 1: outside the domain, a fault to the engine.  Reported per op; an excess
    can only be rounding (the bound test), never more than an ulp of theta_e, and there is none at h = 0 (exact_edges)."""
    for op in (0, 17):
        got = run(batch, op, S, d)
        over = got > S[d["soil"], 3]
        print("theta_from_h op %d: %d of %d points above theta_e%s" % (op, int(over.sum()), len(got), "".join(
            "\n    %s h=%.9g: theta_e + %.3g" % (soil_names[d["soil"][k]], d["x"][k], float(got[k]) - float(S[d["soil"][k], 3]))
            for k in np.nonzero(over)[0][:8])))
        assert (got[over].astype(np.float64) - S[d["soil"][over], 3] <= 2.0 ** -24).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the tangent leaves (lgar_leaf_tangent_batch) against tests/golden/leaf_tangent/leaf_tangent_ref.npz (leaf_ref.tangent)
#
# A tangent backend is a function tbatch(op, x, y, z, seeds=, policy=, dtype=, alpha=, n=, ksat=, theta_e=, theta_r=, nint=) ->
# (value, tangent), numpy arrays of `dtype`: leaf_host.leaf_tangent_batch, or lgar_py_amd.leaf_tangent_batch behind a wrapper.
# ---------------------------------------------------------------------------------------------------------------------------
MARGIN = 8.0              # of the tolerance below; fixed in advance (three factors of 2: the lean log2 / exp2 stated at 2.5e-16
                          # against libm's half ulp, fast_recip at ~1 ulp against 0.5, the fused node's and lean_div's other order)
EPS_FLOOR = 4.0 * 2.0 ** -53  # ... times |D|: where the reference's own error is accidentally nothing
# Four RECORDED CONDITIONINGS widen that bar, each by a term that follows from the arithmetic alone (never from what the code under
# test returns); DESIGN.md section 4 has the measurements that called for them:
# 1. A partial that is a difference of large terms -- the AET along theta_e and theta_r (psi_wp does not depend on them: the terms
#    cancel to nothing, the statement's D is 0 to 1e-44), Geff along Ksat (the sum's dKsat against G / Ksat: D is exactly 0) --
#    carries rounding in proportion to the TERMS: the floor is 4 2^-53 A with A the terms added up by absolute value (the
#    fixture's `cond`, A == |D| wherever nothing cancels), not 4 2^-53 |D| = 0.
# 2. The lean pow (POL_LEAN, pw) is 2^(y log2 x): its relative error grows with |y log2 x|, up to 8e-16 max(1, |y log2 x|) as
#    tests/test_device_math.py asserts it -- at |y log2 x| = 95 that is 7.6e-14, where the reference's torch.pow stays at half
#    an ulp, so no reference error measures it.  A tangent inherits it twice (the value; the logarithm it shares with d/dy):
#    2 x 8e-16 max(1, T) A with T the largest |y log2 x| among the point's pows (the fixture's `powt`).  POL_LIBRARY gets none.
# 3. The exponents.  Reference and kernels form m = fl(1 - fl(1 / n)) and 1 / m in double precision; the statement forms them
#    exactly.  fl(1 / n) is off by up to 2^-53 / n, the difference by 2^-53 m more, the reciprocal by one rounding more: a relative
#    error of up to 2^-53 (2 + 1 / (n m)) in an exponent y -- 4 ulp for n = 1.46, 13 for n = 1.09.  x^y answers a relative error
#    eps of y with |y ln x| eps = T ln 2 eps, and its tangent y x^(y-1) once more with eps: (max(1, T) ln 2 + 1) 2^-53
#    (2 + 1 / (n m)) A.  The reference carries the same rounding (the same bits of m), so E_ref as a rule holds it already; the
#    term is the floor for where the reference's later roundings happen to offset it (h_from_se at Se = 1e-6, n = 1.46: the
#    exponent's rounding alone is 3.9e-15 of D, the reference ends 4.5e-16 from the statement).  Leaves only: no primitive forms m.
# 4. The trapezoid's tangent running sum (the two trapezoids only): the fixture's `drift`, an absolute bound added as it stands --
#    leaf_ref.tangent.drift derives it.  Forward mode walks h2.d += dh.d next to h2 += dh; reverse mode has no such sum.
LEAN_POW_REL = 8e-16
NEIGHBOURS = 2            # on either side, along the operand axis, same soil
LEAN, LIBRARY = 0, 1
NSEED = 7


def tangent_run(tbatch, op, S, d, seeds, policy=LEAN, dtype=np.float64, idx=None):
    """(value, tangent) of the op over the points d[idx] along `seeds` ([N, 7], or None): one call per distinct z."""
    idx = np.arange(len(d["x"])) if idx is None else np.asarray(idx)
    val, tan = np.empty(len(idx), dtype=dtype), np.empty(len(idx), dtype=dtype)
    names = ("alpha", "n", "ksat", "theta_e", "theta_r", "x", "y")
    for z in np.unique(d["z"][idx]):
        w = d["z"][idx] == z
        i = idx[w]
        sd = None if seeds is None else {k: seeds[w, j] for j, k in enumerate(names) if np.any(seeds[w, j] != 0)}
        val[w], tan[w] = tbatch(op, d["x"][i], d["y"][i], float(z), seeds=sd, policy=policy, dtype=dtype, nint=NINT, **soil_kw(S, d["soil"][i]))
    return val, tan


def tangent_tolerance(d, d_ref_statement=None, lean_pow=False, S=None):
    """[N, 7]: MARGIN max(E_ref, 4 2^-53 A) -- A the statement's partial D with its terms added up by absolute value (|D| itself
    where nothing cancels), E_ref the largest |reference autograd - statement| over the point and its NEIGHBOURS neighbours on
    either side in the same soil (where the reference raises: no contribution) -- plus, for the lean pow, 2 x 8e-16 max(1, T) A;
    with the soils S (a leaf: its exponents come from n) the exponents' rounding; for the trapezoids the tangent sum's drift.
    d_ref_statement: the fixture entry whose statement the REFERENCE evaluates where that is not d's own (the fused trapezoid is
    held to the statement without the nudge; the reference computes the one with it)."""
    D = d["grad"]
    with np.errstate(invalid="ignore"):
        e = np.abs(d["ref_grad"] - (D if d_ref_statement is None else d_ref_statement["grad"]))
    e = np.where(np.isfinite(e), e, 0.0)
    E = e.copy()
    soil = d["soil"]
    for s in range(1, NEIGHBOURS + 1):
        same = soil[s:] == soil[:-s]
        E[s:] = np.maximum(E[s:], np.where(same[:, None], e[:-s], 0.0))
        E[:-s] = np.maximum(E[:-s], np.where(same[:, None], e[s:], 0.0))
    A = np.maximum(np.abs(np.where(np.isfinite(D), D, 0.0)), np.where(np.isfinite(d["cond"]), d["cond"], 0.0).astype(np.float64))
    tol = MARGIN * np.maximum(E, EPS_FLOOR * A)
    if lean_pow:
        tol = tol + 2.0 * LEAN_POW_REL * np.maximum(1.0, d["powt"].astype(np.float64))[:, None] * A
    if S is not None:
        n = S[d["soil"], 1]
        m = 1.0 - 1.0 / n
        eps_y = 2.0 ** -53 * (2.0 + 1.0 / (n * m))
        tol = tol + ((np.maximum(1.0, d["powt"].astype(np.float64)) * np.log(2.0) + 1.0) * eps_y)[:, None] * A
    return tol + d["drift"].astype(np.float64)


# what runs the lean pow under POL_LEAN: the leaves (the fused trapezoid's node has none, its end points do) and pw itself
LEAN_POW_OPS = ("theta_from_h", "se_from_h", "k_from_se", "h_from_se", "aet", "geff_closed", "geff", "pw")


# the leaves whose exponents are m, 1 / m, 1 / n (se_from_theta has none)
M_EXPONENT_OPS = ("theta_from_h", "se_from_h", "k_from_se", "h_from_se", "aet", "geff_closed", "geff", "geff_literal")


def _classes_agree(got, ref):
    return (np.isnan(got) == np.isnan(ref)) & (np.isposinf(got) == np.isposinf(ref)) & (np.isneginf(got) == np.isneginf(ref))


SEED_NAMES = ("alpha", "n", "ksat", "theta_e", "theta_r", "x", "y")


def tangent_against_fixture(name, op, tbatch, S, d, soil_names, policy=LEAN, d_ref_statement=None, rng_seed=7):
    """Double precision: each of the 7 partials, one unit seed at a time, and one random mixed direction, within the tolerance of
    the statement; the statement's class where it is inf / NaN (at most 2 % of the points).  Returns the table's lines: worst
    error / tolerance per partial and where."""
    n = len(d["x"])
    D, tol = d["grad"], tangent_tolerance(d, d_ref_statement, lean_pow=(policy == LEAN and name in LEAN_POW_OPS),
                                          S=S if name in M_EXPONENT_OPS else None)
    bad = ~(np.isfinite(d["value"]) & np.isfinite(D).all(axis=1))
    assert bad.sum() <= 0.02 * n, (name, int(bad.sum()), n)
    where = lambda k: "%s x=%.17g y=%.9g" % (soil_names[d["soil"][k]], d["x"][k], d["y"][k])
    lines, failures = [], []
    rng = np.random.default_rng(rng_seed)
    mixed = rng.uniform(-1.0, 1.0, (n, NSEED))
    for j in range(NSEED + 1):
        seeds = mixed if j == NSEED else np.eye(NSEED)[np.full(n, j)]
        val, tan = tangent_run(tbatch, op, S, d, seeds, policy)
        want = (np.where(np.isfinite(D), D, 0.0) * seeds).sum(axis=1)
        t = (tol * np.abs(seeds)).sum(axis=1)
        vcls = _classes_agree(val, d["value"])
        assert vcls.all(), "%s op %d: value of another class than the statement's at %s: %r for %r" % (
            name, op, where(int(np.argmin(vcls))), val[~vcls][0], d["value"][~vcls][0])
        # a point whose statement is inf / NaN (outside the domain: Se > 1): the tangent is of the statement's class -- along every
        # unit seed, also one the function does not depend on, and along the mixed direction
        if bad.any():
            with np.errstate(invalid="ignore"):
                want_bad = (D[bad] * seeds[bad]).sum(axis=1) if j == NSEED else D[bad, j]
            tcls = _classes_agree(tan[bad], want_bad)
            assert tcls.all(), "%s op %d %s: tangent %r where the statement is %r, at %s" % (
                name, op, "mixed" if j == NSEED else SEED_NAMES[j], tan[bad][~tcls][0], want_bad[~tcls][0], where(int(np.nonzero(bad)[0][np.argmin(tcls)])))
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.where(bad, 0.0, np.abs(tan - want))
            err = np.where(np.isnan(err), np.inf, err)  # a NaN tangent where the statement is finite is an error of any size
            ratio = np.where(err == 0, 0.0, np.where(t > 0, err / np.where(t > 0, t, 1.0), np.inf))
            rel = np.where((err > 0) & (want != 0), err / np.abs(np.where(want != 0, want, 1.0)), 0.0)
        k = int(np.argmax(ratio))
        label = "mixed" if j == NSEED else "d/d" + SEED_NAMES[j]
        line = "%-14s op %2d %-8s %-10s %5d points: worst error / tolerance %8.3g (%s: got %.17g, statement %.17g, tolerance %.3g); worst relative error %.2e" % (
            name, op, "library" if policy == LIBRARY else "lean", label, n, ratio[k], where(k), tan[k], want[k], t[k], float(rel.max()))
        print(line)
        lines.append(line)
        if not ratio[k] <= 1.0:
            failures.append(line)
    assert not failures, "beyond the tolerance:\n" + "\n".join(failures)
    return lines


def tangent_values(name, op, leaf_op, tbatch, batch, S, d, dtype, policy=LEAN, exact=True):
    """The value the tangent entry returns is the leaf entry's, bit for bit (leaf_op: the op number there, None: no counterpart),
    and does not depend on the seeds."""
    n = len(d["x"])
    idx = np.arange(n) if dtype == np.float64 else np.nonzero(d["f32ok"])[0]
    rng = np.random.default_rng(11)
    v0, t0 = tangent_run(tbatch, op, S, d, None, policy, dtype, idx)
    v1, _ = tangent_run(tbatch, op, S, d, rng.uniform(-2.0, 2.0, (len(idx), NSEED)), policy, dtype, idx)
    bits = lambda a: a.view(np.uint64 if a.dtype == np.float64 else np.uint32)
    assert np.array_equal(bits(v0), bits(v1)), "%s op %d: the value depends on the seeds" % (name, op)
    assert np.all(t0[~np.isnan(t0)] == 0), "%s op %d: a tangent without a seed" % (name, op)
    if leaf_op is None:
        return None
    got = np.empty(len(idx), dtype=dtype)
    for z in np.unique(d["z"][idx]):
        w = d["z"][idx] == z
        i = idx[w]
        got[w] = batch(leaf_op, d["x"][i], d["y"][i], float(z), nint=NINT, dtype=dtype, **soil_kw(S, d["soil"][i]))
    differ = bits(v0) != bits(got)
    differ &= ~(np.isnan(v0) & np.isnan(got))
    print("%-14s op %2d / leaf op %2d %s: %d of %d values differ from the leaf entry's" % (name, op, leaf_op, np.dtype(dtype).name, int(differ.sum()), len(idx)))
    if exact:
        assert not differ.any(), (name, op, d["x"][idx][differ][0], v0[differ][0], got[differ][0])
    return differ


def tangent_f32(name, op, tbatch, S, d, soil_names, policy=LEAN, library_too=False):
    """Single precision: value and tangent are of the statement's class -- NaN where it is NaN (outside the domain), finite where it
    and its derivative are fp32 numbers of ordinary size (beyond that fp32 may overflow or flush where double precision does not:
    counted in the line, not held to a class); the error against the statement is measured and reported, not asserted (no
    derivable fp32 tangent bound yet).  library_too: POL_LIBRARY gives the same bits as POL_LEAN (in float the library pow IS the
    lean one, pwx in lgar_scalar.hpp)."""
    idx = np.nonzero(d["f32ok"])[0]
    D = d["grad"][idx]
    lines = []
    ordinary = lambda a: np.isfinite(a) & ((a == 0) | ((np.abs(a) > 1e-30) & (np.abs(a) < 1e30)))
    nan_stmt = np.isnan(d["value"][idx]) & np.isnan(D).all(axis=1)
    assert (nan_stmt | (np.isfinite(d["value"][idx]) & np.isfinite(D).all(axis=1))).all(), name  # (the statement has no other class here)
    for j in range(NSEED):
        seeds = np.eye(NSEED)[np.full(len(idx), j)]
        val, tan = tangent_run(tbatch, op, S, d, seeds, policy, F, idx)
        if library_too:
            val2, tan2 = tangent_run(tbatch, op, S, d, seeds, LIBRARY, F, idx)
            assert np.array_equal(val.view(np.uint32), val2.view(np.uint32)) and np.array_equal(tan.view(np.uint32), tan2.view(np.uint32)), (name, op, SEED_NAMES[j])
        assert np.isnan(val[nan_stmt]).all() and np.isnan(tan[nan_stmt]).all(), "%s op %d d/d%s: fp32 value / tangent not NaN where the statement is" % (name, op, SEED_NAMES[j])
        ok = ordinary(d["value"][idx]) & ordinary(D).all(axis=1)
        assert np.isfinite(val[ok]).all(), (name, op)
        cls = np.isfinite(tan[ok])
        assert cls.all(), "%s op %d d/d%s: fp32 tangent %r where the statement is finite, at %s x=%r y=%r" % (
            name, op, SEED_NAMES[j], tan[ok][~cls][0], soil_names[d["soil"][idx][ok][~cls][0]], d["x"][idx][ok][~cls][0], d["y"][idx][ok][~cls][0])
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(ok & (D[:, j] != 0), np.abs(tan.astype(np.float64) - D[:, j]) / np.abs(np.where(D[:, j] != 0, D[:, j], 1.0)), 0.0)
        k = int(np.argmax(rel))
        line = "%-14s op %2d fp32 d/d%-8s %5d points (%d ordinary, %d NaN): median relative error %.2e, worst %.2e (%s x=%.9g y=%.9g)" % (
            name, op, SEED_NAMES[j], len(idx), int(ok.sum()), int(nan_stmt.sum()), float(np.median(rel[ok & (D[:, j] != 0)])) if (ok & (D[:, j] != 0)).any() else 0.0,
            rel[k], soil_names[d["soil"][idx][k]], d["x"][idx][k], d["y"][idx][k])
        print(line)
        lines.append(line)
    return lines


def tangent_departures(tbatch):
    """The two places where lgar_dual.hpp deliberately departs from torch's derivative (leaf_ref.tangent's docstring): asserted
    AS departures -- the kernel's convention is pinned, torch's figure is stated next to it."""
    one = np.ones(3)
    kw = dict(alpha=one, n=one + 0.5, ksat=one, theta_e=one, theta_r=one * 0, nint=NINT)
    x, y = np.array([-2.0, -0.5, -1e-300]), np.array([3.0, 2.0, 1.0])  # torch.pow: d/dx = y x^(y-1) = 12, -2, 1
    for dtype in (np.float64, F):
        xx = x if dtype == np.float64 else np.array([-2.0, -0.5, -1e-30])
        for op in (9, 25):  # pw, pwx<true>
            for seeds in (dict(x=one), dict(y=one), dict(x=one, y=one)):
                _, tan = tbatch(op, xx, y, 0.0, seeds=seeds, policy=LEAN, dtype=dtype, **kw)
                assert np.array_equal(tan, np.zeros(3, dtype=dtype)), ("pw drops the tangent at x < 0", op, dtype, seeds, tan)
        val, tan = tbatch(16, np.zeros(3), None, 0.0, seeds=dict(x=one), policy=LEAN, dtype=dtype, **kw)  # torch.sqrt: inf
        assert np.array_equal(val, np.zeros(3, dtype=dtype)) and np.array_equal(tan, np.zeros(3, dtype=dtype)), ("sq gives 0 at 0", dtype, tan)


def aet_clamp_regimes(tbatch, S, d, dtypes=(np.float64, F)):
    """The AET's clamp, torch.clamp(a, 0, pet): the fixture reaches all of its regimes, the statement has torch's derivative in each
    of them, and the kernel returns it EXACTLY where it is a constant of the arithmetic -- below 0: value 0, every partial 0; above
    pet: value pet, d/dpet = 1, every other partial 0; the exact tie a == pet (psi = 0, dt = 1): the argument's own tangent, which
    is d/dpet = 1 and 0 along psi there.  (tangent_against_fixture holds the same points to the tolerance, which is 0 wherever
    the statement and the reference are.)"""
    pet, dt, v, g = d["y"], d["z"], d["value"], d["grad"]
    lower = (v == 0) & (d["x"] < 0)
    upper = (v == pet) & (dt > 1)
    tie = (v == pet) & (dt == 1) & (d["x"] == 0)
    inside = (v > 0) & (v < pet)
    print("aet: %d points below 0, %d above pet, %d exact ties, %d inside" % (lower.sum(), upper.sum(), tie.sum(), inside.sum()))
    assert lower.sum() >= 40 and upper.sum() >= 40 and tie.sum() >= 20 and inside.sum() >= 600 and (lower | upper | tie | inside).all()
    unit_pet = np.zeros(NSEED); unit_pet[6] = 1.0
    assert (g[lower] == 0).all() and (g[upper] == unit_pet).all() and (g[tie][:, 6] == 1).all() and (g[tie][:, 5] == 0).all()
    # the reference's own autograd says the same (the lower clamp is reached through a negative psi, where the reference's pow
    # guard raises: no reference there)
    assert np.array_equal(d["ref_grad"][upper], g[upper]) and np.isnan(d["ref_grad"][lower]).all()
    for dtype in dtypes:
        for policy in (LEAN, LIBRARY):
            for which, want_pet in ((lower, 0.0), (upper, 1.0)):
                idx = np.nonzero(which & (d["f32ok"] == 1))[0] if dtype == F else np.nonzero(which)[0]
                for j in range(NSEED):
                    val, tan = tangent_run(tbatch, 5, S, d, np.eye(NSEED)[np.full(len(idx), j)], policy, dtype, idx)
                    assert np.array_equal(val, (pet[idx] * want_pet).astype(dtype)), (dtype, policy, want_pet)
                    assert np.array_equal(tan, np.full(len(idx), want_pet if j == 6 else 0.0, dtype=dtype)), (dtype, policy, want_pet, SEED_NAMES[j], tan)
