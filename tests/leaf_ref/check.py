"""TEST INFRASTRUCTURE ONLY: what the host test and the GPU test of the fp32 leaves share -- running a leaf op over the fixture's
points through either backend, the bound check, the exact edges.  numpy only.

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
