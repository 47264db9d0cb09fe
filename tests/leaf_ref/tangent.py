"""TEST INFRASTRUCTURE ONLY: the derivative of the leaf statements (leaf_ref.stmt_*), by mpmath dual numbers at 100 digits (DPS below).

A dual number D carries a value and its SEVEN partial derivatives -- with respect to alpha, n, ksat, theta_e, theta_r and the two
operands x, y of a leaf (leaf_ref.tangent.SEEDS: the seed order of lgar_leaf_tangent_batch, include/lgar.h) -- through the very
formulas leaf_ref states: m = 1 - 1/n is formed from the dual n, so dn reaches every exponent.  What comes out is the exact
derivative of the reference's DISCRETE formulas -- the 121 nodes of the trapezoid included -- with every branch (the 0.1 cm cut,
the |base| <= 1e-8 nudge, the clamps) frozen at the value the statement itself takes.

Branch conventions are torch's, as lgar_py_amd/csrc/lgar_dual.hpp states them:
    abs(x)          sign(x) dx (0 at 0)
    min(a, b)       the smaller argument's derivative; half of each on a tie
    clamp of AET    0 below 0, d pet above pet, the argument's own derivative on a tie (torch.clamp)
    |h| < 0.1       Se = 1, a constant: the node's K is K(Se = 1) with Ksat's and m's derivatives only (k_from_se_one)
    x^y             y x^(y-1) dx + x^y ln x dy for x > 0; 0 at x = 0 (both terms, as torch.pow's backward has them for y > 0)
Two DEPARTURES of lgar_dual.hpp from torch, stated here and asserted as such by the tests (leaf_ref.check.tangent_departures), not treated as errors:
    pw(x, y), x < 0     the tangent is dropped (0), where torch gives y x^(y-1) dx (and NaN along dy); the value is NaN-flagged
                        by the kernels there, no trajectory continues through it
    sq(0)               tangent 0, where torch.sqrt gives inf dx

The fused trapezoid node (geff_node, lgar_vg.hpp) leaves calc_k_from_se's 1e-12 nudge out; that is the same function only where
(alpha h)^n <= 1e-8 implies |h| < 0.1, which fails for n = 3.5 with a small alpha.  So the trapezoid is stated twice: "geff" without
the nudge at the nodes above the cut (what the fused node computes), "geff_literal" with it (the reference's own loop); the gap
between the two is recorded per soil (the fixture's nudge_gap) and must stay under the project's 1e-6 parity bar.
"""
import numpy as np

import leaf_ref as R

try:
    import mpmath
except ImportError:  # (the tests read the committed fixture)
    mpmath = None

# Working precision.  leaf_ref's 40 digits are not enough HERE: the points reach Se = 1e-6 for n = 1.09, where 1 - Se^(1/m) is
# 1 - 1e-72 -- the fp32 fixture stops where fp32 does, this one follows double precision down.  100 digits leave 28 there.
DPS, DPS_DIFF = 100, 150
SEEDS = ("alpha", "n", "ksat", "theta_e", "theta_r", "x", "y")
NS = len(SEEDS)
# leaf functions of the fixture: name -> (tangent op number, reads y)
LEAVES = dict(theta_from_h=(0, False), se_from_h=(1, False), k_from_se=(2, False), h_from_se=(3, False), aet=(5, True),
              geff_closed=(23, True), se_from_theta=(24, False), geff=(4, True), geff_literal=(6, True))
# primitives of lgar_dual.hpp (seeds d_x, d_y only): name -> (op number, reads y)
PRIMS = dict(pw=(9, True), pwx=(25, True), dv=(11, True), dv_dual_real=(26, True), dv_real_dual=(27, True), quotient=(28, True),
             sq=(16, False), lg2=(29, False), ex2=(30, False), lg2p=(7, False), ex2p=(8, False), mn=(31, True), ab=(32, False))
FUNCTIONS = tuple(LEAVES) + tuple(PRIMS)
OP_OF = {k: v[0] for k, v in dict(LEAVES, **PRIMS).items()}
READS_Y = {k: v[1] for k, v in dict(LEAVES, **PRIMS).items()}
# the partials an op can have at all (the others are seeded too and must come out 0, value and class)
POLICY_LEAVES = ("theta_from_h", "se_from_h", "k_from_se", "h_from_se", "aet", "geff_closed", "se_from_theta")


def _mpf(x):
    return x if isinstance(x, mpmath.mpf) else mpmath.mpf(x)


POW_T = [0.0]  # the largest |y log2 x| among the pows of the current point (leaf() resets and reads it)


class D:
    """value + gradient[7] in mpmath numbers, and a[7]: the gradient's terms added up by ABSOLUTE value -- what a partial would be
    if nothing cancelled.  a[k] == |g[k]| where a partial is one product of factors; a[k] >> |g[k]| where it is a difference of
    large terms (the AET along theta_e, which cancels to nothing; Geff along Ksat): any floating-point evaluation carries a
    rounding error in proportion to a[k], not to |g[k]|."""
    __slots__ = ("v", "g", "a")

    def __init__(self, v, g=None, a=None):
        self.v = _mpf(v)
        self.g = g if g is not None else [mpmath.mpf(0)] * NS
        self.a = a if a is not None else [abs(x) for x in self.g]

    @staticmethod
    def seeded(v, k):
        g = [mpmath.mpf(0)] * NS
        g[k] = mpmath.mpf(1)
        return D(v, g)

    @staticmethod
    def lift(x):
        return x if isinstance(x, D) else D(x)

    def _lin(self, v, ca, other=None, cb=None):
        if other is None:
            return D(v, [ca * a for a in self.g], [abs(ca) * a for a in self.a])
        return D(v, [ca * a + cb * b for a, b in zip(self.g, other.g)], [abs(ca) * a + abs(cb) * b for a, b in zip(self.a, other.a)])

    # arithmetic
    def __add__(self, o):
        o = D.lift(o)
        return self._lin(self.v + o.v, 1, o, 1)
    __radd__ = __add__

    def __sub__(self, o):
        o = D.lift(o)
        return self._lin(self.v - o.v, 1, o, -1)

    def __rsub__(self, o):
        return D.lift(o) - self

    def __neg__(self):
        return self._lin(-self.v, -1)

    def __mul__(self, o):
        o = D.lift(o)
        return self._lin(self.v * o.v, o.v, o, self.v)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = D.lift(o)
        q = self.v / o.v
        return self._lin(q, 1 / o.v, o, -q / o.v)

    def __rtruediv__(self, o):
        return D.lift(o) / self

    def __pow__(self, o):
        o = D.lift(o)
        x, y = self.v, o.v
        if x == 0:
            return D(mpmath.mpf(0) if y > 0 else x ** y)
        v = x ** y
        if x > 0:
            POW_T[0] = max(POW_T[0], abs(float(y * mpmath.log(x, 2))))
        return self._lin(v, y * x ** (y - 1), o, v * mpmath.log(x))

    def __rpow__(self, o):
        return D.lift(o) ** self

    def sqrt(self):
        r = mpmath.sqrt(self.v)
        return self._lin(r, 1 / (2 * r))

    def __abs__(self):
        return self._lin(abs(self.v), mpmath.sign(self.v))

    # control flow looks at values
    def __lt__(self, o): return self.v < D.lift(o).v
    def __le__(self, o): return self.v <= D.lift(o).v
    def __gt__(self, o): return self.v > D.lift(o).v
    def __ge__(self, o): return self.v >= D.lift(o).v
    def __eq__(self, o): return self.v == D.lift(o).v
    def __ne__(self, o): return self.v != D.lift(o).v
    __hash__ = None

    def __float__(self):
        return float(self.v)


def dmin(a, b):
    """torch.minimum's derivative: half of each on a tie."""
    a, b = D.lift(a), D.lift(b)
    if a.v < b.v:
        return a
    if b.v < a.v:
        return b
    return a._lin(a.v, mpmath.mpf(1) / 2, b, mpmath.mpf(1) / 2)


class DualSoil:
    """leaf_ref.Soil's attributes as dual numbers seeded along alpha, n, ksat, theta_e, theta_r."""

    def __init__(self, alpha, n, ksat, te, tr):
        self.alpha, self.n, self.ksat, self.te, self.tr = (D.seeded(R.M(v), k) for k, v in enumerate((alpha, n, ksat, te, tr)))
        self.m_exact = 1 - 1 / self.n


def leaf(fn, soil, x, y=0.0, z=0.0, nint=120):
    """(value, gradient[7], near, a[7], T) of leaf `fn` at the (binary) operands x, y, z: floats; inf / NaN where the statement has
    none.  a: the gradient's terms by absolute value (class D); T: the largest |y log2 x| among the leaf's pows."""
    mpmath.mp.dps = DPS
    POW_T[0] = 0.0
    s = DualSoil(*soil)
    X, Y, Z = D.seeded(R.M(x), 5), D.seeded(R.M(y), 6), R.M(z)
    near = R.INF
    try:
        if fn == "theta_from_h":
            r = R.stmt_theta_from_h(s, X)
        elif fn == "se_from_h":
            r = R.stmt_se_from_h(s, X)
        elif fn == "k_from_se":
            r = R.stmt_k_from_se(s, X)
        elif fn == "h_from_se":
            r = R.stmt_h_from_se(s, X)
        elif fn == "se_from_theta":
            r = R.stmt_se_from_theta(s, X)
        elif fn == "aet":
            r = R.stmt_aet(s, X, Y, Z, R.M(R.WP_PSI))
        elif fn == "geff_closed":
            r = R.stmt_geff_closed(s, X, Y)
        elif fn in ("geff", "geff_literal"):
            r, near = R.stmt_geff(s, X, Y, nint, node_nudge=(fn == "geff_literal"))
            # (the statement sums K / Ksat; the reference and the kernels sum K and divide by Ksat at the end: the same function,
            # whose partial along Ksat is a difference of two terms G / Ksat -- `a` must know)
            r = (D.lift(r) * s.ksat) / s.ksat
            r.g[2] = mpmath.mpf(0)  # (exactly: what the two terms leave at 100 digits is no derivative)
        else:
            raise KeyError(fn)
    except (ZeroDivisionError, ValueError, TypeError):  # Se outside (0, 1]: a complex power, a division by zero
        return float("nan"), [float("nan")] * NS, near, [float("nan")] * NS, POW_T[0]
    r = D.lift(r)
    if isinstance(r.v, mpmath.mpc) or any(isinstance(g, mpmath.mpc) for g in r.g):
        return float("nan"), [float("nan")] * NS, near, [float("nan")] * NS, POW_T[0]
    return float(r.v), [float(g) for g in r.g], near, [float(a) for a in r.a], POW_T[0]


class _PlainSoil:
    def __init__(self, alpha, n, ksat, te, tr):
        self.alpha, self.n, self.ksat, self.te, self.tr = (R.M(v) for v in (alpha, n, ksat, te, tr))
        self.m_exact = 1 - 1 / self.n


def drift(fn, soil, x, y, nint=120):
    """[7]: what the trapezoid's TANGENT running sum of heads can add to each partial of Geff, an absolute bound.

    The kernels and the reference walk the nodes by h2 += dh.  A dual-number kernel walks the tangent the same way, h2.d += dh.d:
    nint additions, each rounded by at most 2^-53 of the larger of |h_i.d|, |h_f.d| =: H (the tangent of a node's head is a convex
    combination of the two ends').  Node j's head tangent is then off by at most j 2^-53 H, its K by |dK/dh (h_j)| times that, and
    the sum  G = |sum_j w_j K_j| / Ksat  (w_j = |dh|, |dh| / 2 for the end node) by
        2^-53 H  sum_j w_j |dK_r/dh (h_j)| j  =  2^-53 H nint Q,     Q = sum_j w_j |dK_r/dh (h_j)| j / nint.
    Q is read off a second pass of the statement's trapezoid with dual heads: it is the by-absolute-value partial along h_f (class
    D's `a`: node j moves by j / nint of a move of h_f; the pass's explicit dh term, G / |h_f - h_i|, rides along: an over-estimate).
    Along alpha the input of a node is d(alpha h_j) = h_j.v + alpha h_j.d with h_j.d = -h_j / alpha: the VALUE sum's rounding,
    j 2^-53 h_i = j 2^-53 alpha H, enters a second time, uncancelled, so the bound is doubled along alpha, and along alpha only.
    The reference's reverse mode has no such sum -- the adjoint of h_j with respect to h_i is exactly 1 -- so its own error does not
    measure this; the drift of the VALUE sum it shares with the kernels, and E_ref measures that at the point itself.
    Zero for everything but the two trapezoids."""
    if fn not in ("geff", "geff_literal"):
        return [0.0] * NS
    mpmath.mp.dps = DPS
    s = DualSoil(*soil)
    try:
        heads = [D.lift(R.stmt_h_from_se(s, R.stmt_se_from_theta(s, D.seeded(R.M(t), k)))) for t, k in ((x, 5), (y, 6))]
    except TypeError:  # (Se > 1, a complex power: outside the domain, the statement is NaN, nothing to bound)
        return [0.0] * NS
    if not all(mpmath.isfinite(h.v) for h in heads):
        return [float("inf")] * NS
    H = [max(abs(heads[0].g[k]), abs(heads[1].g[k])) for k in range(NS)]
    p = _PlainSoil(*soil)
    k_first = R.stmt_kr_from_se(p, R.stmt_se_from_theta(p, R.M(x)))
    g, _ = R.stmt_trapezoid(p, D.seeded(heads[0].v, 5), D.seeded(heads[1].v, 6), nint, k_first=k_first, node_nudge=(fn == "geff_literal"))
    Q = D.lift(g).a[6]
    return [float((2 if k == 0 else 1) * mpmath.ldexp(1, -53) * h * nint * Q) for k, h in enumerate(H)]


def prim(fn, x, y):
    """(value, d/dx, d/dy) of a primitive of lgar_dual.hpp as torch differentiates it -- except the two stated departures."""
    mpmath.mp.dps = DPS
    x, y = R.M(x), R.M(y)
    ln2 = mpmath.log(2)
    zero, nan = mpmath.mpf(0), mpmath.nan
    if fn in ("pw", "pwx"):
        if x < 0:
            return nan, zero, zero  # DEPARTURE: the tangent is dropped
        if x == 0:
            return (zero if y > 0 else (mpmath.mpf(1) if y == 0 else mpmath.inf)), zero, zero
        v = x ** y
        return v, y * x ** (y - 1), v * mpmath.log(x)
    if fn in ("dv", "quotient"):
        return x / y, 1 / y, -x / (y * y)
    if fn == "dv_dual_real":
        return x / y, 1 / y, zero
    if fn == "dv_real_dual":
        return x / y, zero, -x / (y * y)
    if fn == "sq":
        if x == 0:
            return zero, zero, zero  # DEPARTURE: 0, not inf
        r = mpmath.sqrt(x)
        return r, 1 / (2 * r), zero
    if fn in ("lg2", "lg2p"):
        return mpmath.log(x, 2), 1 / (x * ln2), zero
    if fn in ("ex2", "ex2p"):
        v = mpmath.power(2, x)
        return v, v * ln2, zero
    if fn == "mn":
        if x == y:
            return x, mpmath.mpf(1) / 2, mpmath.mpf(1) / 2
        return (x, mpmath.mpf(1), zero) if x < y else (y, zero, mpmath.mpf(1))
    if fn == "ab":
        return abs(x), mpmath.sign(x), zero
    raise KeyError(fn)


def check_against_diff(fn, soil, x, y=0.0, z=0.0, nint=120, rel=1e-25):
    """The dual propagation against mpmath.diff at DPS_DIFF digits: every partial of leaf `fn` at one point, as a central difference of
    the PLAIN statement in the perturbed argument.  Meaningful away from the branches (the caller picks such points); returns the
    worst relative difference."""
    grad = leaf(fn, soil, x, y, z, nint)[1]
    mpmath.mp.dps = DPS_DIFF
    base = [R.M(v) for v in soil] + [R.M(x), R.M(y)]

    class _S:
        pass

    def f(k, t):
        a = list(base)
        a[k] = t
        s = _S()
        s.alpha, s.n, s.ksat, s.te, s.tr = a[:5]
        s.m_exact = 1 - 1 / s.n
        X, Y = a[5], a[6]
        if fn == "theta_from_h":
            return R.stmt_theta_from_h(s, X)
        if fn == "se_from_h":
            return R.stmt_se_from_h(s, X)
        if fn == "k_from_se":
            return R.stmt_k_from_se(s, X)
        if fn == "h_from_se":
            return R.stmt_h_from_se(s, X)
        if fn == "se_from_theta":
            return R.stmt_se_from_theta(s, X)
        if fn == "aet":
            return R.stmt_aet(s, X, Y, R.M(z), R.M(R.WP_PSI))
        if fn == "geff_closed":
            return R.stmt_geff_closed(s, X, Y)
        return R.stmt_geff(s, X, Y, nint, node_nudge=(fn == "geff_literal"))[0]

    worst = 0.0
    # (a partial that vanishes analytically -- the AET's along theta_e -- is compared on the scale of the largest elasticity)
    floor = max(abs(_mpf(g) * b) for g, b in zip(grad, base)) * mpmath.mpf(10) ** -25
    for k in range(NS):
        if k == 6 and not READS_Y[fn]:
            continue
        h = abs(base[k]) * mpmath.mpf(10) ** -50 if base[k] != 0 else mpmath.mpf(10) ** -50
        d = mpmath.diff(lambda t: f(k, t), base[k], h=h)
        scale = max(abs(d), abs(_mpf(grad[k])), floor / max(abs(base[k]), mpmath.mpf(10) ** -30), mpmath.mpf(10) ** -300)
        worst = max(worst, float(abs(d - _mpf(grad[k])) / scale))
    mpmath.mp.dps = DPS
    return worst


def load():
    """The committed fixture tests/golden/leaf_tangent/leaf_tangent_ref.npz: (soils [S, 5] float64 -- fp32 values --, soil names,
    {function: dict(soil, x, y, z, f32ok, value, grad [N, 7], ref_grad [N, 7], cond [N, 7], powt [N])}, gap of the nudge [S, 8])."""
    import os
    g = np.load(os.path.join(R.GOLDEN, "leaf_tangent", "leaf_tangent_ref.npz"))
    key = lambda fn, k: "%s.%s" % ("geff_literal" if (fn, k) == ("geff", "ref_grad") else fn, k)  # (one reference for both trapezoids)
    fns = {fn: {k: g[key(fn, k)] for k in ("soil", "x", "y", "z", "f32ok", "value", "grad", "ref_grad", "cond", "powt")} for fn in FUNCTIONS}
    for fn, d in fns.items():
        d["drift"] = g[fn + ".drift"] if fn + ".drift" in g.files else np.zeros(d["grad"].shape, dtype=np.float32)
    return g["soils"], list(g["soil_names"]), fns, g["nudge_gap"]
