"""TEST INFRASTRUCTURE ONLY: the fp32 leaf functions stated from their defining formulas and evaluated with mpmath at 40 digits,
each with a first-order running bound on what the fp32 leaf (lgar_py_amd/csrc/lgar_leaf.hpp) may differ from it by.

THE STATEMENT (stmt_*): the reference's formulas as lgar_vg.hpp cites them --
    m = 1 - 1/n
    theta(h) = theta_r + (theta_e - theta_r) / (1 + (alpha h)^n)^m                      calc_theta_from_h, physics/utils.py:35-51
    Se(theta) = (theta - theta_r) / (theta_e - theta_r)                                calc_se_from_theta, utils.py:102-112
    Se(h) = 1 for |h| < 0.1, else (1 + (alpha h)^n)^-m                                 calc_se_from_h, utils.py:115-131
    K(Se) = Ksat sqrt(Se) (1 - b^m)^2, b = 1 - Se^(1/m), b + 1e-12 where |b| <= 1e-8   calc_k_from_se, utils.py:134-156
    h(Se) = b^(1/n) / alpha, b = Se^(-1/m) - 1, b + 1e-12 where |b| <= 1e-8            calc_h_from_se, utils.py:159-174
    Geff(theta1, theta2) = |sum_j (K_j-1 + K_j) dh / 2| / Ksat over nint intervals between h(Se(theta1)) and h(Se(theta2)),
        K_j = K(Se(h_j))                                                               calc_geff, lgar/green_ampt.py:45-84
    closed form: p = 1 + 2/m, lambda = 2/(p - 3), psi_b = (p+3)(147.8 + 8.1p + 0.092p^2) / (2 alpha p (p-1)(55.6 + 7.4p + p^2)),
        h_c = psi_b (2 + 3 lambda)/(1 + 3 lambda), e = 3 + 1/lambda,
        G = h_c Se(theta2)^e - Se(theta1)^e / (1 - Se(theta1)^e), h_c where that is not finite   green_ampt.py:85-98, utils.py:54-99
    AET = clamp(pet dt / (1 + (psi / psi_wp)^3), 0, pet), psi_wp = h(Se(theta_wp)),
        theta_wp = (theta_fc + theta(wp_psi)) / 2, theta_fc = theta_r + 0.75 (theta_e - theta_r)   calc_aet, lgar/aet.py:17-51
evaluated on the fp32-ROUNDED inputs and soil parameters, m formed exactly from the fp32 n.

THE BOUND (seq_*): the fp32 leaf's own operation sequence, walked in exact arithmetic.  Every value carries the absolute error
the fp32 computation may have accumulated up to it, as SIX coefficients -- the error is at most sum_k coef_k u_k, with u_k the
unit errors of the platform (UNITS_HOST here, UNITS_GPU in tests/test_gpu_leaf_f32.py):
    ARITH   one add, mul, fma, or correctly rounded divide: coef += ulp(result); u = 0.5
    DIV     the policy's quotient dv<POL>: coef += ulp(result); u = 0.5 for the IEEE divide, 2 for a * v_rcp_f32(b) (1.5 for the
            host build's a * (1.0f / b))
    SQRT    coef += ulp(result); u = 0.5 for libm, 1 for v_sqrt_f32
    LOG     log2: coef += ulp(result), plus the propagated dx / (x ln 2); u = 1
    EXP     exp2: coef += ulp(result), plus the propagated |dt| ln 2 result; u = 1
    LOGABS  log2 again: coef += ulp(1.0) -- an absolute floor for results near 0, whose own ulp vanishes; u = 0 for libm's log2f
            (relative accuracy throughout), the measured floor for v_log_f32 (which turned out to need none)
The roundings of m, 1/m, 1/n, -m/2, n - 1 and of the kernel's float literals (0.1, 1e-8, 1e-12, log2(1e-12), the closed form's
polynomial) are operations of the sequence like any other.  Second-order terms: where a product or a logarithm of a value with
error d needs |a| + d or x - d, d is taken at UNITS_MAX (twice the largest unit errors any platform has) -- the bound stays
linear in the units and valid for every platform below UNITS_MAX; a logarithm whose argument may reach 0 has bound inf.
Values are mpmath numbers at 40 digits, coefficients plain Python floats (nothing about a bound needs more).
"""
import math
import os

import numpy as np

try:  # (a machine without mpmath still reads the committed fixture: load(), bound() and the unit errors need none of it)
    import mpmath
    mp = mpmath.mp
except ImportError:
    mpmath = mp = None

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
DPS = 40
ARITH, DIV, SQRT, LOG, EXP, LOGABS = range(6)
COEF_NAMES = ("arith", "div", "sqrt", "log", "exp", "logabs")
# unit errors (in ulp): the host build (libm: log2f / exp2f within 1 ulp, correctly rounded divide and sqrt) ...
# (the host's POL_RCP32 quotient is a * (1.0f / b): two roundings, 1.5 ulp)
UNITS_HOST = dict(lean=(0.5, 0.5, 0.5, 1.0, 1.0, 0.0), rcp32=(0.5, 1.5, 0.5, 1.0, 1.0, 0.0))
# ... the hardware's are in tests/test_gpu_leaf_f32.py, next to the test that measures them
UNITS_MAX = (1.0, 3.0, 2.0, 4.0, 4.0, 8.0)
FACTOR = 2.0  # of the bound: second-order terms and contraction differences; fixed in advance
FLT_MAX = float(np.finfo(np.float32).max)
LN2 = 0.6931471805599453
INF = float("inf")


def M(x):
    """An fp32 (or any binary) number as an exact mpmath number."""
    return mpmath.mpf(float(x))


def ulp32(v):
    """One unit in the last place of fp32 at the magnitude of v (an mpmath number), as a float."""
    if v == 0:
        return math.ldexp(1.0, -149)
    e = mpmath.frexp(v)[1]  # |v| = f 2^e, 0.5 <= f < 1
    return math.ldexp(1.0, max(int(e) - 24, -149))


AMBIGUOUS = [0]   # comparisons of the current point that the operands' errors could turn: the bound is inf (point())
LEFT_RANGE = [0]  # operations of the current point whose fp32 result overflowed (point() resets and reads it)


class T:
    """A value of the sequence: v, what exact arithmetic gives; e, the six coefficients of the fp32 value's absolute error."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v if isinstance(v, mpmath.mpf) else M(v)
        self.e = e if e is not None else [0.0] * 6

    def finite(self):
        return mpmath.isfinite(self.v)

    def dmax(self):
        return sum(c * u for c, u in zip(self.e, UNITS_MAX))


def less(a, b, or_equal=False):
    """a < b as the kernel decides it in fp32; a comparison the operands' errors (at UNITS_MAX) could turn is counted."""
    a, b = _lift(a), _lift(b)
    if not (a.finite() and b.finite()):
        return bool(a.v <= b.v) if or_equal else bool(a.v < b.v)
    if abs(a.v - b.v) <= a.dmax() + b.dmax() and (any(a.e) or any(b.e)):
        AMBIGUOUS[0] += 1
    return bool(a.v <= b.v) if or_equal else bool(a.v < b.v)


def const(true_value, f32_value=None):
    """A float literal of the kernel: the statement's real number, its rounding to fp32 counted as the sequence's error."""
    tv = mpmath.mpf(true_value)
    fv = M(np.float32(float(tv)) if f32_value is None else f32_value)
    t = T(tv)
    t.e[ARITH] = float(abs(fv - tv)) / 0.5
    return t


def _lift(a):
    return a if isinstance(a, T) else T(a)


def _done(v, e, kind):
    """Finish an operation: range of fp32 (overflow to inf, underflow to 0), then the operation's own rounding."""
    if not mpmath.isfinite(v):
        return T(v)
    if abs(v) > FLT_MAX:
        LEFT_RANGE[0] += 1
        return T(mpmath.inf if v > 0 else -mpmath.inf)
    if abs(v) < mpmath.ldexp(1, -150):
        v = mpmath.mpf(0)
    e = list(e)
    if kind is not None and (v != 0 or any(e)):  # (an exact 0 from exact operands is 0 in fp32 too)
        e[kind] += ulp32(v)
    return T(v, e)


def _w(c, x):
    """c x for a coefficient x that may be 0 (stays 0) or inf (stays inf, whatever its weight)."""
    return 0.0 if x == 0.0 else (INF if x == INF else c * x)


def _lin(ca, ea, cb=0.0, eb=None):
    if eb is None:
        return [_w(ca, x) for x in ea]
    return [_w(ca, x) + _w(cb, y) for x, y in zip(ea, eb)]


def add(a, b, kind=ARITH):
    a, b = _lift(a), _lift(b)
    return _done(a.v + b.v, _lin(1.0, a.e, 1.0, b.e), kind)


def sub(a, b, kind=ARITH):
    a, b = _lift(a), _lift(b)
    return _done(a.v - b.v, _lin(1.0, a.e, 1.0, b.e), kind)


def neg(a):
    return T(-a.v, list(a.e))


def _mul_e(a, b):
    if not (a.finite() and b.finite()):
        return [0.0] * 6
    return _lin(float(abs(b.v)), a.e, float(abs(a.v)) + a.dmax(), b.e)


def mul(a, b, kind=ARITH):
    a, b = _lift(a), _lift(b)
    return _done(a.v * b.v, _mul_e(a, b), kind)


def fma(a, b, c):
    a, b, c = _lift(a), _lift(b), _lift(c)
    return _done(a.v * b.v + c.v, _lin(1.0, _mul_e(a, b), 1.0, c.e), ARITH)


def div(a, b, kind):
    a, b = _lift(a), _lift(b)
    if not (a.finite() and b.finite()):
        if mpmath.isinf(b.v) and a.finite():
            return T(0)
        return T(mpmath.nan if (mpmath.isnan(a.v) or mpmath.isnan(b.v) or mpmath.isinf(b.v)) else a.v * mpmath.sign(b.v))
    if b.v == 0:
        return T(mpmath.nan if a.v == 0 else (mpmath.inf if a.v > 0 else -mpmath.inf))
    bm = float(abs(b.v)) - b.dmax()
    if bm <= 0.0:
        return T(a.v / b.v, [INF] * 6)
    return _done(a.v / b.v, _lin(1.0 / bm, a.e, float(abs(a.v / b.v)) / bm, b.e), kind)


def sqrt(a):
    if not a.finite() or a.v < 0:
        return T(a.v if a.v > 0 else mpmath.nan)
    if a.v == 0:
        return T(0, [INF if c > 0 else 0.0 for c in a.e])
    r = mpmath.sqrt(a.v)
    am = float(a.v) - a.dmax()
    if am <= 0.0:
        return T(r, [INF] * 6)
    return _done(r, _lin(0.5 / math.sqrt(am), a.e), SQRT)


def lg2(a):
    if mpmath.isnan(a.v) or a.v < 0:
        return T(mpmath.nan)
    if a.v == 0:
        return T(-mpmath.inf)
    if mpmath.isinf(a.v):
        return T(mpmath.inf)
    if a.v == 1 and not any(a.e):
        return T(0)  # log2 of exactly 1 is exactly 0 (libm and v_log_f32 alike: k_from_se_one rests on it)
    am = float(a.v) - a.dmax()
    if am <= 0.0:
        return T(mpmath.log(a.v, 2), [INF] * 6)
    r = _done(mpmath.log(a.v, 2), _lin(1.0 / (am * LN2), a.e), LOG)
    r.e[LOGABS] += math.ldexp(1.0, -23)
    return r


def ex2(a):
    if mpmath.isnan(a.v):
        return T(mpmath.nan)
    if mpmath.isinf(a.v):
        return T(mpmath.inf if a.v > 0 else 0)
    if a.v == 0 and not any(a.e):
        return T(1)  # 2^0 is exactly 1
    if a.v > 129:
        LEFT_RANGE[0] += 1
        return T(mpmath.inf)
    if a.v < -151:
        return T(0)
    r = mpmath.power(2, a.v)
    d = a.dmax()
    # e^(d ln 2) - 1 against d ln 2 (by mpmath: the same bits on every machine, whatever its libm)
    grow = float(mpmath.expm1(d * LN2)) / (d * LN2) if d > 1e-12 else 1.0
    out = _done(r, _lin(float(r) * LN2 * grow, a.e), EXP)
    if out.finite() and out.v != 0:
        out.e[EXP] = max(out.e[EXP], 0.0) + (math.ldexp(1.0, -126) if abs(out.v) < mpmath.ldexp(1, -126) else 0.0)  # flushed
    return out


def pw(x, y):
    """pow of the fp32 leaves (lgar_scalar.hpp): 2^(y log2 x)."""
    return ex2(mul(y, lg2(_lift(x))))


# ---------------------------------------------------------------------------------------------------------------------------
# the layer as the leaf dispatcher forms it (lgar_leaf.hpp): m = 1 - 1/n, 1/m, 1/n in fp32, correctly rounded divides
# ---------------------------------------------------------------------------------------------------------------------------
class Soil:
    def __init__(self, alpha, n, ksat, te, tr):
        f = lambda v: M(np.float32(v))
        self.alpha, self.n, self.ksat, self.te, self.tr = f(alpha), f(n), f(ksat), f(te), f(tr)
        self.m_exact = 1 - 1 / self.n
        # the sequence's
        self.s_m = sub(1, div(1, self.n, ARITH))
        self.s_inv_m = div(1, self.s_m, ARITH)
        self.s_inv_n = div(1, self.n, ARITH)


C_1EM8 = lambda: const("1e-8")
C_1EM12 = lambda: const("1e-12")
C_CUT = lambda: const("0.1")


def _nudge_seq(base):
    """b + 1e-12 where |b| <= 1e-8 (the kernel compares and adds in fp32)."""
    if base.finite() and less(T(abs(base.v), base.e), C_1EM8(), or_equal=True):
        return add(base, C_1EM12())
    return base


def _nudge(b):
    return b + mpmath.mpf("1e-12") if abs(b) <= mpmath.mpf("1e-8") else b


# ----- statements ------------------------------------------------------------------------------------------------------------
def stmt_theta_from_h(s, h):
    return s.tr + (s.te - s.tr) / (1 + (s.alpha * h) ** s.n) ** s.m_exact


def stmt_se_from_theta(s, theta):
    return (theta - s.tr) / (s.te - s.tr)


def stmt_se_from_h(s, h):
    if abs(h) < mpmath.mpf("0.1"):
        return mpmath.mpf(1)
    return (1 + (s.alpha * h) ** s.n) ** (-s.m_exact)


def _sqrt(x):
    """sqrt of an mpmath number or of anything that brings its own (the dual numbers of leaf_ref.tangent)."""
    return x.sqrt() if hasattr(x, "sqrt") else mpmath.sqrt(x)


def stmt_kr_from_se(s, se, nudge=True):
    """nudge=False: without calc_k_from_se's b + 1e-12 (what the fused trapezoid node leaves out: leaf_ref.tangent)."""
    if se == 0:
        return mpmath.mpf(0)
    b = 1 - se ** (1 / s.m_exact)
    if nudge:
        b = _nudge(b)
    return _sqrt(se) * (1 - b ** s.m_exact) ** 2


def stmt_k_from_se(s, se):
    return s.ksat * stmt_kr_from_se(s, se)


def stmt_h_from_se(s, se):
    if se == 0:
        return mpmath.inf
    b = _nudge(se ** (-1 / s.m_exact) - 1)
    return b ** (1 / s.n) / s.alpha


def stmt_trapezoid(s, h_i, h_f, nint, k_first=None, node_nudge=True):
    """|sum_j (K_j-1 + K_j) dh / 2| / Ksat, nodes h_i + j dh; k_first: K_0 / Ksat where it is not K(Se(h_i)).  Also returns the
    distance of the node nearest the 0.1 cm cut from it, relative (a node AT the cut would make the sum discontinuous).
    node_nudge=False: the nodes above the cut without calc_k_from_se's nudge (those under it are K(Se = 1), nudged, either way)."""
    dh = (h_f - h_i) / nint
    k_prev = stmt_kr_from_se(s, stmt_se_from_h(s, h_i)) if k_first is None else k_first
    g, near = mpmath.mpf(0), mpmath.inf
    for j in range(1, nint + 1):
        h = h_f if j == nint else h_i + j * dh
        near = min(near, abs(h - mpmath.mpf("0.1")) / mpmath.mpf("0.1"))
        k = stmt_kr_from_se(s, stmt_se_from_h(s, h), nudge=node_nudge or bool(abs(h) < mpmath.mpf("0.1")))
        g += (k_prev + k) * dh / 2
        k_prev = k
    return abs(g), float(near)


def stmt_geff(s, theta1, theta2, nint, node_nudge=True):
    se_i, se_f = stmt_se_from_theta(s, theta1), stmt_se_from_theta(s, theta2)
    return stmt_trapezoid(s, stmt_h_from_se(s, se_i), stmt_h_from_se(s, se_f), nint, k_first=stmt_kr_from_se(s, se_i),
                          node_nudge=node_nudge)


def stmt_geff_closed(s, theta1, theta2):
    m = s.m_exact
    p = 1 + 2 / m
    lam = 2 / (p - 3)
    psib = (p + 3) * (mpmath.mpf("147.8") + mpmath.mpf("8.1") * p + mpmath.mpf("0.092") * p * p) / \
        (2 * s.alpha * p * (p - 1) * (mpmath.mpf("55.6") + mpmath.mpf("7.4") * p + p * p))
    h_c = psib * (2 + 3 * lam) / (1 + 3 * lam)
    e = 3 + 1 / lam
    pf = stmt_se_from_theta(s, theta1) ** e
    if pf == 1:
        return h_c
    return h_c * stmt_se_from_theta(s, theta2) ** e - pf / (1 - pf)


def stmt_aet(s, psi, pet, dt, wp_psi):
    theta_fc = s.tr + mpmath.mpf("0.75") * (s.te - s.tr)
    theta_wp = (theta_fc + stmt_theta_from_h(s, wp_psi)) / 2
    psi_wp = stmt_h_from_se(s, stmt_se_from_theta(s, theta_wp))
    a = pet * dt / (1 + (psi / psi_wp) ** 3)
    return min(max(a, mpmath.mpf(0)), pet)


# ----- the fp32 leaves' operation sequences (lgar_vg.hpp, lgar_geff.hpp) ----------------------------------------------------------
def seq_theta_from_h(s, h):
    ap = pw(mul(s.alpha, h), s.n)
    op = pw(add(1, ap), s.s_m)
    return add(mul(div(1, op, DIV), sub(s.te, s.tr)), s.tr)


def seq_se_from_theta(s, theta):
    if _lift(theta).v == s.te:
        return T(1)  # x / x == 1 exactly
    return div(sub(theta, s.tr), sub(s.te, s.tr), ARITH)  # the IEEE divide in every policy


def seq_se_from_h(s, h):
    h = _lift(h)
    # (an operand without error -- the leaf's own input -- is compared as the kernel compares it, with the float 0.1f: no float
    # lies between 0.1 and 0.1f, so the statement decides alike)
    if (abs(h.v) < M(np.float32(0.1))) if not any(h.e) else less(T(abs(h.v), h.e), C_CUT()):
        return T(1)
    return div(1, pw(add(1, pw(mul(s.alpha, h), s.n)), s.s_m), DIV)


def seq_k_from_se(s, se):
    se = _lift(se)
    base = _nudge_seq(sub(1, pw(se, s.s_inv_m)))
    t = sub(1, pw(base, s.s_m))
    return mul(mul(s.ksat, sqrt(se)), mul(t, t))


def seq_h_from_se(s, se):
    base = _nudge_seq(sub(pw(se, neg(s.s_inv_m)), 1))
    return mul(div(1, s.alpha, DIV), pw(base, s.s_inv_n))


def seq_aet(s, psi, pet, dt, wp_psi):
    theta_fc = add(mul(sub(s.te, s.tr), M(0.75)), s.tr)
    wht = seq_theta_from_h(s, wp_psi)
    theta_wp = add(mul(sub(theta_fc, wht), M(0.5)), wht)
    psi_wp = seq_h_from_se(s, seq_se_from_theta(s, theta_wp))
    r = div(psi, psi_wp, ARITH)
    h_ratio = add(1, mul(mul(r, r), r))
    a = mul(mul(pet, div(1, h_ratio, ARITH)), dt)
    if a.finite() and a.v < 0:
        return T(0)
    if a.finite() and a.v > _lift(pet).v:
        return T(pet)
    return a


def seq_geff_from_heads(s, h_i, h_f, nint):
    """geff_f32_from_heads (lgar_geff.hpp): four accumulators, node j at fma(j, dx, x0), the end nodes as one more pair."""
    h_i, h_f = _lift(h_i), _lift(h_f)
    dh = mul(sub(h_f, h_i), div(1, M(float(nint)), ARITH))
    nm1 = sub(s.n, 1)
    hm = mul(M(-0.5), s.s_m, None)  # exact
    x0, dx = mul(s.alpha, h_i), mul(s.alpha, dh)
    xcut = mul(C_CUT(), s.alpha)
    tsat = sub(1, ex2(mul(s.s_m, const(mpmath.log(mpmath.mpf("1e-12"), 2), np.float32(-39.863137)))))
    ksat1 = mul(tsat, tsat)
    one = T(1)

    def sr_tt(x):
        lg = lg2(x)
        P = ex2(mul(nm1, lg))
        l1 = lg2(fma(x, P, 1))
        sr = ex2(mul(hm, l1))
        t = fma(neg(P), mul(sr, sr), 1)
        return sr, mul(t, t)

    def checked(x):
        return (ksat1, one) if less(x, xcut) else sr_tt(x)

    Mn = nint - 1
    pairs = Mn >> 1
    acc = [[T(0), T(0)], [T(0), T(0)]]
    for p in range(pairs):
        for c in (0, 1):
            x = fma(M(float(2 * p + 1 + c)), dx, x0)
            sr, tt = checked(x)
            acc[p & 1][c] = fma(sr, tt, acc[p & 1][c])
    total = add(add(acc[0][0], acc[1][0]), add(acc[0][1], acc[1][1]))
    if Mn & 1:
        sr, tt = checked(fma(M(float(Mn)), dx, x0))
        total = add(total, mul(sr, tt))
    sr, tt = checked(x0)
    k0 = mul(sr, tt)
    sr, tt = checked(mul(s.alpha, h_f))
    kn = mul(sr, tt)
    r = mul(mul(M(0.5), dh, None), add(add(k0, kn), mul(M(2.0), total, None)))
    return T(abs(r.v), r.e)


def seq_heads_of_geff(s, theta1, theta2):
    """Both heads as geff<float> forms them (lgar_geff.hpp): h(Se) with one correctly rounded reciprocal of alpha."""
    inv_alpha = div(1, s.alpha, ARITH)
    ni = neg(s.s_inv_m)
    out = []
    for theta in (theta1, theta2):
        base = _nudge_seq(sub(ex2(mul(ni, lg2(seq_se_from_theta(s, theta)))), 1))
        out.append(mul(inv_alpha, ex2(mul(s.s_inv_n, lg2(base)))))
    return out


def seq_geff(s, theta1, theta2, nint):
    h_i, h_f = seq_heads_of_geff(s, theta1, theta2)
    return seq_geff_from_heads(s, h_i, h_f, nint)


def seq_geff_literal(s, theta1, theta2, nint):
    """geff_literal<float, POL_LEAN> (lgar_vg.hpp): the reference's loop operation by operation, the heads a running sum."""
    se_i, se_f = seq_se_from_theta(s, theta1), seq_se_from_theta(s, theta2)
    h_i, h_f = seq_h_from_se(s, se_i), seq_h_from_se(s, se_f)
    dh = div(sub(h_f, h_i), M(float(nint)), ARITH)
    hdh = mul(dh, M(0.5), None)
    g, k1, h2 = T(0), seq_k_from_se(s, se_i), add(h_i, dh)
    for _ in range(nint):
        se2 = T(1) if less(h2, T(0)) else seq_se_from_h(s, h2)
        k2 = seq_k_from_se(s, se2)
        g = add(g, mul(add(k1, k2), hdh))
        k1, h2 = k2, add(h2, dh)
    r = div(g, s.ksat, ARITH)
    return T(abs(r.v), r.e)


def seq_geff_closed(s, theta1, theta2):
    c = lambda txt: const(txt)
    m = s.s_m
    p = add(1, div(2, m, ARITH))
    lam = div(2, sub(p, 3), ARITH)
    num = mul(add(p, 3), add(add(c("147.8"), mul(c("8.1"), p)), mul(mul(c("0.092"), p), p)))
    den = mul(mul(mul(mul(M(2.0), s.alpha, None), p), sub(p, 1)), add(add(c("55.6"), mul(c("7.4"), p)), mul(p, p)))
    psib = div(num, den, ARITH)
    l3 = mul(M(3.0), lam)
    h_c = div(mul(psib, add(2, l3)), add(1, l3), ARITH)
    e = add(3, div(1, lam, ARITH))
    pf = pw(seq_se_from_theta(s, theta1), e)
    g = sub(mul(h_c, pw(seq_se_from_theta(s, theta2), e)), div(pf, sub(1, pf), ARITH))
    return g if g.finite() else h_c


# ---------------------------------------------------------------------------------------------------------------------------
# one point of a leaf function: (reference value, six coefficients).  Where the sequence leaves fp32's range (an overflowed
# Se^(-1/m): inf) the reference is that inf or NaN: the kernel must give the same class.
# ---------------------------------------------------------------------------------------------------------------------------
FUNCTIONS = ("theta_from_h", "se_from_h", "k_from_se", "h_from_se", "aet", "geff", "geff_literal", "geff_from_heads", "geff_closed",
             "pow", "div", "sqrt")
# leaf ops of a function in float: (op number, units key)
OPS_OF = dict(theta_from_h=((0, "lean"), (17, "rcp32")), se_from_h=((1, "lean"), (18, "rcp32")), k_from_se=((2, "lean"), (19, "rcp32")),
              h_from_se=((3, "lean"), (20, "rcp32")), aet=((5, "lean"), (21, "rcp32")), geff=((4, "lean"),), geff_literal=((6, "lean"),),
              geff_from_heads=((22, "rcp32"),), geff_closed=((23, "rcp32"),), pow=((9, "lean"),), div=((11, "lean"), (15, "rcp32")),
              sqrt=((16, "rcp32"),))
WP_PSI = 15495.0


def point(fn, soil, x, y=0.0, z=0.0, nint=120):
    """(ref, coef[6], near) of function `fn` at the fp32 operands x, y, z for `soil` (a Soil)."""
    mp.dps = DPS
    x, y, z = M(np.float32(x)), M(np.float32(y)), M(np.float32(z))
    near = INF
    LEFT_RANGE[0] = AMBIGUOUS[0] = 0
    if fn == "theta_from_h":
        st, sq_ = stmt_theta_from_h(soil, x), seq_theta_from_h(soil, x)
    elif fn == "se_from_h":
        st, sq_ = stmt_se_from_h(soil, x), seq_se_from_h(soil, x)
    elif fn == "k_from_se":
        st, sq_ = stmt_k_from_se(soil, x), seq_k_from_se(soil, x)
    elif fn == "h_from_se":
        st, sq_ = stmt_h_from_se(soil, x), seq_h_from_se(soil, x)
    elif fn == "aet":
        st, sq_ = stmt_aet(soil, x, y, z, M(WP_PSI)), seq_aet(soil, x, y, z, M(WP_PSI))
    elif fn == "geff":
        (st, near), sq_ = stmt_geff(soil, x, y, nint), seq_geff(soil, x, y, nint)
    elif fn == "geff_literal":
        (st, near), sq_ = stmt_geff(soil, x, y, nint), seq_geff_literal(soil, x, y, nint)
    elif fn == "geff_from_heads":
        (st, near), sq_ = stmt_trapezoid(soil, x, y, nint), seq_geff_from_heads(soil, x, y, nint)
    elif fn == "geff_closed":
        st, sq_ = stmt_geff_closed(soil, x, y), seq_geff_closed(soil, x, y)
    elif fn == "pow":
        st, sq_ = (x ** y if x > 0 else mpmath.mpf(0)), pw(x, y)
    elif fn == "div":
        st, sq_ = x / y, div(x, y, DIV)
    elif fn == "sqrt":
        st, sq_ = mpmath.sqrt(x), sqrt(T(x))
    else:
        raise KeyError(fn)
    if not sq_.finite():
        return float(sq_.v), [0.0] * 6, near, 0.0
    coef = [INF] * 6 if AMBIGUOUS[0] else [float(c) for c in sq_.e]
    if LEFT_RANGE[0]:
        # an intermediate overflowed in fp32 and the result is finite all the same ((alpha h)^n = inf: theta is theta_r, Se is
        # 0): the statement is what the formulas give with that intermediate infinite
        return float(sq_.v), coef, near, 0.0
    # what the two ways of writing the function differ by (a nudge one of them does not apply, a float literal's rounding):
    # reported, and checked against the bound by the generator
    gap = float(abs(st - sq_.v)) if mpmath.isfinite(st) else INF
    return float(st), coef, near, gap


def bound(coef, units):
    """sum_k coef_k u_k over the last axis (coefficients that are inf stay inf, also against a unit of 0)."""
    coef = np.asarray(coef, dtype=np.float64)
    u = np.asarray(units, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        terms = np.where(coef == 0.0, 0.0, coef * u)
        terms = np.where(np.isinf(coef), np.inf, terms)
    return terms.sum(axis=-1)


def load():
    """The committed fixture (tests/golden/leaf_f32/leaf_f32_ref.npz): (soils [S, 5] fp32, soil names, {function: dict(soil, x, y, z, ref, coef)})."""
    g = np.load(os.path.join(GOLDEN, "leaf_f32", "leaf_f32_ref.npz"))
    return g["soils"], list(g["soil_names"]), {fn: {k: g["%s.%s" % (fn, k)] for k in ("soil", "x", "y", "z", "ref", "coef")} for fn in FUNCTIONS}
