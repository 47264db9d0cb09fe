"""TEST INFRASTRUCTURE ONLY: the points of tests/golden/leaf_f32/leaf_f32_ref.npz (written by tests/golden/make_leaf_f32_golden.py) and their
evaluation with leaf_ref.point.  Everything is fp32 on the way in: soils, operands, dt."""
import os

import mpmath
import numpy as np

import leaf_ref as R
from lgar_py_amd import data, workloads

GOLDEN = R.GOLDEN
F = np.float32
NINT = 120
FRACTIONS = (0.02, 0.1, 0.3, 0.5, 0.7, 0.9, 0.98, 1.0)  # of theta_e - theta_r: the Geff pairs of the leaf_kats fixture
NEAR_CUT = 1e-4  # a trapezoid with a node this close (relative) to the 0.1 cm cut is left out: the sum is discontinuous there
SOIL_NAMES = ["vg_table_%02d" % i for i in range(len(data.VG_TABLE))] + ["synthetic_n1.09", "synthetic_n3.5"] + \
             ["perturbed_layer_%d" % i for i in range(3)]


def soils():
    """[S, 5] fp32 (alpha, n, ksat, theta_e, theta_r): the 18 rows of data.VG_TABLE with theta_e / theta_r of the leaf_kats fixture's
    soils in turn (the table itself has none), two synthetic extremes of n, one soil per layer of a perturbed_columns draw."""
    kats = np.load(os.path.join(GOLDEN, "leaf_kats.npz"))["soils"]
    rows = [(a, n, k, kats[i % len(kats), 3], kats[i % len(kats), 4]) for i, (a, n, k) in enumerate(data.VG_TABLE)]
    rows += [(0.02, 1.09, 0.1, kats[0, 3], kats[0, 4]), (0.04, 3.5, 20.0, kats[1, 3], kats[1, 4])]
    p = workloads.perturbed_columns(1, seed=0)
    rows += [tuple(p[k][layer, 0] for k in workloads.PARAM_KEYS) for layer in range(3)]
    return np.array(rows, dtype=np.float64).astype(F)


def heads():
    dense = np.geomspace(1e-5, R.WP_PSI, 48).astype(F)
    cut = F(0.1)
    edges = np.array([0.0, np.nextafter(cut, F(0)), cut, 2e-38, 1e6, np.finfo(F).max], dtype=F)  # 2e-38 alpha is a denormal float
    return np.concatenate([edges, dense])


def _se_of_heads(soil, hs):
    return [F(float(R.stmt_se_from_h(soil, R.M(h)))) for h in hs]


def _se_smallest_finite(soil):
    """The smallest fp32 Se whose Se^(-1/m) stays finite in fp32 whichever way the pow's last bits fall (a margin of 2^-10)."""
    se = (mpmath.mpf(R.FLT_MAX) / (1 + mpmath.ldexp(1, -10))) ** (-soil.m_exact)
    return np.nextafter(F(float(se)), F(1))


def inputs():
    """{function: (soil index, x, y, z)} -- int16 and three fp32 arrays of one length."""
    mpmath.mp.dps = R.DPS
    S = soils()
    kats = np.load(os.path.join(GOLDEN, "leaf_kats.npz"))
    hs = heads()
    out = {fn: [] for fn in R.FUNCTIONS}
    for si, row in enumerate(S):
        soil = R.Soil(*row)
        te, tr = row[3], row[4]
        for h in hs:
            out["theta_from_h"].append((si, h, 0, 0))
            out["se_from_h"].append((si, h, 0, 0))
        ses = _se_of_heads(soil, hs) + list(kats["ses"].astype(F)) + [F(1), F(1) - F(2.0 ** -24), _se_smallest_finite(soil)]
        for se in ses:
            out["k_from_se"].append((si, se, 0, 0))
            out["h_from_se"].append((si, se, 0, 0))
        for dt in kats["aet_dts"]:
            for psi in kats["aet_psis"]:
                for pet in kats["aet_pets"]:
                    out["aet"].append((si, psi, pet, dt))
        thetas = [te if f == 1.0 else min(F(tr + F(f) * F(te - tr)), te) for f in FRACTIONS]
        for a in range(len(thetas)):
            for b in range(a + 1, len(thetas)):
                t1, t2 = thetas[a], thetas[b]
                for fn in ("geff", "geff_literal", "geff_closed"):
                    out[fn].append((si, t1, t2, 0))
                h = [F(float(R.stmt_h_from_se(soil, R.stmt_se_from_theta(soil, R.M(t))))) for t in (t1, t2)]
                out["geff_from_heads"].append((si, h[0], h[1], 0))
        # every node under the cut (the sum is (h_i - h_f) K_r(1)), and a wet end under the cut reached from a moist head
        out["geff_from_heads"] += [(si, 0.05, 0.01, 0), (si, 50.0, 0.01, 0)]
    rng = np.random.default_rng(20250)
    for x in np.geomspace(1e-6, 1e3, 24):
        for y in (-12.0, -5.5, -1.0, -0.3, 0.0826, 0.5, 1.0, 3.7, 12.0):
            if abs(y * np.log2(x)) <= 100:
                out["pow"].append((0, x, y, 0))
    for _ in range(192):
        a, b = 10.0 ** rng.uniform(-12, 12, 2) * rng.choice([-1.0, 1.0], 2)
        out["div"].append((0, a, b, 0))
        out["sqrt"].append((0, abs(a), 0, 0))
    res = {}
    for fn, pts in out.items():
        a = np.array(pts, dtype=np.float64)
        res[fn] = (a[:, 0].astype(np.int16), a[:, 1].astype(F), a[:, 2].astype(F), a[:, 3].astype(F))
    return S, res


def evaluate(fn, S, si, x, y, z):
    """(ref[N] float64, coef[N, 6] float64, near[N], gap[N]) of the points."""
    mpmath.mp.dps = R.DPS
    cache = {}
    ref, coef, near, gap = [], [], [], []
    for i in range(len(x)):
        k = int(si[i])
        if k not in cache:
            cache[k] = R.Soil(*S[k])
        r, c, nr, g = R.point(fn, cache[k], x[i], y[i], z[i], NINT)
        ref.append(r); coef.append(c); near.append(nr); gap.append(g)
    return np.array(ref, dtype=np.float64), np.array(coef, dtype=np.float64).reshape(-1, 6), np.array(near), np.array(gap)

