"""CPU: the fp32 leaf functions of the device code (lgar_py_amd/csrc/lgar_leaf.hpp built for the host with -DLGAR_DEVSIM: the
hardware's log2 / exp2 / sqrt / reciprocal are libm's here) against their 40-digit statement, tests/golden/leaf_f32/leaf_f32_ref.npz, within
the running error bound the fixture carries (tests/leaf_ref: the formulas, the bound model and why its factor is 2).  This pins
the formulas and constants of every float leaf -- ops 0-6, 9, 11 and 15-23 -- and proves the bound machinery without a GPU;
tests/test_gpu_leaf_f32.py asks the same of the hardware's instructions.

Measured here (worst error / bound, the bound already holding the factor 2; the table in DESIGN.md section 4 has every op):
theta_from_h 0.50, the other van Genuchten leaves and the AET 0.24-0.35, the trapezoids and the closed form 0.13-0.26, the
correctly rounded divide and sqrt 0.50 (half an ulp against 2 x 0.5).  Three mutations of the fp32 trapezoid -- -m/2 scaled by
1 + 2^-16, the fifth digit of log2(1e-12), n in place of n - 1 -- each leave the bound at a well-conditioned point."""
import numpy as np
import pytest

import leaf_host
import leaf_ref as R
from leaf_ref import check

F = np.float32
LGAR_E_ARG = -1  # include/lgar.h


@pytest.fixture(scope="module")
def fixture():
    return R.load()


def test_committed_fixture_is_the_generators_output(fixture):
    """Every 16th point of every function, evaluated again with mpmath: the same reference values and coefficients bit for bit."""
    pytest.importorskip("mpmath")
    from leaf_ref import grid
    S, names, fns = fixture
    assert np.array_equal(S, grid.soils()) and names == grid.SOIL_NAMES
    for fn, d in fns.items():
        w = slice(0, None, 16)
        ref, coef, _, _ = grid.evaluate(fn, S, d["soil"][w], d["x"][w], d["y"][w], d["z"][w])
        assert np.array_equal(ref, d["ref"][w], equal_nan=True), fn
        assert np.array_equal(coef, d["coef"][w]), fn


@pytest.mark.parametrize("fn", R.FUNCTIONS)
def test_float_leaf_within_the_bound_of_its_statement(fixture, fn):
    """|got - ref| <= 2 sum_k coef_k u_k at every point with libm's unit errors (1 ulp log2f / exp2f, 0.5 divide and sqrt; the host's
    POL_RCP32 quotient a * (1.0f / b) is two roundings: 1.5), the statement's class where it is inf or NaN, at most 2 % such."""
    S, names, fns = fixture
    for op, key in R.OPS_OF[fn]:
        check.against_fixture(fn, op, check.run(leaf_host.leaf_batch, op, S, fns[fn]), fns[fn], R.UNITS_HOST[key], names)


def test_exact_edges(fixture):
    S, names, _ = fixture
    check.exact_edges(leaf_host.leaf_batch, S, names)


def test_theta_from_h_stays_in_the_domain(fixture):
    S, names, fns = fixture
    check.theta_stays_in_the_domain(leaf_host.leaf_batch, S, fns["theta_from_h"], names)


def test_float_only_ops_are_refused_in_double():
    kw = dict(alpha=[0.01], n=[1.5], ksat=[1.0], theta_e=[0.4], theta_r=[0.1])
    for op in range(15, 24):
        assert leaf_host.leaf_batch_status(op, [0.5], [0.6], dtype=np.float64, **kw)[0] == LGAR_E_ARG
        assert leaf_host.leaf_batch_status(op, [0.5], [0.6], dtype=np.float32, **kw)[0] == 0
    assert leaf_host.leaf_batch_status(24, [0.5], [0.6], **kw)[0] == LGAR_E_ARG
    # (the double leaves go through the same dispatcher: theta_from_h against the closed formula)
    got = leaf_host.leaf_batch(0, [10.0], dtype=np.float64, **kw)[0]
    assert abs(got - (0.1 + 0.3 / (1 + 0.1 ** 1.5) ** (1 - 1 / 1.5))) <= 1e-13
