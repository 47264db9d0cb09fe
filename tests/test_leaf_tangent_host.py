"""CPU: the dual-number arithmetic of the tangent kernels (lgar_py_amd/csrc/lgar_dual.hpp), reached element-wise through
leaf_tangent_eval (lgar_leaf.hpp) built for the host with -DLGAR_DEVSIM (tests/leaf_host: log2 / exp2 / reciprocal are libm's and
the IEEE divide here), against the exact derivative of the reference's discrete formulas
(tests/golden/leaf_tangent/leaf_tangent_ref.npz, written by tests/golden/make_leaf_tangent_golden.py from tests/leaf_ref/tangent.py).

(a) the value is lgar_leaf_batch's bit for bit and does not depend on the seeds; (b) double precision: every partial of every op,
one unit seed at a time, and a random mixed direction, within MARGIN max(E_ref, 4 2^-53 A) of the statement -- E_ref the
reference's own autograd error at the point and its neighbours, A the partial's terms by absolute value; the lean pow's stated
error on top for POL_LEAN (leaf_ref.check.tangent_tolerance, where the recorded conditionings are derived: the lean pow, the
exponents' rounding, the trapezoid's tangent running sum); (c) single precision: classes
and the value identity, errors reported; (e) the argument checks; and the same code under AddressSanitizer + UBSan as a stand-alone
program.  tests/test_gpu_leaf_tangent.py asks (a)-(c) of the hardware and adds the shared trapezoid, which has no host build.
The measured tables are in DESIGN.md section 4."""
import numpy as np
import pytest

import _hostbuild
import leaf_host
import leaf_ref as R
from leaf_ref import check
from leaf_ref import tangent as TG

LGAR_E_ARG = -1  # include/lgar.h
# tangent function -> op of lgar_leaf_batch with the same value, per dtype (None: no counterpart).  The fp32 trapezoid has none:
# the fp32 tangent kernels run the fused loop (geff_fused<Dual<float>>), the fp32 forward kernels the packed one (op 4 there).
LEAF_OP = dict(theta_from_h=0, se_from_h=1, k_from_se=2, h_from_se=3, aet=5, geff=4, geff_literal=6, lg2p=7, ex2p=8, pw=9, dv=11)
LEAF_OP_F32 = dict(LEAF_OP, sq=16, geff=None)


def host_tbatch(op, x, y=None, z=0.0, **kw):
    return leaf_host.leaf_tangent_batch(op, x, y, z, **kw)


def host_batch(op, x, y=None, z=0.0, **kw):
    return leaf_host.leaf_batch(op, x, y, z, **kw)


@pytest.fixture(scope="module")
def fixture():
    return TG.load()


def test_committed_fixture_is_the_generators_output(fixture):
    """Every 16th point of every function evaluated again with mpmath: the same statement bit for bit; the fixture's own rules
    (the 2 % cap, the nudge gap under the parity bar); the dual propagation against mpmath.diff at one point per leaf."""
    pytest.importorskip("mpmath")
    from leaf_ref import grid
    S, names, fns, gap = fixture
    S2, pts = grid.tangent_inputs()
    assert np.array_equal(S, S2) and names == grid.SOIL_NAMES
    for fn, d in fns.items():
        si, x, y, z, ok = pts[fn]
        if len(x) != len(d["x"]):  # (the trapezoids the reference cannot evaluate are left out of the file)
            assert fn in ("geff", "geff_literal") and len(x) - len(d["x"]) <= 8
            have = set(zip(d["soil"].tolist(), d["x"].tolist(), d["y"].tolist()))
            keep = np.array([p in have for p in zip(si.tolist(), x.tolist(), y.tolist())])
            si, x, y, z, ok = (a[keep] for a in (si, x, y, z, ok))
        assert np.array_equal(x, d["x"]) and np.array_equal(y, d["y"]) and np.array_equal(si, d["soil"]) and np.array_equal(ok, d["f32ok"]), fn
        bad = ~(np.isfinite(d["value"]) & np.isfinite(d["grad"]).all(axis=1))
        assert bad.sum() <= 0.02 * len(x), fn
        step = 64 if fn in ("geff", "geff_literal") else 16
        for i in range(0, len(x), step):
            if fn in TG.LEAVES:
                v, g = TG.leaf(fn, S[int(si[i])], x[i], y[i], z[i], check.NINT)[:2]
            else:
                v, dx, dy = TG.prim(fn, x[i], y[i])
                v, g = float(v), [0.0] * 5 + [float(dx), float(dy)]
            assert np.array_equal(np.array([v] + list(g)), np.concatenate([[d["value"][i]], d["grad"][i]]), equal_nan=True), (fn, i)
    for fn in ("geff", "geff_literal"):  # the bound on the tangent running sum: regenerated at three pairs
        d = fns[fn]
        for i in (0, len(d["x"]) // 2, len(d["x"]) - 1):
            again = np.nextafter(np.array(TG.drift(fn, S[int(d["soil"][i])], d["x"][i], d["y"][i], check.NINT)).astype(np.float32), np.float32(np.inf))
            assert np.array_equal(again, d["drift"][i]) and (again[[0, 1, 3, 4, 5, 6]] > 1e-30).all() and again[2] < 1e-44, (fn, i)
    assert gap.shape == (len(S), 8) and gap.max() < 1e-6
    for fn in ("theta_from_h", "k_from_se", "h_from_se", "aet", "geff_closed"):
        d = fns[fn]
        i = len(d["x"]) // 3
        assert TG.check_against_diff(fn, S[int(d["soil"][i])], d["x"][i], d["y"][i], d["z"][i]) <= 1e-15, fn


@pytest.mark.parametrize("fn", TG.FUNCTIONS)
def test_value_is_the_leaf_entrys_and_independent_of_the_seeds(fixture, fn):
    S, names, fns, _ = fixture
    for dtype, table in ((np.float64, LEAF_OP), (np.float32, LEAF_OP_F32)):
        check.tangent_values(fn, TG.OP_OF[fn], table.get(fn), host_tbatch, host_batch, S, fns[fn], dtype)


@pytest.mark.parametrize("fn", TG.FUNCTIONS)
def test_double_tangent_within_the_tolerance_of_the_statement(fixture, fn):
    """(b).  Measured, host build and MI355X: every op within 0.71 of the tolerance (geff d/dtheta_2, vg_table_17); 0.06 ... 0.50
    elsewhere.  The terms of leaf_ref.check.tangent_tolerance beyond MARGIN max(E_ref, floor) and what called for each are in
    DESIGN.md section 4 "Tangent leaves"."""
    S, names, fns, _ = fixture
    ref_stmt = fns["geff_literal"] if fn == "geff" else None  # (the reference computes the trapezoid WITH the nudge)
    for policy in ((check.LEAN, check.LIBRARY) if fn in TG.POLICY_LEAVES else (check.LEAN,)):
        check.tangent_against_fixture(fn, TG.OP_OF[fn], host_tbatch, S, fns[fn], names, policy, ref_stmt)


@pytest.mark.parametrize("fn", TG.FUNCTIONS)
def test_float_tangent_classes(fixture, fn):
    S, names, fns, _ = fixture
    check.tangent_f32(fn, TG.OP_OF[fn], host_tbatch, S, fns[fn], names, library_too=fn in TG.POLICY_LEAVES)


def test_aet_clamp_regimes(fixture):
    """The clamp of the AET below 0, above pet and at the exact tie: reached by the fixture, torch's derivative in the statement
    and in the reference, the kernel's exact in both precisions and both policies."""
    S, names, fns, _ = fixture
    check.aet_clamp_regimes(host_tbatch, S, fns["aet"])


def test_departures_from_torch():
    check.tangent_departures(host_tbatch)


def test_argument_checks():
    kw = dict(alpha=[0.01], n=[1.5], ksat=[1.0], theta_e=[0.4], theta_r=[0.1])
    st = lambda op, **k: leaf_host.leaf_tangent_batch_status(op, [0.2], [0.3], **dict(kw, **k))[0]
    assert st(4) == 0 and st(4, dtype=np.float32) == 0
    for op in (-1, 10, 12, 15, 17, 22, 33):  # no such tangent op
        assert st(op) == LGAR_E_ARG, op
    assert st(0, policy=2) == LGAR_E_ARG and st(0, policy=-1) == LGAR_E_ARG
    assert st(4, null_outputs=True) == LGAR_E_ARG
    assert leaf_host.leaf_tangent_batch_status(4, [0.2], None, **kw)[0] == LGAR_E_ARG  # the trapezoid reads y
    # the shared trapezoid: widths 2 .. 32, double precision, op 4 only -- and not at all on the host build
    for share in (1, 33, -2, 2, 9, 32):
        assert st(4, share=share) == LGAR_E_ARG, share
    assert st(4, share=9, dtype=np.float32) == LGAR_E_ARG and st(6, share=9) == LGAR_E_ARG
    # (the check itself, as the library runs it: lgar_leaf.hpp leaf_tangent_check<false>, through the program below)


def test_stand_alone_program_under_asan_ubsan():
    """Every leaf and tangent op, both precisions, both policies, every unit seed, on the grids' edge points: the host program built
    with AddressSanitizer + UBSan and run as a plain executable; it also runs the library's own form of the argument checks."""
    out = _hostbuild.run_clean([leaf_host.program(sanitize=True)]).split()
    assert out[0] == "ok" and int(out[1]) > 100000
