"""CPU: catchment routing (lgar_catchment_route / lgar_catchment_route_grad, include/lgar.h).

The fold without a dependence between rows, the queue hand-over and the ordinate-gradient accumulation the GPU kernels run
(lgar_py_amd/csrc/lgar_route.hpp) are compiled for the host into a small stand-alone program (tests/post_host).  It is held
BIT FOR BIT to the reference's own recorded giuh_runoff and giuh_runoff_queue (every committed fixture with num_subcycles = 1)
and to the numpy statement of the definition (post_host.route.route_ref: the queue recurrence itself); the same program built with
AddressSanitizer + UBSan runs the same cases.  CatchmentRouting's host logic needs no GPU either."""
import os

import numpy as np
import pytest

from _golden import steps_before_crash
from conftest import GOLDEN, golden_names

import post_host as PH
from post_host import route as RH

RUNOFF, GIUH_RUNOFF = 4, 6  # ACC_NAMES


def _fixtures():
    """(name, runoff [T], giuh_runoff [T], queue after every row [T, K], ordinates [K]) of every fixture the operator is defined
    against: one shift per stored row, rows the reference completed."""
    out = []
    for nm in golden_names():
        g = np.load(os.path.join(GOLDEN, nm + ".npz"))
        if "giuh_queue" not in g.files or int(g["num_subcycles"]) != 1:
            continue
        _, T = steps_before_crash(g)
        if T > 0:
            out.append((nm, g["acc"][:T, RUNOFF].copy(), g["acc"][:T, GIUH_RUNOFF].copy(), g["giuh_queue"][:T].copy(), g["giuh_ordinates"].copy()))
    return out


@pytest.fixture(scope="module")
def fixtures():
    fx = _fixtures()
    assert len(fx) >= 60, len(fx)
    return fx


def test_reference_parity_bit_for_bit(fixtures):
    """Routing the reference's own runoff column with the fixture's ordinates gives the reference's giuh_runoff column and its
    queue after the last row, bit for bit (all fixtures in ONE run of the host program, each a B = 1 case)."""
    got = PH.run(map(RH.case, [dict(mode="forward", x=x[:, None], g=g) for _, x, _, _, g in fixtures]))
    for (nm, x, want, queue, g), (y, q_out) in zip(fixtures, got):
        assert RH.same_bits(y[:, 0], want), nm
        assert RH.same_bits(q_out[:, 0], queue[-1]), nm
    assert sum(float(np.abs(y).max()) > 0 for y, _ in got) >= 30  # (most fixtures do have runoff)


def test_resume_at_a_cut_from_the_reference_queue(fixtures):
    """Cut at three places -- after a single row, in the middle, one row before the end -- and resumed from the REFERENCE's queue
    at the cut (giuh_queue[cut - 1]): the rows behind the cut and the final queue are those of the uncut run, and the rows
    before the cut leave exactly the reference's queue.  This pins the carry to the reference at the cut."""
    cases, index = [], []
    for nm, x, want, queue, g in fixtures:
        T = len(x)
        for cut in sorted({1, T // 2, T - 1}):
            if 0 < cut < T:
                cases.append(dict(mode="forward", x=x[:cut, None], g=g))
                cases.append(dict(mode="forward", x=x[cut:, None], g=g, q_in=queue[cut - 1][:, None]))
                index.append((nm, cut, want, queue))
    got = PH.run(map(RH.case, cases))
    assert len(index) >= 3 * 50
    for i, (nm, cut, want, queue) in enumerate(index):
        (y0, q0), (y1, q1) = got[2 * i], got[2 * i + 1]
        assert RH.same_bits(y0[:, 0], want[:cut]) and RH.same_bits(q0[:, 0], queue[cut - 1]), (nm, cut)
        assert RH.same_bits(y1[:, 0], want[cut:]) and RH.same_bits(q1[:, 0], queue[-1]), (nm, cut)


def _definition_cases():
    """B in {1, 63, 64, 65, 257} x K in {1, 2, 5, 8, 64} x T in {0, 1, K - 1, K, K + 1, 11}, shared and per-catchment ordinates,
    with and without a queue; forward, reverse and the ordinate gradient.  (cases, references), the references by the numpy
    recurrence."""
    rng = np.random.default_rng(12)
    cases, refs = [], []
    for B in RH.SHAPE_B:
        for K in RH.SHAPE_K:
            for T in RH.shape_T(K):
                for per in (False, True):
                    x, gy, g, q_in = RH.mixed_data(rng, T, B, K, per)
                    for q in (None, q_in):
                        cases.append(dict(mode="forward", x=x, g=g, q_in=q))
                        refs.append(RH.route_ref(x, g, q))
                    cases.append(dict(mode="reverse", x=gy, g=g))
                    refs.append((RH.adjoint_ref(gy, g), None))
                cases.append(dict(mode="grad", x=x, gy=gy, K=K))
                refs.append((RH.ordinate_grad_ref(x, gy, K), None))
    return cases, refs


@pytest.fixture(scope="module")
def definition_cases():
    return _definition_cases()


def _check(cases, refs, got):
    assert len(got) == len(refs) == len(cases)
    for c, r, o in zip(cases, refs, got):
        what = (c["mode"], c["x"].shape, c.get("K", None if "g" not in c else np.shape(c["g"])), c.get("q_in") is not None)
        assert RH.same_bits(o[0], r[0]), what
        assert (r[1] is None and o[1] is None) or RH.same_bits(o[1], r[1]), what


def test_host_build_equals_the_numpy_definition_bit_for_bit(definition_cases):
    """The fold of the kernels against the recurrence of the definition: mixed signs, a NaN and -0.0 in the inputs."""
    cases, refs = definition_cases
    _check(cases, refs, PH.run(map(RH.case, cases)))
    # T = 0 hands the queue over as it is; without one it is +0.0
    for c, (y, q) in zip(cases, refs):
        if c["mode"] == "forward" and c["x"].shape[0] == 0:
            assert RH.same_bits(q, np.zeros_like(q) if c["q_in"] is None else c["q_in"])
    # the definition means what it says: within the bound of two fp64 evaluation orders of numpy's own convolution (no NaN)
    rng = np.random.default_rng(3)
    x, g = rng.standard_normal((40, 7)), rng.random((5, 7))
    y, _ = RH.route_ref(x, g)
    bound = (5 + 1) * 2.0 ** -52 * RH.dense_conv(np.abs(x), np.abs(g))
    assert (np.abs(y - RH.dense_conv(x, g)) <= bound).all()
    # ... and the adjoint and the ordinate gradient are the derivatives of that convolution
    v = rng.standard_normal((40, 7))
    # (both inner products are sums of the same 40 x 7 x 5 products in two orders)
    assert abs((y * v).sum() - (x * RH.adjoint_ref(v, g)).sum()) <= (5 + 1 + 280) * 2.0 ** -52 * (RH.dense_conv(np.abs(x), np.abs(g)) * np.abs(v)).sum()
    eps = 1e-6
    gp = g.copy()
    gp[2, 3] += eps
    fd = ((RH.route_ref(x, gp)[0] - y) * v).sum() / eps
    assert abs(fd - RH.ordinate_grad_ref(x, v, 5)[2, 3]) <= 1e-6 * max(1.0, abs(fd))


def test_chunked_routing_equals_one_call(definition_cases):
    """T = 11 in chunks of (3, 1, 7) through the carried queue, K = 5 and K = 8 (a chunk shorter than the queue): the same bits."""
    rng = np.random.default_rng(5)
    for K in (5, 8):
        for per in (False, True):
            x, _, g, q_in = RH.mixed_data(rng, 11, 65, K, per)
            (whole, q_whole), = PH.run(map(RH.case, [dict(mode="forward", x=x, g=g, q_in=q_in)]))
            q, at, parts = q_in, 0, []
            for n in (3, 1, 7):
                (y, q), = PH.run(map(RH.case, [dict(mode="forward", x=x[at:at + n], g=g, q_in=q)]))
                parts.append(y)
                at += n
            assert RH.same_bits(np.concatenate(parts), whole) and RH.same_bits(q, q_whole)


def test_sanitizer_build_on_the_same_cases(definition_cases, fixtures):
    """AddressSanitizer + UBSan build of the same program (a stand-alone executable: nothing is loaded into python; every array
    is allocated at its exact size) over the same cases and three fixtures: clean, with the bits of the plain build's
    references.  Any finding aborts the program."""
    cases, refs = definition_cases
    extra = [dict(mode="forward", x=x[:, None], g=g) for _, x, _, _, g in fixtures[:3]]
    got = PH.run(map(RH.case, cases + extra), sanitize=True)
    _check(cases, refs, got[:len(cases)])
    for (nm, x, want, queue, g), (y, q_out) in zip(fixtures[:3], got[len(cases):]):
        assert RH.same_bits(y[:, 0], want) and RH.same_bits(q_out[:, 0], queue[-1]), nm


# CatchmentRouting's host logic -----------------------------------------------------------------------------------------------
def _routing(*a, **kw):
    from lgar_py_amd.catchments import CatchmentRouting
    return CatchmentRouting(*a, device="cpu", **kw)


def test_routing_shapes_and_transposition():
    import torch
    import lgar_py_amd as lg
    assert lg.CatchmentRouting is not None and callable(lg.catchment_route)
    g = np.random.default_rng(0).random((7, 5))
    r = _routing(g)
    assert (r.K, r.B, r.per_catchment) == (5, 7, True)
    assert tuple(r.ordinates.shape) == (5, 7) and r.ordinates.is_contiguous() and r.ordinates.dtype == torch.float64
    assert np.array_equal(r.ordinates.numpy(), g.T) and np.array_equal(r.ordinates_host.numpy(), g.T)
    assert _routing(torch.tensor(g), n_catchments=7).B == 7
    s = _routing([0.06, 0.51, 0.28, 0.12, 0.03])
    assert (s.K, s.B, s.per_catchment) == (5, None, False) and s.ordinates.tolist() == [0.06, 0.51, 0.28, 0.12, 0.03]
    assert _routing([1.0], n_catchments=9).B == 9 and _routing(np.ones(64)).K == 64 and _routing(np.ones((3, 64))).K == 64
    assert s.queue is None and s.queue_of("runoff") is None
    s.reset()


def test_routing_rejections():
    import torch
    from lgar_py_amd import LgarError
    for bad in (dict(ordinates=[]), dict(ordinates=np.ones(65)), dict(ordinates=np.ones((4, 0))), dict(ordinates=np.ones((4, 65))),
                dict(ordinates=[0.5, float("nan")]), dict(ordinates=[[0.5, float("inf")]]), dict(ordinates=np.ones((4, 5)), n_catchments=3),
                dict(ordinates=np.ones((2, 2, 2))), dict(ordinates=1.0), dict(ordinates=[1.0], n_catchments=-1)):
        with pytest.raises(LgarError):
            _routing(**bad)
    # a routing on the CPU holds the host logic only: the routing itself has no CPU fallback
    r = _routing([0.5, 0.5], n_catchments=3)
    x = torch.zeros(4, 3, dtype=torch.float64)
    for call in (lambda: r.route(x), lambda: r.adjoint(x), lambda: r.ordinate_grad(x, x)):
        with pytest.raises(LgarError, match="no CPU fallback"):
            call()
    with pytest.raises(LgarError):
        r.route(torch.zeros(4, 2, dtype=torch.float64))  # another B
    with pytest.raises(LgarError):
        r.route(torch.zeros(4, 3, dtype=torch.float32))  # fp64 only
