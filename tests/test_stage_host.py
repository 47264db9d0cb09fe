"""lgar_py_amd/_stage.py, the shared host logic of the catchment stages, through the five stages that use it: every class of
wrong input still raises the message the stages raised when each had its own copy of the checks (the literals below were taken
from that version, not computed), and the carried state behaves as every carrier documents it."""
import numpy as np
import pytest
import torch

from baseflow_host import SimCatchmentBaseflow, case_data, same_bits
from lgar_py_amd import LgarError, NetworkPools, network_route_mc, network_route_pool
from network_pool_host import SimCatchmentNetworkPool
from snow_host import SimCatchmentSnow

F64 = torch.float64
ones = lambda *shape, **kw: torch.ones(*shape, dtype=kw.pop("dtype", F64), **kw)


def _baseflow(**kw):
    args = dict(cgw=[0.1, 0.2, 0.3], expon=[1.0, 2.0, 3.0], smax=[5.0, 6.0, 7.0], dt_h=1.0)
    args.update(kw)
    return SimCatchmentBaseflow(**args)


def _snow(**kw):
    args = dict(tlo=[-1.0, -1.0], thi=[1.0, 1.0], tm=0.0, sfcf=1.0, cfmax=0.1, cfr=0.05, cwh=0.1, dt_h=1.0)
    args.update(kw)
    return SimCatchmentSnow(**args)


def _net():
    return SimCatchmentNetworkPool([1, 2, -1])  # a chain of three


def _mc(**kw):
    args = dict(kref=ones(3), beta=0.4, X=0.2, qref=1.0, dt_h=1.0)
    args.update(kw)
    return _net().route_mc(ones(4, 3), **args)


def _pool(reach=None, pool=None, **kw):
    net = _net()
    pools = NetworkPools(net, [1, 2])  # catchment 0 is a reach
    reach = dict(dict(kref=1.0, beta=0.4, X=0.2, qref=1.0), **(reach or {}))
    pool = dict(dict(cq=1.0, m=1.5, s0=0.0, sref=1.0, smax=float("inf")), **(pool or {}))
    return net.route_pool(ones(4, 3), pools, tuple(reach.values()), tuple(pool.values()), kw.pop("dt_h", 1.0), **kw)


CASES = {
    # ---- baseflow: the constructor's block, run()'s tensors, function()'s rows
    "baseflow-dtype": (lambda: _baseflow(cgw=ones(3, dtype=torch.float32)), "cgw must be fp64 (got torch.float32)"),
    "baseflow-2d": (lambda: _baseflow(expon=np.ones((2, 3))), "expon must be a scalar or [B], one entry per catchment (got shape (2, 3))"),
    "baseflow-not-numbers": (lambda: _baseflow(smax="deep"), "smax must be numbers (could not convert string to float: 'deep')"),
    "baseflow-sizes": (lambda: _baseflow(expon=[1.0, 2.0]),
                       "cgw, expon, smax must agree on one number of catchments: [B] each, or scalars with n_catchments= (got [2, 3])"),
    "baseflow-scalars-only": (lambda: _baseflow(cgw=0.1, expon=1.0, smax=5.0),
                              "cgw, expon, smax must agree on one number of catchments: [B] each, or scalars with n_catchments= (got scalars only)"),
    "baseflow-count": (lambda: _baseflow(cgw=0.1, expon=1.0, smax=5.0, n_catchments=-1), "0 .. 2^31 - 1 catchments (got -1)"),
    "baseflow-non-finite": (lambda: _baseflow(smax=[5.0, float("nan"), 7.0]), "smax[1] = nan: every smax must be finite and > 0"),
    "baseflow-rule": (lambda: _baseflow(expon=[1.0, 2.0, 0.0]), "expon[2] = 0.0: every expon must be finite and > 0"),
    "baseflow-first-rule": (lambda: _baseflow(cgw=[0.1, -0.5, 0.3], smax=[0.0, 1.0, 1.0]), "cgw[1] = -0.5: every cgw must be finite and >= 0"),
    "baseflow-dt": (lambda: _baseflow(dt_h=0.0), "dt_h must be finite and > 0 hours (got 0.0)"),
    "baseflow-dt-type": (lambda: _baseflow(dt_h=None),
                         "dt_h must be a number of hours (float() argument must be a string or a real number, not 'NoneType')"),
    "baseflow-run-length": (lambda: _baseflow().run(ones(4, 2)), "recharge must be a fp64 [T, 3] tensor on cpu"),
    "baseflow-run-dtype": (lambda: _baseflow().run(ones(4, 3, dtype=torch.float32)), "recharge must be a fp64 [T, 3] tensor on cpu"),
    "baseflow-run-device": (lambda: _baseflow().run(ones(4, 3, device="meta")), "recharge must be a fp64 [T, 3] tensor on cpu"),
    "baseflow-run-state": (lambda: _baseflow().run(ones(4, 3), state=ones(2)), "state must be a fp64 [3] tensor on cpu"),
    "baseflow-function-length": (lambda: SimCatchmentBaseflow.function(ones(4, 3), ones(2), 1.0, 5.0, 1.0),
                                 "cgw must be a fp64 [3] tensor or a scalar on cpu"),
    "baseflow-function-2d": (lambda: SimCatchmentBaseflow.function(ones(4, 3), 0.1, ones(1, 3), 5.0, 1.0),
                             "expon must be a fp64 [3] tensor or a scalar on cpu"),
    "baseflow-function-device": (lambda: SimCatchmentBaseflow.function(ones(4, 3), 0.1, 1.0, ones(3, device="meta"), 1.0),
                                 "smax must be a fp64 [3] tensor or a scalar on cpu"),
    "baseflow-function-type": (lambda: SimCatchmentBaseflow.function(ones(4, 3), "much", 1.0, 5.0, 1.0),
                               "cgw must be a fp64 [3] tensor or a scalar (could not convert string to float: 'much')"),
    "baseflow-function-state": (lambda: SimCatchmentBaseflow.function(ones(4, 3), 0.1, 1.0, 5.0, 1.0, state=ones(3, 1)),
                                "state must be a fp64 [3] tensor on cpu"),
    # ---- snow: the same block with "cells", the [2, B] pack
    "snow-dtype": (lambda: _snow(tm=ones(2, dtype=torch.float32)), "tm must be fp64 (got torch.float32)"),
    "snow-2d": (lambda: _snow(cfr=np.ones((1, 2))), "cfr must be a scalar or [B], one entry per cell (got shape (1, 2))"),
    "snow-sizes": (lambda: _snow(cwh=[0.1, 0.1, 0.1]),
                   "tlo, thi, tm, sfcf, cfmax, cfr, cwh must agree on one number of cells: [B] each, or scalars with n_catchments= (got [2, 3])"),
    "snow-scalars-only": (lambda: _snow(tlo=-1.0, thi=1.0),
                          "tlo, thi, tm, sfcf, cfmax, cfr, cwh must agree on one number of cells: [B] each, or scalars with n_catchments= "
                          "(got scalars only)"),
    "snow-count": (lambda: _snow(tlo=-1.0, thi=1.0, n_catchments=2 ** 31), "0 .. 2^31 - 1 cells (got 2147483648)"),
    "snow-non-finite": (lambda: _snow(tm=float("inf")), "tm[0] = inf: every tm must be finite"),
    "snow-rule": (lambda: _snow(cfmax=[0.1, -0.1]), "cfmax[1] = -0.1: every cfmax must be finite and >= 0"),
    "snow-transition": (lambda: _snow(tlo=[-1.0, 2.0]), "tlo[1] = 2.0 > thi[1] = 1.0: the transition needs tlo <= thi"),
    "snow-run-length": (lambda: _snow().run(ones(4, 3), ones(4, 3)), "precip must be a fp64 [T, 2] tensor on cpu"),
    "snow-run-rows": (lambda: _snow().run(ones(4, 2), ones(5, 2)), "temp must be a fp64 [4, 2] tensor on cpu"),
    "snow-run-device": (lambda: _snow().run(ones(4, 2), ones(4, 2, device="meta")), "temp must be a fp64 [4, 2] tensor on cpu"),
    "snow-run-state": (lambda: _snow().run(ones(4, 2), ones(4, 2), state=ones(2)), "state must be a fp64 [2, 2] tensor (ice, liq) on cpu"),
    "snow-function-dtype": (lambda: SimCatchmentSnow.function(ones(4, 2), ones(4, 2), -1.0, ones(2, dtype=torch.float32), 0.0, 1.0, 0.1, 0.05, 0.1, 1.0),
                            "thi must be a fp64 [2] tensor or a scalar on cpu"),
    "snow-function-length": (lambda: SimCatchmentSnow.function(ones(4, 2), ones(4, 2), -1.0, 1.0, 0.0, 1.0, 0.1, 0.05, ones(3), 1.0),
                             "cwh must be a fp64 [2] tensor or a scalar on cpu"),
    # ---- the linear route: its matrices name the device as the network was given it
    "route-length": (lambda: _net().route(ones(4, 2), ones(3, 3)), "x must be a fp64 [T, 3] tensor on cpu"),
    "route-dtype": (lambda: _net().route(ones(4, 3, dtype=torch.float32), ones(3, 3)), "x must be a fp64 [T, 3] tensor on cpu"),
    "route-device": (lambda: _net().route(ones(4, 3), ones(3, 3, device="meta")), "coef must be a fp64 [3, 3] tensor on cpu"),
    "route-coef-rows": (lambda: _net().route(ones(4, 3), ones(2, 3)), "coef must be a fp64 [3, 3] tensor on cpu"),
    "route-state": (lambda: _net().route(ones(4, 3), ones(3, 3), state=ones(3, 3)), "state must be a fp64 [2, 3] tensor on cpu"),
    # ---- Muskingum-Cunge: the rows one by one, each with its rule, then the scalars
    "mc-dtype": (lambda: _mc(kref=ones(3, dtype=torch.float32)), "kref must be a fp64 [3] tensor or a scalar on cpu"),
    "mc-length": (lambda: _mc(beta=ones(2)), "beta must be a fp64 [3] tensor or a scalar on cpu"),
    "mc-device": (lambda: _mc(X=ones(3, device="meta")), "X must be a fp64 [3] tensor or a scalar on cpu"),
    "mc-2d": (lambda: _mc(qref=ones(3, 1)), "qref must be a fp64 [3] tensor or a scalar on cpu"),
    "mc-type": (lambda: _mc(beta=None),
                "beta must be a fp64 [3] tensor or a scalar (float() argument must be a string or a real number, not 'NoneType')"),
    "mc-non-finite": (lambda: _mc(kref=torch.tensor([1.0, float("inf"), 1.0], dtype=F64)), "kref[1] = inf: every kref must be finite and > 0"),
    "mc-rule": (lambda: _mc(X=0.6), "X[0] = 0.6: every X must be finite and in 0 .. 0.5"),
    "mc-value-before-type": (lambda: _mc(kref=-1.0, beta=ones(2)), "kref[0] = -1.0: every kref must be finite and > 0"),
    "mc-range": (lambda: _mc(rmin=2.0, rmax=1.0), "rmin, rmax must satisfy 2^-60 <= rmin <= rmax <= 2^60 (got 2.0, 1.0)"),
    "mc-dt": (lambda: _mc(dt_h=float("nan")), "dt_h must be finite and > 0 hours (got nan)"),
    "mc-scalars-type": (lambda: _mc(rmax="wide"), "dt_h, rmin, rmax must be numbers (could not convert string to float: 'wide')"),
    "mc-dt-before-range": (lambda: _mc(dt_h=-1.0, rmin=2.0, rmax=1.0), "dt_h must be finite and > 0 hours (got -1.0)"),
    "mc-function-range": (lambda: network_route_mc(ones(4, 3), _net(), 1.0, 0.4, 0.2, 1.0, 1.0, rmin=2.0 ** -61),
                          "rmin, rmax must satisfy 2^-60 <= rmin <= rmax <= 2^60 (got 4.336808689942018e-19, 64.0)"),
    # ---- reaches and pools: rules only where a value is read, the pool's smax against its s0
    "pool-dtype": (lambda: _pool(pool=dict(cq=ones(2, dtype=torch.float32))), "cq must be a fp64 [2] tensor or a scalar on cpu"),
    "pool-length": (lambda: _pool(pool=dict(m=ones(3))), "m must be a fp64 [2] tensor or a scalar on cpu"),
    "pool-device": (lambda: _pool(pool=dict(sref=ones(2, device="meta"))), "sref must be a fp64 [2] tensor or a scalar on cpu"),
    "pool-2d": (lambda: _pool(pool=dict(s0=ones(2, 1))), "s0 must be a fp64 [2] tensor or a scalar on cpu"),
    "pool-reach-length": (lambda: _pool(reach=dict(kref=ones(2))), "kref must be a fp64 [3] tensor or a scalar on cpu"),
    "pool-non-finite": (lambda: _pool(pool=dict(s0=torch.tensor([0.0, float("nan")], dtype=F64))),
                        "s0[1] = nan (pool at catchment 2): every s0 must be finite"),
    "pool-rule": (lambda: _pool(pool=dict(sref=0.0)), "sref[0] = 0.0 (pool at catchment 1): every sref must be finite and > 0"),
    "pool-smax-below-s0": (lambda: _pool(pool=dict(s0=torch.tensor([1.0, 3.0], dtype=F64), smax=2.0)),
                           "smax[1] = 2.0 (pool at catchment 2): every smax must be >= s0 (+inf: the pool never spills)"),
    "pool-reach-rule": (lambda: _pool(reach=dict(kref=torch.tensor([-1.0, 1.0, 1.0], dtype=F64))),
                        "kref[0] = -1.0: every kref of a reach must be finite and > 0"),
    "pool-range": (lambda: _pool(prmin=4.0, prmax=2.0), "prmin, prmax must satisfy 2^-60 <= prmin <= prmax <= 2^60 (got 4.0, 2.0)"),
    "pool-reach-range-first": (lambda: _pool(rmin=2.0, rmax=1.0, prmin=4.0, prmax=2.0),
                               "rmin, rmax must satisfy 2^-60 <= rmin <= rmax <= 2^60 (got 2.0, 1.0)"),
    "pool-range-type": (lambda: _pool(prmax=None),
                        "prmin, prmax must be numbers (float() argument must be a string or a real number, not 'NoneType')"),
    "pool-function-range": (lambda: network_route_pool(ones(4, 3), _net(), None, (1.0, 0.4, 0.2, 1.0), (1.0, 1.5, 0.0, 1.0, 2.0), 1.0, prmax=2.0 ** 61),
                            "prmin, prmax must satisfy 2^-60 <= prmin <= prmax <= 2^60 (got 9.5367431640625e-07, 2.305843009213694e+18)"),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_wrong_input_keeps_its_message(name):
    call, message = CASES[name]
    with pytest.raises(LgarError) as err:
        call()
    assert str(err.value) == message


def test_a_value_read_nowhere_is_not_checked():
    """route_pool's rules hold only where a value is read: a reach parameter at a pool may be anything."""
    y = _pool(reach=dict(kref=torch.tensor([1.0, float("nan"), -1.0], dtype=F64)))
    assert bool(torch.isfinite(y).all())


def test_carried_state():
    """The one carried-state helper, through CatchmentBaseflow.run at T = 9, B = 3: chunked equals whole, `state` replaces the
    carried state first, carry=False keeps nothing, and the keys do not see each other."""
    r, _, _, par, state, dt_h = case_data(np.random.default_rng(7), 9, 3)
    par[1] = np.abs(par[1])  # (case_data's negative expon is for the raw entry points: the store validates)
    r, state = torch.from_numpy(r), torch.from_numpy(state)
    store = SimCatchmentBaseflow(par[0], par[1], par[2], dt_h)
    bits = lambda a, b: same_bits(a.numpy(), b.numpy())

    whole, s_whole = store.run(r, carry=False, storage=True)
    assert store.state_of() is None  # carry=False keeps nothing
    first = store.run(r[:4])
    assert bits(store.state_of(), s_whole[3])
    second = store.run(r[4:])
    assert bits(torch.cat([first, second]), whole) and bits(store.state_of(), s_whole[8])

    # another key starts from zeros and leaves the first alone
    other = store.run(r[:4], key="other")
    assert bits(other, first) and bits(store.state_of(), s_whole[8]) and bits(store.state_of("other"), s_whole[3])

    # `state` replaces the carried state first, and what the call leaves is carried on
    from_state, s_from = store.run(r, carry=False, state=state, storage=True)
    assert not bits(from_state, whole) and bits(store.state_of(), s_whole[8])
    assert bits(store.run(r[:5], state=state), from_state[:5]) and bits(store.state_of(), s_from[4])
    assert bits(store.run(r[5:]), from_state[5:]) and bits(store.state_of("other"), s_whole[3])

    store.reset()
    assert store.state_of() is None and store.state_of("other") is None
