"""GPU (-m gpu): lgar_catchment_snow_tangent on the hardware against the numpy statement of its recurrence bit for bit
(tests/snow_tangent_host has the statement; the host suite holds it to the adjoint identity), chunked calls, the write into a
wider [T, B, ld] block, CatchmentSnow.tangent and catchment_snow_directions.  Shapes of a few hundred cells: milliseconds each."""
import numpy as np
import pytest

import snow_host as SH
import snow_tangent_host as ST
from _hostbuild import same_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


_uploaded = {}  # id(numpy array) -> (the array, its copy on the device): the product below calls with the same inputs many times


def _up(a):
    if a is None:
        return None
    if id(a) not in _uploaded:
        if len(_uploaded) > 64:
            _uploaded.clear()
        _uploaded[id(a)] = (a, torch.tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda"))
    return _uploaded[id(a)][1]


def _gpu_call(p, ta, par, dt, state, D, dp=None, dta=None, dpar=None, dstate=None, ld=None, k0=0, want_pack=True, want_state=True, fill=7.5):
    """snow_tangent_host.call on the library: (0, dw block, dice, dliq, dstate_out) as numpy arrays"""
    from lgar_py_amd import _capi
    T, B = np.asarray(p).shape
    ld = k0 + D if ld is None else ld
    ins = [_up(a) for a in (p, ta, par, state, dp, dta, dpar, dstate)]
    dw = torch.full((T, B, ld), fill, dtype=torch.float64, device="cuda")
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device="cuda")
    dice, dliq = (nan(D, T, B), nan(D, T, B)) if want_pack else (None, None)
    dso = nan(D, 2, B) if want_state else None
    q = lambda x: None if x is None or x.numel() == 0 else x.data_ptr()
    _capi.launch(_capi.load(), "catchment_snow_tangent", torch.device("cuda"), q(ins[0]), q(ins[1]), T, B, q(ins[2]), float(dt), q(ins[3]), D,
                 q(ins[4]), q(ins[5]), q(ins[6]), q(ins[7]), q(dw), ld, k0, q(dice), q(dliq), q(dso))
    return (0,) + tuple(None if x is None else x.cpu().numpy() for x in (dw, dice, dliq, dso))


@pytest.mark.parametrize("B", ST.SHAPE_B)
def test_kernel_equals_the_numpy_statement_bit_for_bit(B):
    """The full product of snow_tangent_host.statement_product on the hardware: for this B, T in {0, 1, 9, 17} x D in {1, 3, 7} x
    every combination of NULL inputs and wanted outputs x two (ld, k0), all of it with and without the value state (3072
    launches of microseconds each); the regimes and the planted ties of the data are counted as the host suite counts them."""
    calls, reg, tie = ST.statement_product(_gpu_call, B)
    assert calls == 12 * 64 * 2 * 2
    if B >= 63:
        assert all(v > 0 for v in reg.values()) and all(v > 0 for v in tie.values()), (reg, tie)


@pytest.mark.parametrize("which", ["dp", "dta", "dpar", "dstate"])
def test_a_nan_stays_in_its_cell_and_its_direction(which):
    ST.nan_confinement(_gpu_call, which)


def test_chunked_calls_carrying_dstate_equal_one_call_in_bits():
    rng = np.random.default_rng(5)
    B, T, D = 65, 17, 3
    p, ta, _, _, _, par, state, dt = SH.case_data(rng, T, B)
    mixed = lambda *shape: (rng.random(shape) - 0.4) * 10.0 ** rng.integers(-2, 2, shape)
    dp, dta, dpar, dst = mixed(D, T, B), mixed(D, T, B), mixed(D, 7, B), mixed(D, 2, B)
    _, dw, dice, dliq, dso = _gpu_call(p, ta, par, dt, state, D, dp, dta, dpar, dst)
    s, ds, parts = state, dst, []
    for lo, hi in ((0, 1), (1, 8), (8, 9), (9, 17), (17, 17)):
        _, w2, i2, l2, ds = _gpu_call(p[lo:hi], ta[lo:hi], par, dt, s, D, dp[:, lo:hi], dta[:, lo:hi], dpar, ds)
        parts.append((w2, i2, l2))
        s = SH.snow_ref(p[lo:hi], ta[lo:hi], par, dt, s)[3]
    assert same_bits(np.concatenate([x[0] for x in parts]), dw) and same_bits(ds, dso)
    assert same_bits(np.concatenate([x[1] for x in parts], axis=1), dice) and same_bits(np.concatenate([x[2] for x in parts], axis=1), dliq)


def test_catchment_snow_tangent_and_directions():
    import lgar_py_amd as lg
    rng = np.random.default_rng(11)
    B, T = 5, 17
    p, ta, gw, _, _, par, state, dt = SH.case_data(rng, T, B)
    par[1] = np.maximum(par[1], par[0] + 0.5)
    t = lambda x: torch.tensor(x, device="cuda")
    pars = [t(par[j]) for j in range(7)]
    for j in (2, 3, 4):
        pars[j].requires_grad_(True)
    water, fd = lg.catchment_snow_directions(t(p), t(ta), *pars, dt, state=t(np.abs(state)))
    assert fd.K == 3 and fd.d_pet is None and tuple(fd.d_precip.shape) == (3, T, B)
    dpar = np.zeros((3, 7, B))
    for k, j in enumerate((2, 3, 4)):
        dpar[k, j] = 1.0
    want = ST.snow_tangent_ref(p, ta, par, dt, np.abs(state), 3, dpar=dpar)[0]
    assert same_bits(fd.d_precip.permute(1, 2, 0).cpu().numpy(), want)
    assert same_bits(water.cpu().numpy(), SH.snow_ref(p, ta, par, dt, np.abs(state))[0])
    out = lg.catchment_snow(t(p), t(ta), *pars, dt, state=t(np.abs(state)))
    (out * t(gw)).sum().backward()
    for k, j in enumerate((2, 3, 4)):
        got = (fd.d_precip[k] * t(gw)).sum(0)
        assert torch.allclose(got, pars[j].grad, rtol=1e-9, atol=1e-12 * float(pars[j].grad.abs().max())), j
    # the raw call writes into a wider block and refuses one that is too narrow
    snow = lg.CatchmentSnow(*[par[j] for j in range(7)], dt)
    block = torch.full((T, B, 6), 7.5, dtype=torch.float64, device="cuda")
    got = snow.tangent(t(p), t(ta), 3, dpar=t(dpar), state=t(np.abs(state)), out=block, k0=2)[0]
    assert got is block and same_bits(block[:, :, 2:5].cpu().numpy(), want) and bool((block[:, :, [0, 1, 5]] == 7.5).all())
    with pytest.raises(lg.LgarError, match="ld >= k0 \\+ D"):
        snow.tangent(t(p), t(ta), 3, out=block, k0=4)
