"""CPU: the plain fp32 kernels' top-layer step changes no bit.

While every wetting front of a column is still inside the top soil layer, its front table has one shape: m >= 1 in-layer fronts of
layer 0, then the boundary fronts of the layers in order.  A wave whose columns all hold such a table takes the sweep and
calc_dzdt with that shape resolved at compile time (lgar_py_amd/csrc/lgar_column.hpp: is_top_table, sweep_top, calc_dzdt's
`fast`); -DLGAR_NO_TOP_LAYER_STEP compiles the kernels without it.  Here the device code is compiled for the host
(tests/devsim) with and without the switch, and both runs must agree BIT FOR BIT: every per-step accumulator, the final front
table and state, and the status word.  The simulator runs one lane at a time, so each column decides for itself: waves that mix
columns on and off the predicate are the GPU suite's (tests/test_gpu_top_layer_step.py).  Builds with
-DLGAR_COUNT_TOP_LAYER_STEP=1 / =0 count the sub-steps that took the step / the generic code: every family of fixtures takes
both."""
import os

import numpy as np
import pytest

from _golden import engine_keywords
from conftest import GOLDEN

OFF = ("-DLGAR_NO_TOP_LAYER_STEP",)
COUNT_TAKEN, COUNT_GENERIC = ("-DLGAR_COUNT_TOP_LAYER_STEP=1",), ("-DLGAR_COUNT_TOP_LAYER_STEP=0",)
NAMES = ["synth1_phil", "bench_col15731", "crash_insert_water_bench_col2", "six_layer_synth1", "two_layer_synth1",
         "manyfronts_pulse_84"]
# one fixture per family (soil-layer count; the pulsed rain that grows tens of fronts) for the counters
FAMILIES = {"three_layers": "bench_col15731", "six_layers": "six_layer_synth1", "two_layers": "two_layer_synth1",
            "many_fronts": "manyfronts_pulse_84"}
MODES = {"fast": 1, "fast_capacity_chain": 2}
STATE = ["depth", "theta", "psi", "k", "dzdt", "flags", "n_fronts", "scalars", "totals", "status"]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _open(name, flags, search_mode):
    """(engine of one fp32 column of the fixture, its forcing up to and INCLUDING the step at which the reference raised)"""
    from devsim import variants
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    crash = int(g["crash_step"])
    T = g["forcing"].shape[0] if crash < 0 else crash + 1
    eng = variants.VariantEngine(flags, g["alpha"], g["n"], g["ksat"], g["theta_e"], g["theta_r"], g["thickness"], n_columns=1,
                                 dtype=np.float32, search_mode=search_mode, **engine_keywords(g))
    return eng, g["forcing"][:T]


def _state(eng):
    return {nm: _bits(getattr(eng, nm)).copy() for nm in STATE}


def _run(name, flags, search_mode):
    import devsim
    eng, f = _open(name, flags, search_mode)
    eng.geff_wave_calls()  # (zero the counter)
    out = eng.forward(f[:, 0:1], f[:, 1:2], series=devsim.ACC_NAMES, call_sums=True)
    res = {"series:" + nm: _bits(out[nm]) for nm in devsim.ACC_NAMES}
    res["call_sums"] = _bits(out["call_sums"])
    res.update(_state(eng))
    return res, int(eng.geff_wave_calls())


_cache = {}


def _cached_run(name, flags, mode):
    """(computed once, shared by the tests that need it, never changed)"""
    key = (name, flags, mode)
    if key not in _cache:
        _cache[key] = _run(name, flags, MODES[mode])
    return _cache[key]


@pytest.fixture(scope="module")
def variant_libraries():
    from devsim import variants
    variants.prebuild((2, 3, 6), [OFF, COUNT_TAKEN, COUNT_GENERIC])


def _assert_same(got, want):
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key].shape == want[key].shape and got[key].dtype == want[key].dtype, key
        assert np.array_equal(got[key], want[key]), (key, int((got[key] != want[key]).sum()))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", NAMES)
def test_fp32_fast_mode_is_bit_identical_without_the_top_layer_step(variant_libraries, name, mode):
    want, _ = _cached_run(name, OFF, mode)
    got, _ = _cached_run(name, (), mode)
    _assert_same(got, want)
    # (a fixture that never infiltrates moves no front: the comparison would say nothing)
    assert float(np.nansum(want["series:infiltration"].view(np.float32))) > 0.0


@pytest.mark.parametrize("family", list(FAMILIES))
def test_both_the_top_layer_step_and_the_generic_step_are_taken(variant_libraries, family):
    name = FAMILIES[family]
    want, _ = _cached_run(name, (), "fast_capacity_chain")
    got_t, taken = _run(name, COUNT_TAKEN, MODES["fast_capacity_chain"])
    got_g, generic = _run(name, COUNT_GENERIC, MODES["fast_capacity_chain"])
    print("%s (%s): %d sub-steps took the top-layer step, %d the generic one" % (family, name, taken, generic))
    _assert_same(got_t, want)  # (the counting builds compute what the plain build computes)
    _assert_same(got_g, want)
    assert taken > 0 and generic > 0, (taken, generic)


@pytest.mark.parametrize("flags", [(), OFF], ids=["with_the_step", "without_the_step"])
def test_one_row_per_call_equals_the_one_call_run(variant_libraries, flags):
    """The predicate is evaluated when a call loads the state: a run cut into calls of one forcing row each -- every table the
    fixture goes through is loaded once -- must end where the one-call run ends, with the same series on the way."""
    import devsim
    name, mode = "bench_col15731", "fast_capacity_chain"
    want, _ = _cached_run(name, OFF, mode)
    eng, f = _open(name, flags, MODES[mode])
    rows = {nm: [] for nm in devsim.ACC_NAMES}
    for t in range(f.shape[0]):
        out = eng.forward(f[t:t + 1, 0:1], f[t:t + 1, 1:2], series=devsim.ACC_NAMES)
        for nm in devsim.ACC_NAMES:
            rows[nm].append(_bits(out[nm]).copy())
    got = {"series:" + nm: np.concatenate(rows[nm], axis=0) for nm in devsim.ACC_NAMES}
    got.update(_state(eng))
    for key in got:
        assert got[key].shape == want[key].shape, key
        assert np.array_equal(got[key], want[key]), (key, int((got[key] != want[key]).sum()))
