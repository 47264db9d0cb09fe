"""CPU: the plain fp32 kernels' reuse of Geff values changes no bit.

The fp32 fast mode hands a Geff that calc_dzdt computed to insert_water's memo, runs the rare Geff call sites through one
out-of-line body, and takes the trapezoid's end nodes and heads in lockstep.  Each piece has a switch that turns it off
(lgar_py_amd/csrc/lgar_measure.hpp).  Here the device code is compiled for the host (tests/devsim) with each switch, and with
all of them, and every run must give what the plain build gives BIT FOR BIT: every per-step accumulator, the final front
table and state, and the status word."""
import os

import numpy as np
import pytest

from _golden import engine_keywords
from conftest import GOLDEN

SWITCHES = ["-DLGAR_NO_DZDT_MEMO", "-DLGAR_NO_F32_RARE_GEFF", "-DLGAR_NO_GEFF_ENDS"]
VARIANTS = {s[len("-DLGAR_"):].lower(): (s,) for s in SWITCHES}
VARIANTS["all_off"] = tuple(SWITCHES)
NAMES = ["synth1_phil", "bench_col15731", "crash_insert_water_bench_col2", "six_layer_synth1"]
MODES = {"fast": 1, "fast_capacity_chain": 2}
STATE = ["depth", "theta", "psi", "k", "dzdt", "flags", "n_fronts", "scalars", "totals", "status"]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _run(name, flags, search_mode):
    """One fp32 column of the fixture, run up to and INCLUDING the step at which the reference raised (if it did)."""
    import devsim
    from devsim import variants
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    crash = int(g["crash_step"])
    T = g["forcing"].shape[0] if crash < 0 else crash + 1
    f = g["forcing"][:T]
    eng = variants.VariantEngine(flags, g["alpha"], g["n"], g["ksat"], g["theta_e"], g["theta_r"], g["thickness"], n_columns=1,
                                 dtype=np.float32, search_mode=search_mode, **engine_keywords(g))
    out = eng.forward(f[:, 0:1], f[:, 1:2], series=devsim.ACC_NAMES, call_sums=True)
    res = {"series:" + nm: _bits(out[nm]) for nm in devsim.ACC_NAMES}
    res["call_sums"] = _bits(out["call_sums"])
    for nm in STATE:
        res[nm] = _bits(getattr(eng, nm)).copy()
    return res


_plain = {}


def _plain_run(name, mode):
    """(the plain build's run: computed once, shared by the variants' tests, never changed)"""
    if (name, mode) not in _plain:
        _plain[(name, mode)] = _run(name, (), MODES[mode])
    return _plain[(name, mode)]


@pytest.fixture(scope="module")
def variant_libraries():
    from devsim import variants
    variants.prebuild((3, 6), list(VARIANTS.values()))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_fp32_fast_mode_is_bit_identical_with_a_reuse_switched_off(variant_libraries, variant, name, mode):
    want = _plain_run(name, mode)
    got = _run(name, VARIANTS[variant], MODES[mode])
    assert sorted(got) == sorted(want)
    for key in want:
        assert got[key].shape == want[key].shape, key
        assert np.array_equal(got[key], want[key]), (key, int((got[key] != want[key]).sum()))


@pytest.mark.parametrize("name", NAMES)
def test_fixture_runs_what_the_switches_guard(name):
    """The comparison above says nothing about a fixture that never infiltrates (no insert_water, no moving front, no Geff):
    each one must produce infiltration."""
    want = _plain_run(name, "fast_capacity_chain")
    infil = want["series:infiltration"].view(np.float32)
    assert float(np.nansum(infil)) > 0.0
