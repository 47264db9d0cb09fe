"""CPU: the soil-moisture output (lgar_soil_moisture, include/lgar.h) on the REFERENCE's own front tables.

The per-column function the GPU kernel runs (lgar_py_amd/csrc/lgar_moisture.hpp) is compiled for the host into a small
stand-alone program (tests/post_host) and run over the front table the reference recorded at every step of every
trajectory fixture.  Its results must equal the numpy statement of the definition (post_host.moisture.profile_ref) bit for bit, and
the definition itself must close the reference's mass balance: the storage bins that cover the column sum to the recorded
ending_volume (Layer.mass_balance, layers/Layer.py:795-824)."""
import numpy as np
import pytest

from conftest import golden_names

import post_host as PH
from post_host import moisture as MH

TRAJ = [n for n in golden_names() if not n.startswith("grad_")]
NONMONOTONE = {"manyfronts_pulse_84": (2, 4, 6), "bushland_hourly_1500": (1405,)}  # steps with a front above its predecessor


def explicit_edges(Z):
    """[0, 5, 10, 30, 60, 100, Z + 50]; a column shallower than 50 cm drops the inner edges its last one does not exceed (edges
    must increase)."""
    return [e for e in (0.0, 5.0, 10.0, 30.0, 60.0, 100.0) if e < Z + 50.0] + [Z + 50.0]


@pytest.fixture(scope="module")
def results():
    """Every fixture x {explicit edges, layer bins} x {theta, storage} x {fp64, fp32 tables}: ONE run of the host program; the
    numpy reference is computed once per combination and shared by the tests below."""
    cases, keys = [], []
    for name in TRAJ:
        for dtype in (np.float64, np.float32):
            t = MH.tables(name, dtype)
            for edges in (explicit_edges(t["Z"]), None):
                for what in ("theta", "storage"):
                    cases.append(dict(t, edges=edges, what=what))
                    keys.append((name, dtype, edges is None, what))
    got = PH.run(map(MH.case, cases))
    ref = [MH.profile_ref(c["depth"], c["theta"], c["layer"], c["n_fronts"], c["thickness"], c["edges"], c["what"]) for c in cases]
    return {k: (c, a, r) for k, c, a, r in zip(keys, cases, got, ref)}


@pytest.mark.parametrize("name", TRAJ)
def test_reference_tables_bit_for_bit(results, name):
    for layer_bins in (False, True):
        for what in ("theta", "storage"):
            _, got, ref = results[(name, np.float64, layer_bins, what)]
            assert got.dtype == np.float64 and MH.same_bits(got, ref), (layer_bins, what)
            # tables cast to fp32: fp64 arithmetic on the exactly converted inputs, rounded once
            _, got32, ref32 = results[(name, np.float32, layer_bins, what)]
            assert got32.dtype == np.float32 and MH.same_bits(got32, ref32.astype(np.float32)), (layer_bins, what)


def test_mass_closure_on_the_reference_alone(results):
    """Sum of the storage bins == the reference's recorded ending_volume within 1e-12 relative (measured worst 3.9e-16; the
    margin covers 31-front tables), at every step of every fixture -- the steps where the reference leaves a column's depths
    transiently non-monotone included: that is what the signed widths are for.  The explicit bins reach 50 cm below the column
    and close at every step; the layer bins end at the column's bottom, so they close wherever no front has been carried past
    it (the reference does that for a few steps before it crashes on a front at the domain bottom: those steps are counted)."""
    worst, negative_steps, past_bottom = 0.0, 0, 0
    for name in TRAJ:
        for layer_bins in (False, True):
            c, _, ref = results[(name, np.float64, layer_bins, "storage")]
            d, lay, nf = c["depth"], c["layer"], c["n_fronts"]
            inside = np.ones(len(nf), dtype=bool)
            if layer_bins:
                inside = ~((np.arange(d.shape[0])[:, None] < nf[None, :]) & (d > c["Z"])).any(axis=0)
                past_bottom += int((~inside).sum())
            rel = (np.abs(ref.sum(axis=0) - c["volume"]) / np.abs(c["volume"]))[inside]
            worst = max(worst, float(rel.max()))
            assert rel.max() <= 1e-12, (name, layer_bins, int(rel.argmax()), float(rel.max()))
        live = np.arange(1, d.shape[0])[:, None] < nf[None, :]
        neg = (live & (lay[1:] == lay[:-1]) & (d[1:] < d[:-1])).any(axis=0)
        negative_steps += int(neg.sum())
        for step in NONMONOTONE.get(name, ()):
            assert neg[step], (name, step)
    print("worst relative closure %.3g; %d tables with a negative depth step; %d with a front past the column's bottom"
          % (worst, negative_steps, past_bottom))
    assert negative_steps >= 1 and past_bottom <= 100


def test_bins_below_the_column():
    """A bin wholly below the column: theta NaN, storage 0.  A bin straddling the bottom is divided by its in-column width."""
    t = MH.tables("synth1_phil")
    Z = t["Z"]  # 200 cm
    edges = [0.0, 44.0, Z - 10.0, Z + 10.0, Z + 20.0, Z + 30.0]
    th, st = PH.run(map(MH.case, [dict(t, edges=edges, what="theta"), dict(t, edges=edges, what="storage")]))
    assert np.isnan(th[3:]).all() and (st[3:] == 0.0).all() and np.isfinite(th[:3]).all()
    # the straddling bin holds the bottom layer's last 10 cm: its mean theta is that front's theta, not half of it
    last = t["theta"][t["n_fronts"] - 1, np.arange(len(t["n_fronts"]))]
    assert np.abs(th[2] - last).max() <= 1e-14 and np.abs(st[2] - 10.0 * last).max() <= 1e-13
    assert MH.same_bits(th, MH.profile_ref(t["depth"], t["theta"], t["layer"], t["n_fronts"], t["thickness"], edges, "theta"))
    # layer mode never has a bin below the column
    lay, = PH.run(map(MH.case, [dict(t, edges=None, what="theta")]))
    assert np.isfinite(lay).all()


def test_more_bins_than_the_smallest_kernel_capacity():
    """9, 16, 17 and LGAR_MOIST_BINS bins take the 16- and 32-bin instances of the function."""
    t = MH.tables("six_layer_synth1")
    for nb in (9, 16, 17, 32):
        edges = np.linspace(0.0, t["Z"] + 7.0, nb + 1)
        for what in ("theta", "storage"):
            got, = PH.run(map(MH.case, [dict(t, edges=edges, what=what)]))
            assert MH.same_bits(got, MH.profile_ref(t["depth"], t["theta"], t["layer"], t["n_fronts"], t["thickness"], edges, what))


def test_sanitizer_build_on_fixtures_and_a_corrupt_state():
    """AddressSanitizer + UBSan build of the same program (a stand-alone executable: nothing is loaded into python) over two
    fixtures and a hand-made corrupt state -- n_fronts = 255 and layer tag 127 in an 8-slot table: memory safety comes before
    meaning, the counts are clamped and nothing is read out of bounds.  Any finding aborts the program."""
    cases = []
    for name in ("manyfronts_pulse_84", "six_layer_synth1"):
        t = MH.tables(name)
        cases += [dict(t, edges=explicit_edges(t["Z"]), what="theta"), dict(t, edges=None, what="storage")]
    N, F, L = 5, 8, 3
    rng = np.random.default_rng(0)
    bad = dict(depth=rng.random((F, N)) * 200.0, theta=rng.random((F, N)), flags=np.full((F, N), 127, dtype=np.uint8),
               n_fronts=np.full(N, 255, dtype=np.int32), thickness=np.repeat(np.array([44.0, 131.0, 25.0])[:, None], N, axis=1))
    bad["n_fronts"][1] = -7
    cases += [dict(bad, edges=[0.0, 10.0, 300.0], what="theta"), dict(bad, edges=None, what="storage"),
              dict({k: (v.astype(np.float32) if v.dtype == np.float64 else v) for k, v in bad.items()}, edges=None, what="theta")]
    got = PH.run(map(MH.case, cases), sanitize=True)
    plain = PH.run(map(MH.case, cases))
    for a, b in zip(got, plain):
        assert MH.same_bits(a, b)
    assert (got[-2][:, 1] == 0.0).all()  # n_fronts < 0 clamps to an empty table


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["fp64", "fp32"])
def test_totals_replay_adds_row_after_row_in_the_series_dtype(dtype):
    """lgar_totals_replay's host launcher, plain and under AddressSanitizer + UBSan: running[j] gains the rows of series[j] one
    after the other, in the series' own dtype, from what it held; an absent series leaves its row alone, row 7 is never touched,
    and two chunks through the carried block equal one call over all rows."""
    rng = np.random.default_rng(2)
    N, T = 5, 7
    series = [None if j == 2 else ((rng.random((T, N)) - 0.3) * 10.0 ** rng.integers(-3, 4, (T, N))).astype(dtype) for j in range(7)]
    start = rng.random((8, N)).astype(dtype)
    want = start.copy()
    for j, s in enumerate(series):
        for t in range(T if s is not None else 0):
            want[j] = want[j] + s[t]
    call = lambda rows, running: ([("totals_replay", [PH.dtype_code(dtype), N, rows.stop - rows.start],
                                    [None if s is None else s[rows] for s in series] + [running])], running)
    for sanitize in (False, True):
        whole = PH.Out(dtype, 8, N, start=start)
        got, first = PH.run([call(slice(0, T), whole), call(slice(0, 3), PH.Out(dtype, 8, N, start=start))], sanitize=sanitize)
        second, = PH.run([call(slice(3, T), PH.Out(dtype, 8, N, start=first))], sanitize=sanitize)
        assert MH.same_bits(got, want) and MH.same_bits(second, want) and not MH.same_bits(first, want)
        assert MH.same_bits(got[[2, 7]], start[[2, 7]])
