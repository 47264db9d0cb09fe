"""CPU, no engine: the shared checks of tests/_golden.py have teeth.  Each one is fed the REFERENCE's own recorded data in the
role of "engine output" (error 0: inside every bar and cap), then the same data with one element above the check's floor moved
by 0.3 of its bar (must still pass) and by 3 bars (must raise), and the exact-match and cap cases one flip at a time."""
import numpy as np
import pytest

import _golden as G

NACC = 10


def bites(check, arr, idx, unit, match=None):
    """check() passes on arr as it stands and with arr[idx] moved by 0.3 unit, and raises with it moved by 3 units."""
    keep = arr[idx]
    check()
    arr[idx] = keep + 0.3 * unit
    check()
    arr[idx] = keep + 3.0 * unit
    with pytest.raises(AssertionError, match=match):
        check()
    arr[idx] = keep


def flipped(check, arr, idx, value, match=None):
    """check() passes on arr as it stands and raises with arr[idx] = value."""
    keep = arr[idx]
    check()
    arr[idx] = value
    with pytest.raises(AssertionError, match=match):
        check()
    arr[idx] = keep


def as_run(g, ncol=3):
    """The fixture in the shape of _golden.run_trajectory()'s result: ncol replicated columns."""
    crash, T = G.steps_before_crash(g)
    acc = np.repeat(g["acc"][:T, None, :], ncol, 1)
    totals = np.zeros((NACC, ncol))
    totals[:8] = g["acc"][:T, :8].sum(0)[:, None]
    rep = lambda x: np.repeat(np.asarray(x)[:, None], ncol, 1)
    fr = dict(zip(("depth", "theta", "psi", "k", "dzdt"), (rep(g["fronts"][T - 1, :, j]) for j in range(5))))
    fr.update(layer=rep(g["front_layer"][T - 1]), to_bottom=rep(g["front_bottom"][T - 1]), n_fronts=np.full(ncol, g["nfronts"][T - 1]))
    return dict(T=T, crash=crash, init_volume=float(g["init_volume"]), acc=acc, call_sums=totals.copy(), totals=totals,
                status=np.zeros(ncol, dtype=np.int32), fronts=fr)


def as_recording(g, T, ncol=2):
    """The fixture in the shape of _golden.run_row_by_row()'s result (32 front slots, like the engine)."""
    F = min(g["fronts"].shape[1], 32)
    lay, bot = g["front_layer"][:T, :F].astype(np.int16), g["front_bottom"][:T, :F].astype(np.int16)
    last = np.repeat(g["fronts"][T - 1, :F, None, :], ncol, 1)
    return dict(depth=g["fronts"][:T, :F, 0].copy(), theta=g["fronts"][:T, :F, 1].copy(),
                flags=np.where(lay >= 0, lay | (bot << 7), 0).astype(np.uint8), n_fronts=g["nfronts"][:T].astype(np.int32),
                status=np.zeros(ncol, dtype=np.int32), final_depth=last[..., 0].copy(), final_theta=last[..., 1].copy())


@pytest.mark.parametrize("name", ["synth1_phil", "manyfronts_pulse_84"])
def test_native_trajectory_checks(name):
    g = G.load(name)
    run = as_run(g)
    T, acc, fr = run["T"], run["acc"], run["fronts"]
    check = lambda: G.check_native_trajectory(g, run)
    t, j = np.unravel_index(np.argmax(np.abs(g["acc"][:T])), (T, NACC))  # (well above the 1e-6 floor)
    ref = g["acc"][t, j]
    bites(lambda: G.check_accumulators(g, acc[:, 0], T), acc, (t, 0, j), G.NATIVE * ref, "per-step accumulators")
    bites(lambda: G.check_accumulators(g, acc[:, 0], T, G.LITERAL), acc, (t, 0, j), G.LITERAL * ref, "per-step accumulators")
    flipped(check, acc, (t, 1, j), np.nextafter(ref, np.inf), "replicated")  # one bit in a column other than 0
    flipped(check, run["status"], 2, 8, "status")
    run["init_volume"] += 0.3 * G.INIT_VOLUME
    check()
    run["init_volume"] += 2.7 * G.INIT_VOLUME
    with pytest.raises(AssertionError, match="initial volume"):
        check()
    run["init_volume"] = float(g["init_volume"])
    nf = int(g["nfronts"][T - 1])
    for jq, (key, floor, bar) in enumerate((("depth", G.REL_FLOOR, G.NATIVE), ("theta", G.REL_FLOOR, G.NATIVE), ("psi", G.PSI_FLOOR, G.DERIVED),
                                            ("k", G.K_FLOOR, G.DERIVED), ("dzdt", G.DZDT_FLOOR, G.DERIVED))):
        i = int(np.argmax(np.abs(g["fronts"][T - 1, :nf, jq])))
        v = abs(g["fronts"][T - 1, i, jq])
        if v > floor:  # (the pulse fixture ends with every front at rest: dz/dt = 0)
            bites(check, fr[key], (i, 0), bar * v, "last front table, " + key)
    fr["psi"][0, 0] *= 1.5  # the mixed mode's table check does not look at psi, K, dz/dt
    G.check_last_front_table(g, fr, T, derived=False)
    with pytest.raises(AssertionError, match="psi"):
        check()
    fr["psi"][0, 0] = g["fronts"][T - 1, 0, 2]
    flipped(check, fr["layer"], (nf - 1, 0), fr["layer"][nf - 1, 0] ^ 1, "layer")
    flipped(check, fr["to_bottom"], (0, 0), fr["to_bottom"][0, 0] ^ 1, "to_bottom")
    flipped(check, fr["n_fronts"], 1, nf + 1, "n_fronts")
    r = int(np.argmax(run["totals"][:8, 0]))
    bites(check, run["totals"], (r, 0), G.NATIVE * run["totals"][r, 0], "run totals")
    bites(check, run["call_sums"], (r, 0), G.NATIVE * run["call_sums"][r, 0], "call_sums")
    run["call_sums"] = None  # optional
    check()


def test_mixed_mode_checks():
    g = G.load("synth1_phil")
    run = as_run(g, 1)  # (one column: a moved element is not also a column that differs from its replicas)
    T, acc, ref = run["T"], run["acc"], g["acc"]
    check = lambda: G.check_mixed_trajectory(g, run)
    # per-step bar: the ending volume (tens of cm: its own scale, and no part of the totals)
    bites(check, acc, (50, 0, 9), G.MIXED_FLUX * ref[50, 9], "per-step outputs")
    # backstop: a value well below 1/150 of the water moving in its step, where the per-step bar is the looser one
    scale = np.maximum(np.maximum(ref[:, 0:1] + ref[:, 8:9], np.abs(ref)), 1e-3)
    small = np.argwhere((np.abs(ref) > G.REL_FLOOR) & (3 * G.MIXED_STEP_BACKSTOP * np.abs(ref) < 0.3 * G.MIXED_FLUX * scale))
    t, j = small[0]
    bites(check, acc, (t, 0, j), G.MIXED_STEP_BACKSTOP * ref[t, j], "backstop")
    # totals: every step's rain moved by the same fraction (one step alone would meet the per-step bar first)
    rain = acc[:, 0, 0].copy()
    for factor, ok in ((0.3, True), (3.0, False)):
        acc[:, 0, 0] = rain * (1 + factor * G.MIXED_TOTAL)
        if ok:
            check()
        else:
            with pytest.raises(AssertionError, match="run totals"):
                check()
    acc[:, 0, 0] = rain
    fr, nf = run["fronts"], int(g["nfronts"][T - 1])
    bites(check, fr["depth"], (1, 0), G.NATIVE * fr["depth"][1, 0], "depth")
    bites(check, fr["theta"], (1, 0), G.NATIVE * fr["theta"][1, 0], "theta")
    flipped(check, fr["layer"], (nf - 1, 0), fr["layer"][nf - 1, 0] ^ 1, "layer")
    flipped(check, fr["to_bottom"], (0, 0), fr["to_bottom"][0, 0] ^ 1, "to_bottom")
    flipped(check, fr["n_fronts"], 0, nf - 1, "n_fronts")
    flipped(check, run["status"], 0, 1, "status")
    fr["psi"][:] = 0.0  # (not looked at)
    check()
    three = as_run(g, 3)
    flipped(lambda: G.check_mixed_trajectory(g, three), three["acc"], (3, 2, 0), 1.0, "replicated")


@pytest.mark.parametrize("name,bars", [("synth1_phil", G.STEPWISE_NATIVE), ("manyfronts_pulse_84", G.STEPWISE_LITERAL),
                                       ("manyfronts_pulse_84", G.STEPWISE_MIXED_SIM), ("synth1_phil", G.STEPWISE_MIXED_GPU)])
def test_front_table_at_every_step_check(name, bars):
    bar, usual = bars
    g = G.load(name)
    T = G.steps_before_crash(g)[1]
    rec = as_recording(g, T)
    check = lambda: G.check_front_table_at_every_step(g, rec, T, bar, usual)
    Z, TH = rec["depth"], rec["theta"]
    t = T // 2
    bites(check, Z, (t, 0), bar * Z[t, 0], "depth / theta")
    bites(check, TH, (t, 1), bar * TH[t, 1], "depth / theta")
    Z[t, int(rec["n_fronts"][t]):] += 1.0  # rows at and beyond n_fronts are not meaningful
    check()
    nf = int(rec["n_fronts"][t])
    flipped(check, rec["flags"], (t, nf - 1), rec["flags"][t, nf - 1] ^ 1, "layer tags")
    flipped(check, rec["flags"], (t, 0), rec["flags"][t, 0] ^ 0x80, "to_bottom")
    flipped(check, rec["n_fronts"], 3, rec["n_fronts"][3] + 1, "n_fronts")
    flipped(check, rec["status"], 0, 2, "status")
    flipped(check, rec["final_theta"], (0, 1), 0.0, "replicated")
    # the cap: max(1, T // 50) steps between `usual` and `bar` pass, one more does not
    cap = max(1, T // 50)
    mid = 0.5 * (usual + bar) if bar > usual else None
    if mid is not None:
        steps = np.arange(cap + 1) * 2 + 5
        keep = TH[steps, 0].copy()
        TH[steps[:cap], 0] = keep[:cap] * (1 + mid)
        check()
        TH[steps, 0] = keep * (1 + mid)
        with pytest.raises(AssertionError, match="%d of %d steps above the usual" % (cap + 1, T)):
            check()
        TH[steps, 0] = keep


def test_crash_step_check():
    g = G.load("crash_dry_over_wet_300")  # the reference raised ValueError: NAN / NEGBASE bits, no BOTTOM bit
    assert G.steps_before_crash(g) == (277, 277) and G.steps_before_crash(g, 100) == (277, 100)
    status = np.full(5, 2, dtype=np.int32)
    check = lambda: G.check_crash_step(g, status)
    flipped(check, status, 3, 0, "column 3 of 5 is not flagged")
    flipped(check, status, 1, 32)  # flagged, but with the fault kind of an AttributeError
    with pytest.raises(AssertionError, match="did not raise"):
        G.check_crash_step(g, status, raised=False)


def test_oracle_agreement_check():
    g = G.load("synth1_phil")
    T, N = g["acc"].shape[0], 4
    o = dict(ro=np.repeat(g["acc"][:, 4:5], N, 1), acc=np.repeat(g["acc"].sum(0)[:, None], N, 1), st=np.array([0, 0, 2, 0]))
    status, runoff, totals = o["st"].copy(), o["ro"].copy(), o["acc"].copy()
    runoff[:, 2], totals[:, 2] = 7.0, 7.0  # a column the oracle faults on is compared only on request
    check = lambda **kw: G.check_oracle_agreement(o, status, runoff, totals, flips=(), **kw)
    with pytest.raises(AssertionError, match="runoff"):
        check(cols=slice(None))
    t = int(np.argmax(o["ro"][:, 0]))
    scale = max(1.0, o["ro"].max())
    bites(check, runoff, (t, 1), G.NATIVE * scale, "runoff")
    bites(lambda: check(mixed=True), runoff, (t, 1), G.MIXED_FLUX * scale, "runoff")
    bites(lambda: check(scale=10.0), runoff, (t, 1), G.NATIVE * 10.0, "runoff")
    bites(check, totals, (4, 3), G.NATIVE * totals[4, 3], "run totals")  # (total runoff 0.70 cm: above the 1e-3 cm floor)
    bites(lambda: check(mixed=True), totals, (4, 3), G.MIXED_TOTAL * totals[0, 3], "run totals")  # against the total rain
    bites(lambda: check(bar=1e-4), totals, (4, 3), 1e-4 * totals[4, 3], "run totals")
    flipped(check, status, 0, 1, "fault flags differ")
    flipped(check, status, 2, 0, "fault flags differ")
    status[0] = 1
    G.check_oracle_agreement(o, status, runoff, totals, flips={0})  # a named borderline column
    G.check_oracle_agreement(o, status, runoff, totals, flips=None)  # flags not compared
    with pytest.raises(AssertionError, match="fault flags differ"):
        G.check_oracle_agreement(o, status, runoff, totals, flips={1})


def test_gradient_check():
    g = G.load("grad_synth0_12h")
    ref = G.reference_gradients(g)
    assert not any(np.isnan(v).any() for v in ref.values())
    assert np.array_equal(ref["ksat"], np.nan_to_num(g["d_ksat"]) * float(g["frozen_factor"]))
    grads = {k: v.copy() for k, v in ref.items()}
    loss = np.array([float(g["loss"])])
    check = lambda: G.check_gradients(g, loss[0], grads)
    bites(check, loss, 0, G.GRADIENT_LOSS * loss[0], "loss")
    for kind in grads:
        i = int(np.argmin(np.abs(ref[kind])))  # the bar is relative to the LARGEST gradient of the kind, for every layer
        bites(check, grads[kind], i, G.GRADIENT * np.abs(ref[kind]).max(), kind)


def test_bit_identical_check():
    g = G.load("synth1_phil")
    a = dict(runoff=g["acc"][:, 4:5].copy(), depth=g["fronts"][-1, :, 0:1].copy(), n_fronts=g["nfronts"][-1:].copy())
    b = {k: v.copy() for k, v in a.items()}
    check = lambda: G.check_bit_identical(a, b)
    t = int(np.argmax(a["runoff"][:, 0]))
    flipped(check, b["runoff"], (t, 0), np.nextafter(a["runoff"][t, 0], 0.0), "runoff")
    flipped(check, b["n_fronts"], 0, 0, "n_fronts")
    b["depth"][2, 0] += 1.0
    G.check_bit_identical(a, b, fields=("runoff", "n_fronts"))  # only the fields asked for
    with pytest.raises(AssertionError, match="x: depth"):
        G.check_bit_identical(a, b, label="x: ")
