"""The call-record protocol of the stand-alone host programs (tests/_hostprog.hpp, written by tests/_hostbuild.py), through the
baseflow unit's program: the exit statuses, and what an output-only array holds before the call writes it."""
import os
import struct
import subprocess

import numpy as np

import _hostbuild
import baseflow_host as BH


def _status(blob, tmp_path):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as fh:
        fh.write(blob)
    p = subprocess.run([BH.UNIT.program(), fin, fout], capture_output=True, timeout=60)
    return p.returncode, open(fout, "rb").read() if os.path.exists(fout) else None


def _exp_call(n):
    return (2, (n,), (), (np.linspace(0.0, 1.0, n), _hostbuild.Out(np.float64, n)))


def test_exit_statuses(tmp_path):
    blob, _ = _hostbuild.call_records([_exp_call(3)], True)
    assert _status(blob, tmp_path)[0] == 0
    assert _status(blob[:-16 - 8], tmp_path)[0] == 2  # cut after two of the input array's three elements: a short read
    assert _status(blob[:10], tmp_path)[0] == 2  # the call's own header is cut
    unknown, _ = _hostbuild.call_records([(99,) + _exp_call(3)[1:]], True)
    assert _status(unknown, tmp_path)[0] == 4  # no such operation
    wrong_arity, _ = _hostbuild.call_records([(2, (3, 3), (), _exp_call(3)[3])], True)
    assert _status(wrong_arity, tmp_path)[0] == 4  # the operation with a scalar too many
    bad_kind = struct.pack("=i4ii", 1, 2, 1, 0, 2, 3) + struct.pack("=2iq", 8, 7, 3)
    assert _status(bad_kind, tmp_path)[0] == 2  # an array kind the protocol does not have
    assert subprocess.run([BH.UNIT.program()], capture_output=True, timeout=60).returncode == 1  # usage


def test_output_only_array_starts_as_all_ones_bytes():
    """gw_exp writes out[0 .. n): told n = 0 it leaves a three-element output as the program made it, all-ones bytes; an
    output of no elements is a null pointer and comes back empty."""
    untouched, whole, empty = (_hostbuild.Out(np.float64, 3), _hostbuild.Out(np.float64, 3), _hostbuild.Out(np.float64, 0))
    z = np.array([0.0, 0.5, 1.0])
    BH.UNIT.run_calls([(2, (0,), (), (z, untouched)), (2, (3,), (), (z, whole)), (2, (0,), (), (np.zeros(0), empty))])
    assert untouched.value.tobytes() == b"\xff" * 24
    assert _hostbuild.same_bits(whole.value, BH.gw_exp_ref(z))
    assert empty.value.shape == (0,)
    # the same three through the package's own cases
    (a,), (b,) = BH.run([("exp", np.zeros(0)), ("exp", z)])
    assert a.shape == (0,) and _hostbuild.same_bits(b, whole.value)
