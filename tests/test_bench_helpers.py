"""CPU: bench.py's bookkeeping (algorithmic bytes of SURVEY §8d, committed-PMC lookups, CPU-baseline leg on a tiny sample)."""
import importlib.util
import os

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_algorithmic_bytes_match_survey():
    b = _bench()
    # SURVEY §8d's formula B_alg = 4 s + (L 6 s + 2 F_MAX (5 s + 1) + 2 16 s) / T with L = 3, F_MAX = 16; the survey
    # rounds B_col to 840 B (fp32) / 1648 B (fp64), the formula itself gives 872 / 1712
    assert abs(b.alg_bytes_per_col_step(4, 144) - (16 + 872 / 144)) < 1e-12
    assert abs(b.alg_bytes_per_col_step(4, 144) - 21.8) < 0.3 and abs(b.alg_bytes_per_col_step(4, 3000) - 16.3) < 0.05
    assert abs(b.alg_bytes_per_col_step(8, 144) - (32 + 1712 / 144)) < 1e-12 and abs(b.alg_bytes_per_col_step(8, 144) - 43.4) < 0.6


def test_committed_pmc_lookup(monkeypatch):
    """roofline.traffic comes from a committed profile only when that profile was taken on exactly this workload AND with this
    library build (content fingerprint); otherwise it is null with the reason."""
    b = _bench()
    alg = b.alg_bytes_per_col_step(4, 144) * 1048576 * 144
    t, why = b.measured_traffic(12345, 144, "f32")
    assert t is None and "no committed profile" in why
    rec = b._matching_profile(1048576, 144, "f32")
    assert rec is not None and rec["source"].startswith("profiles/r0")
    # as if the profile had been taken with this very build: the figure is reported and stays within 15 % of the 3.33 GB
    # algorithmic figure (no wasted re-reads)
    monkeypatch.setattr(b, "library_fingerprint", lambda: rec.get("library_fingerprint"))
    t, why = b.measured_traffic(1048576, 144, "f32")
    assert t is not None and 1.5e9 < t < 1.15 * alg and rec["source"] in why
    v = b.measured_valu(1048576, 144, "f32")
    assert v is not None and 0.5 < v["busy_frac"] <= 1.0 and v["source"] == rec["source"]
    # ... and with any other build it is not
    monkeypatch.setattr(b, "library_fingerprint", lambda: "0" * 64)
    t, why = b.measured_traffic(1048576, 144, "f32")
    assert t is None and "another build" in why and b.measured_valu(1048576, 144, "f32") is None


def test_options_and_dump_sample():
    """A plain run is lean (--full off by default); --steps below 1 is refused; the dumped columns are a fixed seeded sample,
    every column of a small job, and the dump stays within 64 MB."""
    import numpy as np
    import pytest
    b = _bench()
    a = b.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    a = b.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"
    with pytest.raises(SystemExit):
        b.parse_args(["--steps", "0"])
    assert np.array_equal(b.dump_columns(1000, 144, 4), np.arange(1000))
    for N, T, elem in ((1 << 20, 144, 4), (1 << 20, 144, 8), (10_000, 3000, 8), (1 << 20, 144 * 64, 8)):
        idx = b.dump_columns(N, T, elem)
        assert np.array_equal(idx, b.dump_columns(N, T, elem)) and np.array_equal(idx, np.unique(idx))
        assert 0 < idx.size <= b.DUMP_COLUMNS and idx[-1] < N
        assert 2 * T * elem * idx.size + 8 * T + 2 * 8 * idx.size <= 64 << 20


def test_dump_writes_the_named_columns(tmp_path):
    """dump_outputs gathers exactly the columns dump_columns names: every value encodes its own (step, column)."""
    import numpy as np
    import torch
    b = _bench()
    T, N, L = 5, 3 * b.DUMP_COLUMNS, 3
    code = torch.arange(T * N, dtype=torch.float64).reshape(T, N)
    series = {"runoff": code.float(), "percolation": -code}
    status = torch.arange(N, dtype=torch.int32) % 7
    history = torch.arange(N, dtype=torch.int64) % 5
    soils = [torch.rand(L, N) for _ in range(6)]
    d = b.dump_outputs(str(tmp_path), series, code.sum(1), status, history, soils)
    idx = b.dump_columns(N, T, 4)
    a = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert d["files"] == {nm + ".npy": list(x.shape) for nm, x in a.items()} and idx.size == b.DUMP_COLUMNS
    assert a["runoff"].dtype == np.float32 and np.array_equal(a["runoff"], code.float().numpy()[:, idx])
    assert np.array_equal(a["percolation"], -code.numpy()[:, idx])
    assert np.array_equal(a["status"], idx % 7) and np.array_equal(a["redrawn"], idx % 5)
    assert np.array_equal(a["basin_runoff"], code.sum(1).numpy())
    # the digest covers every column's soils, not only the dumped ones
    soils[2][1, np.setdiff1d(np.arange(N), idx)[0]] += 1
    assert b.dump_outputs(str(tmp_path / "x"), series, code.sum(1), status, history, soils)["inputs_sha256"] != d["inputs_sha256"]


def test_cpu_baseline_leg_runs_on_a_tiny_sample(monkeypatch):
    b = _bench()
    monkeypatch.setenv("LGAR_CPU_THREADS", "2")
    r = b.cpu_baseline(target_s=0.3)
    assert r["kind"] == "port" and r["cores"] == 2 and r["value"] > 1e3 and "columns x 144 steps" in r["sample"]


def test_wait_ranks_stops_the_siblings_of_a_failed_rank():
    """a rank that dies early must not leave the others blocked until the RCCL timeout."""
    import subprocess
    import sys
    import time
    b = _bench()
    t0 = time.time()
    procs = [subprocess.Popen([sys.executable, "-c", "import time; print('rank0 up', flush=True); time.sleep(120)"],
                              stdout=subprocess.PIPE, text=True),
             subprocess.Popen([sys.executable, "-c", "import sys; sys.exit(3)"])]
    out, failed = b.wait_ranks(procs)
    assert failed == (1, 3) and time.time() - t0 < 30
    assert all(p.poll() is not None for p in procs) and "rank0 up" in out
    procs = [subprocess.Popen([sys.executable, "-c", "print('{\"ok\": 1}')"], stdout=subprocess.PIPE, text=True),
             subprocess.Popen([sys.executable, "-c", "pass"])]
    out, failed = b.wait_ranks(procs)
    assert failed is None and out.strip() == '{"ok": 1}'
