"""GPU: the plain fp32 kernels with their reuse of Geff values against the same kernels without it.

The product library is compared with the measurement variant of it built with every reuse switched off
(-DLGAR_NO_F32_REUSE, lgar_py_amd/csrc/lgar_measure.hpp; the fp32 instantiations only, one build per layer count: 2, 3, 6).
Runoff and percolation series, status words and the final state must be equal BIT FOR BIT; the count of wave-level Geff evaluations
must not be higher.  Shapes: the benchmark's ensemble (workloads.perturbed_columns / forcing_scale, no re-draws) at 4 096
columns x 144 steps through the front-capacity chain (the 8-slot kernel bench.py times); the layer sets of the 2- and 6-layer
determinism tests at 512 columns; and a 3-layer job of 4 096 columns under the pulsed rain that grows up to ~30 fronts per
column, with front_slots = 32 and the chain forced, so that the 16-slot kernel (and the 32-slot one) take over the columns the
8-slot kernel hands on.  (front_slots alone cannot make the chain START at 16 slots -- that takes more sub-steps per step --
and fewer than 32 rows make most of these columns overflow.)"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

STATE = ["depth", "theta", "psi", "k", "dzdt", "flags", "n_fronts", "scalars", "totals"]


OFF_FLAGS = ["-DLGAR_ONLY_F32", "-DLGAR_NO_F32_REUSE"]


def _load_beside(path):
    """A second library next to the loaded one: _capi.load() binds whatever LGAR_LIB names, once per process."""
    from lgar_py_amd import _capi, build as B
    saved = (_capi._lib, B.LIB, os.environ.get("LGAR_LIB"))
    try:
        _capi._lib, B.LIB, os.environ["LGAR_LIB"] = None, path, path
        return _capi.load()
    finally:
        _capi._lib, B.LIB = saved[0], saved[1]
        if saved[2] is None:
            del os.environ["LGAR_LIB"]
        else:
            os.environ["LGAR_LIB"] = saved[2]


@pytest.fixture(scope="module")
def libraries():
    """(product library, {layer count: library with every reuse switched off}).  A measurement build holds one layer count
    (its read-backs exist once per layer count's translation unit, build.build_variant): three small builds, side by side."""
    import concurrent.futures as cf
    from lgar_py_amd import _capi, build as B
    product = _capi.load()
    with cf.ThreadPoolExecutor(max_workers=3) as ex:
        paths = list(ex.map(lambda n: B.build_variant("f32_reuse_off_l%d" % n, OFF_FLAGS, layers=(n,)), (2, 3, 6)))
    off = {n: _load_beside(p) for n, p in zip((2, 3, 6), paths)}
    assert _capi.load() is product and all(lib is not product for lib in off.values())
    return product, off


def _bench_job(N, **kw):
    import lgar_py_amd as lg
    from lgar_py_amd import workloads as W
    P = W.perturbed_columns(N, seed=0)
    sc = torch.tensor(W.forcing_scale(N, seed=1000), device="cuda")
    f = W.synth1_forcing()
    eng = lg.LgarEngine(P["alpha"], P["n"], P["ksat"], P["theta_e"], P["theta_r"], P["thickness"], dt_h=300.0 / 3600.0,
                        ponded_depth_max=0.0, dtype=torch.float32, **kw)
    pr = (torch.tensor(f[:, 0], device="cuda")[:, None] * sc[None, :]).float().contiguous()
    return eng, pr, torch.zeros_like(pr)


def _golden_job(name, N, **kw):
    """the perturbed ensemble of the determinism tests (tests/test_gpu_properties.py) around a fixture's soil and forcing"""
    import lgar_py_amd as lg
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    rng = np.random.default_rng(11)
    L = len(g["alpha"])
    pert = lambda v: np.asarray(v, dtype=np.float64)[:, None] * (1.0 + 0.1 * (2.0 * rng.random((L, N)) - 1.0))
    eng = lg.LgarEngine(pert(g["alpha"]), pert(g["n"]), pert(g["ksat"]), pert(g["theta_e"]), pert(g["theta_r"]),
                        np.repeat(np.asarray(g["thickness"], dtype=np.float64)[:, None], N, 1), dt_h=float(g["dt_h"]),
                        num_subcycles=int(g["num_subcycles"]), ponded_depth_max=float(g["pdm"]), initial_psi=float(g["initial_psi"]),
                        wilting_point_psi=float(g["wilting_point_psi"]), nint=int(g["nint"]), dtype=torch.float32, **kw)
    sc = torch.tensor(0.7 + 0.6 * rng.random(N), device="cuda")
    f = torch.tensor(g["forcing"], device="cuda")
    pr = (f[:, 0:1] * sc[None, :]).float().contiguous()
    pe = f[:, 1:2].expand(-1, N).float().contiguous()
    return eng, pr, pe


CASES = {
    "bench_3_layers_4096": lambda: _bench_job(4096, search_mode=2),
    "two_layers_512": lambda: _golden_job("two_layer_synth1", 512, search_mode=2),
    "six_layers_512": lambda: _golden_job("six_layer_synth1", 512, search_mode=2),
    "three_layers_4096_16_slot_kernel": lambda: _golden_job("manyfronts_pulse_84", 4096, search_mode=2, front_slots=32),
}


def _run(eng, lib, pr, pe):
    eng.lib = lib
    eng.reset()
    eng.geff_wave_calls()  # (zero the counter)
    o = eng.forward(pr, pe, series=("runoff", "percolation"), check=False)
    torch.cuda.synchronize()
    res = {"runoff": o["runoff"], "percolation": o["percolation"], "status": eng.status}
    res.update({nm: getattr(eng, nm) for nm in STATE})
    res = {k: v.detach().cpu().numpy().copy() for k, v in res.items()}
    return res, int(eng.geff_wave_calls())


@pytest.mark.parametrize("case", list(CASES))
def test_fp32_kernels_equal_the_kernels_without_reuse_bit_for_bit(libraries, case):
    product, off = libraries
    eng, pr, pe = CASES[case]()
    want, calls_off = _run(eng, off[eng.L], pr, pe)
    got, calls = _run(eng, product, pr, pe)
    print("%s: wave-level Geff evaluations %d with reuse, %d without" % (case, calls, calls_off))
    ok = want["status"] == 0
    assert int(ok.sum()) > ok.size // 2  # (most columns run to the end: the comparison is one of trajectories, not of faults)
    if case.endswith("16_slot_kernel"):
        assert int(((want["n_fronts"] > 8) & ok).sum()) > ok.size // 10  # the kernels behind the 8-slot one ran
    for key in want:
        a, b = got[key], want[key]
        assert a.shape == b.shape and a.dtype == b.dtype, key
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        assert np.array_equal(a, b), (key, int((a != b).sum()))
    assert calls_off > 0 and calls <= calls_off, (calls, calls_off)
