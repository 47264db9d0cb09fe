"""GPU: the plain fp32 kernels with their top-layer step against the same kernels without it.

A wave whose 64 columns all hold a top-layer table (m >= 1 in-layer fronts of layer 0, then the layers' boundary fronts in order)
takes the sweep and calc_dzdt with that shape resolved at compile time; one column off the predicate sends the whole wave through
the generic code (lgar_py_amd/csrc/lgar_column.hpp: is_top_table, sweep_top, calc_dzdt's `fast`).  The product library is
compared with the variant built with -DLGAR_NO_TOP_LAYER_STEP (the fp32 instantiations only, one build per layer count: 2, 3, 6):
every output series, the status words and the whole final state must be equal BYTE FOR BYTE, and a job run twice must repeat
itself.  Shapes, the smallest that can still go wrong:
  * 256 columns of the benchmark's ensemble x 144 steps = four waves; from step ~112 on fronts enter layer 1 column by column, so
    waves mix lanes on and off the predicate (asserted on the final tables) -- through the capacity chain (the 8-slot kernel
    bench.py times) and, without the chain, in the 32-slot kernel alone;
  * 128 columns whose top layer is 5 cm thick: fronts enter layer 1 within the first storm pulse;
  * 65 columns: a ragged second wave, 63 padding lanes;
  * the pulsed rain that grows up to ~30 fronts per column, 256 columns with 32 rows and the chain forced: the 16-slot and the
    32-slot kernels take over;
  * 2-layer and 6-layer soils, 64 columns each."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

STATE = ["depth", "theta", "psi", "k", "dzdt", "flags", "n_fronts", "scalars", "totals"]
SERIES = ("precip", "PET", "AET", "infiltration", "runoff", "percolation", "giuh_runoff", "discharge", "ponded_water",
          "ending_volume")  # (every per-step accumulator: lgar_py_amd._capi.ACC_NAMES)
OFF_FLAGS = ["-DLGAR_ONLY_F32", "-DLGAR_NO_TOP_LAYER_STEP"]


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
    """(product library, {layer count: library without the top-layer step}); a measurement build holds one layer count."""
    import concurrent.futures as cf
    from lgar_py_amd import _capi, build as B
    product = _capi.load()
    with cf.ThreadPoolExecutor(max_workers=3) as ex:
        paths = list(ex.map(lambda n: B.build_variant("top_step_off_l%d" % n, OFF_FLAGS, layers=(n,)), (2, 3, 6)))
    off = {n: _load_beside(p) for n, p in zip((2, 3, 6), paths)}
    assert _capi.load() is product and all(lib is not product for lib in off.values())
    return product, off


def _bench_job(N, top_cm=None, **kw):
    import lgar_py_amd as lg
    from lgar_py_amd import workloads as W
    P = W.perturbed_columns(N, seed=0)
    if top_cm is not None:
        P["thickness"][0, :] = top_cm
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
    "bench_256_capacity_chain": lambda: _bench_job(256, search_mode=2),
    "bench_256_32_slot_kernel": lambda: _bench_job(256),
    "thin_top_layer_128": lambda: _bench_job(128, top_cm=5.0, search_mode=2),
    "ragged_65": lambda: _bench_job(65, search_mode=2),
    "pulsed_rain_256_16_and_32_slot_kernels": lambda: _golden_job("manyfronts_pulse_84", 256, search_mode=2, front_slots=32),
    "two_layers_64": lambda: _golden_job("two_layer_synth1", 64, search_mode=2),
    "six_layers_64": lambda: _golden_job("six_layer_synth1", 64, search_mode=2),
}


def _run(eng, lib, pr, pe):
    eng.lib = lib
    eng.reset()
    o = eng.forward(pr, pe, series=SERIES, check=False)
    torch.cuda.synchronize()
    res = {"series:" + nm: o[nm] for nm in SERIES}
    res["status"] = eng.status
    res.update({nm: getattr(eng, nm) for nm in STATE})
    return {k: v.detach().cpu().numpy().copy() for k, v in res.items()}


def _off_predicate(res, L):
    """per column: does its final table hold a front that is no boundary front and sits below layer 0?"""
    fl, nf = res["flags"].astype(np.int64), res["n_fronts"].astype(np.int64)
    live = np.arange(fl.shape[0])[:, None] < nf[None, :]
    return (live & ((fl & 0x80) == 0) & ((fl & 0x7f) > 0)).any(axis=0)


@pytest.mark.parametrize("case", list(CASES))
def test_fp32_kernels_equal_the_kernels_without_the_top_layer_step_byte_for_byte(libraries, case):
    product, off = libraries
    eng, pr, pe = CASES[case]()
    want = _run(eng, off[eng.L], pr, pe)
    got = _run(eng, product, pr, pe)
    again = _run(eng, product, pr, pe)
    ok = want["status"] == 0
    assert int(ok.sum()) > ok.size // 2  # (most columns run to the end: the comparison is one of trajectories, not of faults)
    assert float(want["series:infiltration"].sum()) > 0.0  # (... and of columns whose fronts move)
    if case.startswith("pulsed_rain"):
        assert int(((want["n_fronts"] > 8) & ok).sum()) > ok.size // 10  # the kernels behind the 8-slot one ran
    if case.startswith("bench_256"):
        # waves that mix columns on and off the predicate: by the end every wave holds both kinds
        offp = _off_predicate(want, eng.L)
        for w in range(0, offp.size, 64):
            assert 0 < int(offp[w:w + 64].sum()) < 64, (w, int(offp[w:w + 64].sum()))
    if case.startswith("thin_top_layer"):
        assert int(_off_predicate(want, eng.L).sum()) > ok.size // 2  # fronts did enter layer 1
    for key in want:
        for other in (got, again):
            a, b = other[key], want[key]
            assert a.shape == b.shape and a.dtype == b.dtype, key
            assert a.tobytes() == b.tobytes(), (key, int((a.view(np.uint8) != b.view(np.uint8)).sum()))
