"""CPU: the tangent with a forcing direction (lgar_forward_tangent_forced; LgarEngine.tangent / tangent_window with d_precip /
d_pet) on the host build of the kernels' own headers (tests/forced_host).  The oracles: the reference's own x.grad for its loss
(tests/golden/forcing_grad), the window family bit for bit, a lane's own single-direction launch.  The bodies are
tests/_forcing_tangent.py's, which the GPU suite runs too; the host build runs one lane at a time, so the lanes of a group never
share the trapezoid here (share = 0 only)."""
import numpy as np
import pytest
import torch

import _forcing_tangent as FT
import _golden as G
import _hostbuild


def _make(g, N, soil=None, **kw):
    import forced_host
    if soil is not None:
        return forced_host.ForcedSimEngine(*soil, **kw)
    return forced_host.ForcedSimEngine(*G.soil(g), n_columns=N, **dict(G.engine_keywords(g), **kw))


# the literal searches take ~100x the evaluations: the short fixture here, every fixture on the GPU
PARITY = [(n, m, False) for n in FT.CASES for m in (1, 2)] + [("grad_synth0_12h", 0, False), ("grad_synth0_12h", 1, True),
                                                               ("grad_two_layer_phil_150", 2, True)]


@pytest.mark.parametrize("name, mode, mixed", PARITY, ids=["%s-mode%d%s" % (n, m, "-mixed" if x else "") for n, m, x in PARITY])
def test_forcing_gradient_matches_reference_autograd(name, mode, mixed):
    FT.reference_parity(_make, "cpu", name, mode, mixed)


@pytest.mark.parametrize("dtype, mode", [(torch.float64, 1), (torch.float64, 2), (torch.float64, 0), (torch.float32, 1)],
                         ids=["f64_fast", "f64_chain", "f64_literal", "f32"])
def test_null_tangents_leave_the_bits_of_tangent_window(dtype, mode):
    FT.null_tangents(_make, "cpu", dtype, mode)


@pytest.mark.parametrize("group", FT.GROUPS)
def test_every_lane_of_a_mixed_group_is_its_own_launch_bit_for_bit(group):
    FT.layouts(_make, "cpu", group, 0)


@pytest.mark.parametrize("name, dtype, mode, middle", [("grad_synth0_12h", torch.float64, 1, None), ("grad_synth0_12h", torch.float32, 1, None),
                                                       ("grad_synth0_12h", torch.float64, 0, None), ("grad_manyfronts_60", torch.float64, 2, 45)],
                         ids=["synth0_f64", "synth0_f32", "synth0_literal", "manyfronts_chain"])
def test_chunked_windows_are_one_call_bit_for_bit(name, dtype, mode, middle):
    FT.chunked_windows(_make, "cpu", name, dtype, mode, middle)


def test_raw_entry_point_refuses_what_the_header_says():
    import forced_host
    lib = forced_host.library(3)
    keep = []

    def alloc(shape, dtype, fill):
        a = np.empty(shape, dtype=dtype)
        a[...] = fill
        keep.append(a)
        return a.ctypes.data

    FT.refusals(lib.forcedhost_forward_tangent_forced, alloc)


def test_engine_refuses_forcing_tangents_of_another_shape():
    from lgar_py_amd import LgarError
    g, pr, pe, w = FT.storm_job("cpu")
    eng = _make(g, 3)
    with pytest.raises(LgarError, match=r"d_precip must be \[T, Nf, forcing_group\] = \[24, 3, 1\]"):
        eng.tangent({}, pr, pe, w_runoff=w, d_precip=pr[:-1])
    with pytest.raises(LgarError, match=r"d_pet must be \[T, Nf, forcing_group\]"):
        eng.tangent_window({}, pr, pe, w_runoff=w, d_pet=pe[:, :2])
    assert float(eng.tangent({}, pr, pe, w_runoff=w, d_precip=pr[:, :, None])[0].abs().sum()) > 0.0  # [T, Nf, 1] will do


@pytest.fixture
def sim(monkeypatch):
    """the simulator's engine and catchment map behind lgar_py_amd.autograd, in this test only"""
    import devsim
    import forced_host
    import lgar_py_amd.autograd as A
    monkeypatch.setattr(A, "LgarEngine", forced_host.ForcedSimEngine)
    monkeypatch.setattr(A, "CatchmentMap", devsim.SimCatchmentMap)


def test_lgar_series_without_forcing_directions_is_what_it_was(sim):
    FT.series_baseline(_make, "cpu")


def test_scaled_forcing_gradients_match_reference_autograd(sim):
    FT.series_scale_matches_reference("cpu")


def test_cell_gradients_equal_the_other_association(sim):
    FT.series_cells_two_ways(_make, "cpu")


def test_snow_parameters_and_scales_two_ways(sim):
    import snow_host
    import snow_tangent_host
    FT.snow_chain_two_ways(_make, "cpu", snow_tangent_host.SimSnow, snow_host.SimCatchmentSnow.function)


def test_lgar_series_refuses_what_forcing_directions_cannot_do(sim):
    FT.series_refuses("cpu")


def test_stand_alone_program_runs_clean_under_the_sanitizers():
    """forced_host_main.cpp: a parameter and a forcing direction together, one call against the cut run, in double and single
    precision, with and without the capacity chain, under AddressSanitizer + UBSan (host code in a program of its own)."""
    import forced_host
    assert _hostbuild.run_clean([forced_host.program(sanitize=True)]).strip() == "ok"
