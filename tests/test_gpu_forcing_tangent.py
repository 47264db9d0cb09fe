"""GPU (-m gpu): the tangent kernels that take a forcing direction (lgar_forward_tangent_forced, lgar_tangent_forced_kernel)
against the reference's own x.grad for its loss (tests/golden/forcing_grad), the window kernels bit for bit, a lane's own
single-direction launch -- the bodies of tests/_forcing_tangent.py, which the simulator's suite runs on the host build -- and,
what only the hardware has, the lanes of a mixed group sharing the trapezoid.  One to 300 lanes: every case takes seconds."""
import ctypes as C

import numpy as np
import pytest

import _forcing_tangent as FT
import _golden as G

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _make(g, N, soil=None, geff_mode=0, **kw):
    import lgar_py_amd as lg
    if geff_mode:
        kw["geff_precision"] = "f32"
    if soil is not None:
        return lg.LgarEngine(*soil, **kw)
    return lg.LgarEngine(*G.soil(g), n_columns=N, **dict(G.engine_keywords(g), **kw))


PARITY = [(n, m, False) for n in FT.CASES for m in (1, 2, 0)] + [(n, m, True) for n in FT.CASES for m in (1, 2)]


@pytest.mark.parametrize("name, mode, mixed", PARITY, ids=["%s-mode%d%s" % (n, m, "-mixed" if x else "") for n, m, x in PARITY])
def test_forcing_gradient_matches_reference_autograd(name, mode, mixed):
    """grad_manyfronts_60 in mode 2 goes through the capacity chain: its 120 lanes are handed over to the 32-slot kernel (the
    fixture's front counts pass 8) and none is left with LGAR_ST_RESUME (status 0)."""
    FT.reference_parity(_make, "cuda", name, mode, mixed)


@pytest.mark.parametrize("dtype, mode", [(torch.float64, 1), (torch.float64, 2), (torch.float64, 0), (torch.float32, 1)],
                         ids=["f64_fast", "f64_chain", "f64_literal", "f32"])
def test_null_tangents_leave_the_bits_of_tangent_window(dtype, mode):
    FT.null_tangents(_make, "cuda", dtype, mode)


@pytest.mark.parametrize("group", FT.GROUPS)
def test_every_lane_of_a_mixed_group_is_its_own_launch_bit_for_bit(group):
    FT.layouts(_make, "cuda", group, 0)


@pytest.mark.parametrize("group", [g for g in FT.GROUPS if g >= 2])
def test_lanes_of_a_mixed_group_share_the_trapezoid(group):
    FT.layouts(_make, "cuda", group, group)


@pytest.mark.parametrize("name, dtype, mode, middle", [("grad_synth0_12h", torch.float64, 1, None), ("grad_synth0_12h", torch.float32, 1, None),
                                                       ("grad_synth0_12h", torch.float64, 0, None), ("grad_manyfronts_60", torch.float64, 2, 45)],
                         ids=["synth0_f64", "synth0_f32", "synth0_literal", "manyfronts_chain"])
def test_chunked_windows_are_one_call_bit_for_bit(name, dtype, mode, middle):
    FT.chunked_windows(_make, "cuda", name, dtype, mode, middle)


def test_raw_entry_point_refuses_what_the_header_says():
    from lgar_py_amd import _capi
    lib = _capi.load()
    keep = []

    def alloc(shape, dtype, fill):
        a = np.empty(shape, dtype=dtype)
        a[...] = fill
        keep.append(torch.tensor(a, device="cuda"))
        return keep[-1].data_ptr()

    tickets = torch.zeros(_capi.NTICKETS, dtype=torch.int32, device="cuda")

    def raw(*args):
        rc = lib.lgar_forward_tangent_forced(*args, C.c_void_p(torch.cuda.current_stream().cuda_stream), tickets.data_ptr())
        torch.cuda.synchronize()
        return rc

    FT.refusals(raw, alloc)


def test_lgar_series_without_forcing_directions_is_what_it_was():
    FT.series_baseline(_make, "cuda")


def test_scaled_forcing_gradients_match_reference_autograd():
    FT.series_scale_matches_reference("cuda")


@pytest.mark.parametrize("shared", [False, True], ids=["own_lanes", "shared_trapezoid"])
def test_cell_gradients_equal_the_other_association(shared, monkeypatch):
    """Written down from a run on the hardware: profiles/r18/two_associations.txt."""
    FT.series_cells_two_ways(_make, "cuda", 1 if shared else 1 << 30, monkeypatch)


def test_snow_parameters_and_scales_two_ways():
    """The measured gaps: profiles/r18/two_associations.txt."""
    import lgar_py_amd as lg
    FT.snow_chain_two_ways(_make, "cuda:0", lg.CatchmentSnow, lg.catchment_snow)


def test_lgar_series_without_forcing_directions_has_the_parents_bits():
    """The parameter gradients of grad_synth0_12h through lgar_series, bit for bit those the parent commit's library gave on this
    hardware (tests/golden/forcing_grad/series_baseline_parent.npz, stored from a run of that library)."""
    FT.series_parent_bits("cuda")


def test_lgar_series_refuses_what_forcing_directions_cannot_do():
    FT.series_refuses("cuda")
