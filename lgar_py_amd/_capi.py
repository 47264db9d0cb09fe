"""ctypes binding of the C-ABI declared in include/lgar.h (liblgar_hip.so).

There is no CPU fallback: if the HIP library is missing or cannot be loaded, every entry point
raises.  Torch is used only for device memory and streams; the signatures carry raw pointers.  open_library and launch are
the one way into the library: every entry point the package calls goes through them.
"""
import ctypes as C
import os

import torch

from . import build as _build

FMAX, LMIN, LMAX, GMAX = 32, 2, 6, 8
CAP_SMALL, CAP_MID = 8, 16
NCOUNTERS = 4
NTICKETS = 8
MOIST_BINS = 32  # LGAR_MOIST_BINS
ROUTE_KMAX = 64  # LGAR_ROUTE_KMAX
SCORE_BLOCK, SCORE_NMOM = 64, 7  # LGAR_SCORE_BLOCK, LGAR_SCORE_NMOM
GW_ZMAX = 40.0  # LGAR_GW_ZMAX
MOIST_WHAT = {"theta": 0, "storage": 1}  # lgar_soil_moisture's `what`
ST_RESUME, ST_FAULT_MASK = 128, 0x7F
NSCAL = 3 + GMAX
NACC = 10
F32, F64 = 0, 1
ACC_NAMES = ["precip", "PET", "AET", "infiltration", "runoff", "percolation", "giuh_runoff", "discharge",
             "ponded_water", "ending_volume"]
ST_NAN, ST_NEGBASE, ST_THETA_ORDER, ST_OVERFLOW, ST_ITERCAP, ST_BOTTOM, ST_STRUCT = 1, 2, 4, 8, 16, 32, 64
STATUS_NAMES = {1: "NaN", 2: "negative pow base", 4: "theta order", 8: "front overflow", 16: "iteration cap",
                32: "front reached domain bottom", 64: "structural error"}
ABI_VERSION = 4  # LGAR_ABI_VERSION of include/lgar.h this binding mirrors
EXPORTS = ["lgar_version", "lgar_abi_version", "lgar_sizeof_dims", "lgar_fmax", "lgar_lmax", "lgar_cooperating_lanes", "lgar_state_init", "lgar_forward", "lgar_forward_tangent", "lgar_forward_tangent_window", "lgar_forward_tangent_forced",
           "lgar_soil_moisture", "lgar_soil_moisture_tangent", "lgar_totals_replay", "lgar_catchment_sums", "lgar_catchment_spread", "lgar_catchment_route", "lgar_catchment_route_grad",
           "lgar_catchment_moments_workspace", "lgar_catchment_moments", "lgar_catchment_moments_grad", "lgar_network_route", "lgar_network_route_grad", "lgar_network_route_mc", "lgar_network_route_mc_grad", "lgar_network_route_pool", "lgar_network_route_pool_grad", "lgar_catchment_baseflow", "lgar_catchment_baseflow_grad", "lgar_catchment_snow", "lgar_catchment_snow_grad", "lgar_catchment_snow_tangent", "lgar_catchment_canopy", "lgar_catchment_canopy_grad", "lgar_catchment_canopy_tangent", "lgar_leaf_batch", "lgar_leaf_tangent_batch", "lgar_valu_probe", "lgar_valu_probe_insts"]


class LgarDims(C.Structure):
    _fields_ = [("n_columns", C.c_int32), ("n_layers", C.c_int32), ("n_steps", C.c_int32),
                ("num_subcycles", C.c_int32), ("nint", C.c_int32), ("n_giuh", C.c_int32),
                ("search_mode", C.c_int32), ("bottom_mode", C.c_int32), ("use_closed_form_G", C.c_int32), ("front_slots", C.c_int32),
                ("dt_h", C.c_double), ("initial_psi", C.c_double), ("ponded_depth_max", C.c_double),
                ("wilting_point_psi", C.c_double), ("frozen_factor", C.c_double), ("giuh", C.c_double * GMAX),
                ("iter_cap", C.c_int64), ("forcing_columns", C.c_int32), ("forcing_group", C.c_int32),
                ("tangent_share", C.c_int32), ("geff_mode", C.c_int32), ("forward_lanes", C.c_int32), ("reserved4", C.c_int32)]


class LgarParams(C.Structure):
    _fields_ = [(nm, C.c_void_p) for nm in ("alpha", "n", "ksat", "theta_e", "theta_r", "thickness")]


class LgarState(C.Structure):
    _fields_ = [(nm, C.c_void_p) for nm in ("depth", "theta", "psi", "k", "dzdt", "flags", "n_fronts", "scalars",
                                            "totals", "tickets")]


class LgarForcing(C.Structure):
    # (LgarForcing(precip, pet) leaves column_map NULL: no map)
    _fields_ = [("precip", C.c_void_p), ("pet", C.c_void_p), ("column_map", C.c_void_p)]


class LgarTangentWindow(C.Structure):
    # pointers to LgarState structs (the caller keeps them alive across the call), and the [N] gradient the fold continues from
    _fields_ = [(nm, C.c_void_p) for nm in ("state_in", "dstate_in", "state_out", "dstate_out", "grad_in")]


class LgarStepOut(C.Structure):
    _fields_ = [("series", C.c_void_p * NACC), ("basin", C.c_void_p), ("weights", C.c_void_p), ("basin_mask", C.c_uint32), ("reserved", C.c_uint32), ("counters", C.c_void_p), ("call_sums", C.c_void_p)]


def make_dims(*, n_columns, n_layers, dt_h=1.0, num_subcycles=1, initial_psi=2000.0, ponded_depth_max=0.0,
              wilting_point_psi=15495.0, frozen_factor=1.0, nint=120, giuh_ordinates=(0.06, 0.51, 0.28, 0.12, 0.03), iter_cap=0,
              search_mode=1, bottom_mode=0, use_closed_form_G=False, front_slots=None, geff_mode=0, forward_lanes=0):
    """A filled LgarDims for an engine's keywords (LgarEngine's names; n_steps and the forcing layout are per call).  Plain
    assignments: the caller has checked what it wants checked."""
    d = LgarDims()
    d.n_columns, d.n_layers, d.n_steps, d.num_subcycles = n_columns, n_layers, 0, int(num_subcycles)
    d.nint, d.n_giuh, d.search_mode = int(nint), len(giuh_ordinates), int(search_mode)
    d.dt_h, d.initial_psi, d.ponded_depth_max = float(dt_h), float(initial_psi), float(ponded_depth_max)
    d.wilting_point_psi, d.frozen_factor = float(wilting_point_psi), float(frozen_factor)
    for i, g in enumerate(giuh_ordinates):
        d.giuh[i] = float(g)
    d.iter_cap, d.bottom_mode, d.use_closed_form_G = int(iter_cap), int(bottom_mode), int(bool(use_closed_form_G))
    d.geff_mode, d.forward_lanes = int(geff_mode), int(forward_lanes)
    d.front_slots = int(front_slots) if front_slots else FMAX
    return d


class LgarError(RuntimeError):
    pass


_lib = None


def lib_path():
    return _build.LIB


def load():
    """Load liblgar_hip.so, (re)building it first when it is missing or was built from other sources (content
    fingerprint, build.py); raise loudly if that is impossible."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.LIB
    if not os.environ.get("LGAR_LIB"):  # an explicitly selected library (measurement variants) is taken as it is
        try:
            _build.build()
        except Exception as e:  # noqa: BLE001
            raise LgarError("liblgar_hip.so is missing or stale and could not be built (%s); there is no CPU fallback" % e)
    try:
        lib = C.CDLL(path)
    except OSError as e:
        raise LgarError("cannot load %s: %s; there is no CPU fallback" % (path, e))
    p = C.POINTER
    i32, vp, dbl = C.c_int32, C.c_void_p, C.c_double
    # an older library (a measurement variant selected with LGAR_LIB, a stale copy) would misread LgarDims or take garbage for
    # an argument it does not know: refuse it before the first call
    if not hasattr(lib, "lgar_abi_version"):
        raise LgarError("%s predates lgar_abi_version(): rebuild it (ABI %d expected)" % (path, ABI_VERSION))
    lib.lgar_abi_version.restype = i32
    lib.lgar_sizeof_dims.restype = i32
    if lib.lgar_abi_version() != ABI_VERSION or lib.lgar_sizeof_dims() != C.sizeof(LgarDims):
        raise LgarError("%s has ABI %d / sizeof(LgarDims) %d, this binding needs %d / %d: rebuild it"
                        % (path, lib.lgar_abi_version(), lib.lgar_sizeof_dims(), ABI_VERSION, C.sizeof(LgarDims)))
    lib.lgar_version.restype = C.c_char_p
    lib.lgar_fmax.restype = i32
    lib.lgar_lmax.restype = i32
    lib.lgar_cooperating_lanes.restype = i32
    lib.lgar_cooperating_lanes.argtypes = [p(LgarDims), i32]
    lib.lgar_state_init.restype = i32
    lib.lgar_state_init.argtypes = [p(LgarDims), p(LgarParams), p(LgarState), vp, i32, vp]
    lib.lgar_forward.restype = i32
    lib.lgar_forward.argtypes = [p(LgarDims), p(LgarParams), p(LgarState), p(LgarForcing), p(LgarStepOut), vp, i32, vp]
    if hasattr(lib, "lgar_forward_tangent") or not os.environ.get("LGAR_LIB"):  # measurement variants omit it
        lib.lgar_forward_tangent.restype = i32
        lib.lgar_forward_tangent.argtypes = [p(LgarDims), p(LgarParams), p(LgarParams), p(LgarForcing), vp, vp, vp, vp, vp,
                                             i32, vp, vp]
    if hasattr(lib, "lgar_forward_tangent_window") or not os.environ.get("LGAR_LIB"):  # (a library selected by hand may predate it)
        lib.lgar_forward_tangent_window.restype = i32
        lib.lgar_forward_tangent_window.argtypes = [p(LgarDims), p(LgarParams), p(LgarParams), p(LgarForcing), vp, vp,
                                                    p(LgarTangentWindow), vp, vp, vp, i32, vp, vp]
    if hasattr(lib, "lgar_forward_tangent_forced") or not os.environ.get("LGAR_LIB"):  # (a library selected by hand may predate it)
        lib.lgar_forward_tangent_forced.restype = i32
        lib.lgar_forward_tangent_forced.argtypes = [p(LgarDims), p(LgarParams), p(LgarParams), p(LgarForcing), p(LgarForcing), vp, vp,
                                                    p(LgarTangentWindow), vp, vp, vp, i32, vp, vp]
    if hasattr(lib, "lgar_soil_moisture") or not os.environ.get("LGAR_LIB"):  # (a measurement variant built before it existed)
        lib.lgar_soil_moisture.restype = i32
        lib.lgar_soil_moisture.argtypes = [p(LgarDims), p(LgarParams), p(LgarState), vp, i32, i32, vp, vp, vp, i32, vp]
        lib.lgar_totals_replay.restype = i32
        lib.lgar_totals_replay.argtypes = [p(LgarDims), p(LgarStepOut), i32, vp, i32, vp]
    if hasattr(lib, "lgar_soil_moisture_tangent") or not os.environ.get("LGAR_LIB"):  # (a library selected by hand may predate it)
        lib.lgar_soil_moisture_tangent.restype = i32
        lib.lgar_soil_moisture_tangent.argtypes = [p(LgarDims), p(LgarParams), p(LgarState), p(LgarState), vp, i32, i32, vp, vp, i32,
                                                   vp, i32, vp]
    if hasattr(lib, "lgar_catchment_sums") or not os.environ.get("LGAR_LIB"):  # (a library selected by hand may predate them)
        lib.lgar_catchment_sums.restype = i32
        lib.lgar_catchment_sums.argtypes = [vp, i32, i32, vp, i32, vp, i32, vp, vp, vp, vp, i32, vp]
        lib.lgar_catchment_spread.restype = i32
        lib.lgar_catchment_spread.argtypes = [vp, i32, i32, vp, i32, vp, vp, vp, i32, vp]
    if hasattr(lib, "lgar_catchment_route") or not os.environ.get("LGAR_LIB"):
        lib.lgar_catchment_route.restype = i32
        lib.lgar_catchment_route.argtypes = [vp, i32, i32, vp, i32, i32, vp, vp, vp, i32, vp]
        lib.lgar_catchment_route_grad.restype = i32
        lib.lgar_catchment_route_grad.argtypes = [vp, vp, i32, i32, i32, vp, vp]
    if hasattr(lib, "lgar_catchment_moments") or not os.environ.get("LGAR_LIB"):
        lib.lgar_catchment_moments_workspace.restype = C.c_int64
        lib.lgar_catchment_moments_workspace.argtypes = [i32, i32]
        lib.lgar_catchment_moments.restype = i32
        lib.lgar_catchment_moments.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp]
        lib.lgar_catchment_moments_grad.restype = i32
        lib.lgar_catchment_moments_grad.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp, vp]
    if hasattr(lib, "lgar_network_route") or not os.environ.get("LGAR_LIB"):
        lib.lgar_network_route.restype = i32
        lib.lgar_network_route.argtypes = [vp, i32, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp]
        lib.lgar_network_route_grad.restype = i32
        lib.lgar_network_route_grad.argtypes = [vp, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp]
    if hasattr(lib, "lgar_network_route_mc") or not os.environ.get("LGAR_LIB"):
        lib.lgar_network_route_mc.restype = i32
        lib.lgar_network_route_mc.argtypes = [vp, i32, i32, vp, dbl, dbl, dbl, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp]
        lib.lgar_network_route_mc_grad.restype = i32
        lib.lgar_network_route_mc_grad.argtypes = [vp, i32, i32, vp, dbl, dbl, dbl, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    if hasattr(lib, "lgar_network_route_pool") or not os.environ.get("LGAR_LIB"):
        lib.lgar_network_route_pool.restype = i32
        lib.lgar_network_route_pool.argtypes = [vp, i32, i32, vp, vp, i32, dbl, dbl, dbl, dbl, dbl, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]
        lib.lgar_network_route_pool_grad.restype = i32
        lib.lgar_network_route_pool_grad.argtypes = [vp, i32, i32, vp, vp, i32, dbl, dbl, dbl, dbl, dbl, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp,
                                                     vp, i32, vp, vp, vp, vp, vp]
    if hasattr(lib, "lgar_catchment_baseflow") or not os.environ.get("LGAR_LIB"):
        lib.lgar_catchment_baseflow.restype = i32
        lib.lgar_catchment_baseflow.argtypes = [vp, i32, i32, vp, dbl, vp, vp, vp, vp, vp]
        lib.lgar_catchment_baseflow_grad.restype = i32
        lib.lgar_catchment_baseflow_grad.argtypes = [vp, vp, vp, vp, i32, i32, vp, dbl, vp, vp, vp, vp, vp]
    if hasattr(lib, "lgar_catchment_snow") or not os.environ.get("LGAR_LIB"):
        lib.lgar_catchment_snow.restype = i32
        lib.lgar_catchment_snow.argtypes = [vp, vp, i32, i32, vp, dbl, vp, vp, vp, vp, vp, vp]
        lib.lgar_catchment_snow_grad.restype = i32
        lib.lgar_catchment_snow_grad.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, dbl, vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "lgar_catchment_snow_tangent") or not os.environ.get("LGAR_LIB"):  # (a library selected by hand may predate it)
        lib.lgar_catchment_snow_tangent.restype = i32
        lib.lgar_catchment_snow_tangent.argtypes = [vp, vp, i32, i32, vp, dbl, vp, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]
    if hasattr(lib, "lgar_catchment_canopy") or not os.environ.get("LGAR_LIB"):  # (a library selected by hand may predate it)
        lib.lgar_catchment_canopy.restype = i32
        lib.lgar_catchment_canopy.argtypes = [vp, vp, vp, i32, i32, vp, dbl, vp, vp, vp, vp, vp, vp, vp]
        lib.lgar_catchment_canopy_grad.restype = i32
        lib.lgar_catchment_canopy_grad.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, dbl, vp, vp, vp, vp, vp, vp, vp]
        lib.lgar_catchment_canopy_tangent.restype = i32
        lib.lgar_catchment_canopy_tangent.argtypes = [vp, vp, vp, i32, i32, vp, dbl, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp]
    lib.lgar_leaf_batch.restype = i32
    lib.lgar_leaf_batch.argtypes = [i32, i32, vp, vp, dbl, vp, vp, vp, vp, vp, i32, dbl, vp, i32, vp]
    if hasattr(lib, "lgar_leaf_tangent_batch") or not os.environ.get("LGAR_LIB"):  # (a library selected by hand may predate it)
        lib.lgar_leaf_tangent_batch.restype = i32
        lib.lgar_leaf_tangent_batch.argtypes = [i32, i32, i32, i32, vp, vp, dbl] + [vp] * 12 + [i32, dbl, vp, vp, i32, vp]
    lib.lgar_valu_probe_insts.restype = i32
    lib.lgar_valu_probe_insts.argtypes = [i32]
    lib.lgar_valu_probe.restype = i32
    lib.lgar_valu_probe.argtypes = [i32, i32, i32, i32, vp, vp]
    if lib.lgar_fmax() != FMAX or lib.lgar_lmax() != LMAX:
        raise LgarError("liblgar_hip.so was built with different LGAR_FMAX/LGAR_LMAX than the Python binding")
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        raise LgarError("%s failed with code %d (%s)" % (what, rc, {-1: "bad argument", -2: "launch error",
                                                                     -3: "no device"}.get(rc, "?")))


def ptr(t):
    """The address a tensor's data starts at; None (a null pointer) for None."""
    return None if t is None else t.data_ptr()


def dtype_code(dtype, what):
    """LGAR_F32 / LGAR_F64 of a torch dtype; any other dtype raises `what` (the caller's message)."""
    if dtype == torch.float64:
        return F64
    if dtype == torch.float32:
        return F32
    raise LgarError(what)


def open_library(device, what):
    """The loaded library for a ROCm device; anything else raises `what` (a message with one %s for the device): there is no
    CPU fallback."""
    if torch.device(device).type != "cuda" or not torch.cuda.is_available():
        raise LgarError(what % (device,))
    return load()


def launch(lib, name, device, *args, tail=()):
    """Entry point lgar_<name> of `lib` on `device` and its current stream: `args`, then the stream, then `tail` (what the
    header puts behind the stream: lgar_forward_tangent's tickets).  A non-zero return raises.  A library that stands in for
    the HIP library on another device (open_library gives none: a test's host build of the device code) gets a null stream."""
    fn = getattr(lib, "lgar_" + name)
    if device.type != "cuda":
        rc = fn(*args, None, *tail)
    else:
        with torch.cuda.device(device):
            rc = fn(*args, C.c_void_p(torch.cuda.current_stream(device).cuda_stream), *tail)
    check(rc, "lgar_" + name)
