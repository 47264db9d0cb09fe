"""TEST INFRASTRUCTURE ONLY: the device-code simulator (tests/devsim/devsim.cpp) and the engine that runs on it.

The simulator is lgar_py_amd/csrc's device code (column physics, per-lane kernel bodies, front-capacity chain) compiled
for the host with -DLGAR_DEVSIM, one lane at a time.  SimEngine is the product's LgarEngine with that library in the HIP
library's place, so CPU tests run the code the GPU executes against the reference's golden vectors, and the product's own
host code -- argument checks, struct filling, the model, the autograd tape, the agent (install()) -- without a GPU.  The
post-processing entry points (soil moisture, totals replay, catchment sums and routing) come from tests/post_host's library,
behind SimEngine, SimCatchmentMap and SimCatchmentRouting.  Never imported by the product package; never timed.
"""
import ctypes as C
import hashlib
import os
import subprocess
import threading

import numpy as np
import torch

import _hostbuild
import post_host
from _hostbuild import CLANG, CSRC, ROOT  # noqa: F401
# the one mirror of include/lgar.h (tests/test_capi_host.py checks it against the header)
from lgar_py_amd import _capi
from lgar_py_amd._capi import ACC_NAMES, LgarDims, LgarError, LgarForcing, LgarParams, LgarState, LgarStepOut  # noqa: F401
from lgar_py_amd.catchments import CatchmentMap, CatchmentRouting
from lgar_py_amd.engine import LgarEngine

_HERE = os.path.dirname(os.path.abspath(__file__))
_libs = {}
_lock = threading.Lock()


def lib(n_layers, flags=(), sanitize=None):
    """libdevsim_<L>.so, built on first use (one soil-layer count per library keeps each build under a minute).  flags: extra
    compiler flags (a tuple of -D... strings: tests/devsim/variants.py) -> libdevsim_v<tag>_<L>.so."""
    # DEVSIM_SANITIZE=1: the AddressSanitizer + UBSan build (the process must run under LD_PRELOAD of clang's asan runtime:
    # tests/test_sanitizers.py)
    san = os.environ.get("DEVSIM_SANITIZE") == "1" if sanitize is None else bool(sanitize)
    key = (n_layers, tuple(flags), san)
    with _lock:
        if key in _libs:
            return _libs[key]
    # (compiles run outside the lock: prebuild() runs several at once)
    tag = ("san_" if san else "") + ("v%s_" % hashlib.sha256(" ".join(flags).encode()).hexdigest()[:10] if flags else "")
    # (the sanitizer build at -O0: a minute instead of six at -O1; its fixtures run in a second either way)
    extra = ["-O0"] + _hostbuild.SANITIZE + ["-shared-libsan"] if san else []
    so = _hostbuild.build(os.path.join(_HERE, "libdevsim_%s%d.so" % (tag, n_layers)), os.path.join(_HERE, "devsim.cpp"),
                          _hostbuild.device_headers(), ["-fPIC", "-shared"] + extra + list(flags) + ["-DLGAR_LAYERS(X)=X(%d)" % n_layers],
                          "the device-code simulator")
    L = C.CDLL(so)
    p, i32, vp = C.POINTER, C.c_int32, C.c_void_p
    L.devsim_state_init.argtypes = [p(LgarDims), p(LgarParams), p(LgarState), vp, i32]
    L.devsim_forward.argtypes = [p(LgarDims), p(LgarParams), p(LgarState), p(LgarForcing), p(LgarStepOut), vp, i32]
    L.devsim_tangent.argtypes = [p(LgarDims), p(LgarParams), p(LgarParams), p(LgarForcing), vp, vp, vp, vp, vp, i32]
    with _lock:
        return _libs.setdefault(key, L)


def sanitizer_runtime():
    """clang's AddressSanitizer runtime (what a process loading the DEVSIM_SANITIZE build must LD_PRELOAD)."""
    out = subprocess.check_output([CLANG, "-print-file-name=libclang_rt.asan-x86_64.so"], text=True).strip()
    return out if os.path.isabs(out) and os.path.exists(out) else None


def prebuild(layers=(2, 3, 4)):
    """Build several layer counts concurrently (conftest calls this once per session)."""
    import concurrent.futures as cf
    with cf.ThreadPoolExecutor(max_workers=len(layers)) as ex:
        list(ex.map(lib, layers))


def _PostLibrary():
    """libposthost.so (tests/post_host) under the HIP library's names.  The catchment sums run one row per wave, the kernel the
    library itself picks for all but huge jobs (the same bits)."""
    return _hostbuild.AsHipLibrary(("", "posthost", post_host.library),
                                   hook=lambda name, fn: (lambda *args: fn(*args[:-1], 1)) if name == "lgar_catchment_sums" else None)


class SimCatchmentMap(CatchmentMap):
    """lgar_py_amd.catchments.CatchmentMap (device="cpu") with the host build of the catchment kernels in the library's place."""

    def _open(self):
        return _PostLibrary()


class SimCatchmentRouting(CatchmentRouting):
    """lgar_py_amd.catchments.CatchmentRouting (device="cpu") with the host build of the routing kernels in the library's place."""

    def _open(self):
        return _PostLibrary()


class SimEngine(LgarEngine):
    """lgar_py_amd.engine.LgarEngine with the simulator in the library's place: torch CPU tensors, the devsim_* entry points.
    Everything about the calling surface is the product's own code.  Also takes numpy dtypes and geff_mode=0|1 for
    geff_precision; forward() does not raise on a faulted column unless asked (check=True): tests read `status`.
    basin_scratch_bytes defaults to 0: the simulator sums basins in the kernel body, a scratch series would be dead weight."""

    _new_series = staticmethod(torch.zeros)  # whole buffers are compared bit for bit, rows no kernel writes included

    def __init__(self, *params, dtype=torch.float64, geff_mode=None, basin_scratch_bytes=0, **kw):
        if geff_mode is not None:
            kw["geff_precision"] = "f32" if geff_mode else "native"
        if not isinstance(dtype, torch.dtype):
            dtype = {"float64": torch.float64, "float32": torch.float32}.get(np.dtype(dtype).name, dtype)
        super().__init__(*params, dtype=dtype, basin_scratch_bytes=basin_scratch_bytes, **kw)

    def forward(self, precip, pet, series=("runoff", "percolation"), out=None, check=False, **kw):
        return super().forward(precip, pet, series, out, check, **kw)

    def _open(self, n_layers, device):
        return lib(n_layers), torch.device("cpu")

    def _call(self, name, *args, counters=None):
        if name in ("soil_moisture", "totals_replay"):
            if name == "soil_moisture":
                *args, _, basin = args  # (weights belong to the basin sums)
                if basin is not None:
                    raise LgarError("the device-code simulator has no basin sums of the soil moisture: the summation order of "
                                    "lgar_basin_reduce_kernel has no host form")
            return _capi.launch(_PostLibrary(), name, self.device, *args, self._dt)
        fn = getattr(self.lib, "devsim_" + {"forward_tangent": "tangent"}.get(name, name))
        _capi.check(fn(*args, self._dt), "devsim: lgar_" + name)

    def step_rows_host(self, precip_row, pet_row):
        a = lambda t: torch.as_tensor(t, dtype=torch.float64).reshape(1, -1)
        res = self.forward(a(precip_row), a(pet_row), series=("runoff", "percolation"), call_sums=True)
        return res["call_sums"], res["runoff"][0], res["percolation"][0], self.status.clone()

    def cooperating_lanes(self):
        raise LgarError("the device-code simulator has no lgar_cooperating_lanes")


def install():
    """Put the simulator behind the model and the autograd tape (in THIS process)."""
    import lgar_py_amd.autograd as A
    import lgar_py_amd.model as M
    M.LgarEngine = A.LgarEngine = SimEngine
