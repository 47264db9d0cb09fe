"""TEST INFRASTRUCTURE ONLY: the host build of the tangent with a forcing direction (lgar_forward_tangent_forced: forced_host.cpp,
the headers of lgar_py_amd/csrc under -DLGAR_DEVSIM, one library per soil-layer count), the stand-alone program around it
(forced_host_main.cpp, also built with AddressSanitizer + UBSan) and ForcedSimEngine: window_host.WindowSimEngine -- the product's
LgarEngine over the device-code simulator and the window host build -- with forward_tangent_forced sent to this build.  Never
imported by the product."""
import ctypes as C
import os
import threading

import _hostbuild
import window_host
from lgar_py_amd import _capi
from lgar_py_amd._capi import LgarDims, LgarForcing, LgarParams, LgarTangentWindow

_HERE = os.path.dirname(os.path.abspath(__file__))
_CPP = os.path.join(_HERE, "forced_host.cpp")
_libs = {}
_lock = threading.Lock()


def library(n_layers):
    """libforcedhost_<L>.so, built on first use: forcedhost_forward_tangent_forced(the arguments of include/lgar.h up to the
    dtype)."""
    with _lock:
        if n_layers not in _libs:
            so = _hostbuild.build(os.path.join(_HERE, "libforcedhost_%d.so" % n_layers), _CPP, _hostbuild.device_headers(),
                                  ["-fPIC", "-shared", "-DLGAR_LAYERS(X)=X(%d)" % n_layers], "the forced-tangent host library")
            L = C.CDLL(so)
            p, vp = C.POINTER, C.c_void_p
            L.forcedhost_forward_tangent_forced.argtypes = [p(LgarDims), p(LgarParams), p(LgarParams), p(LgarForcing), p(LgarForcing),
                                                            vp, vp, p(LgarTangentWindow), vp, vp, vp, C.c_int32]
            _libs[n_layers] = L
        return _libs[n_layers]


def program(sanitize=False):
    """The stand-alone program (three soil layers), built on first use; sanitize: AddressSanitizer + UBSan at -O0, any finding
    aborts."""
    flags = ["-DLGAR_LAYERS(X)=X(3)"] + (["-O0"] + _hostbuild.SANITIZE if sanitize else [])
    return _hostbuild.build(os.path.join(_HERE, "forced_host_main_san" if sanitize else "forced_host_main"),
                            os.path.join(_HERE, "forced_host_main.cpp"), [_CPP] + _hostbuild.device_headers(), flags,
                            "the forced-tangent host program")


class ForcedSimEngine(window_host.WindowSimEngine):
    """window_host.WindowSimEngine with lgar_forward_tangent_forced on the host build above: everything else about tangent,
    tangent_window and the forcing tangents is the product's own code."""

    def _call(self, name, *args, counters=None):
        if name != "forward_tangent_forced":
            return super()._call(name, *args, counters=counters)
        _capi.check(library(self.L).forcedhost_forward_tangent_forced(*args, self._dt), "forced_host: lgar_" + name)
