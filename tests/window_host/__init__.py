"""TEST INFRASTRUCTURE ONLY: the host build of the resumable tangent (lgar_forward_tangent_window: window_host.cpp, the headers
of lgar_py_amd/csrc under -DLGAR_DEVSIM, one library per soil-layer count), the stand-alone program around it
(window_host_main.cpp, also built with AddressSanitizer + UBSan) and WindowSimEngine: devsim.SimEngine -- the product's
LgarEngine over the device-code simulator -- with forward_tangent_window sent to this build.  Never imported by the product."""
import ctypes as C
import os
import threading

import _hostbuild
import devsim
from lgar_py_amd import _capi
from lgar_py_amd._capi import LgarDims, LgarForcing, LgarParams, LgarTangentWindow

_HERE = os.path.dirname(os.path.abspath(__file__))
_CPP = os.path.join(_HERE, "window_host.cpp")
_libs = {}
_lock = threading.Lock()


def library(n_layers):
    """libwindowhost_<L>.so, built on first use: winhost_forward_tangent_window(the arguments of include/lgar.h up to the dtype)."""
    with _lock:
        if n_layers not in _libs:
            so = _hostbuild.build(os.path.join(_HERE, "libwindowhost_%d.so" % n_layers), _CPP, _hostbuild.device_headers(),
                                  ["-fPIC", "-shared", "-DLGAR_LAYERS(X)=X(%d)" % n_layers], "the resumable-tangent host library")
            L = C.CDLL(so)
            p, vp = C.POINTER, C.c_void_p
            L.winhost_forward_tangent_window.argtypes = [p(LgarDims), p(LgarParams), p(LgarParams), p(LgarForcing), vp, vp,
                                                         p(LgarTangentWindow), vp, vp, vp, C.c_int32]
            _libs[n_layers] = L
        return _libs[n_layers]


def program(sanitize=False):
    """The stand-alone program (three soil layers), built on first use; sanitize: AddressSanitizer + UBSan at -O0, any finding
    aborts."""
    flags = ["-DLGAR_LAYERS(X)=X(3)"] + (["-O0"] + _hostbuild.SANITIZE if sanitize else [])
    return _hostbuild.build(os.path.join(_HERE, "window_host_main_san" if sanitize else "window_host_main"),
                            os.path.join(_HERE, "window_host_main.cpp"), [_CPP] + _hostbuild.device_headers(), flags,
                            "the resumable-tangent host program")


class WindowSimEngine(devsim.SimEngine):
    """devsim.SimEngine with lgar_forward_tangent_window on the host build above: everything else about tangent_window,
    snapshot and restore is the product's own code."""

    def _call(self, name, *args, counters=None):
        if name != "forward_tangent_window":
            return super()._call(name, *args, counters=counters)
        _capi.check(library(self.L).winhost_forward_tangent_window(*args, self._dt), "window_host: lgar_" + name)


def install():
    """Put WindowSimEngine behind the autograd functions (in THIS process); returns what to put back."""
    import lgar_py_amd.autograd as A
    before = A.LgarEngine
    A.LgarEngine = WindowSimEngine
    return before
