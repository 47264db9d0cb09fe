"""TEST INFRASTRUCTURE ONLY: the one host build of the post-processing headers (lgar_py_amd/csrc/lgar_moisture.hpp,
lgar_catchment.hpp, lgar_route.hpp, compiled for the host with -DLGAR_DEVSIM) and its front-end.  post_host.hpp holds the
host-side launchers of the six entry points; post_host.cpp is the stand-alone program around them (run() below; also built
with AddressSanitizer + UBSan), libposthost.so the same header as a shared library (library(): what the device-code simulator
puts behind the product's calling surface).  The numpy statements of the definitions, and the calls of the program the tests'
cases turn into, are in the submodules moisture, catchment and route.
The build, the program's call records (tests/_hostprog.hpp) and same_bits are tests/_hostbuild.py's: UNIT below.
Never imported by the product package.
"""
import ctypes as C
import os

import numpy as np

import _hostbuild
from _hostbuild import Out, same_bits  # noqa: F401
from lgar_py_amd._capi import F32, F64, LgarDims, LgarParams, LgarState, LgarStepOut

_HERE = os.path.dirname(os.path.abspath(__file__))
# the operation codes of post_host.cpp
OPS = ("soil_moisture", "totals_replay", "catchment_sums", "catchment_spread", "catchment_route", "catchment_route_grad")


def dtype_code(dtype):
    assert dtype in (np.float32, np.float64)
    return F64 if dtype == np.float64 else F32


# (an array of no elements goes to these entry points at an address of its own, not as a null pointer)
UNIT = _hostbuild.HostUnit(_HERE, "post_host", "posthost", ["lgar_%s.hpp" % nm for nm in ("moisture", "catchment", "route")], "post-processing",
                           null_when_empty=False)


def library():
    """libposthost.so: posthost_<entry point>(the arguments of include/lgar.h without the stream), loaded once."""
    p, i32, vp = C.POINTER, C.c_int32, C.c_void_p
    return UNIT.library({"soil_moisture": [p(LgarDims), p(LgarParams), p(LgarState), vp, i32, i32, vp, i32],
                         "totals_replay": [p(LgarDims), p(LgarStepOut), i32, vp, i32],
                         "catchment_sums": [vp, i32, i32, vp, i32, vp, i32, vp, vp, vp, vp, i32, i32],
                         "catchment_spread": [vp, i32, i32, vp, i32, vp, vp, vp, i32],
                         "catchment_route": [vp, i32, i32, vp, i32, i32, vp, vp, vp, i32], "catchment_route_grad": [vp, vp, i32, i32, i32, vp]})


def run(cases, sanitize=False):
    """ONE run of the host program over every case.  A case is (calls, result): calls is a list of (operation, int32 scalars,
    arrays) in the argument order post_host.cpp states, an array being a numpy array (an input), None (a null pointer) or an
    Out; result is an Out of those calls, or a tuple of them and of None.  Returns the result of every case with the arrays the
    program wrote in the Outs' places."""
    cases = list(cases)
    UNIT.run_calls([(OPS.index(op), scalars, (), arrays) for case_calls, _ in cases for op, scalars, arrays in case_calls], sanitize)
    return [result.value if isinstance(result, Out) else _hostbuild.values(result) for _, result in cases]
