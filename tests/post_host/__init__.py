"""TEST INFRASTRUCTURE ONLY: the one host build of the post-processing headers (lgar_py_amd/csrc/lgar_moisture.hpp,
lgar_catchment.hpp, lgar_route.hpp, compiled for the host with -DLGAR_DEVSIM) and its front-end.  post_host.hpp holds the
host-side launchers of the six entry points; post_host.cpp is the stand-alone program around them (run() below; also built
with AddressSanitizer + UBSan), libposthost.so the same header as a shared library (library(): what the device-code simulator
puts behind the product's calling surface).  The numpy statements of the definitions, and the calls of the program the tests'
cases turn into, are in the submodules moisture, catchment and route.  Never imported by the product package.
"""
import ctypes as C
import os
import struct
import tempfile

import numpy as np

import _hostbuild
from _hostbuild import CSRC, ROOT
from lgar_py_amd._capi import F32, F64, LgarDims, LgarParams, LgarState, LgarStepOut

_HERE = os.path.dirname(os.path.abspath(__file__))
_HPP = os.path.join(_HERE, "post_host.hpp")
_DEPS = [os.path.join(CSRC, "lgar_%s.hpp" % nm) for nm in ("moisture", "catchment", "route")] + [os.path.join(ROOT, "include", "lgar.h")]
# the operation codes of post_host.cpp
OPS = ("soil_moisture", "totals_replay", "catchment_sums", "catchment_spread", "catchment_route", "catchment_route_grad")


def same_bits(a, b):
    """Bit-for-bit equality of two float arrays (NaNs must sit in the same places)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = np.uint64 if a.dtype == np.float64 else np.uint32
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(u)[~na] == b.view(u)[~nb]).all())


def dtype_code(dtype):
    assert dtype in (np.float32, np.float64)
    return F64 if dtype == np.float64 else F32


def program(sanitize=False):
    """The host program, built on first use with the ROCm clang (sanitize: AddressSanitizer + UBSan, any finding aborts)."""
    return _hostbuild.build(os.path.join(_HERE, "post_host_san" if sanitize else "post_host"), os.path.join(_HERE, "post_host.cpp"),
                            [_HPP] + _DEPS, _hostbuild.SANITIZE if sanitize else [], "the post-processing host program")


def library():
    """libposthost.so: posthost_<entry point>(the arguments of include/lgar.h without the stream), loaded once."""
    global _lib
    if _lib is None:
        _lib = C.CDLL(_hostbuild.build(os.path.join(_HERE, "libposthost.so"), _HPP, _DEPS, ["-fPIC", "-shared"],
                                       "the post-processing host library"))
        p, i32, vp = C.POINTER, C.c_int32, C.c_void_p
        _lib.posthost_soil_moisture.argtypes = [p(LgarDims), p(LgarParams), p(LgarState), vp, i32, i32, vp, i32]
        _lib.posthost_totals_replay.argtypes = [p(LgarDims), p(LgarStepOut), i32, vp, i32]
        _lib.posthost_catchment_sums.argtypes = [vp, i32, i32, vp, i32, vp, i32, vp, vp, vp, vp, i32, i32]
        _lib.posthost_catchment_spread.argtypes = [vp, i32, i32, vp, i32, vp, vp, vp, i32]
        _lib.posthost_catchment_route.argtypes = [vp, i32, i32, vp, i32, i32, vp, vp, vp, i32]
        _lib.posthost_catchment_route_grad.argtypes = [vp, vp, i32, i32, i32, vp]
    return _lib


_lib = None


class Out:
    """An output array of a call: the program allocates it at exactly this size and writes it back.  start: what it holds
    before the call (an array that is input and output), default: nothing meaningful."""

    def __init__(self, dtype, *shape, start=None):
        self.dtype, self.shape, self.start, self.value = np.dtype(dtype), shape, start, None


def run(cases, sanitize=False):
    """ONE run of the host program over every case.  A case is (calls, result): calls is a list of (operation, int32 scalars,
    arrays) in the argument order post_host.cpp states, an array being a numpy array (an input), None (a null pointer) or an
    Out; result is an Out of those calls, or a tuple of them and of None.  Returns the result of every case with the arrays the
    program wrote in the Outs' places."""
    cases = list(cases)
    calls = [call for case_calls, _ in cases for call in case_calls]
    blob, outs = [struct.pack("i", len(calls))], []
    for op, scalars, arrays in calls:
        blob.append(struct.pack("3i%di" % len(scalars), OPS.index(op), len(scalars), len(arrays), *scalars))
        for a in arrays:
            if a is None:
                blob.append(struct.pack("2iq", 1, 3, 0))
            elif isinstance(a, Out):
                blob.append(struct.pack("2iq", a.dtype.itemsize, 1 if a.start is None else 2, int(np.prod(a.shape))))
                if a.start is not None:
                    blob.append(np.ascontiguousarray(a.start, dtype=a.dtype).reshape(a.shape).tobytes())
                outs.append(a)
            else:
                a = np.ascontiguousarray(a)
                blob += [struct.pack("2iq", a.dtype.itemsize, 0, a.size), a.tobytes()]
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as fh:
            fh.write(b"".join(blob))
        _hostbuild.run_clean([program(sanitize), fin, fout])
        raw = open(fout, "rb").read()
    at = 0
    for o in outs:
        n = int(np.prod(o.shape)) * o.dtype.itemsize
        o.value = np.frombuffer(raw[at:at + n], dtype=o.dtype).reshape(o.shape).copy()
        at += n
    assert at == len(raw)
    take = lambda r: None if r is None else r.value
    return [take(result) if isinstance(result, Out) else tuple(take(r) for r in result) for _, result in cases]
