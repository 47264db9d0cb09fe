"""TEST INFRASTRUCTURE ONLY: the host build of the leaf dispatcher (lgar_py_amd/csrc/lgar_leaf.hpp compiled with -DLGAR_DEVSIM:
the hardware's log2 / exp2 / sqrt / reciprocal become libm's, correctly rounded divide and sqrt) and its ctypes front-end.
leaf_batch() takes what lgar_py_amd.leaf_batch takes, in numpy.  Never imported by the product package."""
import ctypes as C
import os

import numpy as np

import _hostbuild
from lgar_py_amd._capi import F32, F64

_HERE = os.path.dirname(os.path.abspath(__file__))
_lib = None


def library():
    global _lib
    if _lib is None:
        _lib = C.CDLL(_hostbuild.build(os.path.join(_HERE, "libleafhost.so"), os.path.join(_HERE, "leaf_host.cpp"),
                                       _hostbuild.device_headers(), ["-fPIC", "-shared", "-DLGAR_DEVSIM"],
                                       "the leaf dispatcher's host library"))
        vp, i32, dbl = C.c_void_p, C.c_int32, C.c_double
        _lib.leafhost_batch.restype = i32
        _lib.leafhost_batch.argtypes = [i32, i32, vp, vp, dbl, vp, vp, vp, vp, vp, i32, dbl, vp, i32]
        _lib.leafhost_tangent_batch.restype = i32
        _lib.leafhost_tangent_batch.argtypes = [i32, i32, i32, i32, vp, vp, dbl] + [vp] * 12 + [i32, dbl, vp, vp, i32]
    return _lib


def program(sanitize=False):
    """The stand-alone program around the same code (leaf_host_main.cpp), built on first use; sanitize: AddressSanitizer + UBSan
    at -O0, any finding aborts."""
    flags = ["-DLGAR_DEVSIM"] + (["-O0"] + _hostbuild.SANITIZE if sanitize else [])
    return _hostbuild.build(os.path.join(_HERE, "leaf_host_main_san" if sanitize else "leaf_host_main"),
                            os.path.join(_HERE, "leaf_host_main.cpp"), [os.path.join(_HERE, "leaf_host.cpp")] + _hostbuild.device_headers(),
                            flags, "the leaf dispatchers' host program")


SEEDS = ("alpha", "n", "ksat", "theta_e", "theta_r", "x", "y")  # lgar_py_amd.engine.LEAF_SEEDS


def leaf_tangent_batch_status(op, x, y=None, z=0.0, *, alpha, n, ksat, theta_e, theta_r, seeds=None, policy=0, share=0, nint=120,
                              wilting_point_psi=15495.0, dtype=np.float64, null_outputs=False):
    """(status, value, tangent) of tangent op number `op` along `seeds` ({name of SEEDS: [n]}; a name left out is a seed of 0)."""
    prep = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(dtype))
    x, y, alpha, n, ksat, theta_e, theta_r = map(prep, (x, y, alpha, n, ksat, theta_e, theta_r))
    sd = [prep((seeds or {}).get(k)) for k in SEEDS]
    value, tangent = np.empty_like(x), np.empty_like(x)
    ptr = lambda a: None if a is None else a.ctypes.data
    st = library().leafhost_tangent_batch(int(op), int(policy), int(share), x.size, ptr(x), ptr(y), float(z), ptr(alpha), ptr(n), ptr(ksat),
                                          ptr(theta_e), ptr(theta_r), *[ptr(s) for s in sd], int(nint), float(wilting_point_psi),
                                          None if null_outputs else ptr(value), None if null_outputs else ptr(tangent),
                                          F64 if dtype == np.float64 else F32)
    return st, value, tangent


def leaf_tangent_batch(op, x, y=None, z=0.0, **kw):
    st, value, tangent = leaf_tangent_batch_status(op, x, y, z, **kw)
    assert st == 0, (op, st)
    return value, tangent


def leaf_batch_status(op, x, y=None, z=0.0, *, alpha, n, ksat, theta_e, theta_r, nint=120, wilting_point_psi=15495.0, dtype=np.float32):
    """(status, out) of op number `op` over the items."""
    prep = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(dtype))
    x, y, alpha, n, ksat, theta_e, theta_r = map(prep, (x, y, alpha, n, ksat, theta_e, theta_r))
    out = np.empty_like(x)
    ptr = lambda a: None if a is None else a.ctypes.data
    st = library().leafhost_batch(int(op), x.size, ptr(x), ptr(y), float(z), ptr(alpha), ptr(n), ptr(ksat), ptr(theta_e), ptr(theta_r),
                                  int(nint), float(wilting_point_psi), ptr(out), F64 if dtype == np.float64 else F32)
    return st, out


def leaf_batch(op, x, y=None, z=0.0, **kw):
    st, out = leaf_batch_status(op, x, y, z, **kw)
    assert st == 0, (op, st)
    return out
