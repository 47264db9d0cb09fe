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
    return _lib


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
