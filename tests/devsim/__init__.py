"""TEST INFRASTRUCTURE ONLY: ctypes front-end of the device-code simulator (tests/devsim/devsim.cpp).

The simulator is lgar_py_amd/csrc's device code (column physics, per-lane kernel bodies, front-capacity chain) compiled
for the host with -DLGAR_DEVSIM, one lane at a time.  CPU tests use it to run the code the GPU executes against the
reference's golden vectors.  Never imported by the product package; never timed.
"""
import ctypes as C
import hashlib
import os
import subprocess
import threading

import numpy as np

import _hostbuild
from _hostbuild import CLANG, CSRC, ROOT  # noqa: F401
# the one mirror of include/lgar.h (tests/test_capi_host.py checks it against the header)
from lgar_py_amd._capi import (ACC_NAMES, FMAX, GMAX, NACC, NCOUNTERS, NSCAL, LgarDims, LgarForcing, LgarParams,  # noqa: F401
                               LgarState, LgarStepOut, make_dims)

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


class SimEngine:
    """Host-memory twin of lgar_py_amd.engine.LgarEngine running the simulator (numpy arrays, same layouts)."""

    def __init__(self, alpha, n, ksat, theta_e, theta_r, thickness, *, n_columns=None, dt_h=1.0, num_subcycles=1,
                 initial_psi=2000.0, ponded_depth_max=0.0, wilting_point_psi=15495.0, frozen_factor=1.0, nint=120,
                 giuh_ordinates=(0.06, 0.51, 0.28, 0.12, 0.03), dtype=np.float64, iter_cap=0, search_mode=1, bottom_mode=0,
                 use_closed_form_G=False, front_slots=None, geff_mode=0):
        self.dtype = np.dtype(dtype)
        self._dt = 1 if self.dtype == np.float64 else 0

        def prep(x):
            t = np.asarray(x, dtype=np.float64)
            if t.ndim == 1:
                t = np.repeat(t[:, None], n_columns, axis=1)
            return np.ascontiguousarray(t.astype(self.dtype))

        self.alpha, self.n, self.ksat = prep(alpha), prep(n), prep(ksat)
        self.theta_e, self.theta_r, self.thickness = prep(theta_e), prep(theta_r), prep(thickness)
        L, N = self.alpha.shape
        self.L, self.N = L, N
        self.lib = lib(L)
        d = self.dims = make_dims(
            n_columns=N, n_layers=L, dt_h=dt_h, num_subcycles=num_subcycles, initial_psi=initial_psi,
            ponded_depth_max=ponded_depth_max, wilting_point_psi=wilting_point_psi, frozen_factor=frozen_factor, nint=nint,
            giuh_ordinates=giuh_ordinates, iter_cap=iter_cap, search_mode=search_mode, bottom_mode=bottom_mode,
            use_closed_form_G=use_closed_form_G, front_slots=front_slots, geff_mode=geff_mode)
        F = d.front_slots
        z = lambda *s, dt=self.dtype: np.zeros(s, dtype=dt)
        self.depth, self.theta, self.psi, self.k, self.dzdt = z(F, N), z(F, N), z(F, N), z(F, N), z(F, N)
        self.flags, self.n_fronts = z(F, N, dt=np.uint8), z(N, dt=np.int32)
        self.scalars, self.totals, self.status = z(NSCAL, N), z(NACC, N), z(N, dt=np.int32)
        self.counters = z(NCOUNTERS, dt=np.uint64)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        self._params = LgarParams(*[ptr(t) for t in (self.alpha, self.n, self.ksat, self.theta_e, self.theta_r, self.thickness)])
        self._state = LgarState(*[ptr(t) for t in (self.depth, self.theta, self.psi, self.k, self.dzdt, self.flags,
                                                   self.n_fronts, self.scalars, self.totals)] + [None])
        self.reset()

    def reset(self):
        rc = self.lib.devsim_state_init(C.byref(self.dims), C.byref(self._params), C.byref(self._state),
                                        self.status.ctypes.data_as(C.c_void_p), self._dt)
        assert rc == 0, rc

    def forward(self, precip, pet, series=("runoff", "percolation"), basin=(), weights=None, call_sums=False, forcing_group=1):
        precip = np.ascontiguousarray(np.asarray(precip, dtype=np.float64).astype(self.dtype))
        pet = np.ascontiguousarray(np.asarray(pet, dtype=np.float64).astype(self.dtype))
        T = precip.shape[0]
        assert precip.shape == pet.shape and self.N % (precip.shape[1] * forcing_group) == 0
        self.dims.forcing_columns = precip.shape[1]
        self.dims.forcing_group = forcing_group
        res, so = {}, LgarStepOut()
        for nm in series:
            buf = np.zeros((T, self.N), dtype=self.dtype)
            res[nm] = buf
            so.series[ACC_NAMES.index(nm)] = buf.ctypes.data_as(C.c_void_p)
        keep = []
        if basin:
            block = np.zeros((NACC, T))
            so.basin = block.ctypes.data_as(C.c_void_p)
            for nm in basin:
                so.basin_mask |= 1 << ACC_NAMES.index(nm)
                res["basin:" + nm] = block[ACC_NAMES.index(nm)]
            if weights is not None:
                w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).astype(self.dtype))
                keep.append(w)
                so.weights = w.ctypes.data_as(C.c_void_p)
        so.counters = self.counters.ctypes.data_as(C.c_void_p)
        if call_sums:
            res["call_sums"] = np.zeros((NACC, self.N), dtype=self.dtype)
            so.call_sums = res["call_sums"].ctypes.data_as(C.c_void_p)
        self.dims.n_steps = T
        fo = LgarForcing(precip.ctypes.data_as(C.c_void_p), pet.ctypes.data_as(C.c_void_p))
        rc = self.lib.devsim_forward(C.byref(self.dims), C.byref(self._params), C.byref(self._state), C.byref(fo), C.byref(so),
                                     self.status.ctypes.data_as(C.c_void_p), self._dt)
        assert rc == 0, rc
        return res

    def tangent(self, direction, precip, pet, w_runoff=None, w_perc=None, want_series=False, forcing_group=1):
        prep = lambda t: None if t is None else np.ascontiguousarray(np.asarray(t, dtype=np.float64).astype(self.dtype))
        precip, pet, w_runoff, w_perc = prep(precip), prep(pet), prep(w_runoff), prep(w_perc)
        T = precip.shape[0]
        assert self.N % (precip.shape[1] * forcing_group) == 0
        self.dims.forcing_columns = precip.shape[1]
        self.dims.forcing_group = forcing_group
        dirs = {k: prep(direction.get(k)) for k in ("alpha", "n", "ksat")}
        ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        dstruct = LgarParams(ptr(dirs["alpha"]), ptr(dirs["n"]), ptr(dirs["ksat"]), None, None, None)
        grad = np.zeros(self.N, dtype=self.dtype)
        ser = np.zeros((T, self.N), dtype=self.dtype) if want_series else None
        st = np.zeros(self.N, dtype=np.int32)
        self.dims.n_steps = T
        fo = LgarForcing(ptr(precip), ptr(pet))
        rc = self.lib.devsim_tangent(C.byref(self.dims), C.byref(self._params), C.byref(dstruct), C.byref(fo), ptr(w_runoff),
                                     ptr(w_perc), ptr(grad), ptr(ser), ptr(st), self._dt)
        assert rc == 0, rc
        return grad, ser, st

    def fronts(self):
        fl = self.flags
        return dict(depth=self.depth, theta=self.theta, psi=self.psi, k=self.k, dzdt=self.dzdt,
                    layer=(fl & 0x7F).astype("int8"), to_bottom=(fl >> 7).astype("int8"), n_fronts=self.n_fronts)
