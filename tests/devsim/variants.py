"""TEST INFRASTRUCTURE ONLY: the device-code simulator (tests/devsim) built with extra -D switches.

The device code carries switches that turn one piece of work OFF (lgar_py_amd/csrc/lgar_measure.hpp lists them); a CPU test
compares a run with a switch against the run without it.  `engine(flags, ...)` is devsim.SimEngine on a simulator library built
with those flags (libdevsim_<tag>_<L>.so next to the plain ones, rebuilt when a source is newer).
"""
import ctypes as C
import hashlib
import os
import subprocess
import threading

import devsim

_libs = {}
_lock = threading.Lock()


def variant_lib(n_layers, flags):
    """The simulator for one soil-layer count compiled with the extra compiler flags `flags` (a tuple of -D... strings)."""
    flags = tuple(flags)
    if not flags:
        return devsim.lib(n_layers)
    key = (n_layers, flags)
    with _lock:
        if key in _libs:
            return _libs[key]
    # (compiles run outside the lock: prebuild() runs several at once)
    tag = hashlib.sha256(" ".join(flags).encode()).hexdigest()[:10]
    here = os.path.dirname(os.path.abspath(devsim.__file__))
    so = os.path.join(here, "libdevsim_v%s_%d.so" % (tag, n_layers))
    deps = [os.path.join(here, "devsim.cpp"), os.path.join(devsim.ROOT, "include", "lgar.h")] + \
           [os.path.join(devsim.CSRC, f) for f in os.listdir(devsim.CSRC) if f.endswith(".hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        if not os.path.exists(devsim.CLANG):
            raise RuntimeError("clang++ of the ROCm toolchain not found: cannot build the device-code simulator")
        tmp = "%s.%d.%d.tmp" % (so, os.getpid(), threading.get_ident())
        subprocess.check_call([devsim.CLANG, "-x", "c++", "-std=c++17", "-O1", "-ffp-contract=off", "-fPIC", "-shared"] +
                              list(flags) + ["-I", os.path.join(devsim.ROOT, "include"),
                                             "-DDEVSIM_LAYERS(X)=X(%d)" % n_layers, os.path.join(here, "devsim.cpp"), "-o", tmp])
        os.replace(tmp, so)
    L = C.CDLL(so)
    p, i32, vp = C.POINTER, C.c_int32, C.c_void_p
    L.devsim_state_init.argtypes = [p(devsim.LgarDims), p(devsim.LgarParams), p(devsim.LgarState), vp, i32]
    L.devsim_forward.argtypes = [p(devsim.LgarDims), p(devsim.LgarParams), p(devsim.LgarState), p(devsim.LgarForcing),
                                 p(devsim.LgarStepOut), vp, i32]
    with _lock:
        _libs.setdefault(key, L)
        return _libs[key]


class VariantEngine(devsim.SimEngine):
    """devsim.SimEngine running a variant library (forward path only)."""

    def __init__(self, flags, alpha, *args, **kw):
        self._variant_flags = tuple(flags)
        self._variant = None
        super().__init__(alpha, *args, **kw)

    # SimEngine.__init__ stores the plain library in self.lib and calls reset(): the variant takes its place from then on
    def reset(self):
        if self._variant is None:
            self._variant = variant_lib(self.L, self._variant_flags)
        self.lib = self._variant
        super().reset()


def prebuild(n_layers, flag_sets):
    """Build several variants concurrently."""
    import concurrent.futures as cf
    jobs = [(n, tuple(fl)) for n in n_layers for fl in flag_sets]
    with cf.ThreadPoolExecutor(max_workers=min(8, len(jobs))) as ex:
        list(ex.map(lambda j: variant_lib(*j), jobs))
